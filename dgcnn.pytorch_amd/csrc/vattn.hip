// Fused forward of the kNN vector attention (reference models/attention.py:
// 107-150, VectorAttention.forward after its three projections): per edge
// (i, j = idx[i][s]) of the kNN graph
//   delta = pos[j] - pos[i]
//   r = W2p relu(W1p delta + b1p) + b2p                     pos_mlp  (3 -> Hp -> Dm)
//   s = Wa2 relu(Wa1 (D_j + r) + ba1) + ba2                 attn_mlp (Dm -> H -> Dm)
//   a = softmax(s over the Dm channels)
// and per point   agg_c = sum_s a_sc (V_j + r)_c / max(sqrt(sum_s a_sc^2), 1e-12)
// (F.normalize over the k neighbours folded into the aggregation). Only agg
// (B N x Dm fp32) is written: no per-edge tensor reaches HBM.
//
// A block is four waves that share the staged weights and otherwise work alone:
// wave w takes points w, w + 4, ... of the block's VA_PPB, one at a time. The
// point's k edge rows, padded to ceil(k / 16) row tiles, are the MFMA row
// tiles. Per tile the wave writes relu(pos layer 1) (K = 3: plain fp32 FMAs) to
// its LDS tile in the A-operand layout, multiplies by W2p (r stays in the
// accumulators for the rest of the tile), writes u = D_j + r back to the same
// tile, runs Dm -> H in four groups of four column tiles into its h tile, then
// H -> Dm, and takes the softmax across the row's 64 channels in the
// accumulator layout (4 column tiles in registers x 16 lanes by shuffles),
// with the row maximum subtracted. The running sums sum a (V_j + r) and sum a^2
// live in registers over the tiles; rows >= k contribute 0 by select. Gathers,
// softmax, norm and aggregation are fp32 in both modes.
//
// Two operand modes from the one template. bf16: v_mfma_f32_16x16x32_bf16; the
// weights are rounded once per block into LDS (80 KB with the row padding) and
// the activation tiles are rounded as they are staged. fp32: exact products on
// v_mfma_f32_16x16x4_f32 (as gemm32.hip); the weights (147 KB) do not fit next
// to the tiles, so their fragments are re-read from L2 as float4 (the MFMA's k
// slot of lane group g is element 4 g + j of a 16-wide K step for both
// operands, so one 16-byte load feeds four MFMAs). The tile / column-group
// loops are rolled (DESIGN's instruction-cache lesson). A cloud's blocks stay
// on one XCD (dgx_xcd_cloud_map): its D / V rows are served from that L2.
#include "common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int VA_DM = 64, VA_H = 256, VA_HP = 64, VA_KMAX = 64;
constexpr int VA_WAVES = 4, VA_PPW = 8, VA_PPB = VA_WAVES * VA_PPW, VA_THREADS = 64 * VA_WAVES;

template <bool BF>
struct VaT {
    using T = typename std::conditional<BF, __bf16, float>::type;
    static constexpr int PAD = BF ? 8 : 4;             // 16 bytes: staggers the rows over the banks
    static constexpr int P64 = 64 + PAD, P256 = 256 + PAD;
    static constexpr size_t kConst = 64 * sizeof(float4) + (VA_DM + VA_H + VA_DM) * sizeof(float);
    static constexpr size_t kWeights = BF ? (size_t)(VA_DM * P64 + VA_H * P64 + VA_DM * P256) * sizeof(__bf16) : 0;
    static constexpr size_t kWave = (size_t)(16 * P64 + 16 * P256) * sizeof(T);
    static constexpr size_t kLds = kConst + kWeights + VA_WAVES * kWave;
};

__device__ __forceinline__ float relu_nan(float v) { return v < 0.f ? 0.f : v; }   // NaN stays NaN, as torch's relu

// acc[ct] += A (16 x K, LDS tile) * W[16 (ct0 + ct) + n][.]^T for NT column tiles.
// acc[ct][r] is row 4 g + r, column 16 (ct0 + ct) + r16 of the product.
template <bool BF, int K, int NT, typename WT>
__device__ __forceinline__ void va_mma(const typename VaT<BF>::T* __restrict__ At, int lda, const WT* __restrict__ W,
                                       int ldw, int ct0, f32x4* acc, int r16, int g) {
    if constexpr (BF) {
#pragma unroll
        for (int ks = 0; ks < K / 32; ++ks) {
            const bf16x8 af = *reinterpret_cast<const bf16x8*>(At + r16 * lda + 32 * ks + 8 * g);
#pragma unroll
            for (int ct = 0; ct < NT; ++ct) {
                const bf16x8 bf = *reinterpret_cast<const bf16x8*>(W + (16 * (ct0 + ct) + r16) * ldw + 32 * ks + 8 * g);
                acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bf, acc[ct], 0, 0, 0);
            }
        }
    } else {
#pragma unroll 2
        for (int q = 0; q < K / 16; ++q) {
            const float4 a4 = *reinterpret_cast<const float4*>(At + r16 * lda + 16 * q + 4 * g);
            const float a[4] = {a4.x, a4.y, a4.z, a4.w};
#pragma unroll
            for (int ct = 0; ct < NT; ++ct) {
                const float4 b4 = *reinterpret_cast<const float4*>(W + (16 * (ct0 + ct) + r16) * ldw + 16 * q + 4 * g);
                const float bv[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], bv[j], acc[ct], 0, 0, 0);
            }
        }
    }
}

template <bool BF>
__global__ __launch_bounds__(VA_THREADS) void vattn_fwd_kernel(
    const float* __restrict__ D, const float* __restrict__ V, const float* __restrict__ pos,
    const int32_t* __restrict__ idx, int B, int N, int k, int tiles, int64_t gstride,
    const float* __restrict__ pw1, const float* __restrict__ pb1, const float* __restrict__ pw2,
    const float* __restrict__ pb2, const float* __restrict__ aw1, const float* __restrict__ ab1,
    const float* __restrict__ aw2, const float* __restrict__ ab2, float* __restrict__ agg) {
    using X = VaT<BF>;
    using T = typename X::T;
    constexpr int P64 = X::P64, P256 = X::P256;
    extern __shared__ __attribute__((aligned(16))) uint8_t va_lds[];
    int b, tile;
    if (!dgx_xcd_cloud_map(blockIdx.x, B, tiles, b, tile)) return;   // block-uniform: before any barrier
    float4* w1s = reinterpret_cast<float4*>(va_lds);                  // pos layer 1: (w_x, w_y, w_z, bias) per channel
    float* b2s = reinterpret_cast<float*>(w1s + 64);                  // b2p | ba1 | ba2
    float* ba1s = b2s + VA_DM;
    float* ba2s = ba1s + VA_H;
    __bf16* W2s = reinterpret_cast<__bf16*>(va_lds + X::kConst);      // bf16 mode: the three MFMA weights
    __bf16* Wa1s = W2s + VA_DM * P64;
    __bf16* Wa2s = Wa1s + VA_H * P64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    T* ut = reinterpret_cast<T*>(va_lds + X::kConst + X::kWeights + wave * X::kWave);   // 16 x 64: e, then u
    T* ht = ut + 16 * P64;                                                              // 16 x 256: h
    if (tid < VA_HP) w1s[tid] = make_float4(pw1[3 * tid], pw1[3 * tid + 1], pw1[3 * tid + 2], pb1[tid]);
    if (tid < VA_DM) { b2s[tid] = pb2[tid]; ba2s[tid] = ab2[tid]; }
    ba1s[tid] = ab1[tid];
    if constexpr (BF) {
        for (int e = tid; e < VA_DM * VA_HP; e += VA_THREADS) W2s[(e >> 6) * P64 + (e & 63)] = (__bf16)pw2[e];
        for (int e = tid; e < VA_H * VA_DM; e += VA_THREADS) Wa1s[(e >> 6) * P64 + (e & 63)] = (__bf16)aw1[e];
        for (int e = tid; e < VA_DM * VA_H; e += VA_THREADS) Wa2s[(e >> 8) * P256 + (e & 255)] = (__bf16)aw2[e];
    }
    __syncthreads();
    const int g = lane >> 4, r16 = lane & 15;
    const int KT = (k + 15) >> 4;
    // every wave runs the same trip counts (all barriers are met): a wave whose
    // point lies past the cloud's end recomputes point N - 1 and stores nothing
#pragma unroll 1
    for (int it = 0; it < VA_PPW; ++it) {
        const int p = tile * VA_PPB + it * VA_WAVES + wave;
        const bool live = p < N;
        const int64_t i = (int64_t)b * N + min(p, N - 1);
        const float cx = pos[i * 3], cy = pos[i * 3 + 1], cz = pos[i * 3 + 2];
        float S1[4] = {0.f, 0.f, 0.f, 0.f}, S2[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
        for (int rt = 0; rt < KT; ++rt) {
            // A-layout role: edge row r16 of the tile; rows >= k repeat row k - 1 and are masked at the end
            const int ja = idx[i * k + min(16 * rt + r16, k - 1)];
            const int64_t ga = (int64_t)b * gstride + ja;
            const float dx = pos[ga * 3] - cx, dy = pos[ga * 3 + 1] - cy, dz = pos[ga * 3 + 2] - cz;
            int64_t gc[4];   // C-layout role: rows 4 g + r
#pragma unroll
            for (int r = 0; r < 4; ++r) gc[r] = ((int64_t)b * gstride + __shfl(ja, 4 * g + r)) * VA_DM;
            // e = relu(W1p delta + b1p) for the 16 channels of this lane's A fragments
            if constexpr (BF) {
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    bf16x8 o;
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const float4 w = w1s[32 * ks + 8 * g + j];
                        o[j] = (__bf16)relu_nan(fmaf(w.z, dz, fmaf(w.y, dy, fmaf(w.x, dx, w.w))));
                    }
                    *reinterpret_cast<bf16x8*>(ut + r16 * P64 + 32 * ks + 8 * g) = o;
                }
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    float o[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float4 w = w1s[16 * q + 4 * g + j];
                        o[j] = relu_nan(fmaf(w.z, dz, fmaf(w.y, dy, fmaf(w.x, dx, w.w))));
                    }
                    *reinterpret_cast<float4*>(ut + r16 * P64 + 16 * q + 4 * g) = make_float4(o[0], o[1], o[2], o[3]);
                }
            }
            __syncthreads();
            f32x4 rr[4];   // r = pos_mlp(delta): rows 4 g + r, channels 16 ct + r16
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) rr[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
            if constexpr (BF) va_mma<BF, VA_HP, 4>(ut, P64, W2s, P64, 0, rr, r16, g);
            else va_mma<BF, VA_HP, 4>(ut, P64, pw2, VA_HP, 0, rr, r16, g);
            // biases are added to the finished sums: the products accumulate at their own magnitude
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) rr[ct] += b2s[16 * ct + r16];
            __syncthreads();   // e is read: the tile now takes u = D_j + r
#pragma unroll
            for (int ct = 0; ct < 4; ++ct)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    ut[(4 * g + r) * P64 + 16 * ct + r16] = (T)(D[gc[r] + 16 * ct + r16] + rr[ct][r]);
            __syncthreads();
#pragma unroll 1
            for (int c4 = 0; c4 < VA_H / 64; ++c4) {
                f32x4 hh[4];
#pragma unroll
                for (int ct = 0; ct < 4; ++ct) hh[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
                if constexpr (BF) va_mma<BF, VA_DM, 4>(ut, P64, Wa1s, P64, 4 * c4, hh, r16, g);
                else va_mma<BF, VA_DM, 4>(ut, P64, aw1, VA_DM, 4 * c4, hh, r16, g);
#pragma unroll
                for (int ct = 0; ct < 4; ++ct)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        ht[(4 * g + r) * P256 + 64 * c4 + 16 * ct + r16] =
                            (T)relu_nan(hh[ct][r] + ba1s[64 * c4 + 16 * ct + r16]);
            }
            __syncthreads();
            f32x4 ss[4];
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) ss[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
            if constexpr (BF) va_mma<BF, VA_H, 4>(ht, P256, Wa2s, P256, 0, ss, r16, g);
            else va_mma<BF, VA_H, 4>(ht, P256, aw2, VA_H, 0, ss, r16, g);
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) ss[ct] += ba2s[16 * ct + r16];
            // softmax over the row's 64 channels: 4 here, 16 lanes of the group
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float m = fmaxf(fmaxf(ss[0][r], ss[1][r]), fmaxf(ss[2][r], ss[3][r]));
#pragma unroll
                for (int o = 1; o < 16; o <<= 1) m = fmaxf(m, __shfl_xor(m, o));
                float ev[4], sum = 0.f;
#pragma unroll
                for (int ct = 0; ct < 4; ++ct) { ev[ct] = expf(ss[ct][r] - m); sum += ev[ct]; }
#pragma unroll
                for (int o = 1; o < 16; o <<= 1) sum += __shfl_xor(sum, o);
                const bool valid = 16 * rt + 4 * g + r < k;
#pragma unroll
                for (int ct = 0; ct < 4; ++ct) {
                    const float a = ev[ct] / sum;
                    const float w = V[gc[r] + 16 * ct + r16] + rr[ct][r];
                    S1[ct] += valid ? a * w : 0.f;
                    S2[ct] += valid ? a * a : 0.f;
                }
            }
        }
        // the four lane groups hold rows 4 g .. of the same channels
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
            S1[ct] += __shfl_xor(S1[ct], 16);
            S2[ct] += __shfl_xor(S2[ct], 16);
            S1[ct] += __shfl_xor(S1[ct], 32);
            S2[ct] += __shfl_xor(S2[ct], 32);
        }
        float s1 = S1[0], s2 = S2[0];   // group g writes column tile g
#pragma unroll
        for (int u = 1; u < 4; ++u) { s1 = g == u ? S1[u] : s1; s2 = g == u ? S2[u] : s2; }
        if (live) agg[i * VA_DM + 16 * g + r16] = s1 / fmaxf(sqrtf(s2), 1e-12f);
    }
}

bool va_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" {

int dgx_vattn_fused_shape(int Dm, int H, int Hp, int k) {
    return Dm == VA_DM && H == VA_H && Hp == VA_HP && k >= 1 && k <= VA_KMAX;
}

int dgx_vattn_fwd_points(void) { return VA_PPB; }

int dgx_vattn_fwd(const float* D, const float* V, int64_t rows, const float* pos, const int32_t* idx, int B, int N,
                  int k, int64_t gather_stride, const float* pos_w1, const float* pos_b1, const float* pos_w2,
                  const float* pos_b2, const float* attn_w1, const float* attn_b1, const float* attn_w2,
                  const float* attn_b2, int Dm, int H, int Hp, int bf16, float* agg, void* stream) {
    if (B < 0 || N < 0 || k < 1 || Dm < 1 || H < 1 || Hp < 1 || gather_stride < 0) return DGX_EINVAL;
    if (!dgx_vattn_fused_shape(Dm, H, Hp, k)) return DGX_EUNSUPPORTED;
    if (B == 0 || N == 0) return DGX_OK;
    if (!D || !V || !pos || !idx || !pos_w1 || !pos_b1 || !pos_w2 || !pos_b2 || !attn_w1 || !attn_b1 || !attn_w2 ||
        !attn_b2 || !agg)
        return DGX_EINVAL;
    // the gathered row of cloud b is b * gather_stride + id, id < N: inside the tables
    if ((int64_t)(B - 1) * gather_stride + N > rows) return DGX_EINVAL;
    if (!va_al16(pos_w2) || !va_al16(attn_w1) || !va_al16(attn_w2)) return DGX_EUNSUPPORTED;
    const int tiles = (N + VA_PPB - 1) / VA_PPB;
    const dim3 grid((unsigned)dgx_xcd_cloud_grid(B, tiles));
    hipStream_t st = dgx_stream(stream);
    if (bf16)
        hipLaunchKernelGGL((vattn_fwd_kernel<true>), grid, dim3(VA_THREADS), VaT<true>::kLds, st, D, V, pos, idx, B, N,
                           k, tiles, gather_stride, pos_w1, pos_b1, pos_w2, pos_b2, attn_w1, attn_b1, attn_w2, attn_b2,
                           agg);
    else
        hipLaunchKernelGGL((vattn_fwd_kernel<false>), grid, dim3(VA_THREADS), VaT<false>::kLds, st, D, V, pos, idx, B,
                           N, k, tiles, gather_stride, pos_w1, pos_b1, pos_w2, pos_b2, attn_w1, attn_b1, attn_w2,
                           attn_b2, agg);
    DGX_CHECK_LAUNCH();
    return DGX_OK;
}

}  // extern "C"
