// Batches assembled on the device from a device-resident dataset: what the
// reference's input side does per step on the host (data.py:353-364: up to
// three small torch ops per item in a random order; the default collate; the
// one-hot loop main_partseg_dist.py:241-244; three H2D copies; permute(0, 2, 1)
// and .contiguous()) as one launch that reads the stored clouds and writes the
// batch the model takes: sample selection, point shuffle, the augmentations,
// the (B, C, N) layout, seg - seg_start and the one-hot label.
//
// One workgroup per output cloud. It reads its slot's item id from `order`,
// draws the cloud's parameters (include/dgx.h states every word of the
// Philox4x32-10 layout; dgx.cpu restates it), sorts the words (key << 32) | j
// of the cloud's first N points in LDS with a bitonic network over the next
// power of two (padded with all-ones; the words are distinct, so the keys alone
// fix the permutation) and then walks the output points, one lane per point:
// a gathered read of the point's C channels, the augmentations with every
// multiply and add rounded on its own (contraction is switched off for this
// file: no FMA is formed, so the host reproduces the points bit for bit), and
// writes that are coalesced along N for each channel.
//
// Cursor and batch count belong to the launch as a whole, as in metrics.hip:
// every workgroup reads the cursor when it starts and takes a ticket when it is
// done, and the one that draws the last ticket advances them and puts the
// ticket back to 0. No workgroup waits for another.
//
// Nothing read from memory is used as an address before it is checked: an item
// id outside [0, n_items) or a label outside [0, ncat) is counted in `invalid`
// and its cloud written as zeros; a workgroup whose slot lies at or beyond
// n_epoch writes nothing and adds to `overrun`.
#include "common.h"

// hipcc contracts a * b + c into an FMA by default, across statements too, and HIP's __fmul_rn / __fadd_rn are
// plain operators that do not stop it: every operation below keeps its own rounding
#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ float fmul(float x, float y) { return x * y; }
__device__ __forceinline__ float fadd(float x, float y) { return x + y; }

constexpr int BA_THREADS = 512;
constexpr int BA_MAX_POINTS = 4096;   // 4096 x 8 bytes = 32 KiB of LDS

enum { BA_CURSOR = 0, BA_EPOCH = 1, BA_INVALID = 2, BA_OVERRUN = 3, BA_BATCHES = 4, BA_TICKET = 5 };
enum { BA_T = 0, BA_J = 1, BA_R = 2 };

struct BaArgs {
    const float* points;
    const int32_t* seg;
    const int32_t* label;
    int64_t n_items, P;
    int C;
    const int32_t* order;
    int64_t n_epoch;
    unsigned long long* state;
    int64_t N;
    int M;                // shuffle: the next power of two >= N (LDS words); else 0
    int64_t seg_start;
    int ncat;
    uint32_t k0, k1;      // the seed's low and high word
    uint32_t flags;
    float* out;
    int64_t* seg_out;
    int64_t* label_out;
    float* onehot;
    int32_t* perm;
    float* params;
    float* noise;
};

struct Words {
    uint32_t w[4];
};

__device__ __forceinline__ Words philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        c0 = h1 ^ c1 ^ k0;
        c1 = l1;
        c2 = h0 ^ c3 ^ k1;
        c3 = l0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return {{c0, c1, c2, c3}};
}

__device__ __forceinline__ float unit(uint32_t w) { return (float)(w >> 8) * 0x1p-24f; }             // [0, 1), exact
__device__ __forceinline__ float radius(uint32_t w) {                                                 // Box-Muller's r
    return sqrtf(fmul(-2.0f, logf((float)((w >> 8) + 1u) * 0x1p-24f)));
}
__device__ __forceinline__ float jit(float z) { return fminf(fmaxf(fmul(0.01f, z), -0.02f), 0.02f); }

// the three augmentations of order o, two bits each, first applied lowest
__device__ __forceinline__ uint32_t sequence(uint32_t o) {
    constexpr uint32_t T = BA_T, J = BA_J, R = BA_R;
    constexpr uint32_t seq[6] = {T | J << 2 | R << 4, T | R << 2 | J << 4, J | T << 2 | R << 4,
                                 J | R << 2 | T << 4, R | T << 2 | J << 4, R | J << 2 | T << 4};
    uint32_t s = seq[0];
#pragma unroll
    for (uint32_t i = 1; i < 6; ++i) s = o == i ? seq[i] : s;
    return s;
}

__global__ __launch_bounds__(BA_THREADS) void batch_assemble_kernel(const BaArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long ba_words[];   // a.M words (shuffle only)
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int64_t N = a.N;
    const int C = a.C;
    const int64_t cursor = (int64_t)a.state[BA_CURSOR];
    const uint32_t epoch = (uint32_t)a.state[BA_EPOCH];
    const int64_t slot = cursor + b;
    const bool live = cursor >= 0 && slot < a.n_epoch;

    int64_t item = -1, lab = 0;
    bool ok = false;
    if (live) {
        item = a.order[slot];
        ok = item >= 0 && item < a.n_items;
        if (ok && a.label) {
            lab = a.label[item];
            if (a.ncat > 0 && (lab < 0 || lab >= a.ncat)) ok = false;
        }
    }

    if (live && !ok) {   // a bad item id or label: the cloud as zeros
        for (int64_t e = tid; e < C * N; e += BA_THREADS) a.out[b * C * N + e] = 0.f;
        for (int64_t n = tid; n < N; n += BA_THREADS) {
            if (a.seg_out) a.seg_out[b * N + n] = 0;
            if (a.perm) a.perm[b * N + n] = 0;
        }
        if (a.noise)
            for (int64_t e = tid; e < N * 3; e += BA_THREADS) a.noise[b * N * 3 + e] = 0.f;
        if (a.onehot)
            for (int j = tid; j < a.ncat; j += BA_THREADS) a.onehot[b * a.ncat + j] = 0.f;
        if (a.params && tid < 16) a.params[b * 16 + tid] = 0.f;
        if (a.label_out && tid == 0) a.label_out[b] = 0;
    }

    if (live && ok) {
        const uint32_t it = (uint32_t)item;
        // the cloud's parameters (stream 0): every lane draws the same
        uint32_t aug = (a.flags >> 1) & 3u, o = 0, sw = 0;
        float scale[3] = {1.f, 1.f, 1.f}, shift[3] = {0.f, 0.f, 0.f}, theta = 0.f, cs = 1.f, sn = 0.f;
        if (aug) {
            const Words p0 = philox(it, epoch, 0, 0, a.k0, a.k1);
            if (aug == 2) {
                o = p0.w[0] % 6u;
                sw = p0.w[1] & 7u;
            } else {
                sw = 1u << BA_T;
            }
            if (a.flags & DGX_BATCH_FORCE) {
                o = min((a.flags >> 4) & 7u, 5u);
                sw = (a.flags >> 7) & 7u;
            }
            const Words p1 = philox(it, epoch, 0, 1, a.k0, a.k1);
            const Words p2 = philox(it, epoch, 0, 2, a.k0, a.k1);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                scale[c] = fadd(2.0f / 3.0f, fmul(unit(p1.w[c]), 5.0f / 6.0f));
                shift[c] = fadd(-0.2f, fmul(unit(p2.w[c]), 0.4f));
            }
            const float z = fmul(radius(p0.w[2]), cospif(fmul(2.0f, unit(p0.w[3]))));
            theta = fmul(6.28318530717958647692f, z);
            cs = cosf(theta);
            sn = sinf(theta);
        }
        const uint32_t seq = sequence(o);
        const bool jitter = (sw >> BA_J) & 1u;
        const bool draw = a.noise != nullptr || jitter;

        if (a.M) {   // the shuffle: sort (key << 32) | j
            for (int q = tid; q < (a.M + 3) / 4; q += BA_THREADS) {
                const Words k = philox(it, epoch, 1, (uint32_t)q, a.k0, a.k1);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int j = 4 * q + r;
                    if (j < a.M) ba_words[j] = j < N ? ((unsigned long long)k.w[r] << 32) | (uint32_t)j : ~0ull;
                }
            }
            __syncthreads();
            for (int k = 2; k <= a.M; k <<= 1) {
                for (int j = k >> 1; j > 0; j >>= 1) {
                    for (int i = tid; i < a.M; i += BA_THREADS) {
                        const int x = i ^ j;
                        if (x > i) {
                            const unsigned long long u = ba_words[i], v = ba_words[x];
                            if ((u > v) == ((i & k) == 0)) {
                                ba_words[i] = v;
                                ba_words[x] = u;
                            }
                        }
                    }
                    __syncthreads();
                }
            }
        }

        const float* cloud = a.points + item * a.P * C;
        const int32_t* cseg = a.seg ? a.seg + item * a.P : nullptr;
        for (int64_t n = tid; n < N; n += BA_THREADS) {
            // src < N by construction: the low word of a sorted (key, j) word with j < N (the N smallest)
            const int64_t src = a.M ? (int64_t)(uint32_t)ba_words[n] : n;
            if (a.perm) a.perm[b * N + n] = (int32_t)src;
            if (a.seg_out) a.seg_out[b * N + n] = (int64_t)cseg[src] - a.seg_start;
            const float* p = cloud + src * C;
            if (!aug) {
                for (int c = 0; c < C; ++c) a.out[(b * C + c) * N + n] = p[c];
                continue;
            }
            float v[3] = {p[0], p[1], p[2]};   // C == 3
            float nz[3] = {0.f, 0.f, 0.f};
            if (draw) {
                const Words g = philox(it, epoch, 2, (uint32_t)n, a.k0, a.k1);
                float s0, c0, s1, c1;
                sincospif(fmul(2.0f, unit(g.w[1])), &s0, &c0);
                sincospif(fmul(2.0f, unit(g.w[3])), &s1, &c1);
                const float r0 = radius(g.w[0]), r1 = radius(g.w[2]);
                nz[0] = jit(fmul(r0, c0));
                nz[1] = jit(fmul(r0, s0));
                nz[2] = jit(fmul(r1, c1));
                if (a.noise)
                    for (int c = 0; c < 3; ++c) a.noise[(b * N + n) * 3 + c] = nz[c];
            }
#pragma unroll
            for (int step = 0; step < 3; ++step) {
                const uint32_t op = (seq >> (2 * step)) & 3u;
                if (!((sw >> op) & 1u)) continue;
                if (op == BA_T) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) v[c] = fadd(fmul(v[c], scale[c]), shift[c]);
                } else if (op == BA_J) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) v[c] = fadd(v[c], nz[c]);
                } else {
                    const float x = v[0], z = v[2];
                    v[0] = fadd(fmul(x, cs), fmul(z, sn));
                    v[2] = fadd(-fmul(x, sn), fmul(z, cs));
                }
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) a.out[(b * 3 + c) * N + n] = v[c];
        }
        if (a.onehot)
            for (int j = tid; j < a.ncat; j += BA_THREADS) a.onehot[b * a.ncat + j] = j == lab ? 1.f : 0.f;
        if (tid == 0) {
            if (a.label_out) a.label_out[b] = lab;
            if (a.params) {
                float* q = a.params + b * 16;
                q[0] = (float)o;
                for (int c = 0; c < 3; ++c) {
                    q[1 + c] = (float)((sw >> c) & 1u);
                    q[4 + c] = scale[c];
                    q[7 + c] = shift[c];
                }
                q[10] = theta;
                q[11] = cs;
                q[12] = sn;
                q[13] = __uint_as_float(it);
                q[14] = __uint_as_float(epoch);
                q[15] = 0.f;
            }
        }
    }

    __syncthreads();   // every lane has read the cursor
    if (tid == 0) {
        if (live && !ok) atomicAdd(&a.state[BA_INVALID], 1ull);
        if (!live) atomicAdd(&a.state[BA_OVERRUN], 1ull);
        // every workgroup has read the cursor before it takes its ticket: the last ticket may move it
        __threadfence();
        if (atomicAdd(&a.state[BA_TICKET], 1ull) == (unsigned long long)gridDim.x - 1) {
            a.state[BA_TICKET] = 0;
            if (cursor >= 0 && cursor < a.n_epoch)
                a.state[BA_CURSOR] = (unsigned long long)min(cursor + (int64_t)gridDim.x, a.n_epoch);
            a.state[BA_BATCHES] += 1ull;
        }
    }
}

}  // namespace

extern "C" {

int dgx_batch_max_points(void) { return BA_MAX_POINTS; }

int dgx_batch_assemble(const float* points, const int32_t* seg, const int32_t* label, int64_t n_items, int64_t P,
                       int C, const int32_t* order, int64_t n_epoch, int64_t* state, int B, int64_t N,
                       int64_t seg_start, int ncat, uint64_t seed, uint32_t flags, float* out, int64_t* seg_out,
                       int64_t* label_out, float* onehot, int32_t* perm, float* params, float* noise, void* stream) {
    if (!points || !order || !state || !out) return DGX_EINVAL;
    if (n_items < 1 || n_items > INT32_MAX || P < 1 || C < 1 || n_epoch < 0 || B < 1 || N < 1 || N > P)
        return DGX_EINVAL;
    if ((seg != nullptr) != (seg_out != nullptr)) return DGX_EINVAL;
    if (label_out && !label) return DGX_EINVAL;
    if (ncat < 0 || (ncat > 0) != (onehot != nullptr) || (ncat > 0 && !label)) return DGX_EINVAL;
    const uint32_t aug = (flags >> 1) & 3u;
    if (aug > 2 || (flags >> 10)) return DGX_EINVAL;
    if ((flags & DGX_BATCH_FORCE) && (aug != 2 || ((flags >> 4) & 7u) > 5)) return DGX_EINVAL;
    if (!(flags & DGX_BATCH_FORCE) && (flags >> 4)) return DGX_EINVAL;
    if (aug && C != 3) return DGX_EINVAL;
    if (!aug && noise) return DGX_EINVAL;
    const bool shuffle = flags & DGX_BATCH_SHUFFLE;
    if (shuffle && N > BA_MAX_POINTS) return DGX_EUNSUPPORTED;
    if (N > INT32_MAX || (int64_t)C * N > ((int64_t)1 << 40) / B) return DGX_EUNSUPPORTED;
    if (reinterpret_cast<uintptr_t>(points) % 4 || reinterpret_cast<uintptr_t>(seg) % 4 ||
        reinterpret_cast<uintptr_t>(label) % 4 || reinterpret_cast<uintptr_t>(order) % 4 ||
        reinterpret_cast<uintptr_t>(state) % 8 || reinterpret_cast<uintptr_t>(out) % 4 ||
        reinterpret_cast<uintptr_t>(seg_out) % 8 || reinterpret_cast<uintptr_t>(label_out) % 8 ||
        reinterpret_cast<uintptr_t>(onehot) % 4 || reinterpret_cast<uintptr_t>(perm) % 4 ||
        reinterpret_cast<uintptr_t>(params) % 4 || reinterpret_cast<uintptr_t>(noise) % 4)
        return DGX_EINVAL;

    BaArgs a;
    a.points = points;
    a.seg = seg;
    a.label = label;
    a.n_items = n_items;
    a.P = P;
    a.C = C;
    a.order = order;
    a.n_epoch = n_epoch;
    a.state = reinterpret_cast<unsigned long long*>(state);
    a.N = N;
    a.M = 0;
    if (shuffle) {
        a.M = 1;
        while (a.M < N) a.M <<= 1;
    }
    a.seg_start = seg_start;
    a.ncat = ncat;
    a.k0 = (uint32_t)seed;
    a.k1 = (uint32_t)(seed >> 32);
    a.flags = flags;
    a.out = out;
    a.seg_out = seg_out;
    a.label_out = label_out;
    a.onehot = onehot;
    a.perm = perm;
    a.params = params;
    a.noise = noise;
    hipLaunchKernelGGL(batch_assemble_kernel, dim3((unsigned)B), dim3(BA_THREADS), (size_t)a.M * 8, dgx_stream(stream),
                       a);
    return hipGetLastError() == hipSuccess ? DGX_OK : DGX_ELAUNCH;
}

}  // extern "C"
