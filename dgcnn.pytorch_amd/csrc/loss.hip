// Label-smoothed cross entropy (reference loss.py:4-21) as a loss head:
// forward = one row kernel + a one-workgroup sum of its partials, backward =
// one kernel. torch runs the same expression as a dozen launches and about ten
// passes over the logits, with fp32 temporaries of fp16 logits.
//
// Per row i, logits x[0..C), label y, weights w_j = w_true (j == y) or w_other:
//   mx = max_j x_j,  S = sum_j exp(x_j - mx),  lse = mx + log S
//   L  = W log S + sum_j w_j (mx - x_j)          W = w_true + (C - 1) w_other
//   loss = (1/M) sum_i L_i
//   dx_j = (g / M) (W exp(x_j - lse) - w_j)      g read from device memory
// L is written as a sum of non-negative terms, so logits near 1e4 lose nothing.
//
// Precision: the sums, the exponentials of the forward and lse (kept as fp64)
// are fp64. fp32 is not enough for the gradient: where exp(x_j - lse) is near
// w_j / W the difference cancels, and an fp32 lse (half an ulp of it is a
// relative error of the exponential) or an fp32 exponential (1 ulp) then lands
// several fp16 / bf16 units from the exact value (3 elements of 205 k at
// (4099, 50) bf16 with fp32 throughout). To keep the fp64 work small the
// forward's exp(-d) is a short one of its own (ce_exp_neg, relative error
// 3e-13) and the backward takes fp32 for the exponential and
// the difference unless the difference cancels (ce_grad), which a few elements
// in a thousand do. Each result is rounded once, to fp32 and from there to the
// logits' dtype.
//
// Layouts (no copy for either): class-contiguous (M, C) rows and
// point-contiguous (B, C, N) planes. Both forward kernels give one workgroup
// the same CE_ROWS consecutive rows, one lane per row with the same row code,
// and sum the rows' losses in the same tree, so they agree bit for bit.
//   rows:   a workgroup's rows are one contiguous byte range; it is loaded
//           flat, 16 bytes per lane, into LDS (rows of 50 halves are not 16-byte
//           aligned one by one), and each lane walks its row there. A row too
//           wide for that (fewer than CE_MIN_TILE_ROWS in 32 KB) is read by its
//           lane from global memory.
//   planes: lane n reads x[b, j, n] for j = 0..C-1, coalesced across lanes.
// Determinism: per-workgroup partials in the workspace, summed in a fixed
// order by ce_sum_kernel. No atomics, no counters, nothing to reset: a
// replayed graph recomputes every word it reads.
//
// A label is only compared with the class index, never used as an address: an
// out-of-range label matches no class and makes that row's loss and gradient
// NaN (a GradScaler then skips the step).
#include <algorithm>

#include "ce_row.h"

namespace {

constexpr int CE_ROWS = 128;            // rows per workgroup = threads per workgroup
constexpr int CE_TILE_BYTES = 32768;    // LDS staging of the rows kernel
constexpr int CE_MIN_TILE_ROWS = 32;    // narrower tiles leave most lanes idle: read global memory instead

// exp(-d) for d >= 0 in fp64, relative error about 1e-13 (the gradient needs lse to about 1e-10):
// -d = n ln 2 + r with |r| <= ln 2 / 2, a degree-10 Taylor polynomial in r, scaled by 2^n.
// NaN stays NaN; d = inf gives 0.
__device__ __forceinline__ double ce_exp_neg(double d) {
    const double t = -d;
    const double n = rint(t * 1.4426950408889634);
    double r = fma(n, -6.93147180369123816490e-01, t);   // ln 2, high and low part
    r = fma(n, -1.90821492927058770002e-10, r);
    double p = 1.0 / 3628800.0;
    p = fma(p, r, 1.0 / 362880.0);
    p = fma(p, r, 1.0 / 40320.0);
    p = fma(p, r, 1.0 / 5040.0);
    p = fma(p, r, 1.0 / 720.0);
    p = fma(p, r, 1.0 / 120.0);
    p = fma(p, r, 1.0 / 24.0);
    p = fma(p, r, 1.0 / 6.0);
    p = fma(p, r, 0.5);
    p = fma(p, r, 1.0);
    p = fma(p, r, 1.0);
    return d > 745.0 ? 0.0 : ldexp(p, (int)n);
}

struct CeRow {
    double lse, loss;
    int arg;
};

// One row; ld(j) is logit j as fp32. The first maximum wins the arg-max.
template <class Ld>
__device__ __forceinline__ CeRow ce_row(Ld ld, int C, int64_t y, float w_true, float w_other, double W) {
    // both passes fetch CE_BATCH logits before they use them (see ce_row_max)
    float mx;
    int arg;
    ce_row_max(ld, C, mx, arg);
    double S = 0.0, T = 0.0;
    bool found = false;
    for (int j0 = 0; j0 < C; j0 += CE_BATCH) {
        float v[CE_BATCH];
#pragma unroll
        for (int u = 0; u < CE_BATCH; ++u) v[u] = ld(min(j0 + u, C - 1));
#pragma unroll
        for (int u = 0; u < CE_BATCH; ++u) {
            const int j = j0 + u;
            if (j < C) {
                const double d = (double)mx - (double)v[u];   // >= 0
                S += ce_exp_neg(d);
                const bool hit = (int64_t)j == y;
                found = found || hit;
                const float w = hit ? w_true : w_other;
                if (w != 0.f) T += (double)w * d;   // weight 0 (no smoothing) ignores a -inf logit
            }
        }
    }
    const double lS = log(S);
    CeRow r;
    r.lse = (double)mx + lS;
    r.loss = found ? W * lS + T : __longlong_as_double(0x7ff8000000000000LL);
    r.arg = arg;
    return r;
}

// red[0] = sum of red[0..CE_ROWS) in a fixed tree (CE_ROWS threads).
__device__ __forceinline__ void ce_block_sum(double* red) {
    __syncthreads();
    for (int s = CE_ROWS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
}

template <int DT>
__global__ __launch_bounds__(CE_ROWS) void ce_fwd_rows_kernel(const typename Elt<DT>::T* __restrict__ x, int64_t M,
                                                              int C, int tile_rows, const void* __restrict__ labels,
                                                              int l64, float w_true, float w_other, double W,
                                                              double* __restrict__ lse, int64_t* __restrict__ pred,
                                                              double* __restrict__ partial) {
    using T = typename Elt<DT>::T;
    __shared__ __attribute__((aligned(16))) unsigned char tile[CE_TILE_BYTES + 16];
    __shared__ double red[CE_ROWS];
    const int tid = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * CE_ROWS;
    const int nrows = (int)min((int64_t)CE_ROWS, M - r0);
    red[tid] = 0.0;
    if (tile_rows == 0) {
        if (tid < nrows) {
            const int64_t row = r0 + tid;
            const T* p = x + row * C;
            const CeRow r = ce_row([p](int j) { return Elt<DT>::ld(p + j); }, C, ce_label(labels, l64, row), w_true,
                                   w_other, W);
            lse[row] = r.lse;
            if (pred) pred[row] = r.arg;
            red[tid] = r.loss;
        }
    } else {
        for (int t0 = 0; t0 < nrows; t0 += tile_rows) {
            const int tr = min(tile_rows, nrows - t0);
            // rows [r0 + t0, r0 + t0 + tr) are the bytes [beg, end); stage the 16-byte granules that cover them
            const uintptr_t beg = reinterpret_cast<uintptr_t>(x + (r0 + t0) * C);
            const uintptr_t a0 = beg & ~(uintptr_t)15;
            ce_stage_rows<T, CE_ROWS>(tile, beg, (size_t)tr * C * sizeof(T), tid);
            __syncthreads();
            if (tid < tr) {
                const int64_t row = r0 + t0 + tid;
                const T* p = reinterpret_cast<const T*>(tile + (beg - a0)) + (size_t)tid * C;
                const CeRow r = ce_row([p](int j) { return Elt<DT>::ld(p + j); }, C, ce_label(labels, l64, row),
                                       w_true, w_other, W);
                lse[row] = r.lse;
                if (pred) pred[row] = r.arg;
                red[t0 + tid] = r.loss;
            }
            __syncthreads();
        }
    }
    ce_block_sum(red);
    if (tid == 0) partial[blockIdx.x] = red[0];
}

template <int DT>
__global__ __launch_bounds__(CE_ROWS) void ce_fwd_planes_kernel(const typename Elt<DT>::T* __restrict__ x, int64_t M,
                                                                int C, int64_t N, const void* __restrict__ labels,
                                                                int l64, float w_true, float w_other, double W,
                                                                double* __restrict__ lse, int64_t* __restrict__ pred,
                                                                double* __restrict__ partial) {
    using T = typename Elt<DT>::T;
    __shared__ double red[CE_ROWS];
    const int tid = threadIdx.x;
    const int64_t row = (int64_t)blockIdx.x * CE_ROWS + tid;
    red[tid] = 0.0;
    if (row < M) {
        const int64_t b = row / N, n = row - b * N;
        const T* p = x + b * C * N + n;
        const CeRow r = ce_row([p, N](int j) { return Elt<DT>::ld(p + (int64_t)j * N); }, C,
                               ce_label(labels, l64, row), w_true, w_other, W);
        lse[row] = r.lse;
        if (pred) pred[row] = r.arg;
        red[tid] = r.loss;
    }
    ce_block_sum(red);
    if (tid == 0) partial[blockIdx.x] = red[0];
}

// loss = (sum of the partials) / M: thread t adds partials t, t + 256, ... in order, then a fixed tree.
__global__ __launch_bounds__(256) void ce_sum_kernel(const double* __restrict__ partial, int64_t parts, int64_t M,
                                                     float* __restrict__ loss) {
    __shared__ double red[256];
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < parts; i += 256) s += partial[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
        __syncthreads();
    }
    if (threadIdx.x == 0) *loss = (float)(red[0] / (double)M);
}

struct CeScale {   // W and g / M, in fp64 and rounded to fp32
    double W, gs;
    float Wf, gsf;
};

// One gradient element. fp32 for the exponential and the difference costs about 5e-7 of W p (the
// rounding of x - lse near -5.5 where p is near w / W, expf's ulp, W's rounding); that is inside one
// unit of a 16-bit result (2^-11 of it at least) while |W p - w| >= 2^-8 w, four times the need.
// Below that the difference is taken in fp64.
__device__ __forceinline__ float ce_grad(float xv, double l, bool hit, bool valid, float w_true, float w_other,
                                         const CeScale& K) {
    if (!valid) return __uint_as_float(0x7fc00000u);
    const float w = hit ? w_true : w_other;
    const double a = (double)xv - l;
    const float r = fmaf(K.Wf, expf((float)a), -w);
    if (fabsf(r) >= 0x1p-8f * w) return K.gsf * r;
    return (float)(K.gs * (K.W * exp(a) - (double)w));   // also where r is NaN
}

__device__ __forceinline__ CeScale ce_scale(double W, const float* g, double inv_m) {
    CeScale K;
    K.W = W;
    K.gs = (double)*g * inv_m;
    K.Wf = (float)W;
    K.gsf = (float)K.gs;
    return K;
}

// Class-contiguous backward: elementwise over the flat M * C range, 16 bytes per lane.
template <int DT>
__global__ __launch_bounds__(256) void ce_bwd_rows_kernel(const typename Elt<DT>::T* __restrict__ x,
                                                          typename Elt<DT>::T* __restrict__ dx, int64_t total, int C,
                                                          const void* __restrict__ labels, int l64, float w_true,
                                                          float w_other, double W, const double* __restrict__ lse,
                                                          const float* __restrict__ g, double inv_m, int vec) {
    using T = typename Elt<DT>::T;
    constexpr int V = 16 / (int)sizeof(T);
    const int64_t e0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * V;
    if (e0 >= total) return;
    const CeScale K = ce_scale(W, g, inv_m);
    const int n = (int)min((int64_t)V, total - e0);
    __attribute__((aligned(16))) T in[V], out[V];
    const bool wide = vec && n == V;
    if (wide) {
        *reinterpret_cast<uint4*>(in) = *reinterpret_cast<const uint4*>(x + e0);
    } else {
        for (int i = 0; i < n; ++i) in[i] = x[e0 + i];
    }
    int64_t row = e0 / C;
    int j = (int)(e0 - row * C);
    double l = lse[row];
    int64_t y = ce_label(labels, l64, row);
#pragma unroll
    for (int i = 0; i < V; ++i) {
        if (i < n) {
            out[i] = Elt<DT>::cv(ce_grad(Elt<DT>::ld(&in[i]), l, (int64_t)j == y, y >= 0 && y < C, w_true, w_other, K));
            if (++j == C && i + 1 < n) {
                j = 0;
                ++row;
                l = lse[row];
                y = ce_label(labels, l64, row);
            }
        }
    }
    if (wide) {
        *reinterpret_cast<uint4*>(dx + e0) = *reinterpret_cast<const uint4*>(out);
    } else {
        for (int i = 0; i < n; ++i) dx[e0 + i] = out[i];
    }
}

template <int DT>
__global__ __launch_bounds__(CE_ROWS) void ce_bwd_planes_kernel(const typename Elt<DT>::T* __restrict__ x,
                                                                typename Elt<DT>::T* __restrict__ dx, int64_t M, int C,
                                                                int64_t N, const void* __restrict__ labels, int l64,
                                                                float w_true, float w_other, double W,
                                                                const double* __restrict__ lse,
                                                                const float* __restrict__ g, double inv_m) {
    const int64_t row = (int64_t)blockIdx.x * CE_ROWS + threadIdx.x;
    if (row >= M) return;
    const CeScale K = ce_scale(W, g, inv_m);
    const int64_t b = row / N, n = row - b * N, off = b * C * N + n;
    const double l = lse[row];
    const int64_t y = ce_label(labels, l64, row);
    const bool valid = y >= 0 && y < C;
    for (int j0 = 0; j0 < C; j0 += CE_BATCH) {   // loads ahead of their use, as in ce_row
        float v[CE_BATCH];
#pragma unroll
        for (int u = 0; u < CE_BATCH; ++u) v[u] = Elt<DT>::ld(x + off + (int64_t)min(j0 + u, C - 1) * N);
#pragma unroll
        for (int u = 0; u < CE_BATCH; ++u) {
            const int j = j0 + u;
            if (j < C)
                dx[off + (int64_t)j * N] = Elt<DT>::cv(ce_grad(v[u], l, (int64_t)j == y, valid, w_true, w_other, K));
        }
    }
}

enum { CE_ROWS_LAYOUT = 1, CE_PLANES_LAYOUT = 2 };

// Shape / stride checks shared by the two entry points; the layout, or a DGX_E* code.
int ce_layout(int dtype, int64_t B, int64_t C, int64_t N, int64_t sb, int64_t sc, int64_t sn) {
    if (dtype != DGX_CE_F32 && dtype != DGX_CE_F16 && dtype != DGX_CE_BF16) return DGX_EINVAL;
    if (B < 1 || N < 1 || C < 2) return DGX_EINVAL;
    if (C > INT32_MAX || B > INT64_MAX / N || B * N > (int64_t)CE_ROWS * INT32_MAX || B * N > INT64_MAX / C)
        return DGX_EUNSUPPORTED;
    if (sc == 1 && (N == 1 || sn == C) && (B == 1 || sb == N * C)) return CE_ROWS_LAYOUT;
    if ((N == 1 || sn == 1) && sc == N && (B == 1 || sb == C * N)) return CE_PLANES_LAYOUT;
    return DGX_EUNSUPPORTED;
}

double ce_total_weight(float w_true, float w_other, int64_t C) {
    return (double)w_true + (double)(C - 1) * (double)w_other;
}

}  // namespace

extern "C" {

size_t dgx_smoothed_ce_workspace_bytes(int64_t M) {
    return M < 1 ? 0 : (size_t)((M + CE_ROWS - 1) / CE_ROWS) * sizeof(double);
}

#define CE_DISPATCH(dtype, CALL)                              \
    switch (dtype) {                                          \
        case DGX_CE_F32: { CALL(DGX_CE_F32); break; }         \
        case DGX_CE_F16: { CALL(DGX_CE_F16); break; }         \
        default: { CALL(DGX_CE_BF16); break; }                \
    }

int dgx_smoothed_ce_fwd(const void* logits, int dtype, int64_t B, int64_t C, int64_t N, int64_t sb, int64_t sc,
                        int64_t sn, const void* labels, int label_is_i64, float w_true, float w_other, double* lse,
                        float* loss, int64_t* pred, void* ws, size_t ws_bytes, void* stream) {
    if (!logits || !labels || !lse || !loss || !ws) return DGX_EINVAL;
    const int layout = ce_layout(dtype, B, C, N, sb, sc, sn);
    if (layout < 0) return layout;
    const int64_t M = B * N;
    const size_t es = dtype == DGX_CE_F32 ? 4 : 2;
    if (reinterpret_cast<uintptr_t>(logits) % es || reinterpret_cast<uintptr_t>(lse) % 8 ||
        reinterpret_cast<uintptr_t>(ws) % 8 || ws_bytes < dgx_smoothed_ce_workspace_bytes(M))
        return DGX_EINVAL;
    const int64_t parts = (M + CE_ROWS - 1) / CE_ROWS;
    const double W = ce_total_weight(w_true, w_other, C);
    double* partial = static_cast<double*>(ws);
    hipStream_t st = dgx_stream(stream);
    if (layout == CE_ROWS_LAYOUT) {
        int tile_rows = (int)std::min<int64_t>(CE_ROWS, CE_TILE_BYTES / (C * (int64_t)es));
        if (tile_rows < CE_MIN_TILE_ROWS) tile_rows = 0;
#define CE_CALL(DT)                                                                                               \
    hipLaunchKernelGGL(ce_fwd_rows_kernel<DT>, dim3((unsigned)parts), dim3(CE_ROWS), 0, st,                       \
                       static_cast<const Elt<DT>::T*>(logits), M, (int)C, tile_rows, labels, label_is_i64, w_true, \
                       w_other, W, lse, pred, partial)
        CE_DISPATCH(dtype, CE_CALL)
#undef CE_CALL
    } else {
#define CE_CALL(DT)                                                                                          \
    hipLaunchKernelGGL(ce_fwd_planes_kernel<DT>, dim3((unsigned)parts), dim3(CE_ROWS), 0, st,                \
                       static_cast<const Elt<DT>::T*>(logits), M, (int)C, N, labels, label_is_i64, w_true,   \
                       w_other, W, lse, pred, partial)
        CE_DISPATCH(dtype, CE_CALL)
#undef CE_CALL
    }
    DGX_CHECK_LAUNCH();
    hipLaunchKernelGGL(ce_sum_kernel, dim3(1), dim3(256), 0, st, partial, parts, M, loss);
    return hipGetLastError() == hipSuccess ? DGX_OK : DGX_ELAUNCH;
}

int dgx_smoothed_ce_bwd(const void* logits, int dtype, int64_t B, int64_t C, int64_t N, int64_t sb, int64_t sc,
                        int64_t sn, const void* labels, int label_is_i64, float w_true, float w_other,
                        const double* lse, const float* g, void* dlogits, void* stream) {
    if (!logits || !labels || !lse || !g || !dlogits) return DGX_EINVAL;
    const int layout = ce_layout(dtype, B, C, N, sb, sc, sn);
    if (layout < 0) return layout;
    const int64_t M = B * N;
    const size_t es = dtype == DGX_CE_F32 ? 4 : 2;
    if (reinterpret_cast<uintptr_t>(logits) % es || reinterpret_cast<uintptr_t>(dlogits) % es ||
        reinterpret_cast<uintptr_t>(lse) % 8 || reinterpret_cast<uintptr_t>(g) % 4)
        return DGX_EINVAL;
    const double W = ce_total_weight(w_true, w_other, C);
    const double inv_m = 1.0 / (double)M;
    hipStream_t st = dgx_stream(stream);
    if (layout == CE_ROWS_LAYOUT) {
        const int64_t total = M * C, per = 256 * (16 / (int64_t)es);
        const int64_t grid = (total + per - 1) / per;
        if (grid > INT32_MAX) return DGX_EUNSUPPORTED;
        const int vec = ((reinterpret_cast<uintptr_t>(logits) | reinterpret_cast<uintptr_t>(dlogits)) & 15) == 0;
#define CE_CALL(DT)                                                                                             \
    hipLaunchKernelGGL(ce_bwd_rows_kernel<DT>, dim3((unsigned)grid), dim3(256), 0, st,                          \
                       static_cast<const Elt<DT>::T*>(logits), static_cast<Elt<DT>::T*>(dlogits), total, (int)C, \
                       labels, label_is_i64, w_true, w_other, W, lse, g, inv_m, vec)
        CE_DISPATCH(dtype, CE_CALL)
#undef CE_CALL
    } else {
        const int64_t grid = (M + CE_ROWS - 1) / CE_ROWS;
#define CE_CALL(DT)                                                                                            \
    hipLaunchKernelGGL(ce_bwd_planes_kernel<DT>, dim3((unsigned)grid), dim3(CE_ROWS), 0, st,                   \
                       static_cast<const Elt<DT>::T*>(logits), static_cast<Elt<DT>::T*>(dlogits), M, (int)C, N, \
                       labels, label_is_i64, w_true, w_other, W, lse, g, inv_m)
        CE_DISPATCH(dtype, CE_CALL)
#undef CE_CALL
    }
    return hipGetLastError() == hipSuccess ? DGX_OK : DGX_ELAUNCH;
}

}  // extern "C"
