// Multi-tensor SGD: torch.optim.SGD's update (momentum, dampening, weight
// decay, Nesterov, maximize) over a list of fp32 parameters in ONE launch.
//
// torch's fused SGD (multi_tensor_apply, 65536-element chunks, one workgroup
// per chunk) runs a DGCNN's ~0.6 M parameters on ~22 workgroups: 28 us per
// train step at cfg2, latency-bound. Here each tensor is cut into 1024-element
// pieces, one workgroup per piece (the piece's tensor is found by a
// workgroup-uniform search of the piece offsets), four consecutive elements
// per thread with 16-byte accesses where aligned. Per element, in torch's
// order (torch/optim/sgd.py):
//   g = maximize ? -grad : grad;  g = g + wd * p
//   buf = first ? g : momentum * buf + (1 - dampening) * g
//   g = nesterov ? g + momentum * buf : buf;   p = p - lr * g
//
// Adam / AdamW (adam_kernel) and the GradScaler pieces (sgd_amp_kernel,
// unscale_kernel) use the same job table. Adam touches four or five arrays per
// parameter where SGD touches three, and torch's default (foreach) form is a
// dozen multi-tensor launches. The scaler's state reaches the update kernels as
// two device pointers: grad_scale (g is divided by it on load, .grad stays
// scaled) and found_inf (non-zero: the launch writes nothing), so a
// GradScaler.step needs no host read of the inf flag.
#include "common.h"

namespace {

constexpr int SGD_MAX = 48;   // tensors per launch (kernel argument block)

struct SgdJobs {
    float* p[SGD_MAX];
    const float* g[SGD_MAX];
    float* m[SGD_MAX];
    int64_t numel[SGD_MAX];
    int blk[SGD_MAX + 1];   // first workgroup of each tensor, blk[n] = grid
    int n;
};

constexpr int SGD_PIECE = 1024;   // elements per workgroup (256 threads x 4)

__device__ __forceinline__ float sgd_elem(float pv, float g, float* m, int64_t i, float lr, float wd, float mom,
                                          float damp, int nesterov, int maximize, int first) {
    if (maximize) g = -g;
    if (wd != 0.f) g = g + wd * pv;
    if (mom != 0.f) {
        const float b = first ? g : mom * m[i] + (1.f - damp) * g;
        m[i] = b;
        g = nesterov ? g + mom * b : b;
    }
    return pv - lr * g;
}

__global__ __launch_bounds__(256) void sgd_kernel(SgdJobs J, float lr, float wd, float mom, float damp, int nesterov,
                                                  int maximize, int first) {
    int lo = 0, hi = J.n - 1;   // the tensor t with blk[t] <= blockIdx.x < blk[t + 1] (workgroup-uniform)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (J.blk[mid] <= (int)blockIdx.x) lo = mid;
        else hi = mid - 1;
    }
    float* __restrict__ p = J.p[lo];
    const float* __restrict__ gr = J.g[lo];
    float* __restrict__ m = J.m[lo];
    const int64_t n = J.numel[lo];
    const int64_t i0 = (int64_t)(blockIdx.x - J.blk[lo]) * SGD_PIECE + 4 * threadIdx.x;
    const bool vec = i0 + 3 < n && ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(gr) |
                                     reinterpret_cast<uintptr_t>(m)) & 15) == 0;
    if (vec) {
        const float4 pv = *reinterpret_cast<const float4*>(p + i0);
        const float4 gv = *reinterpret_cast<const float4*>(gr + i0);
        float4 o;
        o.x = sgd_elem(pv.x, gv.x, m, i0, lr, wd, mom, damp, nesterov, maximize, first);
        o.y = sgd_elem(pv.y, gv.y, m, i0 + 1, lr, wd, mom, damp, nesterov, maximize, first);
        o.z = sgd_elem(pv.z, gv.z, m, i0 + 2, lr, wd, mom, damp, nesterov, maximize, first);
        o.w = sgd_elem(pv.w, gv.w, m, i0 + 3, lr, wd, mom, damp, nesterov, maximize, first);
        *reinterpret_cast<float4*>(p + i0) = o;
    } else {
        for (int64_t i = i0; i < min(n, i0 + 4); ++i)
            p[i] = sgd_elem(p[i], gr[i], m, i, lr, wd, mom, damp, nesterov, maximize, first);
    }
}

// The tensor t with blk[t] <= blockIdx.x < blk[t + 1] (workgroup-uniform).
__device__ __forceinline__ int job_of(const int* blk, int n) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (blk[mid] <= (int)blockIdx.x) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// Piece offsets of a job table; DGX_OK, or the error the entry point returns.
template <class Jobs>
int fill_pieces(Jobs& J, int n, const int64_t* numels) {
    J.n = n;
    J.blk[0] = 0;
    for (int t = 0; t < n; ++t) {
        if (numels[t] < 0) return DGX_EINVAL;
        J.numel[t] = numels[t];
        const int64_t pieces = (numels[t] + SGD_PIECE - 1) / SGD_PIECE;
        if ((int64_t)J.blk[t] + pieces > (1LL << 30)) return DGX_EUNSUPPORTED;
        J.blk[t + 1] = J.blk[t] + (int)pieces;
    }
    return DGX_OK;
}

// dgx_sgd_step_f32's update under a GradScaler: g / *grad_scale on load, and
// nothing written when *found_inf != 0 (torch's FusedSgdKernel.cu rule).
__global__ __launch_bounds__(256) void sgd_amp_kernel(SgdJobs J, float lr, float wd, float mom, float damp,
                                                      int nesterov, int maximize, int first,
                                                      const float* __restrict__ grad_scale,
                                                      const float* __restrict__ found_inf) {
    if (found_inf && *found_inf != 0.f) return;
    const int t = job_of(J.blk, J.n);
    float* __restrict__ p = J.p[t];
    const float* __restrict__ gr = J.g[t];
    float* __restrict__ m = J.m[t];
    const int64_t n = J.numel[t];
    const float gs = grad_scale ? *grad_scale : 1.f;
    const int64_t i0 = (int64_t)(blockIdx.x - J.blk[t]) * SGD_PIECE + 4 * threadIdx.x;
    const bool vec = i0 + 3 < n && ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(gr) |
                                     reinterpret_cast<uintptr_t>(m)) & 15) == 0;
    if (vec) {
        const float4 pv = *reinterpret_cast<const float4*>(p + i0);
        float4 gv = *reinterpret_cast<const float4*>(gr + i0);
        if (grad_scale) gv = make_float4(gv.x / gs, gv.y / gs, gv.z / gs, gv.w / gs);
        float4 o;
        o.x = sgd_elem(pv.x, gv.x, m, i0, lr, wd, mom, damp, nesterov, maximize, first);
        o.y = sgd_elem(pv.y, gv.y, m, i0 + 1, lr, wd, mom, damp, nesterov, maximize, first);
        o.z = sgd_elem(pv.z, gv.z, m, i0 + 2, lr, wd, mom, damp, nesterov, maximize, first);
        o.w = sgd_elem(pv.w, gv.w, m, i0 + 3, lr, wd, mom, damp, nesterov, maximize, first);
        *reinterpret_cast<float4*>(p + i0) = o;
    } else {
        for (int64_t i = i0; i < min(n, i0 + 4); ++i)
            p[i] = sgd_elem(p[i], grad_scale ? gr[i] / gs : gr[i], m, i, lr, wd, mom, damp, nesterov, maximize,
                            first);
    }
}

// ---- Adam / AdamW: torch/optim/adam.py::_single_tensor_adam (non-capturable
// branch), op by op in fp32. Scalars are rounded to fp32 where torch's Python
// scalars enter an fp32 tensor op.
struct AdamJobs {
    float* p[SGD_MAX];
    const float* g[SGD_MAX];
    float* m[SGD_MAX];
    float* v[SGD_MAX];
    float* vmax[SGD_MAX];   // amsgrad only
    float* step[SGD_MAX];   // 0-dim fp32 per tensor: steps taken so far
    int64_t numel[SGD_MAX];
    int blk[SGD_MAX + 1];
    int n;
};

struct AdamHyper {
    float lr;
    const float* lr_dev;   // read instead of lr when set
    double beta1, beta2;
    float eps, wd;
    int decoupled, amsgrad, maximize;
    const float* grad_scale;
    const float* found_inf;
};

struct AdamScalars {   // per tensor (they depend on its step count)
    float decay;       // 1 - lr * wd (decoupled weight decay)
    float wd;
    float w1, b2, w2;  // 1 - beta1, beta2, 1 - beta2
    float bc2_sqrt, eps, neg_step_size;
    float gs;
    int decoupled, maximize, unscale;
};

__device__ __forceinline__ void adam_elem(float& p, float g, float& m, float& v, float& vmax, bool amsgrad,
                                          const AdamScalars& S) {
    if (S.unscale) g = g / S.gs;
    if (S.maximize) g = -g;
    if (S.wd != 0.f) {
        if (S.decoupled) p = p * S.decay;
        else g = g + S.wd * p;
    }
    // ATen lerp (aten/src/ATen/native/Lerp.h)
    const float d = g - m;
    m = S.w1 < 0.5f ? m + S.w1 * d : g - d * (1.f - S.w1);
    v = v * S.b2;
    v = v + S.w2 * (g * g);
    float vd = v;
    if (amsgrad) {
        vd = (vmax > v || vmax != vmax) ? vmax : v;   // torch.maximum: a NaN on either side stays
        vmax = vd;
    }
    const float denom = sqrtf(vd) / S.bc2_sqrt + S.eps;
    p = p + S.neg_step_size * (m / denom);
}

__global__ __launch_bounds__(256) void adam_kernel(AdamJobs J, AdamHyper H) {
    if (H.found_inf && *H.found_inf != 0.f) return;
    const int t = job_of(J.blk, J.n);
    float* __restrict__ p = J.p[t];
    const float* __restrict__ gr = J.g[t];
    float* __restrict__ m = J.m[t];
    float* __restrict__ v = J.v[t];
    float* __restrict__ vmax = H.amsgrad ? J.vmax[t] : nullptr;
    const int64_t n = J.numel[t];

    const double lr = H.lr_dev ? (double)*H.lr_dev : (double)H.lr;
    const double step = (double)*J.step[t] + 1.0;   // the count is advanced by adam_count_kernel afterwards
    const double bc1 = 1.0 - pow(H.beta1, step);
    const double bc2 = 1.0 - pow(H.beta2, step);
    AdamScalars S;
    S.decay = (float)(1.0 - lr * (double)H.wd);
    S.wd = H.wd;
    S.w1 = (float)(1.0 - H.beta1);
    S.b2 = (float)H.beta2;
    S.w2 = (float)(1.0 - H.beta2);
    S.bc2_sqrt = (float)sqrt(bc2);
    S.eps = H.eps;
    S.neg_step_size = -(float)(lr / bc1);
    S.gs = H.grad_scale ? *H.grad_scale : 1.f;
    S.unscale = H.grad_scale != nullptr;
    S.decoupled = H.decoupled;
    S.maximize = H.maximize;

    const int64_t i0 = (int64_t)(blockIdx.x - J.blk[t]) * SGD_PIECE + 4 * threadIdx.x;
    const bool vec = i0 + 3 < n &&
                     ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(gr) | reinterpret_cast<uintptr_t>(m) |
                       reinterpret_cast<uintptr_t>(v) | reinterpret_cast<uintptr_t>(vmax)) & 15) == 0;
    if (vec) {
        float4 pv = *reinterpret_cast<const float4*>(p + i0);
        const float4 gv = *reinterpret_cast<const float4*>(gr + i0);
        float4 mv = *reinterpret_cast<const float4*>(m + i0);
        float4 vv = *reinterpret_cast<const float4*>(v + i0);
        float4 xv = vmax ? *reinterpret_cast<const float4*>(vmax + i0) : make_float4(0.f, 0.f, 0.f, 0.f);
        adam_elem(pv.x, gv.x, mv.x, vv.x, xv.x, vmax != nullptr, S);
        adam_elem(pv.y, gv.y, mv.y, vv.y, xv.y, vmax != nullptr, S);
        adam_elem(pv.z, gv.z, mv.z, vv.z, xv.z, vmax != nullptr, S);
        adam_elem(pv.w, gv.w, mv.w, vv.w, xv.w, vmax != nullptr, S);
        *reinterpret_cast<float4*>(p + i0) = pv;
        *reinterpret_cast<float4*>(m + i0) = mv;
        *reinterpret_cast<float4*>(v + i0) = vv;
        if (vmax) *reinterpret_cast<float4*>(vmax + i0) = xv;
    } else {
        for (int64_t i = i0; i < min(n, i0 + 4); ++i) {
            float pi = p[i], mi = m[i], vi = v[i], xi = vmax ? vmax[i] : 0.f;
            adam_elem(pi, gr[i], mi, vi, xi, vmax != nullptr, S);
            p[i] = pi;
            m[i] = mi;
            v[i] = vi;
            if (vmax) vmax[i] = xi;
        }
    }
}

// Advances the step counts after adam_kernel (same stream, so every workgroup
// of it has read them): one workgroup, one thread per tensor.
struct AdamCounts {
    float* step[SGD_MAX];
    int n;
};

__global__ __launch_bounds__(64) void adam_count_kernel(AdamCounts C, const float* __restrict__ found_inf) {
    if (found_inf && *found_inf != 0.f) return;
    if ((int)threadIdx.x < C.n) *C.step[threadIdx.x] += 1.f;
}

// ---- torch._amp_foreach_non_finite_check_and_unscale_ (AmpKernels.cu):
// g *= *inv_scale (no write when it is 1), *found_inf = 1 on a non-finite value.
struct UnscaleJobs {
    float* g[SGD_MAX];
    int64_t numel[SGD_MAX];
    int blk[SGD_MAX + 1];
    int n;
};

__device__ __forceinline__ bool finite_f32(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

__global__ __launch_bounds__(256) void unscale_kernel(UnscaleJobs J, const float* __restrict__ inv_scale,
                                                      float* __restrict__ found_inf) {
    const int t = job_of(J.blk, J.n);
    float* __restrict__ g = J.g[t];
    const int64_t n = J.numel[t];
    const float inv = *inv_scale;
    const int64_t i0 = (int64_t)(blockIdx.x - J.blk[t]) * SGD_PIECE + 4 * threadIdx.x;
    bool bad = false;
    if (i0 + 3 < n && (reinterpret_cast<uintptr_t>(g) & 15) == 0) {
        float4 gv = *reinterpret_cast<const float4*>(g + i0);
        bad = !(finite_f32(gv.x) && finite_f32(gv.y) && finite_f32(gv.z) && finite_f32(gv.w));
        if (inv != 1.f) {
            gv = make_float4(gv.x * inv, gv.y * inv, gv.z * inv, gv.w * inv);
            *reinterpret_cast<float4*>(g + i0) = gv;
        }
    } else {
        for (int64_t i = i0; i < min(n, i0 + 4); ++i) {
            const float x = g[i];
            bad = bad || !finite_f32(x);
            if (inv != 1.f) g[i] = x * inv;
        }
    }
    if (bad) *found_inf = 1.f;   // every writer stores the same value
}

}  // namespace

extern "C" {

int dgx_sgd_step_f32(int n, float* const* params, const float* const* grads, float* const* momentum_bufs,
                     const int64_t* numels, float lr, float weight_decay, float momentum, float dampening,
                     int nesterov, int maximize, int first, void* stream) {
    if (n < 0 || n > SGD_MAX || (n > 0 && (!params || !grads || !numels))) return DGX_EINVAL;
    if (momentum != 0.f && !momentum_bufs) return DGX_EINVAL;
    if (n == 0) return DGX_OK;
    SgdJobs J{};
    J.n = n;
    J.blk[0] = 0;
    for (int t = 0; t < n; ++t) {
        if (numels[t] < 0) return DGX_EINVAL;
        if (numels[t] != 0 && (!params[t] || !grads[t] || (momentum != 0.f && !momentum_bufs[t])))
            return DGX_EINVAL;   // a zero-element tensor may have no storage
        J.p[t] = params[t];
        J.g[t] = grads[t];
        J.m[t] = momentum != 0.f ? momentum_bufs[t] : nullptr;
        J.numel[t] = numels[t];
        const int64_t pieces = (numels[t] + SGD_PIECE - 1) / SGD_PIECE;
        if ((int64_t)J.blk[t] + pieces > (1LL << 30)) return DGX_EUNSUPPORTED;
        J.blk[t + 1] = J.blk[t] + (int)pieces;
    }
    if (J.blk[n] == 0) return DGX_OK;
    hipLaunchKernelGGL(sgd_kernel, dim3((unsigned)J.blk[n]), dim3(256), 0, dgx_stream(stream), J, lr, weight_decay,
                       momentum, dampening, nesterov, maximize, first);
    return hipGetLastError() == hipSuccess ? DGX_OK : DGX_ELAUNCH;
}

int dgx_sgd_step_amp_f32(int n, float* const* params, const float* const* grads, float* const* momentum_bufs,
                         const int64_t* numels, float lr, float weight_decay, float momentum, float dampening,
                         int nesterov, int maximize, int first, const float* grad_scale, const float* found_inf,
                         void* stream) {
    if (n < 0 || n > SGD_MAX || (n > 0 && (!params || !grads || !numels))) return DGX_EINVAL;
    if (momentum != 0.f && !momentum_bufs) return DGX_EINVAL;
    if (n == 0) return DGX_OK;
    SgdJobs J{};
    for (int t = 0; t < n; ++t) {   // a zero-element tensor may have no storage
        if (numels[t] != 0 && (!params[t] || !grads[t] || (momentum != 0.f && !momentum_bufs[t]))) return DGX_EINVAL;
        J.p[t] = params[t];
        J.g[t] = grads[t];
        J.m[t] = momentum != 0.f ? momentum_bufs[t] : nullptr;
    }
    if (const int rc = fill_pieces(J, n, numels)) return rc;
    if (J.blk[n] == 0) return DGX_OK;
    hipLaunchKernelGGL(sgd_amp_kernel, dim3((unsigned)J.blk[n]), dim3(256), 0, dgx_stream(stream), J, lr, weight_decay,
                       momentum, dampening, nesterov, maximize, first, grad_scale, found_inf);
    return hipGetLastError() == hipSuccess ? DGX_OK : DGX_ELAUNCH;
}

int dgx_adam_step_f32(int n, float* const* params, const float* const* grads, float* const* exp_avgs,
                      float* const* exp_avg_sqs, float* const* max_exp_avg_sqs, float* const* steps,
                      const int64_t* numels, float lr, const float* lr_dev, double beta1, double beta2, double eps,
                      double weight_decay, int decoupled_weight_decay, int amsgrad, int maximize,
                      const float* grad_scale, const float* found_inf, void* stream) {
    if (n < 0 || n > SGD_MAX || (n > 0 && (!params || !grads || !exp_avgs || !exp_avg_sqs || !steps || !numels)))
        return DGX_EINVAL;
    if (amsgrad && n > 0 && !max_exp_avg_sqs) return DGX_EINVAL;
    if (n == 0) return DGX_OK;
    AdamJobs J{};
    AdamCounts C{};
    C.n = n;
    for (int t = 0; t < n; ++t) {
        if (!steps[t]) return DGX_EINVAL;
        if (numels[t] != 0 && (!params[t] || !grads[t] || !exp_avgs[t] || !exp_avg_sqs[t] ||
                               (amsgrad && !max_exp_avg_sqs[t])))   // a zero-element tensor may have no storage
            return DGX_EINVAL;
        J.p[t] = params[t];
        J.g[t] = grads[t];
        J.m[t] = exp_avgs[t];
        J.v[t] = exp_avg_sqs[t];
        J.vmax[t] = amsgrad ? max_exp_avg_sqs[t] : nullptr;
        J.step[t] = C.step[t] = steps[t];
    }
    if (const int rc = fill_pieces(J, n, numels)) return rc;
    AdamHyper H{};
    H.lr = lr;
    H.lr_dev = lr_dev;
    H.beta1 = beta1;
    H.beta2 = beta2;
    H.eps = (float)eps;
    H.wd = (float)weight_decay;
    H.decoupled = decoupled_weight_decay;
    H.amsgrad = amsgrad;
    H.maximize = maximize;
    H.grad_scale = grad_scale;
    H.found_inf = found_inf;
    if (J.blk[n] != 0) {
        hipLaunchKernelGGL(adam_kernel, dim3((unsigned)J.blk[n]), dim3(256), 0, dgx_stream(stream), J, H);
        DGX_CHECK_LAUNCH();
    }
    // torch counts a step for a zero-element parameter too
    hipLaunchKernelGGL(adam_count_kernel, dim3(1), dim3(64), 0, dgx_stream(stream), C, found_inf);
    return hipGetLastError() == hipSuccess ? DGX_OK : DGX_ELAUNCH;
}

int dgx_amp_unscale_f32(int n, float* const* grads, const int64_t* numels, const float* inv_scale, float* found_inf,
                        void* stream) {
    if (n < 0 || n > SGD_MAX || (n > 0 && (!grads || !numels)) || !inv_scale || !found_inf) return DGX_EINVAL;
    if (n == 0) return DGX_OK;
    UnscaleJobs J{};
    for (int t = 0; t < n; ++t) {
        if (numels[t] != 0 && !grads[t]) return DGX_EINVAL;
        J.g[t] = grads[t];
    }
    if (const int rc = fill_pieces(J, n, numels)) return rc;
    if (J.blk[n] == 0) return DGX_OK;
    hipLaunchKernelGGL(unscale_kernel, dim3((unsigned)J.blk[n]), dim3(256), 0, dgx_stream(stream), J, inv_scale,
                       found_inf);
    return hipGetLastError() == hipSuccess ? DGX_OK : DGX_ELAUNCH;
}

}  // extern "C"
