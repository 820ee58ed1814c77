// Row code shared by the loss head (loss.hip) and the segmentation metrics
// (metrics.hip): how a logit of each dtype is read, a row's maximum and
// arg-max, and the staging of a run of class-contiguous rows in LDS. Both
// files take their arg-max from ce_row_max, so they agree on every row.
#pragma once
#include <hip/hip_fp16.h>

#include "common.h"

namespace {

constexpr int CE_BATCH = 8;   // logits a lane loads ahead of their use

template <int DT> struct Elt;
template <> struct Elt<DGX_CE_F32> {
    using T = float;
    static __device__ __forceinline__ float ld(const T* p) { return *p; }
    static __device__ __forceinline__ T cv(float v) { return v; }
};
template <> struct Elt<DGX_CE_F16> {
    using T = uint16_t;
    static __device__ __forceinline__ float ld(const T* p) { return __half2float(__ushort_as_half(*p)); }
    static __device__ __forceinline__ T cv(float v) { return __half_as_ushort(__float2half_rn(v)); }
};
template <> struct Elt<DGX_CE_BF16> {
    using T = uint16_t;
    static __device__ __forceinline__ float ld(const T* p) { return __uint_as_float((uint32_t)*p << 16); }
    static __device__ __forceinline__ T cv(float v) {   // round to nearest even; NaN stays NaN
        const uint32_t u = __float_as_uint(v);
        if ((u & 0x7fffffffu) > 0x7f800000u) return (T)((u >> 16) | 0x40u);
        return (T)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
    }
};

// A label / class id array of int64 (is64 != 0) or int32 elements.
__device__ __forceinline__ int64_t ce_label(const void* labels, int l64, int64_t row) {
    return l64 ? static_cast<const int64_t*>(labels)[row] : (int64_t) static_cast<const int32_t*>(labels)[row];
}

// Maximum and arg-max of one row; ld(j) is logit j as fp32. The first maximum
// wins. A NaN never compares greater: a row whose logit 0 is NaN keeps class 0,
// a NaN elsewhere is passed over.
// The pass fetches CE_BATCH logits before it uses them: one lane walks a whole row, and a load
// waited for at every class leaves the row bound by memory latency.
template <class Ld>
__device__ __forceinline__ void ce_row_max(Ld ld, int C, float& mx, int& arg) {
    mx = ld(0);
    arg = 0;
    for (int j0 = 0; j0 < C; j0 += CE_BATCH) {
        float v[CE_BATCH];
#pragma unroll
        for (int u = 0; u < CE_BATCH; ++u) v[u] = ld(min(j0 + u, C - 1));
#pragma unroll
        for (int u = 0; u < CE_BATCH; ++u) {
            if (j0 + u < C && v[u] > mx) {
                mx = v[u];
                arg = j0 + u;
            }
        }
    }
}

// Stage the bytes [beg, beg + bytes) of global memory (a run of whole rows of elements T; such rows
// are not 16-byte aligned one by one) in `tile` with NT threads: flat 16-byte loads of the aligned
// granules inside the range, element loads for the ragged granule in front and the one behind.
// The range then starts at tile + (beg & 15). tile is 16-byte aligned and holds bytes + 16 at least.
// The caller synchronises the workgroup before it reads the tile.
template <class T, int NT>
__device__ __forceinline__ void ce_stage_rows(unsigned char* tile, uintptr_t beg, size_t bytes, int tid) {
    const uintptr_t end = beg + bytes;
    const uintptr_t a0 = beg & ~(uintptr_t)15;
    // granules [first, full) lie inside the range: 16-byte loads, four in flight per lane
    const int first = beg == a0 ? 0 : 1, full = (int)((end - a0) >> 4);
#pragma unroll 4
    for (int q = first + tid; q < full; q += NT)
        *reinterpret_cast<uint4*>(tile + (q << 4)) = *reinterpret_cast<const uint4*>(a0 + ((uintptr_t)q << 4));
    // the granule in front of them and the one behind: only the elements inside the range
    if (tid < 2) {
        const uintptr_t src = tid == 0 ? a0 : a0 + ((uintptr_t)full << 4);
        const uintptr_t lo = src > beg ? src : beg, hi = src + 16 < end ? src + 16 : end;
        if (tid == 1 || first == 1)
            for (uintptr_t o = lo; o < hi; o += sizeof(T))
                *reinterpret_cast<T*>(tile + (o - a0)) = *reinterpret_cast<const T*>(o);
    }
}

}  // namespace
