// Segmentation / classification metrics accumulated on the device: what the
// reference's loops do per step on the host (main_partseg_dist.py:266-274 and
// :259: arg-max, two blocking copies, lists of labels, loss.item()) and at the
// epoch's end in Python loops (calculate_shape_IoU :63-84, calculate_sem_IoU,
// sklearn's accuracy scores) as one launch per step that only adds integers.
//
// State (caller-owned device memory, see include/dgx.h): the (C, C) int64
// confusion table [true][pred]; per recorded shape and part slot the integer
// intersection I and union U of calculate_shape_IoU; a block of int64 words
// (cursor, invalid, overflow, count, ticket); the fp32 loss sum. Every ratio
// (I / U, diag / rowsum, trace / total) is left to the host, which divides the
// same integers the reference's loops count: results are equal bit for bit.
//
// One workgroup builds the (true, pred) counts of its points in an LDS uint32
// C x C table with LDS integer atomics, one lane per point:
//   with categories   one workgroup per shape; the shape's part slots are read
//                     off the table (I = t[p][p], U = rowsum[p] + colsum[p] - I)
//                     and stored at slot cursor + b;
//   without           workgroups take grid-strided chunks of SM_THREADS points,
//                     SM_MIN_CHUNKS each at least, on at most SM_MAX_BLOCKS workgroups.
// Either way the workgroup then adds the table's non-zero entries to the global
// one. All accumulation across workgroups is integer atomicAdd: the result does
// not depend on the order of arrival.
//
// Logits: the arg-max is ce_row_max, the loss head's own (ce_row.h), so the
// classes are those dgx_smoothed_ce_fwd returns. Point-contiguous planes are
// read one lane per point, coalesced across lanes for each class;
// class-contiguous rows (100 bytes at C = 50 in fp16: not 16-byte aligned one by
// one) are staged flat in LDS, 16 bytes per lane, and walked there.
//
// Cursor, count and loss sum belong to the launch as a whole: every workgroup
// reads the cursor when it starts and takes a ticket when it is done, and the
// one that draws the last ticket advances them and puts the ticket back to 0.
// No workgroup waits for another.
//
// Nothing read from the data is used as an address before it is checked: a
// label or prediction outside [0, C), a category outside [0, ncat) or a part
// range outside the table or the slot row is counted in `invalid` and skipped;
// a shape beyond `capacity` is counted in `overflow` and not written.
#include <algorithm>

#include "ce_row.h"

namespace {

constexpr int SM_THREADS = 1024;        // threads per workgroup = points per chunk: a shape has one workgroup,
                                        // so the largest there is
constexpr int SM_MAX_CLASSES = 128;     // 128 x 128 uint32 = 64 KiB of LDS
constexpr int SM_TILE_BYTES = 32768;    // LDS staging of class-contiguous rows (64 rows of 128 fp32 at least)
constexpr int SM_MAX_BLOCKS = 2048;     // grid cap of the chunked path
constexpr int SM_MIN_CHUNKS = 4;        // chunks a workgroup of that path takes at least: it zeroes and flushes a table
constexpr int SM_INT_PRED = 3;          // SRC of ready integer predictions; 0..2 are DGX_CE_*

enum { SM_CURSOR = 0, SM_INVALID = 1, SM_OVERFLOW = 2, SM_COUNT = 3, SM_TICKET = 4 };

struct SmArgs {
    const void* src;      // logits or integer predictions
    int rows_layout;      // logits: class-contiguous (else point-contiguous planes)
    int p64;              // integer predictions are int64
    int64_t B, N;
    int C;
    const void* seg;
    int s64;
    const void* cat;      // NULL: no per-shape record
    int c64;
    const int32_t* part_start;
    const int32_t* part_count;
    int ncat;
    unsigned long long* confusion;
    int32_t* iu;
    int32_t* nparts;
    int64_t capacity;
    int max_parts;
    unsigned long long* state;
    float* loss_sum;
    const float* loss;
};

template <int SRC> struct SmElt { using T = typename Elt<SRC>::T; };
template <> struct SmElt<SM_INT_PRED> { using T = unsigned char; };

// TAB = entries of the LDS table (C * C <= TAB).
template <int SRC, int TAB>
__global__ __launch_bounds__(SM_THREADS) void seg_metrics_kernel(const SmArgs a) {
    using T = typename SmElt<SRC>::T;
    constexpr bool STAGED = SRC != SM_INT_PRED;
    __shared__ uint32_t tab[TAB];
    __shared__ __attribute__((aligned(16))) unsigned char tile[STAGED ? SM_TILE_BYTES + 16 : 16];
    __shared__ uint32_t bad;         // invalid points (and the shape's category) of this workgroup
    __shared__ int64_t cursor;
    const int tid = threadIdx.x;
    const int C = a.C;
    const int64_t M = a.B * a.N;
    const bool shapes = a.cat != nullptr;

    for (int e = tid; e < C * C; e += SM_THREADS) tab[e] = 0;
    if (tid == 0) {
        bad = 0;
        cursor = (int64_t)a.state[SM_CURSOR];
    }
    __syncthreads();

    // the chunks of this workgroup: chunk c covers the flat rows [base + c * SM_THREADS, ...) below `stop`
    int64_t base, stop, c, cstep;
    if (shapes) {
        base = (int64_t)blockIdx.x * a.N;
        stop = base + a.N;
        c = 0;
        cstep = 1;
    } else {
        base = 0;
        stop = M;
        c = blockIdx.x;
        cstep = gridDim.x;
    }
    for (;; c += cstep) {
        const int64_t r0 = base + c * SM_THREADS;
        if (r0 >= stop) break;
        const int cnt = (int)min((int64_t)SM_THREADS, stop - r0);
        if (SRC == SM_INT_PRED || !a.rows_layout) {
            if (tid < cnt) {
                const int64_t row = r0 + tid;
                int64_t p;
                if constexpr (SRC == SM_INT_PRED) {
                    p = ce_label(a.src, a.p64, row);
                } else {
                    const int64_t b = row / a.N, n = row - b * a.N, N = a.N;
                    const T* x = static_cast<const T*>(a.src) + b * C * N + n;
                    float mx;
                    int arg;
                    ce_row_max([x, N](int j) { return Elt<SRC>::ld(x + (int64_t)j * N); }, C, mx, arg);
                    p = arg;
                }
                const int64_t y = ce_label(a.seg, a.s64, row);
                if (y >= 0 && y < C && p >= 0 && p < C) atomicAdd(&tab[(int)y * C + (int)p], 1u);
                else atomicAdd(&bad, 1u);
            }
        } else if constexpr (STAGED) {
            const int tile_rows = min(SM_THREADS, SM_TILE_BYTES / (C * (int)sizeof(T)));   // 64 to 1024
            for (int t0 = 0; t0 < cnt; t0 += tile_rows) {
                const int tr = min(tile_rows, cnt - t0);
                const uintptr_t beg = reinterpret_cast<uintptr_t>(static_cast<const T*>(a.src) + (r0 + t0) * C);
                __syncthreads();   // the lanes of the tile before are done with it
                ce_stage_rows<T, SM_THREADS>(tile, beg, (size_t)tr * C * sizeof(T), tid);
                __syncthreads();
                if (tid < tr) {
                    const int64_t row = r0 + t0 + tid;
                    const T* x = reinterpret_cast<const T*>(tile + (beg & 15)) + (size_t)tid * C;
                    float mx;
                    int arg;
                    ce_row_max([x](int j) { return Elt<SRC>::ld(x + j); }, C, mx, arg);
                    const int64_t y = ce_label(a.seg, a.s64, row);
                    if (y >= 0 && y < C) atomicAdd(&tab[(int)y * C + arg], 1u);
                    else atomicAdd(&bad, 1u);
                }
            }
        }
    }
    __syncthreads();

    if (shapes) {   // this shape's part slots, at slot cursor + b
        const int64_t slot = cursor + blockIdx.x;
        const int64_t cat = ce_label(a.cat, a.c64, blockIdx.x);
        int start = 0, count = 0;
        bool ok = cat >= 0 && cat < a.ncat;
        if (ok) {
            start = a.part_start[cat];
            count = a.part_count[cat];
            ok = start >= 0 && count >= 0 && count <= a.max_parts && start <= C - count;
        }
        if (!ok) count = 0;
        const bool fits = slot >= 0 && slot < a.capacity;
        if (fits) {
            const int wave = tid / DGX_WAVE, lane = tid % DGX_WAVE;
            int32_t* out = a.iu + slot * a.max_parts * 2;
            for (int q = wave; q < a.max_parts; q += SM_THREADS / DGX_WAVE) {   // one wave per part slot
                uint32_t inter = 0, uni = 0;
                if (q < count) {
                    const int p = start + q;
                    uint32_t s = 0;
                    for (int j = lane; j < C; j += DGX_WAVE) s += tab[p * C + j] + tab[j * C + p];   // row + column
                    for (int o = DGX_WAVE / 2; o > 0; o >>= 1) s += __shfl_xor(s, o);
                    inter = tab[p * C + p];
                    uni = s - inter;
                }
                if (lane == 0) {
                    out[2 * q] = (int32_t)inter;
                    out[2 * q + 1] = (int32_t)uni;
                }
            }
            if (tid == 0) a.nparts[slot] = count;
        }
        if (tid == 0) {
            if (!ok) atomicAdd(&bad, 1u);
            if (!fits) atomicAdd(&a.state[SM_OVERFLOW], 1ull);
        }
    }

    // the non-zero counts into the global table
    for (int e = tid; e < C * C; e += SM_THREADS) {
        const uint32_t v = tab[e];
        if (v) atomicAdd(&a.confusion[e], (unsigned long long)v);
    }
    __syncthreads();
    if (tid == 0) {
        if (bad) atomicAdd(&a.state[SM_INVALID], (unsigned long long)bad);
        // every workgroup has read the cursor before it takes its ticket: the last ticket may move it
        __threadfence();
        if (atomicAdd(&a.state[SM_TICKET], 1ull) == (unsigned long long)gridDim.x - 1) {
            a.state[SM_TICKET] = 0;
            if (shapes) a.state[SM_CURSOR] = (unsigned long long)(cursor + a.B);
            a.state[SM_COUNT] += (unsigned long long)a.B;
            if (a.loss) *a.loss_sum = *a.loss_sum + *a.loss;
        }
    }
}

template <int SRC>
void sm_launch(const SmArgs& a, unsigned grid, hipStream_t st) {
    if (a.C <= 64) hipLaunchKernelGGL((seg_metrics_kernel<SRC, 64 * 64>), dim3(grid), dim3(SM_THREADS), 0, st, a);
    else hipLaunchKernelGGL((seg_metrics_kernel<SRC, SM_MAX_CLASSES * SM_MAX_CLASSES>), dim3(grid), dim3(SM_THREADS),
                            0, st, a);
}

}  // namespace

extern "C" {

int dgx_seg_metrics_max_classes(void) { return SM_MAX_CLASSES; }

int dgx_seg_metrics_update(const void* scores, int dtype, int64_t B, int64_t C, int64_t N, int64_t sb, int64_t sc,
                           int64_t sn, const void* seg, int seg_is_i64, const void* cat, int cat_is_i64,
                           const int32_t* part_start, const int32_t* part_count, int ncat, int64_t* confusion,
                           int32_t* iu, int32_t* nparts, int64_t capacity, int max_parts, int64_t* state,
                           const float* loss, float* loss_sum, void* stream) {
    if (!scores || !seg || !confusion || !state) return DGX_EINVAL;
    if (B < 1 || N < 1 || C < 2) return DGX_EINVAL;
    if (C > SM_MAX_CLASSES) return DGX_EUNSUPPORTED;
    const bool ints = dtype == DGX_SEG_PRED_I64 || dtype == DGX_SEG_PRED_I32;
    const bool logits = dtype == DGX_CE_F32 || dtype == DGX_CE_F16 || dtype == DGX_CE_BF16;
    if (!ints && !logits) return DGX_EINVAL;
    // a workgroup's uint32 counts hold its points: one shape's N, or its share of M over the chunked grid
    // (a part's I and U are at most N and stored as int32; its row + column sum, at most 2 N, is a uint32)
    if (B > INT32_MAX || N > INT32_MAX || B > ((int64_t)1 << 40) / N) return DGX_EUNSUPPORTED;
    int rows_layout = 0;
    if (logits) {
        if (sc == 1 && (N == 1 || sn == C) && (B == 1 || sb == N * C)) rows_layout = 1;
        else if (!((N == 1 || sn == 1) && sc == N && (B == 1 || sb == C * N))) return DGX_EUNSUPPORTED;
    }
    const size_t es = ints ? (dtype == DGX_SEG_PRED_I64 ? 8 : 4) : (dtype == DGX_CE_F32 ? 4 : 2);
    if (reinterpret_cast<uintptr_t>(scores) % es || reinterpret_cast<uintptr_t>(seg) % (seg_is_i64 ? 8 : 4) ||
        reinterpret_cast<uintptr_t>(confusion) % 8 || reinterpret_cast<uintptr_t>(state) % 8)
        return DGX_EINVAL;
    if (cat) {
        if (!part_start || !part_count || ncat < 1 || capacity < 0 || max_parts < 1 || max_parts > SM_MAX_CLASSES)
            return DGX_EINVAL;
        if (capacity > 0 && (!iu || !nparts)) return DGX_EINVAL;
        if (reinterpret_cast<uintptr_t>(cat) % (cat_is_i64 ? 8 : 4) || reinterpret_cast<uintptr_t>(iu) % 4 ||
            reinterpret_cast<uintptr_t>(nparts) % 4)
            return DGX_EINVAL;
    }
    if (loss && !loss_sum) return DGX_EINVAL;
    if (reinterpret_cast<uintptr_t>(loss) % 4 || reinterpret_cast<uintptr_t>(loss_sum) % 4) return DGX_EINVAL;

    SmArgs a;
    a.src = scores;
    a.rows_layout = rows_layout;
    a.p64 = dtype == DGX_SEG_PRED_I64;
    a.B = B;
    a.N = N;
    a.C = (int)C;
    a.seg = seg;
    a.s64 = seg_is_i64;
    a.cat = cat;
    a.c64 = cat_is_i64;
    a.part_start = part_start;
    a.part_count = part_count;
    a.ncat = ncat;
    a.confusion = reinterpret_cast<unsigned long long*>(confusion);
    a.iu = iu;
    a.nparts = nparts;
    a.capacity = cat ? capacity : 0;
    a.max_parts = max_parts;
    a.state = reinterpret_cast<unsigned long long*>(state);
    a.loss_sum = loss_sum;
    a.loss = loss;
    const int64_t chunks = (B * N + SM_THREADS - 1) / SM_THREADS;
    const unsigned grid =
        cat ? (unsigned)B : (unsigned)std::min<int64_t>((chunks + SM_MIN_CHUNKS - 1) / SM_MIN_CHUNKS, SM_MAX_BLOCKS);
    hipStream_t st = dgx_stream(stream);
    switch (dtype) {
        case DGX_CE_F32: sm_launch<DGX_CE_F32>(a, grid, st); break;
        case DGX_CE_F16: sm_launch<DGX_CE_F16>(a, grid, st); break;
        case DGX_CE_BF16: sm_launch<DGX_CE_BF16>(a, grid, st); break;
        default: sm_launch<SM_INT_PRED>(a, grid, st); break;
    }
    return hipGetLastError() == hipSuccess ? DGX_OK : DGX_ELAUNCH;
}

}  // extern "C"
