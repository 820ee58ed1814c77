// libdgx_torch.so — the PyTorch-ROCm C++ layer of the engine and the ONE place
// the launch schedule and its BatchNorm bookkeeping live.
//
// Every launch goes to libdgx.so's C ABI (include/dgx.h) straight from C++.
// The schedule of DGCNN's EdgeConv chain (reference models/dgcnn.py:84-100),
// of its conv5 (dgcnn.py:74-78, 100-102) and of PositionEmbedding's per-edge
// MLP (models/layers.py:45-52), forward and backward, in every configuration the reference's scripts run it in:
//   precision   bf16 GEMM operands (BASELINE cfg2; what torch.autocast asks for,
//               main_partseg_dist.py:253) or the fp32 parity mode;
//   BatchNorm   training (batch statistics, running-stat update with a momentum
//               or the cumulative average), eval (running statistics), and
//               SyncBatchNorm (main_partseg_dist.py:189: the per-layer sums are
//               all-reduced over the module's process group through
//               _c10d_functional, one fp64 collective per layer and direction);
//   shapes      any (B, C, N, k): the fused kNN where its kernel is built for
//               the shape, the generic kNN elsewhere.
// Ops (TORCH_LIBRARY dgx_host):
//   chain_forward / chain_backward        the block chain (dgx.edgeconv's
//                                         autograd Function and dgx::edgeconv_chain call these)
//   pointconv_forward / pointconv_backward conv5 + BN + LeakyReLU (dgx.pointconv, dgx::pointconv)
//   edge_mlp2_forward / edge_mlp2_backward PositionEmbedding's edge MLP (dgx.edgemlp, dgx::edge_mlp2);
//                                         its kNN graph comes in from the caller
//   bn_batch_stats / bn_backward_consts   one layer's BatchNorm finalize, forward / backward (dgx.bn)
//   dgcnn                                 DGCNN.forward as one op with a C++ autograd node
//                                         (eager training: ~60 launches without a Python frame)
//   gemm_xwt / gemm_xw / gemm_atb / gemm32 / gemm_edge_dz_ok / weight_prep / weight_prep_one
//                                         the schedule's GEMM and weight-prep helpers, one op each (dgx.gemm)
//   weight_prep_layout                    the weight-prep buffer's layout, host only (dgx.gemm.prep_layout restates it)
//   knn / knn_image_buffers               the kNN dispatch the chain runs too, and its prepared-operand scratch
//   knn_timing                            per-thread HIP-event timing of the kNN selection launches
//   reverse_graphs                        CSR in-edge lists of kNN graphs, 8 graphs per launch
//   graph_feature / graph_feature_backward get_graph_feature's edge tensor after the kNN, and its gradient
//   vattn_forward                          the fused kNN vector attention (attention.py:115-150)
//   layout                                the name tables of the saved-state lists and the opts word
//                                         (dgx.schedule names the same fields: one layout, checked by a test)
#include <ATen/ATen.h>
#include <ATen/core/dispatch/Dispatcher.h>
#include <torch/library.h>
#include <torch/csrc/autograd/custom_function.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <array>
#include <cstdint>
#include <optional>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

#include "../../include/dgx.h"

namespace {

using at::Tensor;
using torch::autograd::AutogradContext;
using torch::autograd::variable_list;

constexpr int kEpiStore = 0, kEpiAccum = 1, kEpiStats = 2, kEpiSlab = 3, kEpiStats16 = 4;
constexpr int kSmallKMax = 16;                                   // dgx.gemm.SMALLK_MAX

void check(int rc, const char* what) {
  TORCH_CHECK(rc == 0, "dgx: ", what, " failed (", rc, ": ", dgx_strerror(rc), ")");
}

template <typename T = float>
T* P(const Tensor& t) { return t.defined() && t.numel() ? static_cast<T*>(t.data_ptr()) : nullptr; }

int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// A/B switches of the schedule (dgx.edgeconv / dgx.gemm environment flags), one word:
// bit i is switch kOptNames[i] (dgx.schedule.OPT_BITS), bits 8-15 the slab cap
enum OptBit { kScatterPacked, kFoldBnBwd, kFuseKnnImage, kFuseEdgeDz, kSplit32, kSplit32Edge, kNumOptBits };
const char* const kOptNames[kNumOptBits] = {"SCATTER_PACKED", "FOLD_BN_BWD", "FUSE_KNN_IMAGE", "FUSE_EDGE_DZ",
                                            "SPLIT32",        "SPLIT32_EDGE"};
struct Opts {                // one member per OptBit, in that order, then the slab cap
  bool packed;               // bf16 / split fp32: backward scatter reads packed dz|slot words
  bool fold_bwd;             // BN backward finalize in the scatter's prologue
  bool fuse_image;           // blocks' apply writes the next kNN's operand image
  bool fuse_edge_dz;         // bf16: block l-1's dz from block l's dX GEMM epilogue
  bool split32;              // fp32 mode: conv5 GEMMs as 3-pass split bf16 (hi.hi + hi.lo + lo.hi)
  bool split_edge;           // with split32: EdgeConv dW / dX as 3-pass split bf16 on the scatter's split dPQ planes
  int64_t slab_cap_mb;       // split-K slab cap of small weight gradients (0 = off)
};
Opts decode(int64_t o) {
  auto bit = [o](OptBit b) { return ((o >> b) & 1) != 0; };
  return Opts{bit(kScatterPacked), bit(kFoldBnBwd),  bit(kFuseKnnImage), bit(kFuseEdgeDz), bit(kSplit32),
              bit(kSplit32Edge),   (o >> 8) & 0xff};
}

struct Dev {
  at::TensorOptions f32, f64, bf16, i32, i64, u8;
  void* stream;
  explicit Dev(const Tensor& t) {
    f32 = t.options().dtype(at::kFloat);
    f64 = t.options().dtype(at::kDouble);
    bf16 = t.options().dtype(at::kBFloat16);
    i32 = t.options().dtype(at::kInt);
    i64 = t.options().dtype(at::kLong);
    u8 = t.options().dtype(at::kByte);
    stream = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(t.device().index()).stream();
  }
};

std::vector<std::optional<Tensor>> to_vec(const c10::List<std::optional<Tensor>>& l) {
  std::vector<std::optional<Tensor>> v;
  for (size_t i = 0; i < l.size(); ++i) v.push_back(l.get(i));
  return v;
}

Tensor defined_or_none(const std::optional<Tensor>& t) {
  return (t.has_value() && t->defined() && t->numel() > 0) ? *t : Tensor();
}

// ------------------------------------------------------------ kNN timing ----
// Optional per-thread instrumentation (bench.py's roofline leg): HIP events
// around every kNN selection launch of this thread while enabled.
struct KnnRec {
  hipEvent_t e0, e1;
  double flops;
  int64_t B, C, N, k;
};
thread_local bool t_knn_timing = false;
thread_local std::vector<KnnRec> t_knn_recs;

// ------------------------------------------------------------ BatchNorm ----
// The nn.BatchNorm fields the schedule reads (dgx.bn.op_args), per layer.
struct BnSpec {
  bool training = true, track = true;
  Tensor rm, rv, nbt;              // module buffers, read (undefined when absent)
  Tensor rm_out, rv_out, nbt_out;  // where updates go (the buffers themselves: in place)
  double momentum = 0.1;           // < 0: cumulative average (momentum=None)
  double eps = 1e-5;
  std::string group;               // SyncBatchNorm process group name ("": local statistics)
  bool use_batch() const { return training || (!rm.defined() && !rv.defined()); }
  bool update() const { return training && track && rm.defined(); }
};

// per-channel state of one BN layer (dgx.bn.Stats names the same fields)
struct Stats {
  Tensor scale, shift, mean, invstd;
  std::string group;
  bool eval = false;
};

// bn_t: 6 per layer (rm, rv, nbt, rm_out, rv_out, nbt_out), bn_f: (momentum, eps, slope),
// bn_i: (training, track), groups: one name per layer
std::vector<BnSpec> parse_bn(const std::vector<std::optional<Tensor>>& bn_t, const std::vector<double>& bn_f,
                             const std::vector<int64_t>& bn_i, const std::vector<std::string>& groups, int L,
                             int tensors_per_layer) {
  TORCH_CHECK((int)bn_t.size() == tensors_per_layer * L && (int)bn_f.size() == 3 * L && (int)bn_i.size() == 2 * L &&
                  (int)groups.size() == L,
              "dgx: BatchNorm argument lists do not match the layer count");
  std::vector<BnSpec> out(L);
  for (int l = 0; l < L; ++l) {
    BnSpec& s = out[l];
    const int b = tensors_per_layer * l;
    s.rm = defined_or_none(bn_t[b]);
    s.rv = defined_or_none(bn_t[b + 1]);
    s.nbt = defined_or_none(bn_t[b + 2]);
    if (tensors_per_layer == 6) {
      s.rm_out = defined_or_none(bn_t[b + 3]);
      s.rv_out = defined_or_none(bn_t[b + 4]);
      s.nbt_out = defined_or_none(bn_t[b + 5]);
    }
    if (!s.rm_out.defined()) s.rm_out = s.rm;
    if (!s.rv_out.defined()) s.rv_out = s.rv;
    if (!s.nbt_out.defined()) s.nbt_out = s.nbt;
    s.momentum = bn_f[3 * l];
    s.eps = bn_f[3 * l + 1];
    s.training = bn_i[2 * l] != 0;
    s.track = bn_i[2 * l + 1] != 0;
    s.group = groups[l];
  }
  return out;
}

// a tall (rows, 2, co) partial array pre-reduced to ~128 rows
std::pair<Tensor, int> compact(const Dev& d, const Tensor& partials, int rows, int co) {
  if (rows <= 1024) return {partials, rows};
  const int R = 128, S = rows / R, left = rows - S * R;
  Tensor out = at::empty({R + left, 2, co}, d.f32);
  check(dgx_slab_reduce_f32(P(partials), S, R, 2 * co, R, P(out), 2 * co, d.stream), "bn partial reduce");
  if (left) out.narrow(0, R, left).copy_(partials.view({-1, 2, co}).narrow(0, (int64_t)S * R, left));
  return {out, R + left};
}

// SyncBatchNorm: [global sums (2, C) | global count] in fp64 after ONE all-reduce
// over the module's process group; the count stays on
// the device for the fp64 finalize kernels (no host synchronisation)
Tensor allreduce_sums(const Dev& d, const Tensor& partials, int rows, int co, double count, const std::string& group) {
  Tensor buf = at::empty({2 * co + 1}, d.f64);
  Tensor sums = buf.narrow(0, 0, 2 * co).view({2, co});
  at::sum_out(sums, partials.view({-1, 2, co}).narrow(0, 0, rows).to(at::kDouble), {0});
  buf.narrow(0, 2 * co, 1).fill_(count);
  static auto ar = c10::Dispatcher::singleton()
                       .findSchemaOrThrow("_c10d_functional::all_reduce_", "")
                       .typed<Tensor&(Tensor&, std::string, std::string)>();
  static auto wait = c10::Dispatcher::singleton()
                         .findSchemaOrThrow("_c10d_functional::wait_tensor", "")
                         .typed<Tensor(const Tensor&)>();
  ar.call(buf, "sum", group);
  wait.call(buf);
  return buf;
}

// batch mean / var from per-block (sum y, sum y^2) partials
// over `count` elements; running statistics updated as nn.BatchNorm would
Stats batch_stats(const Dev& d, const Tensor& partials, int rows, double count, const Tensor& gamma,
                  const Tensor& beta, const BnSpec& bn) {
  const int co = (int)gamma.size(0);
  Stats st{at::empty({co}, d.f32), at::empty({co}, d.f32), at::empty({co}, d.f32), at::empty({co}, d.f32),
           bn.group, false};
  const bool upd = bn.update();
  double factor = 0.0;
  const int64_t* nbt_in = nullptr;
  int64_t* nbt_new = nullptr;
  Tensor nbt_tmp;
  if (upd && bn.nbt.defined()) {
    factor = bn.momentum;
    nbt_in = P<int64_t>(bn.nbt);
    if (bn.momentum < 0.0 && bn.nbt_out.data_ptr() == bn.nbt.data_ptr()) {
      nbt_tmp = at::empty_like(bn.nbt);   // the cumulative form reads the counter: no in-place alias
      nbt_new = P<int64_t>(nbt_tmp);
    } else {
      nbt_new = P<int64_t>(bn.nbt_out);
    }
  } else if (upd) {
    factor = bn.momentum < 0.0 ? 0.0 : bn.momentum;
  }
  const float* rm = upd ? P(bn.rm) : nullptr;
  const float* rv = upd ? P(bn.rv) : nullptr;
  float* rm_new = upd ? P(bn.rm_out) : nullptr;
  float* rv_new = upd ? P(bn.rv_out) : nullptr;
  auto pr = compact(d, partials, rows, co);
  if (!bn.group.empty()) {
    Tensor sums = allreduce_sums(d, pr.first, pr.second, co, count, bn.group);
    check(dgx_bn_finalize_out_f64(P<double>(sums), 1, co, -1.0, P(gamma), P(beta), rm, rv, factor, bn.eps,
                                  P(st.scale), P(st.shift), P(st.mean), P(st.invstd), nbt_in, rm_new, rv_new, nbt_new,
                                  d.stream),
          "bn finalize (sync)");
  } else {
    check(dgx_bn_finalize_out_f32(P(pr.first), pr.second, co, count, P(gamma), P(beta), rm, rv, factor, bn.eps,
                                  P(st.scale), P(st.shift), P(st.mean), P(st.invstd), nbt_in, rm_new, rv_new, nbt_new,
                                  d.stream),
          "bn finalize");
  }
  if (nbt_tmp.defined()) bn.nbt.copy_(nbt_tmp);
  return st;
}

// eval-mode affine from the running statistics
Stats running_stats(const Dev& d, const Tensor& gamma, const Tensor& beta, const BnSpec& bn) {
  const int co = (int)gamma.size(0);
  TORCH_CHECK(bn.rm.defined() && bn.rv.defined(), "dgx: running statistics missing for an eval-mode BatchNorm");
  Stats st;
  st.scale = at::empty({co}, d.f32);
  st.shift = at::empty({co}, d.f32);
  check(dgx_bn_eval_affine_f32(co, P(gamma), P(beta), P(bn.rm), P(bn.rv), bn.eps, P(st.scale), P(st.shift), d.stream),
        "bn eval affine");
  st.mean = bn.rm.detach().clone();
  st.invstd = at::rsqrt(bn.rv.detach() + bn.eps);
  st.eval = true;
  return st;
}

// (dgamma, dbeta, c0, c1) from (sum g, sum g*yhat) partials
std::array<Tensor, 4> backward_consts(const Dev& d, const Tensor& partials, int rows, double count, const Stats& st) {
  const int co = (int)st.scale.size(0);
  std::array<Tensor, 4> r{at::empty({co}, d.f32), at::empty({co}, d.f32), at::empty({co}, d.f32),
                          at::empty({co}, d.f32)};
  auto pr = compact(d, partials, rows, co);
  if (st.group.empty()) {
    check(dgx_bn_bwd_finalize_f32(P(pr.first), pr.second, co, count, P(st.scale), P(st.mean), P(st.invstd), P(r[0]),
                                  P(r[1]), P(r[2]), P(r[3]), 0, d.stream),
          "bn bwd finalize");
    if (st.eval) {
      r[2].zero_();
      r[3].zero_();
    }
  } else {  // SyncBatchNorm: input gradient from global sums, gamma/beta gradients rank-local
    Tensor sums = allreduce_sums(d, pr.first, pr.second, co, count, st.group);
    check(dgx_bn_bwd_finalize_f64(P<double>(sums), 1, co, -1.0, P(st.scale), P(st.mean), P(st.invstd), nullptr,
                                  nullptr, P(r[2]), P(r[3]), 0, d.stream),
          "bn bwd finalize (sync)");
    Tensor loc = pr.first.view({-1, 2, co}).narrow(0, 0, pr.second).to(at::kDouble).sum(0);
    r[1].copy_(loc[0]);
    r[0].copy_(loc[1]);
  }
  return r;
}

// ----------------------------------------------------------------- GEMMs ----
// Weight-gradient slab sums of one backward, deferred to as few launches as
// possible (dgx_slab_reduce_multi_f32: each element summed in
// dgx_slab_reduce_f32's order, so the gradients are those of per-GEMM reduces)
struct SlabJobs {
  std::vector<Tensor> slab, out;
  std::vector<int> S, rows, cols, split;
  std::vector<int64_t> ldo;
  void add(const Dev& d, const Tensor& sl, int s, int r, int cl, int sp, const Tensor& o) {
    if ((int)slab.size() == 8) flush(d.stream);
    slab.push_back(sl);
    out.push_back(o);
    S.push_back(s);
    rows.push_back(r);
    cols.push_back(cl);
    split.push_back(sp);
    ldo.push_back(o.stride(0));
  }
  void flush(void* stream) {
    const int n = (int)slab.size();
    if (n == 0) return;
    std::vector<const float*> sp(n);
    std::vector<float*> op(n);
    for (int j = 0; j < n; ++j) {
      sp[j] = static_cast<const float*>(slab[j].data_ptr());
      op[j] = static_cast<float*>(out[j].data_ptr());
    }
    check(dgx_slab_reduce_multi_f32(n, sp.data(), S.data(), rows.data(), cols.data(), split.data(), op.data(),
                                    ldo.data(), stream),
          "slab reduce (multi)");
    slab.clear();
    out.clear();
    S.clear();
    rows.clear();
    cols.clear();
    split.clear();
    ldo.clear();
  }
};

void reduce_slab(const Dev& d, const Tensor& slab, int used, int M, int N, int split, Tensor& out, SlabJobs* defer) {
  TORCH_CHECK(out.scalar_type() == at::kFloat && out.dim() == 2 && (out.stride(1) == 1 || out.size(1) == 1),
              "dgx gemm: output must be a row-major fp32 view");
  if (defer) {
    defer->add(d, slab, used, M, N, split, out);
    return;
  }
  check(dgx_slab_reduce_f32(P(slab), used, M, N, split, P(out), out.stride(0), d.stream), "slab reduce");
}

// row stride of a 2-D row-major fp32 / bf16 operand
int64_t ld2(const Tensor& t) {
  TORCH_CHECK(t.dim() == 2 && (t.stride(1) == 1 || t.size(1) == 1),
              "dgx gemm: operand must be a 2-D row-major view, got strides ", t.strides());
  TORCH_CHECK(t.scalar_type() == at::kFloat || t.scalar_type() == at::kBFloat16, "dgx gemm: fp32/bf16 operands only");
  return t.size(0) > 1 ? t.stride(0) : std::max<int64_t>(1, t.size(1));
}
// row stride of a bf16 operand of the LDS-DMA path
int64_t ld16(const Tensor& t) {
  TORCH_CHECK(t.scalar_type() == at::kBFloat16 && t.dim() == 2 && (t.stride(1) == 1 || t.size(1) == 1),
              "dgx gemm (bf16 path): operands must be row-major bf16 2-D views");
  return t.size(0) > 1 ? t.stride(0) : std::max<int64_t>(8, t.size(1));
}
bool is16(const Tensor& t) { return t.scalar_type() == at::kBFloat16; }

// register-staged bf16 MFMA GEMM, fp32 or bf16 operands
void gemm16(const Dev& d, const Tensor& a, bool a_ic, const Tensor& b, bool b_ic, int M, int N, int K, int epi,
            float* out, int64_t ldc, float* part, int splits) {
  check(dgx_gemm_bf16(a.data_ptr(), is16(a), a_ic, ld2(a), b.data_ptr(), is16(b), b_ic, ld2(b), M, N, K, epi, splits,
                      out, ldc, part, d.stream),
        "gemm bf16");
}

// out (M,N) = x (M,K) w (N,K)^T (+ BN column partials)
Tensor mm_xwt(const Dev& d, const Tensor& x, const Tensor& w, Tensor* part, Tensor* out_view = nullptr) {
  const int M = (int)x.size(0), K = (int)x.size(1), N = (int)w.size(0);
  Tensor out = out_view ? *out_view : at::empty({M, N}, d.f32);
  TORCH_CHECK(out.scalar_type() == at::kFloat && out.dim() == 2 && (out.stride(1) == 1 || N == 1),
              "dgx gemm: output must be a row-major fp32 view");
  if (part) *part = at::empty({dgx_gemm_stats_rows(M), 2, N}, d.f32);
  gemm16(d, x, false, w, false, M, N, K, part ? kEpiStats : kEpiStore, P(out), out.stride(0), part ? P(*part) : nullptr,
         1);
  return out;
}

// out (M,N) (+)= x (M,K) w (K,N)
void mm_xw(const Dev& d, const Tensor& x, const Tensor& w, Tensor& out, bool accumulate) {
  const int M = (int)x.size(0), K = (int)x.size(1), N = (int)w.size(1);
  TORCH_CHECK(out.scalar_type() == at::kFloat && out.dim() == 2 && (out.stride(1) == 1 || N == 1),
              "dgx gemm: output must be a row-major fp32 view");
  gemm16(d, x, false, w, true, M, N, K, accumulate ? kEpiAccum : kEpiStore, P(out), out.stride(0), nullptr, 1);
}

// out = a^T b for a (R, M), b (R, N): split-K slabs, fixed-order sum; split_rows un-stacks [W1;W2]
void mm_atb(const Dev& d, const Tensor& a, const Tensor& b, Tensor& out, int split_rows, SlabJobs* defer) {
  const int R = (int)a.size(0), M = (int)a.size(1), N = (int)b.size(1);
  const int S = dgx_gemm_splits(M, N, R);
  Tensor slab = at::empty({S, M, N}, d.f32);
  gemm16(d, a, true, b, true, M, N, R, kEpiSlab, P(slab), N, nullptr, S);
  reduce_slab(d, slab, dgx_gemm_slabs(R, S), M, N, split_rows > 0 ? split_rows : M, out, defer);
}

// out (M,N) = a (M,K) b (K,N), fp32 or bf16 operands rounded to bf16 while staged; transposed
// views are read in place, the weight-gradient form (a long reduction over rows) is split-K
Tensor mm16(const Dev& d, Tensor a, Tensor b) {
  const int M = (int)a.size(0), K = (int)a.size(1), N = (int)b.size(1);
  if (a.stride(1) != 1 && a.stride(0) != 1) a = a.contiguous();
  if (b.stride(1) != 1 && b.stride(0) != 1) b = b.contiguous();
  const bool a_ic = a.stride(1) != 1, b_ic = b.stride(1) == 1;
  Tensor A = a_ic ? a.t() : a, Bv = b_ic ? b : b.t();
  Tensor out = at::empty({M, N}, d.f32);
  if (K >= 2048 && a_ic && b_ic)
    mm_atb(d, A, Bv, out, 0, nullptr);
  else
    gemm16(d, A, a_ic, Bv, b_ic, M, N, K, kEpiStore, P(out), out.stride(0), nullptr, 1);
  return out;
}

// whether the LDS-DMA path takes this k-contiguous bf16 operand
bool lds_ok(const Tensor& x16, int64_t K) {
  return x16.defined() && x16.numel() && is16(x16) && K % 64 == 0 && x16.stride(0) % 8 == 0 &&
         reinterpret_cast<uintptr_t>(x16.data_ptr()) % 16 == 0;
}

// out (M,N) = x16 (M,K) w16 (N,Kw)^T (Kw = 2K: split weight [hi | lo]);
// part: BN column partials (with out_bf16 the product is stored bf16); addend: out = addend + ...
Tensor lds_xwt(const Dev& d, const Tensor& x16, const Tensor& w16, Tensor* part, bool out_bf16,
               const Tensor* addend = nullptr, Tensor* out_view = nullptr) {
  const int M = (int)x16.size(0), K = (int)x16.size(1), N = (int)w16.size(0), Kw = (int)w16.size(1);
  TORCH_CHECK(Kw == K || Kw == 2 * K, "dgx gemm: weight k extent does not match the operand's");
  TORCH_CHECK(!out_bf16 || part, "dgx gemm: a bf16 product is only stored together with its statistics");
  Tensor out = out_view ? *out_view : at::empty({M, N}, out_bf16 ? d.bf16 : d.f32);
  TORCH_CHECK(out.scalar_type() == (out_bf16 ? at::kBFloat16 : at::kFloat) && out.dim() == 2 && out.stride(1) == 1,
              "dgx gemm: output view dtype/layout does not match the epilogue");
  TORCH_CHECK(!addend || (addend->scalar_type() == at::kFloat && addend->dim() == 2 && addend->stride(1) == 1),
              "dgx gemm: addend must be a row-major fp32 view");
  if (part) *part = at::empty({dgx_gemm_stats_rows(M), 2, N}, d.f32);
  const int epi = part ? (out_bf16 ? kEpiStats16 : kEpiStats) : (addend ? kEpiAccum : kEpiStore);
  check(dgx_gemm_lds_bf16(x16.data_ptr(), ld16(x16), w16.data_ptr(), ld16(w16), 0, M, N, Kw, K, epi, 1, P(out),
                          out.stride(0), part ? P(*part) : nullptr, addend ? P(*addend) : nullptr,
                          addend ? addend->stride(0) : 0, d.stream),
        "gemm lds nt");
  return out;
}

// out = a16^T b16 (split-K slabs, the small-output slab cap)
void lds_atb(const Dev& d, const Tensor& a16, const Tensor& b16, Tensor& out, int split_rows, int64_t slab_cap_mb,
             SlabJobs* defer) {
  const int R = (int)a16.size(0), M = (int)a16.size(1), N = (int)b16.size(1);
  int S = dgx_gemm_splits(M, N, R);
  const int64_t bytes = (int64_t)M * N * 4;
  if (slab_cap_mb > 0 && bytes < (1 << 20)) S = (int)std::max<int64_t>(1, std::min<int64_t>(S, (slab_cap_mb << 20) / bytes));
  const int used = dgx_gemm_lds_slabs(R, S);
  Tensor slab = at::empty({used, M, N}, d.f32);
  check(dgx_gemm_lds_bf16(a16.data_ptr(), ld16(a16), b16.data_ptr(), ld16(b16), 1, M, N, R, R, kEpiSlab, S, P(slab), N,
                          nullptr, nullptr, 0, d.stream),
        "gemm lds tn");
  reduce_slab(d, slab, used, M, N, split_rows > 0 ? split_rows : M, out, defer);
}

// out = sum_i a_i^T b_i over the pairs (same shapes): every pair's split-K slabs in
// one buffer, summed by one fixed-order reduce (the fp32 mode's 3-pass weight gradients)
void lds_atb_sum(const Dev& d, const std::vector<std::pair<Tensor, Tensor>>& ab, Tensor& out, SlabJobs* defer) {
  const int R = (int)ab[0].first.size(0), M = (int)ab[0].first.size(1), N = (int)ab[0].second.size(1);
  const int S = dgx_gemm_splits(M, N, R);
  const int used = dgx_gemm_lds_slabs(R, S);
  const int n = (int)ab.size();
  Tensor slab = at::empty({(int64_t)n * used, M, N}, d.f32);
  for (int i = 0; i < n; ++i) {
    const Tensor &a16 = ab[i].first, &b16 = ab[i].second;
    check(dgx_gemm_lds_bf16(a16.data_ptr(), ld16(a16), b16.data_ptr(), ld16(b16), 1, M, N, R, R, kEpiSlab, S,
                            P(slab) + (int64_t)i * used * M * N, N, nullptr, nullptr, 0, d.stream),
          "gemm lds tn");
  }
  reduce_slab(d, slab, n * used, M, N, M, out, defer);
}

// fp32 -> (hi, lo) bf16 planes (dgx_split_bf16)
std::pair<Tensor, Tensor> split16(const Dev& d, const Tensor& x) {
  const int64_t M = x.size(0), K = x.size(1);
  Tensor hi = at::empty({M, K}, d.bf16), lo = at::empty({M, K}, d.bf16);
  check(dgx_split_bf16(P(x), M > 1 ? x.stride(0) : K, M, (int)K, hi.data_ptr(), lo.data_ptr(), K, d.stream),
        "split bf16");
  return {hi, lo};
}

// whether dgx_gemm_edge_dz_bf16 takes this block's input-gradient GEMM (dX columns = cin, K = dPQ width)
bool edge_dz_ok(const Tensor& dpq16, int cin) {
  const int64_t K = dpq16.size(1);
  return is16(dpq16) && cin % 8 == 0 && cin <= 128 && K % 64 == 0 && dpq16.stride(0) % 8 == 0 &&
         reinterpret_cast<uintptr_t>(dpq16.data_ptr()) % 16 == 0;
}

// (tensor, ic, ld) of an fp32 operand read in place; kd = the dim holding "k"
struct Op32 {
  Tensor t;
  int ic;
  int64_t ld;
};
Op32 op32(Tensor t, int kd) {
  if (t.scalar_type() != at::kFloat) t = t.to(at::kFloat);
  const int od = 1 - kd;
  if (t.stride(kd) == 1 || t.size(kd) == 1)
    return {t, 0, t.size(od) > 1 ? std::max<int64_t>({t.stride(od), t.size(kd), 1}) : std::max<int64_t>(t.size(kd), 1)};
  if (t.stride(od) == 1 || t.size(od) == 1)
    return {t, 1, t.size(kd) > 1 ? std::max<int64_t>({t.stride(kd), t.size(od), 1}) : std::max<int64_t>(t.size(od), 1)};
  t = kd == 1 ? t.contiguous() : t.t().contiguous().t();
  return op32(t, kd);
}

// out (M,N) (+)= a (M,K) b (K,N) on the fp32 MFMA GEMM (parity mode); addend: out = addend + a b;
// a long reduction over few outputs (the weight gradients) is split-K, summed in a fixed order
Tensor mm32(const Dev& d, const Tensor& a, const Tensor& b, Tensor* out_view, bool accumulate,
            const Tensor* addend = nullptr) {
  const int M = (int)a.size(0), K = (int)a.size(1), N = (int)b.size(1);
  TORCH_CHECK(b.size(0) == K, "dgx mm32: inner dims differ");
  Op32 A = op32(a, 1), Bo = op32(b, 0);
  Tensor out = out_view ? *out_view : at::empty({M, N}, d.f32);
  TORCH_CHECK(out.scalar_type() == at::kFloat && out.dim() == 2 && (out.stride(1) == 1 || N == 1),
              "dgx mm32: output must be a row-major fp32 2-D view");
  TORCH_CHECK(!addend || (addend->scalar_type() == at::kFloat && addend->dim() == 2 && addend->stride(1) == 1),
              "dgx mm32: addend must be a row-major fp32 view");
  const int S = (K >= 2048 && !accumulate && !addend) ? dgx_gemm_f32_splits(M, N, K) : 1;
  if (S > 1) {
    const int used = dgx_gemm_f32_slabs(K, S);
    Tensor slab = at::empty({used, M, N}, d.f32);
    check(dgx_gemm_f32(P(A.t), A.ic, (int)A.ld, P(Bo.t), Bo.ic, (int)Bo.ld, M, N, K, kEpiSlab, S, P(slab), N, nullptr, 0,
                       d.stream),
          "gemm f32 (split-K)");
    check(dgx_slab_reduce_f32(P(slab), used, M, N, M, P(out), out.stride(0), d.stream), "slab reduce");
  } else {
    check(dgx_gemm_f32(P(A.t), A.ic, (int)A.ld, P(Bo.t), Bo.ic, (int)Bo.ld, M, N, K,
                       (accumulate || addend) ? kEpiAccum : kEpiStore, 1, P(out), M > 1 ? out.stride(0) : std::max(N, 1),
                       addend ? P(*addend) : nullptr, addend ? addend->stride(0) : 0, d.stream),
          "gemm f32");
  }
  return out;
}

// out (M, N) = a^T b over the R rows of a (R, M) and b (R, N) on the fp32 MFMA
// GEMM (the parity mode's weight gradients): split-K slabs summed in a fixed
// order — deferred into the backward's one multi-job reduce — with split_rows
// un-stacking [W1; W2] into the reference layout [W1 | W2] (no cat)
void mm32_atb(const Dev& d, const Tensor& a, const Tensor& b, Tensor& out, int split_rows, SlabJobs* defer) {
  const int R = (int)a.size(0), M = (int)a.size(1), N = (int)b.size(1);
  TORCH_CHECK(b.size(0) == R, "dgx mm32_atb: row counts differ");
  Op32 A = op32(a.t(), 1), Bo = op32(b, 0);
  const int S = dgx_gemm_f32_splits(M, N, R);
  const int used = dgx_gemm_f32_slabs(R, S);
  Tensor slab = at::empty({used, M, N}, d.f32);
  check(dgx_gemm_f32(P(A.t), A.ic, (int)A.ld, P(Bo.t), Bo.ic, (int)Bo.ld, M, N, R, kEpiSlab, S, P(slab), N, nullptr, 0,
                     d.stream),
        "gemm f32 (split-K)");
  reduce_slab(d, slab, used, M, N, split_rows > 0 ? split_rows : M, out, defer);
}

// reference conv weight (Co, 2C[,1,1]) = [W1 | W2] -> stacked [W1; W2] (2Co, C) (dgx.edgeconv.split_weight)
Tensor split_weight(const Tensor& w, int cin, int co) {
  Tensor r = w.reshape({co, 2 * cin});
  return at::cat({r.narrow(1, 0, cin), r.narrow(1, cin, cin)}, 0).contiguous();
}

// -------------------------------------------------------- bf16 weight prep ----
// one bf16 buffer, per job (nt (R, [2]C), tn (C, R)), 16-byte aligned views (dgx.gemm.prep_layout restates
// this layout for the tracing paths; dgx_host::weight_prep_layout reports it and a test holds the two equal)
struct PrepJob {
  Tensor w;
  int rows, cols;
  bool stacked, split;
  bool tsplit = false;   // tn as [hi^T | lo^T] too
};
std::vector<std::pair<Tensor, Tensor>> prep_views(const Tensor& buf, const std::vector<PrepJob>& jobs,
                                                  int64_t* total_out = nullptr) {
  std::vector<std::pair<Tensor, Tensor>> v;
  int64_t total = 0;
  for (const auto& j : jobs) {
    const int64_t R = j.stacked ? 2 * j.rows : j.rows;
    const int64_t n_tn = (j.tsplit ? 2 : 1) * R * j.cols, n_nt = (j.split ? 2 : 1) * R * j.cols;
    const int64_t p_nt = cdiv(n_nt, 8) * 8, p_tn = cdiv(n_tn, 8) * 8;
    if (buf.defined())
      v.emplace_back(buf.narrow(0, total, n_nt).view({R, j.split ? 2 * j.cols : j.cols}),
                     buf.narrow(0, total + p_nt, n_tn).view({j.cols, j.tsplit ? 2 * R : R}));
    total += p_nt + p_tn;
  }
  if (total_out) *total_out = total;
  return v;
}

// one weight's bf16 copies: (nt (R, cols), tn (cols, R)), R = 2 rows for a stacked EdgeConv weight [W1; W2]
std::pair<Tensor, Tensor> prep_weight(const Dev& d, const Tensor& w, int rows, int cols, bool stacked = false) {
  TORCH_CHECK(w.scalar_type() == at::kFloat, "dgx weight prep: fp32 weights expected");
  const int R = stacked ? 2 * rows : rows;
  Tensor nt = at::empty({R, cols}, d.bf16), tn = at::empty({cols, R}, d.bf16);
  Tensor wc = w.contiguous();
  check(dgx_weight_prep_bf16(P(wc), rows, cols, stacked, nt.data_ptr(), tn.data_ptr(), d.stream), "weight prep");
  return {nt, tn};
}

// every job's bf16 copies in one launch, into `buf` when given
std::pair<Tensor, std::vector<std::pair<Tensor, Tensor>>> prep_weights(const Dev& d, const std::vector<PrepJob>& jobs,
                                                                       Tensor buf = Tensor()) {
  TORCH_CHECK(jobs.size() <= 8, "dgx weight prep: at most 8 weights per launch");
  int64_t total = 0;
  prep_views(Tensor(), jobs, &total);
  if (!buf.defined()) buf = at::empty({total}, d.bf16);
  TORCH_CHECK(buf.numel() == total && buf.scalar_type() == at::kBFloat16 && buf.is_contiguous(),
              "dgx weight prep: buffer does not match the jobs' layout");
  auto views = prep_views(buf, jobs);
  const int n = (int)jobs.size();
  std::vector<Tensor> keep(n);
  std::vector<const float*> W(n);
  std::vector<void*> NT(n), TN(n);
  std::vector<int> CO(n), CI(n), ST(n);
  for (int j = 0; j < n; ++j) {
    TORCH_CHECK(jobs[j].w.scalar_type() == at::kFloat, "dgx weight prep: fp32 weights expected");
    keep[j] = jobs[j].w.detach().contiguous();
    W[j] = P(keep[j]);
    NT[j] = views[j].first.data_ptr();
    TN[j] = views[j].second.data_ptr();
    CO[j] = jobs[j].rows;
    CI[j] = jobs[j].cols;
    ST[j] = (int)jobs[j].stacked | (2 * (int)jobs[j].split) | (4 * (int)jobs[j].tsplit);
  }
  check(dgx_weight_prep_multi_bf16(n, W.data(), CO.data(), CI.data(), ST.data(), NT.data(), TN.data(), d.stream),
        "weight prep");
  return {buf, views};
}

// ------------------------------------------------------------------- kNN ----
// (xx, image) scratch of one fused-kernel kNN call: dgx_knn_prepare_f32's outputs, or a producer kernel's
std::pair<Tensor, Tensor> knn_image_buffers(const at::TensorOptions& f32, int B, int C, int N) {
  const size_t img_bytes = dgx_knn_image_bytes(B, C, N);
  return {at::empty({(int64_t)B * N}, f32), at::empty({(int64_t)((std::max<size_t>(img_bytes, 4) + 3) / 4)}, f32)};
}

// the reference's sum(x**2, dim=1) rounding order for x's strides (dgx.ops.reduction_order)
int reduction_order(const Tensor& x) {
  return (x.size(1) > 1 && x.size(2) > 1 && x.stride(1) < x.stride(2)) ? DGX_ORDER_VEC8X4 : DGX_ORDER_STRIDED;
}

// The kNN dispatch: (ids (B,N,k) of type `ids`, the selected values or an undefined tensor) of a (B,C,N) fp32
// view. The fused kernel unless the shape or `generic` asks for the other; prepared: its |x|^2 + operand image,
// already written. Every check comes before the first allocation or launch.
std::pair<Tensor, Tensor> knn(const Dev& d, const Tensor& xv, int k, int order, at::ScalarType ids, bool values,
                              bool generic, const std::pair<Tensor, Tensor>* prepared) {
  const int B = (int)xv.size(0), C = (int)xv.size(1), N = (int)xv.size(2);
  TORCH_CHECK(k >= 1 && k <= N, "knn: selected index k out of range (k=", k, ", N=", N, ")");
  generic = generic || !dgx_knn_fast_shape(C, k, N);
  TORCH_CHECK(!(generic && prepared), "knn: prepared operands exist for the fused kernel's shapes only");
  TORCH_CHECK_NOT_IMPLEMENTED(!generic || k <= dgx_knn_generic_max_k(), "dgx knn: k = ", k, " > ",
                              dgx_knn_generic_max_k(), " neighbours");
  const size_t img_bytes = generic ? 0 : dgx_knn_image_bytes(B, C, N);
  TORCH_CHECK(!prepared || (prepared->first.numel() == (int64_t)B * N &&
                            (size_t)prepared->second.numel() * 4 >= img_bytes),
              "knn: prepared |x|^2 / image buffers do not match the cloud");
  Tensor idx = at::empty({B, N, k}, ids == at::kLong ? d.i64 : d.i32);
  Tensor vals = values ? at::empty({B, N, k}, d.f32) : Tensor();
  int64_t* i64 = ids == at::kLong ? P<int64_t>(idx) : nullptr;
  int32_t* i32 = ids == at::kLong ? nullptr : P<int32_t>(idx);
  if (generic) {   // same values, same canonical order; a view with neither inner stride 1 is read from a copy
    Tensor x = xv;
    if (x.stride(2) != 1 && x.stride(1) != 1) x = x.contiguous();
    const size_t ws_bytes = dgx_knn_generic_workspace_bytes(B, C, N);
    Tensor ws = at::empty({(int64_t)((ws_bytes + 3) / 4)}, d.f32);
    check(dgx_knn_generic_f32(P(x), x.stride(0), x.stride(1), x.stride(2), B, C, N, k, order, i64, i32, P(vals),
                              P(ws), ws_bytes, d.stream),
          "knn (generic)");
    return {idx, vals};
  }
  const float* xp = static_cast<const float*>(xv.data_ptr());
  std::pair<Tensor, Tensor> bufs;
  if (prepared) {
    bufs = *prepared;
  } else {   // |x|^2 and the MFMA operand image in one pass over x
    bufs = knn_image_buffers(d.f32, B, C, N);
    check(dgx_knn_prepare_f32(xp, xv.stride(0), xv.stride(1), xv.stride(2), B, C, N, order, P(bufs.first),
                              P(bufs.second), img_bytes, d.stream),
          "knn prepare");
  }
  KnnRec rec{};
  if (t_knn_timing) {
    (void)hipEventCreate(&rec.e0);
    (void)hipEventCreate(&rec.e1);
    (void)hipEventRecord(rec.e0, static_cast<hipStream_t>(d.stream));
  }
  check(dgx_knn_select_f32(xp, xv.stride(0), xv.stride(1), xv.stride(2), P(bufs.first), B, C, N, k, i64, i32, P(vals),
                           P(bufs.second), img_bytes, d.stream),
        "knn");
  if (t_knn_timing) {
    (void)hipEventRecord(rec.e1, static_cast<hipStream_t>(d.stream));
    rec.flops = 2.0 * B * (double)N * N * C;
    rec.B = B;
    rec.C = C;
    rec.N = N;
    rec.k = k;
    t_knn_recs.push_back(rec);
  }
  return {idx, vals};
}

// Reverse kNN graphs (CSR of in-edges: rowptr (M+1), edges (M k)) of same-shaped int32 (B,N,k) graphs, 8 per
// launch (dgx_graph_reverse_multi's limit): the graphs' workgroups share the chip
std::pair<std::vector<Tensor>, std::vector<Tensor>> reverse_graphs(const Dev& d, const std::vector<Tensor>& idxs, int B,
                                                                   int N, int k) {
  const int n = (int)idxs.size();
  const int64_t M = (int64_t)B * N;
  std::vector<Tensor> rowptr(n), edges(n);
  for (int base = 0; base < n; base += 8) {
    const int m = std::min(8, n - base);
    std::vector<const int32_t*> ip(m);
    std::vector<int32_t*> rp(m), ep(m);
    for (int j = 0; j < m; ++j) {
      rowptr[base + j] = at::empty({M + 1}, d.i32);
      edges[base + j] = at::empty({M * k}, d.i32);
      ip[j] = P<int32_t>(idxs[base + j]);
      rp[j] = P<int32_t>(rowptr[base + j]);
      ep[j] = P<int32_t>(edges[base + j]);
    }
    check(dgx_graph_reverse_multi(m, ip.data(), B, N, k, rp.data(), ep.data(), d.stream), "reverse graphs");
  }
  return {rowptr, edges};
}

// --------------------------------------------------------- EdgeConv chain ----
struct Layer {
  Tensor w, gamma, beta;   // conv weight (Co, 2C[,1,1]) as applied to (x_j, x_i), BN affine
  BnSpec bn;
  double slope = 0.2;
  int cin = 0, co = 0;
};

// the fp32 mode's stacked weights [W1; W2] of the blocks `need` selects, in one
// launch (dgx_weight_stack_multi_f32; <= 8 per launch); others stay undefined
std::vector<Tensor> stack_weights_f32(const Dev& d, const std::vector<Layer>& L, const std::vector<bool>& need) {
  std::vector<Tensor> out(L.size());
  std::vector<const float*> W;
  std::vector<float*> O;
  std::vector<int> Co, C;
  auto flush = [&]() {
    if (W.empty()) return;
    check(dgx_weight_stack_multi_f32((int)W.size(), W.data(), Co.data(), C.data(), O.data(), d.stream),
          "weight stack");
    W.clear();
    O.clear();
    Co.clear();
    C.clear();
  };
  for (size_t l = 0; l < L.size(); ++l) {
    if (!need[l]) continue;
    const Layer& ly = L[l];
    TORCH_CHECK(ly.w.is_contiguous(), "dgx: contiguous conv weights expected");
    out[l] = at::empty({2 * ly.co, ly.cin}, d.f32);
    W.push_back(P(ly.w));
    O.push_back(P(out[l]));
    Co.push_back(ly.co);
    C.push_back(ly.cin);
    if (W.size() == 8) flush();
  }
  flush();
  return out;
}

// a chain's saved list: x_pm, then per block these fields (dgx.schedule.CHAIN_FIELDS)
enum ChainField { kIdx, kPQ, kYsel, kArg, kSumP, kScale, kShift, kMean, kInvstd, kPerLayer };
const char* const kChainNames[kPerLayer] = {"idx", "PQ", "ysel", "arg", "sumP", "scale", "shift", "mean", "invstd"};
const Tensor& field(const std::vector<Tensor>& saved, int l, ChainField f) { return saved[1 + kPerLayer * l + f]; }

struct ChainOut {
  Tensor xcat, xcat16, prep;        // xcat16 / prep empty when not made
  std::vector<Tensor> saved;        // x_pm + kPerLayer per block (empty tensors for non-selecting blocks)
  std::vector<Stats> stats;
  bool have16 = false;
};

// Whether block li's GEMMs read the bf16 twin + bf16 weight copies (forward and backward agree)
bool block_uses_prep(bool bf16, int li, bool prev_selecting, int cin, int64_t total, int64_t off_in) {
  return bf16 && li > 0 && prev_selecting && cin % 64 == 0 && total % 8 == 0 && off_in % 8 == 0;
}

std::vector<PrepJob> chain_prep_jobs(const std::vector<Layer>& L) {
  std::vector<PrepJob> jobs;
  for (size_t li = 1; li < L.size(); ++li) jobs.push_back({L[li].w, L[li].co, L[li].cin, true, true});
  return jobs;
}

// The block chain of dgcnn.py:84-100 (dgx.edgeconv): activations point-major in ONE
// concat buffer xcat (B*N, sum Co); block l reads its input as a column slice and
// writes its output into its own slice (torch.cat of dgcnn.py:100 is free).
ChainOut chain_forward_impl(const Dev& d, const Tensor& x_in, int k, std::vector<Layer>& L, bool bf16, bool need_grad,
                            const std::vector<std::pair<Tensor, Tensor>>* preps_in, const Tensor& idx0,
                            const Opts& o) {
  Tensor x = x_in.scalar_type() == at::kFloat ? x_in : x_in.to(at::kFloat);
  const int B = (int)x.size(0), C0 = (int)x.size(1), N = (int)x.size(2);
  const int64_t M = (int64_t)B * N;
  const int n = (int)L.size();
  int64_t total = 0;
  for (auto& ly : L) total += ly.co;
  if (need_grad) {
    // the backward's pull scatter stages a cloud's one-channel slices in LDS: a
    // cloud it cannot take is refused here, before the forward has run.
    // One block stands for all: the scatter doubles its point parts until the
    // slice fits or parts * 64 >= N, an end state the channel count does not change.
    const int pk = (bf16 || o.split32) && o.packed;
    if (!L.empty())
      TORCH_CHECK(dgx_edge_bwd_scatter_fits(B, N, L[0].co, pk),
                  "dgx chain: the EdgeConv backward takes at most N = ", dgx_edge_bwd_scatter_max_n(B, L[0].co, pk),
                  " points per cloud (B = ", B, ", ", pk ? "packed dz" : "dz + slot bytes", "), got N = ", N,
                  "; larger clouds run forward-only (torch.no_grad)");
  }
  ChainOut r;
  r.xcat = at::empty({M, total}, d.f32);
  Tensor xcat16 = bf16 ? at::empty({M, total}, d.bf16) : Tensor();
  Tensor x_pm = x.permute({0, 2, 1}).reshape({M, C0}).contiguous();
  r.saved.push_back(x_pm);
  std::vector<std::pair<Tensor, Tensor>> preps;
  if (preps_in) {
    preps = *preps_in;
  } else if (bf16 && n > 1) {
    auto pw = prep_weights(d, chain_prep_jobs(L));
    r.prep = pw.first;
    preps = pw.second;
  }
  const double count = (double)M * k;
  std::vector<Tensor> w32;   // fp32 mode: every block's stacked weight, one launch
  if (!bf16) {
    std::vector<bool> need(n);
    for (int l = 0; l < n; ++l) need[l] = L[l].cin > kSmallKMax;
    w32 = stack_weights_f32(d, L, need);
  }
  bool have16 = false, prev_selecting = false;
  std::pair<Tensor, Tensor> next_prepared;
  bool have_prepared = false;
  int64_t off_in = 0, off = 0;
  for (int li = 0; li < n; ++li) {
    Layer& ly = L[li];
    const int cin = ly.cin, co = ly.co;
    Tensor X, idx, PQ;
    if (li == 0) {
      TORCH_CHECK(cin == C0, "dgx chain: block 1 takes the cloud's ", C0, " channels, its weight ", cin);
      X = x_pm;
      if (idx0.defined()) {
        TORCH_CHECK(idx0.scalar_type() == at::kInt && idx0.is_contiguous() && idx0.size(0) == B && idx0.size(1) == N &&
                        idx0.size(2) == k,
                    "dgx chain: idx0 must be contiguous int32 (B, N, k)");
        idx = idx0;
      } else {
        idx = knn(d, x, k, reduction_order(x), at::kInt, false, false, nullptr).first;
      }
    } else {
      X = r.xcat.narrow(1, off_in, cin);
      // blocks 2-4 see contiguous (B,C,N) features (max over dim -1), hence the strided order
      Tensor xv = r.xcat.as_strided({B, cin, N}, {N * total, 1, total}, r.xcat.storage_offset() + off_in);
      idx = knn(d, xv, k, DGX_ORDER_STRIDED, at::kInt, false, false, have_prepared ? &next_prepared : nullptr).first;
    }
    have_prepared = false;
    if (cin <= kSmallKMax) {
      // raw coordinates (block 1, K = 3): exact fp32 in every mode, the reference weight layout read as is
      Tensor wr = ly.w.reshape({co, 2 * cin}).contiguous();
      PQ = at::empty({M, 2 * co}, d.f32);
      Tensor Xc = X.stride(1) == 1 ? X : X.contiguous();
      check(dgx_gemm_smallk_split_f32(P(Xc), M > 1 ? Xc.stride(0) : cin, P(wr), (int)M, co, cin, P(PQ), 2 * co, d.stream),
            "gemm small-k");
    } else if (bf16) {
      Tensor X16 = li > 0 ? xcat16.narrow(1, off_in, cin) : Tensor();
      if (have16 && block_uses_prep(bf16, li, prev_selecting, cin, total, off_in) && lds_ok(X16, cin) &&
          (int)preps.size() >= li) {
        PQ = lds_xwt(d, X16, preps[li - 1].first, nullptr, false);   // split weight [hi | lo]: 16 significant bits
      } else {
        PQ = mm_xwt(d, X, split_weight(ly.w, cin, co), nullptr);   // fp32 operands rounded while staged
      }
    } else {
      PQ = mm32(d, X, w32[li].t(), nullptr, false);
    }
    float* out = P(r.xcat) + off;
    void* out16 = bf16 ? static_cast<void*>(static_cast<at::BFloat16*>(xcat16.data_ptr()) + off) : nullptr;
    const bool use_batch = ly.bn.use_batch();
    if (use_batch || need_grad) {
      Tensor ysel = at::empty({M, co}, d.f32), arg = at::empty({M, co}, d.u8), sumP = at::empty({M, co}, d.f32);
      const int prow = dgx_edge_partials_rows(B, N, co);
      Tensor partials = at::empty({prow, 2, co}, d.f32);
      check(dgx_edge_fwd_gather_f32(P(PQ), (int)PQ.stride(0), P<int32_t>(idx), B, N, k, co, P(ly.gamma), P(ysel),
                                    P<uint8_t>(arg), P(sumP), P(partials), prow, d.stream),
            "edge gather");
      Stats st = use_batch ? batch_stats(d, partials, prow, count, ly.gamma, ly.beta, ly.bn)
                           : running_stats(d, ly.gamma, ly.beta, ly.bn);
      if (o.fuse_image && li + 1 < n && (co == 64 || co == 128) && N % 32 == 0 && dgx_knn_fast_shape(co, k, N)) {
        // the apply also writes the next block's kNN |x|^2 and operand image
        next_prepared = knn_image_buffers(d.f32, B, co, N);
        have_prepared = true;
        check(dgx_bn_lrelu_apply_knn_image_f32(P(ysel), B, N, co, P(st.scale), P(st.shift), (float)ly.slope, out,
                                               (int)total, out16, P(next_prepared.first), P(next_prepared.second),
                                               (size_t)next_prepared.second.numel() * 4, d.stream),
              "bn apply + knn image");
      } else {
        check(dgx_bn_lrelu_apply_f32(P(ysel), (int)M, co, P(st.scale), P(st.shift), (float)ly.slope, out, (int)total,
                                     out16, d.stream),
              "bn apply");
      }
      have16 = bf16;
      prev_selecting = true;
      r.saved.insert(r.saved.end(), {idx, PQ, ysel, arg, sumP, st.scale, st.shift, st.mean, st.invstd});   // ChainField order
      r.stats.push_back(st);
    } else {   // inference with running statistics: one fused select + affine + LReLU pass
      Stats st = running_stats(d, ly.gamma, ly.beta, ly.bn);
      check(dgx_edge_fwd_eval_f32(P(PQ), (int)PQ.stride(0), P<int32_t>(idx), B, N, k, co, P(st.scale), P(st.shift),
                                  (float)ly.slope, out, (int)total, d.stream),
            "edge eval");
      have16 = false;
      prev_selecting = false;
      for (int j = 0; j < kPerLayer; ++j) r.saved.push_back(at::empty({0}, d.f32));
      r.stats.push_back(st);
    }
    off_in = off;
    off += co;
  }
  r.have16 = have16;
  r.xcat16 = have16 ? xcat16 : at::empty({0}, d.bf16);
  if (!r.prep.defined()) r.prep = at::empty({0}, d.bf16);
  return r;
}

struct ChainGrads {
  Tensor dx;
  std::vector<Tensor> dw, dgamma, dbeta;
};

// Backward of the chain (autograd of dgcnn.py:84-98): per block in reverse, dz + BN
// backward, reverse kNN graph scatter into dPQ, then dW = dPQ^T X and dX += dPQ [W1; W2]
// (the latter written straight into the gradient of the concat slice it came from).
ChainGrads chain_backward_impl(const Dev& d, Tensor dxcat, bool dxcat_owned, const Tensor& xcat, const Tensor& xcat16,
                               const std::vector<Tensor>& saved, const std::vector<Layer>& L,
                               const std::vector<Stats>& stats, const std::vector<std::pair<Tensor, Tensor>>& preps,
                               int B, int C0, int N, int k, bool bf16, bool x_needs_grad, const Opts& o,
                               SlabJobs* slabs) {
  const int n = (int)L.size();
  const int64_t M = (int64_t)B * N;
  int64_t total = 0;
  for (auto& ly : L) total += ly.co;
  const Tensor& x_pm = saved[0];
  ChainGrads g;
  g.dw.resize(n);
  g.dgamma.resize(n);
  g.dbeta.resize(n);
  if (dxcat.scalar_type() != at::kFloat) dxcat = dxcat.to(at::kFloat);
  dxcat = dxcat.contiguous();
  Tensor dnew;
  if (bf16) {
    // the incoming gradient stays read-only: block l's input gradient is written as
    // addend (incoming slice) + dPQ Wcat into a fresh buffer
    const int64_t lead = total - L.back().co;
    dnew = at::empty({M, std::max<int64_t>(lead, 1)}, d.f32);
  } else if (!dxcat_owned) {
    dxcat = dxcat.clone();
  }
  std::vector<bool> selecting(n);
  std::vector<Tensor> idxs(n);
  for (int li = 0; li < n; ++li) {
    idxs[li] = field(saved, li, kIdx);
    selecting[li] = idxs[li].numel() > 0;
    TORCH_CHECK(selecting[li], "dgx chain backward: block ", li + 1, " ran without its backward state");
    TORCH_CHECK(idxs[li].scalar_type() == at::kInt && idxs[li].is_contiguous(),
                "dgx: kNN ids must be contiguous int32");
  }
  // reverse kNN graphs of every block, at the start of the backward on its stream (a build on a side stream
  // overlapping the forward measured slower, 1.63 vs 1.56 ms/step at cfg2: the concurrent kernels contend for
  // the L2 the kNN operand images live in)
  const auto [rowptr, edges] = reverse_graphs(d, idxs, B, N, k);
  const double count = (double)M * k;
  // packed dz|slot words (18 significant bits of dz) in bf16 mode, and in the
  // fp32 mode whose conv5 GEMMs are split bf16 (2^-16 per product: the same
  // precision class); exact dz + slot bytes with exact fp32 products
  const bool packed = (bf16 || o.split32) && o.packed;
  std::vector<Tensor> w32;   // fp32 mode: stacked weights of the blocks whose input gradient is formed
  // fp32 mode, split class: blocks whose dW / dX run as 3-pass split bf16 GEMMs on
  // the scatter's (hi, lo) dPQ planes, with [W1; W2]^T as [hi^T | lo^T] (one prep launch)
  std::vector<bool> esplit(n, false);
  std::vector<Tensor> wsplit(n);
  Tensor wsplit_buf;
  if (!bf16) {
    std::vector<PrepJob> jobs;
    std::vector<int> at;
    for (int l = 1; l < n; ++l) {
      esplit[l] = o.split32 && o.split_edge && packed && L[l].cin % 64 == 0 && L[l].co % 32 == 0 &&
                  L[l].w.is_contiguous();
      if (esplit[l]) {
        jobs.push_back(PrepJob{L[l].w, L[l].co, L[l].cin, true, false, true});
        at.push_back(l);
      }
    }
    if (!jobs.empty()) {
      auto pw = prep_weights(d, jobs);
      wsplit_buf = pw.first;
      for (size_t i = 0; i < at.size(); ++i) wsplit[at[i]] = pw.second[i].second;   // (cin, 4co)
    }
    std::vector<bool> need(n);
    for (int l = 0; l < n; ++l) need[l] = (l > 0 || x_needs_grad) && !esplit[l];
    w32 = stack_weights_f32(d, L, need);
  }
  Tensor pre_dz, pre_part;
  int pre_rows = 0;
  bool have_pre = false;
  int64_t off = total;
  for (int li = n - 1; li >= 0; --li) {
    const Layer& ly = L[li];
    const int cin = ly.cin, co = ly.co;
    off -= co;
    const int64_t prev = li > 0 ? off - L[li - 1].co : 0;
    const Tensor &PQ = field(saved, li, kPQ), &ysel = field(saved, li, kYsel),
                 &arg = field(saved, li, kArg), &sumP = field(saved, li, kSumP);
    const Stats& st = stats[li];
    const Tensor X = li == 0 ? x_pm : xcat.narrow(1, prev, cin);
    const bool uses_prep = block_uses_prep(bf16, li, li > 0 && selecting[li - 1], cin, total, prev) &&
                           lds_ok(xcat16.defined() && xcat16.numel() ? xcat16.narrow(1, prev, cin) : Tensor(), cin) &&
                           (int)preps.size() >= li;
    Tensor dz, partials;
    int nblk;
    if (have_pre) {   // dz + partials already made by block li+1's dX GEMM epilogue
      dz = pre_dz;
      partials = pre_part;
      nblk = pre_rows;
      have_pre = false;
    } else {
      const float* dY;
      int64_t ldy;
      if (bf16 && li < n - 1) {
        dY = P(dnew) + off;
        ldy = dnew.stride(0);
      } else {
        dY = P(dxcat) + off;
        ldy = dxcat.stride(0);
      }
      nblk = (int)std::max<int64_t>(1, std::min<int64_t>(1024, (M + 63) / 64));
      dz = at::empty({M, co}, d.f32);
      partials = at::empty({nblk, 2, co}, d.f32);
      if (packed) {
        // dz words carry the selected slot in their 6 low mantissa bits (the dPQ they feed is bf16)
        check(dgx_edge_bwd_dz_packed_f32(dY, (int)ldy, P(ysel), P<uint8_t>(arg), (int)M, co, P(st.scale), P(st.shift),
                                         P(st.mean), P(st.invstd), (float)ly.slope, P(dz), P(partials), nblk, d.stream),
              "edge bwd dz");
      } else {
        check(dgx_edge_bwd_dz_f32(dY, (int)ldy, P(ysel), (int)M, co, P(st.scale), P(st.shift), P(st.mean),
                                  P(st.invstd), (float)ly.slope, P(dz), P(partials), nblk, d.stream),
              "edge bwd dz");
      }
    }
    // dPQ only feeds GEMMs: bf16 (what the GEMM would round it to) in bf16 mode,
    // its (hi, lo) bf16 planes in the fp32 mode's split class
    const bool es = !bf16 && esplit[li];
    const int out_mode = bf16 ? 1 : (es ? 3 : 0);
    Tensor dPQs = es ? at::empty({3, M, 2 * co}, d.bf16) : Tensor();   // (hi, lo, hi)
    Tensor dPQ = es ? dPQs[0] : at::empty({M, 2 * co}, bf16 ? d.bf16 : d.f32);
    Tensor dgamma, dbeta, c0, c1;
    const bool fold = st.group.empty() && o.fold_bwd;
    if (fold) {
      dgamma = at::empty({co}, d.f32);
      dbeta = at::empty({co}, d.f32);
      c0 = at::empty({co}, d.f32);
      c1 = at::empty({co}, d.f32);
    }
    if (fold) {   // BN backward finalize in the scatter's prologue (one launch)
      check(dgx_edge_bwd_scatter_fin_f32(P(PQ), (int)PQ.stride(0), P<int32_t>(rowptr[li]), P<int32_t>(edges[li]), P(dz),
                                         packed ? nullptr : P<uint8_t>(arg), P(sumP), B, N, k, co, P(partials), nblk,
                                         count, P(st.scale), P(st.mean), P(st.invstd), (int)st.eval, P(dgamma), P(dbeta),
                                         P(c0), P(c1), dPQ.data_ptr(), out_mode, (int)packed, d.stream),
            "edge bwd scatter");
    } else {   // SyncBatchNorm: the all-reduce sits between the partials and the finalize
      auto r = backward_consts(d, partials, nblk, count, st);
      dgamma = r[0];
      dbeta = r[1];
      c0 = r[2];
      c1 = r[3];
      if (packed)
        check(dgx_edge_bwd_scatter_packed_f32(P(PQ), (int)PQ.stride(0), P<int32_t>(rowptr[li]), P<int32_t>(edges[li]),
                                              P(dz), P(sumP), B, N, k, co, P(st.scale), P(c0), P(c1), dPQ.data_ptr(),
                                              out_mode, d.stream),
              "edge bwd scatter");
      else
        check(dgx_edge_bwd_scatter_f32(P(PQ), (int)PQ.stride(0), P<int32_t>(rowptr[li]), P<int32_t>(edges[li]), P(dz),
                                       P<uint8_t>(arg), P(sumP), B, N, k, co, P(st.scale), P(c0), P(c1), dPQ.data_ptr(),
                                       out_mode, d.stream),
              "edge bwd scatter");
    }
    g.dgamma[li] = dgamma;
    g.dbeta[li] = dbeta;
    if (bf16) {
      // dW = dPQ^T X, un-stacked to the reference layout [W1 | W2]
      Tensor gw = at::empty({co, 2 * cin}, d.f32);
      if (uses_prep)
        lds_atb(d, dPQ, xcat16.narrow(1, prev, cin), gw, co, o.slab_cap_mb, slabs);
      else
        mm_atb(d, dPQ, X, gw, co, slabs);
      g.dw[li] = gw.view(ly.w.sizes());
      if (li > 0) {
        Tensor add = dxcat.narrow(1, prev, cin);
        if (uses_prep && o.fuse_edge_dz && packed && selecting[li - 1] && edge_dz_ok(dPQ, cin)) {
          // block li-1's dY = add + dPQ [W1;W2]: its LeakyReLU' + packed dz + BN partials in the epilogue
          const Stats& stp = stats[li - 1];
          const Tensor& w16 = preps[li - 1].second;   // (cin, 2co)
          const int rows = dgx_gemm_edge_dz_rows((int)M, cin);
          pre_dz = at::empty({M, cin}, d.f32);
          pre_part = at::empty({rows, 2, cin}, d.f32);
          check(dgx_gemm_edge_dz_bf16(dPQ.data_ptr(), ld16(dPQ), w16.data_ptr(), ld16(w16), (int)M, cin, 2 * co,
                                      P(add), add.stride(0), P(field(saved, li - 1, kYsel)),
                                      P<uint8_t>(field(saved, li - 1, kArg)), P(stp.scale), P(stp.shift),
                                      P(stp.mean), P(stp.invstd), (float)L[li - 1].slope, P(pre_dz), P(pre_part), rows,
                                      d.stream),
                "gemm edge dz");
          pre_rows = rows;
          have_pre = true;
        } else {
          Tensor dst = dnew.narrow(1, prev, cin);
          if (uses_prep) {
            lds_xwt(d, dPQ, preps[li - 1].second, nullptr, false, &add, &dst);
          } else {
            dst.copy_(add);
            mm_xw(d, dPQ, split_weight(ly.w, cin, co), dst, true);
          }
        }
      } else if (x_needs_grad) {
        Tensor dx = at::empty({M, C0}, d.f32);
        mm_xw(d, dPQ, split_weight(ly.w, cin, co), dx, false);
        g.dx = dx.view({B, N, C0}).permute({0, 2, 1});
      }
    } else if (es) {
      // 3-pass split bf16: dW = [hi; lo; hi]^T [X_hi; X_hi; X_lo] as ONE TN GEMM over
      // 3 B*N rows (one set of split-K slabs, un-stacked to [W1 | W2] by the deferred
      // reduce); dX += dPQ_hi (W_hi + W_lo) + dPQ_lo W_hi
      const Tensor dPQl = dPQs[1];
      Tensor xp = at::empty({3, M, cin}, d.bf16);
      check(dgx_split_bf16(P(X), X.stride(0), M, cin, xp[0].data_ptr(), xp[2].data_ptr(), cin, d.stream),
            "split bf16");
      xp[1].copy_(xp[0]);
      Tensor gw = at::empty({co, 2 * cin}, d.f32);
      lds_atb(d, dPQs.view({3 * M, 2 * co}), xp.view({3 * M, cin}), gw, co, o.slab_cap_mb, slabs);
      g.dw[li] = gw.view(ly.w.sizes());
      Tensor dst = dxcat.narrow(1, prev, cin);
      const Tensor& tn = wsplit[li];
      lds_xwt(d, dPQ, tn, nullptr, false, &dst, &dst);
      lds_xwt(d, dPQl, tn.narrow(1, 0, 2 * co), nullptr, false, &dst, &dst);
    } else {
      Tensor gw = at::empty({co, 2 * cin}, d.f32);   // dW = dPQ^T X, un-stacked to [W1 | W2] by the reduce
      mm32_atb(d, dPQ, X, gw, co, slabs);
      g.dw[li] = gw.view(ly.w.sizes());
      if (li > 0) {
        Tensor dst = dxcat.narrow(1, prev, cin);
        mm32(d, dPQ, w32[li], &dst, true);
      } else if (x_needs_grad) {
        g.dx = mm32(d, dPQ, w32[li], nullptr, false).view({B, N, C0}).permute({0, 2, 1});
      }
    }
  }
  return g;
}

// ---------------------------------------------------------------- conv5 ----
enum PcField { kXop, kZ, kPcScale, kPcShift, kPcMean, kPcInvstd, kNt, kTn, kXhi, kXlo, kNumPcFields };
const char* const kPcNames[kNumPcFields] = {"Xop", "Z", "scale", "shift", "mean", "invstd", "nt", "tn", "xhi", "xlo"};

struct PcState {
  Tensor Xop, W, Z, nt, tn;
  Tensor xhi, xlo;   // fp32 mode, 3-pass split bf16: X's planes (nt / tn then hold [hi | lo] weights)
  Stats st;
  bool bf16 = false;
  int B = 0, N = 0;
  double slope = 0.2;

  // the saved list of conv5 (dgx.schedule.PC_FIELDS): undefined tensors travel as empty ones
  std::vector<Tensor> pack(const Dev& d) const {
    auto e16 = [&](const Tensor& t) { return t.defined() ? t : at::empty({0}, d.bf16); };
    return {Xop, Z, st.scale, st.shift, st.mean, st.invstd, e16(nt), e16(tn), e16(xhi), e16(xlo)};
  }
  // ... and back, from s[0 .. kNumPcFields) (weight: conv5's, any trailing 1x1 dims)
  static PcState unpack(const Tensor* s, const std::string& group, bool eval, const Tensor& weight, bool bf16, int B,
                        int N, double slope) {
    auto opt = [](const Tensor& t) { return t.numel() ? t : Tensor(); };
    PcState r;
    r.Xop = s[kXop];
    r.Z = s[kZ];
    r.st = Stats{s[kPcScale], s[kPcShift], s[kPcMean], s[kPcInvstd], group, eval};
    r.nt = opt(s[kNt]);
    r.tn = opt(s[kTn]);
    r.xhi = opt(s[kXhi]);
    r.xlo = opt(s[kXlo]);
    r.W = weight.reshape({weight.size(0), r.Xop.size(1)});
    r.bf16 = bf16;
    r.B = B;
    r.N = N;
    r.slope = slope;
    return r;
  }
};

// conv5 -> BN -> LeakyReLU on the point-major concat buffer (dgx.pointconv, dgcnn.py:100-102):
// out (B, Co, N); bf16: Z stored bf16 with the BN statistics from the GEMM's fp32 sums
Tensor pointconv_forward_impl(const Dev& d, const Tensor& X_in, const Tensor& X16, int B, int N, const Layer& ly,
                              bool bf16, Tensor nt, Tensor tn, PcState* state, bool split32 = false) {
  Tensor X = X_in.scalar_type() == at::kFloat ? X_in : X_in.to(at::kFloat);
  const int64_t M = X.size(0), K = X.size(1);
  const int Co = (int)ly.w.size(0);
  Tensor W = ly.w.reshape({Co, K});
  const bool use_batch = ly.bn.use_batch();
  Tensor Z, gemm_part, Xop = X, xhi, xlo;
  if (bf16) {
    // the LDS-DMA GEMMs take conv5 only when its backward fits them too: dX = dZ W has Co as
    // its inner dimension (whole 64-wide K-steps) and dW = dZ^T X has Co output rows
    if (X16.defined() && X16.numel() && lds_ok(X16, K) && Co % 64 == 0) {
      Xop = X16;
      if (!nt.defined() || !nt.numel()) {
        std::tie(nt, tn) = prep_weight(d, W, Co, (int)K);
      }
      Z = use_batch ? lds_xwt(d, X16, nt, &gemm_part, true) : lds_xwt(d, X16, nt, nullptr, false);
    } else {
      nt = Tensor();
      tn = Tensor();
      Z = mm_xwt(d, X, W, use_batch ? &gemm_part : nullptr);
    }
  } else if (split32 && K % 64 == 0 && Co % 64 == 0 && Co >= 8) {
    // fp32 mode, 3-pass split bf16 on the bf16 MFMA: Z = X_hi (W_hi + W_lo)^T + X_lo W_hi^T
    // (x and w with 16 significant bits each; ~2^-16 relative per product, fp32 sums)
    auto xs = split16(d, X);
    xhi = xs.first;
    xlo = xs.second;
    auto pw = prep_weights(d, {PrepJob{W, Co, (int)K, false, true, true}});
    nt = pw.second[0].first;    // (Co, 2K) [W_hi | W_lo]
    tn = pw.second[0].second;   // (K, 2Co) [W_hi^T | W_lo^T]
    Z = lds_xwt(d, xhi, nt, nullptr, false);
    Tensor w_hi = nt.narrow(1, 0, K);
    lds_xwt(d, xlo, w_hi, nullptr, false, &Z, &Z);
  } else {
    nt = Tensor();
    tn = Tensor();
    Z = mm32(d, X, W.t(), nullptr, false);
  }
  Tensor out = at::empty({B, Co, N}, d.f32);
  Stats st;
  if (use_batch) {
    Tensor partials = gemm_part;
    int rows;
    if (partials.defined()) {
      rows = (int)partials.size(0);
    } else {
      rows = dgx_colstats_rows(M);
      partials = at::empty({rows, 2, Co}, d.f32);
      check(dgx_colstats_f32(P(Z), Co, M, Co, P(partials), rows, d.stream), "colstats");
    }
    st = batch_stats(d, partials, rows, (double)M, ly.gamma, ly.beta, ly.bn);
  } else {
    st = running_stats(d, ly.gamma, ly.beta, ly.bn);
  }
  if (is16(Z))
    check(dgx_pointconv_apply_bf16(Z.data_ptr(), B, N, Co, P(st.scale), P(st.shift), (float)ly.slope, P(out), d.stream),
          "pointconv apply bf16");
  else
    check(dgx_pointconv_apply_f32(P(Z), Co, B, N, Co, P(st.scale), P(st.shift), (float)ly.slope, P(out), d.stream),
          "pointconv apply");
  if (state) *state = PcState{Xop, W, Z, nt, tn, xhi, xlo, st, bf16, B, N, ly.slope};
  return out;
}

// its backward: dX (M, K) fp32, dW (Co, K), dgamma, dbeta
std::array<Tensor, 4> pointconv_backward_impl(const Dev& d, Tensor dout, const PcState& s, SlabJobs* slabs) {
  const int64_t M = s.Z.size(0);
  const int Co = (int)s.Z.size(1);
  const int B = s.B, N = s.N;
  dout = dout.to(at::kFloat).contiguous();
  const bool z16 = is16(s.Z);
  const Stats& st = s.st;
  const int64_t K = s.Xop.size(1);
  if (!s.bf16 && s.xhi.defined() && s.Z.is_contiguous() && Co % 4 == 0) {
    // fp32 mode, split GEMMs: two passes over (dout, Z) — BN-backward reductions,
    // then dZ straight into its split-bf16 planes (no fp32 dz / dZ round trip)
    const int rows = dgx_pointconv_bf16_rows(B, N);
    Tensor partials = at::empty({rows, 2, Co}, d.f32);
    check(dgx_pointconv_bwd_split_f32(P(dout), P(s.Z), B, N, Co, P(st.scale), P(st.shift), P(st.mean), P(st.invstd),
                                      (float)s.slope, nullptr, nullptr, P(partials), nullptr, nullptr, 0, d.stream),
          "pointconv bwd stats f32");
    auto cs = backward_consts(d, partials, rows, (double)M, st);
    Tensor zhi = at::empty({M, Co}, d.bf16), zlo = at::empty({M, Co}, d.bf16);
    check(dgx_pointconv_bwd_split_f32(P(dout), P(s.Z), B, N, Co, P(st.scale), P(st.shift), nullptr, nullptr,
                                      (float)s.slope, P(cs[2]), P(cs[3]), nullptr, zhi.data_ptr(), zlo.data_ptr(), 1,
                                      d.stream),
          "pointconv bwd dZ split");
    Tensor dW = at::empty({Co, K}, d.f32);
    lds_atb_sum(d, {{zhi, s.xhi}, {zhi, s.xlo}, {zlo, s.xhi}}, dW, slabs);
    Tensor dX = lds_xwt(d, zhi, s.tn, nullptr, false);                       // dZ_hi (W_hi + W_lo)
    Tensor wt_hi = s.tn.narrow(1, 0, Co);
    lds_xwt(d, zlo, wt_hi, nullptr, false, &dX, &dX);                        // + dZ_lo W_hi
    return {dX, dW, cs[0], cs[1]};
  }
  const int rows = z16 ? dgx_pointconv_bf16_rows(B, N) : dgx_pointconv_bwd_rows(B, N);
  Tensor partials = at::empty({rows, 2, Co}, d.f32);
  Tensor dZ = at::empty({M, Co}, s.bf16 ? d.bf16 : d.f32);
  Tensor dz;
  if (z16) {   // two passes over (dout, Z): BN-backward reductions, then dZ directly
    check(dgx_pointconv_bwd_bf16(P(dout), s.Z.data_ptr(), B, N, Co, P(st.scale), P(st.shift), P(st.mean),
                                 P(st.invstd), (float)s.slope, nullptr, nullptr, P(partials), nullptr, 0, d.stream),
          "pointconv bwd stats");
  } else {
    dz = at::empty({M, Co}, d.f32);
    check(dgx_pointconv_bwd_f32(P(dout), P(s.Z), Co, B, N, Co, P(st.scale), P(st.shift), P(st.mean), P(st.invstd),
                                (float)s.slope, P(dz), P(partials), d.stream),
          "pointconv bwd");
  }
  auto cs = backward_consts(d, partials, rows, (double)M, st);
  if (z16)
    check(dgx_pointconv_bwd_bf16(P(dout), s.Z.data_ptr(), B, N, Co, P(st.scale), P(st.shift), nullptr, nullptr,
                                 (float)s.slope, P(cs[2]), P(cs[3]), nullptr, dZ.data_ptr(), 1, d.stream),
          "pointconv bwd dZ");
  else
    check(dgx_pointconv_input_grad(P(dz), P(s.Z), Co, M, Co, P(st.scale), P(cs[2]), P(cs[3]), dZ.data_ptr(),
                                   (int)s.bf16, d.stream),
          "pointconv dZ");
  Tensor dW = at::empty({Co, K}, d.f32), dX;
  if (s.bf16) {   // bf16 MFMA: dW = dZ^T X (split-K, deterministic), dX = dZ W
    if (s.nt.defined()) {
      lds_atb(d, dZ, s.Xop, dW, 0, 0, slabs);
      dX = lds_xwt(d, dZ, s.tn, nullptr, false);
    } else {
      mm_atb(d, dZ, s.Xop, dW, 0, slabs);
      dX = at::empty({M, K}, d.f32);
      mm_xw(d, dZ, s.W, dX, false);
    }
  } else if (s.xhi.defined()) {   // 3-pass split bf16 (the forward's planes and weights)
    auto zs = split16(d, dZ);
    lds_atb_sum(d, {{zs.first, s.xhi}, {zs.first, s.xlo}, {zs.second, s.xhi}}, dW, slabs);
    dX = lds_xwt(d, zs.first, s.tn, nullptr, false);                       // dZ_hi (W_hi + W_lo)
    Tensor wt_hi = s.tn.narrow(1, 0, Co);
    lds_xwt(d, zs.second, wt_hi, nullptr, false, &dX, &dX);               // + dZ_lo W_hi
  } else {   // fp32 MFMA GEMMs (dW: split-K over the B*N rows)
    dW = mm32(d, dZ.t(), s.Xop, nullptr, false);
    dX = mm32(d, dZ, s.W, nullptr, false);
  }
  return {dX, dW, cs[0], cs[1]};
}

// ------------------------------------------------------------------- ops ----
// a block as the backward needs it: weight, widths, slope (make_layers adds the forward's BN fields)
Layer weight_layer(const Tensor& w, double slope) {
  Layer ly;
  ly.w = w;
  ly.slope = slope;
  ly.co = (int)w.size(0);
  ly.cin = (int)(w.size(1) / 2);
  return ly;
}

std::vector<Layer> make_layers(const std::vector<Tensor>& weights, const std::vector<Tensor>& gammas,
                               const std::vector<Tensor>& betas, std::vector<BnSpec> bns,
                               const std::vector<double>& slopes) {
  const int n = (int)weights.size();
  TORCH_CHECK((int)gammas.size() == n && (int)betas.size() == n && (int)bns.size() == n && (int)slopes.size() == n,
              "dgx: per-layer argument lists differ in length");
  std::vector<Layer> L(n);
  for (int l = 0; l < n; ++l) {
    const Tensor& w = weights[l];
    TORCH_CHECK(w.scalar_type() == at::kFloat && w.is_cuda(), "dgx: fp32 device conv weights expected");
    L[l] = weight_layer(w, slopes[l]);
    L[l].gamma = gammas[l];
    L[l].beta = betas[l];
    L[l].bn = std::move(bns[l]);
  }
  return L;
}

std::vector<Stats> stats_from_saved(const std::vector<Tensor>& saved, int n, const std::vector<int64_t>& eval,
                                    const std::vector<std::string>& groups) {
  std::vector<Stats> st(n);
  for (int l = 0; l < n; ++l)
    st[l] = Stats{field(saved, l, kScale), field(saved, l, kShift), field(saved, l, kMean), field(saved, l, kInvstd),
                  groups[l], eval[l] != 0};
  return st;
}

// dgx_host::chain_forward
std::tuple<Tensor, Tensor, std::vector<Tensor>, Tensor> chain_forward(
    const Tensor& x, int64_t k, std::vector<Tensor> weights, std::vector<Tensor> gammas, std::vector<Tensor> betas,
    const c10::List<std::optional<Tensor>>& bn_t_l, std::vector<double> bn_f, std::vector<int64_t> bn_i,
    std::vector<std::string> groups, std::vector<double> slopes, bool bf16, bool need_grad,
    const std::optional<Tensor>& prep, const std::optional<Tensor>& idx0, int64_t opts) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 3, "dgx chain: (B, C, N) device cloud expected");
  auto bn_t = to_vec(bn_t_l);
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  Dev d(x);
  const int n = (int)weights.size();
  auto L = make_layers(weights, gammas, betas, parse_bn(bn_t, bn_f, bn_i, groups, n, 6), slopes);
  Tensor pbuf = defined_or_none(prep);
  std::vector<std::pair<Tensor, Tensor>> views;
  if (pbuf.defined()) views = prep_views(pbuf, chain_prep_jobs(L));
  ChainOut r = chain_forward_impl(d, x, (int)k, L, bf16, need_grad, pbuf.defined() ? &views : nullptr,
                                  defined_or_none(idx0), decode(opts));
  return {r.xcat, r.xcat16, r.saved, pbuf.defined() ? pbuf : r.prep};
}

// dgx_host::chain_backward
std::tuple<Tensor, std::vector<Tensor>, std::vector<Tensor>, std::vector<Tensor>> chain_backward(
    const Tensor& dxcat, const Tensor& xcat, const Tensor& xcat16, std::vector<Tensor> saved,
    std::vector<Tensor> weights, const std::optional<Tensor>& prep, std::vector<int64_t> shape, int64_t k,
    std::vector<int64_t> eval, std::vector<std::string> groups, std::vector<double> slopes, bool bf16,
    bool x_needs_grad, int64_t opts) {
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(xcat.device());
  Dev d(xcat);
  const int n = (int)weights.size();
  TORCH_CHECK((int)saved.size() == 1 + kPerLayer * n && (int)eval.size() == n && (int)groups.size() == n,
              "dgx chain backward: saved state does not match the layer count");
  std::vector<Layer> L(n);
  for (int l = 0; l < n; ++l) L[l] = weight_layer(weights[l], slopes[l]);
  Tensor pbuf = defined_or_none(prep);
  std::vector<std::pair<Tensor, Tensor>> views;
  if (pbuf.defined()) views = prep_views(pbuf, chain_prep_jobs(L));
  auto st = stats_from_saved(saved, n, eval, groups);
  SlabJobs slabs;
  ChainGrads g = chain_backward_impl(d, dxcat, false, xcat, xcat16, saved, L, st, views, (int)shape[0], (int)shape[1],
                                     (int)shape[2], (int)k, bf16, x_needs_grad, decode(opts), &slabs);
  slabs.flush(d.stream);
  if (!g.dx.defined()) g.dx = at::empty({0}, d.f32);
  return {g.dx, g.dw, g.dgamma, g.dbeta};
}

// dgx_host::pointconv_forward -> (out, PcState::pack)
std::tuple<Tensor, std::vector<Tensor>> pointconv_forward(
    const Tensor& X, const Tensor& X16, int64_t B, int64_t N, const Tensor& weight, const Tensor& gamma,
    const Tensor& beta, const c10::List<std::optional<Tensor>>& bn_t_l, std::vector<double> bn_f,
    std::vector<int64_t> bn_i, std::string group, bool bf16, const std::optional<Tensor>& nt,
    const std::optional<Tensor>& tn, int64_t opts) {
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(X.device());
  Dev d(X);
  auto bn_t = to_vec(bn_t_l);
  Layer ly;
  ly.w = weight;
  ly.gamma = gamma;
  ly.beta = beta;
  ly.bn = parse_bn(bn_t, bn_f, bn_i, {group}, 1, 6)[0];
  ly.slope = bn_f[2];
  PcState s;
  Tensor out = pointconv_forward_impl(d, X, X16, (int)B, (int)N, ly, bf16, defined_or_none(nt), defined_or_none(tn), &s,
                                      decode(opts).split32);
  return {out, s.pack(d)};
}

// dgx_host::pointconv_backward -> (dX, dW, dgamma, dbeta). The fp32 mode's split
// planes and weights are rebuilt from X / the weight when the caller did not keep
// them (the torch.library op): dgx_split_bf16 is deterministic.
std::tuple<Tensor, Tensor, Tensor, Tensor> pointconv_backward(const Tensor& dout, std::vector<Tensor> saved,
                                                              const Tensor& weight, int64_t B, int64_t N, double slope,
                                                              bool eval, std::string group, bool bf16, int64_t opts) {
  TORCH_CHECK(saved.size() == kNumPcFields, "dgx pointconv backward: ", (int)kNumPcFields, " saved tensors expected");
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(saved[kZ].device());
  Dev d(saved[kZ]);
  PcState s = PcState::unpack(saved.data(), group, eval, weight, bf16, (int)B, (int)N, slope);
  const int64_t K = s.Xop.size(1), Co = weight.size(0);
  if (!bf16 && !s.xhi.defined() && decode(opts).split32 && s.Xop.scalar_type() == at::kFloat && K % 64 == 0 &&
      Co % 64 == 0) {
    auto xs = split16(d, s.Xop);
    s.xhi = xs.first;
    s.xlo = xs.second;
    auto pw = prep_weights(d, {PrepJob{s.W, (int)Co, (int)K, false, true, true}});
    s.nt = pw.second[0].first;
    s.tn = pw.second[0].second;
  }
  SlabJobs slabs;
  auto r = pointconv_backward_impl(d, dout, s, &slabs);
  slabs.flush(d.stream);
  return {r[0], r[1].view(weight.sizes()), r[2], r[3]};
}

// ------------------------------------------ PositionEmbedding's edge MLP ----
// max_k conv2(conv1(get_graph_feature(x, k))) of reference models/layers.py:45-52 (dgx.edgemlp)
// as one stage. The edge tensor is never built: conv1 is PQ = X [W1; W2]^T (y_e = P_j + Q_i, as
// in the chain) with its BN statistics from the EdgeConv gather kernel.
//   bf16, C1 = 64, C2 in {64, 128}, k <= 64: ONE forward kernel builds each 16-edge h1 tile,
//   runs conv2 on the MFMA and keeps the max over k and the BN2 statistics (h1, z2 never reach
//   HBM); with C2 = 128 ONE backward kernel recomputes them and forms gE, the BN1 partials
//   and dW2; otherwise h1 is kept for the dZ2 / dH1 GEMMs;
//   every other shape and the fp32 mode: h1 per edge row, conv2 as one GEMM over the E = B*N*k
//   rows, max over k, dense dZ2, the two conv2 GEMMs, LReLU/BN1 backward in place.
// Then the gather over the kNN graph and its reverse forms dP / dQ. The fp32 mode is exact
// fp32 here whatever the opts word says of split GEMMs.
// the saved list (dgx.schedule.EMLP_FIELDS): absent tensors travel as empty ones
enum EmlpField { kEX, kEIdx, kEPQ, kESumP, kEH1, kEZ2, kEYsel, kEArg, kEScale1, kEShift1, kEMean1, kEInvstd1,
                 kEScale2, kEShift2, kEMean2, kEInvstd2, kENt, kETn, kNumEmlpFields };
const char* const kEmlpNames[kNumEmlpFields] = {"X",      "idx",    "PQ",      "sumP",   "H1",     "Z2",
                                                "ysel",   "arg",    "scale1",  "shift1", "mean1",  "invstd1",
                                                "scale2", "shift2", "mean2",   "invstd2", "nt",    "tn"};

bool emlp_fused_bwd_ok(bool fused_bwd, bool bf16, int C1, int C2, int k) {
  return fused_bwd && bf16 && C1 == 64 && C2 == 128 && k <= 64;
}

// dgx_host::edge_mlp2_forward -> (out (B, C2, N), saved). idx: the kNN graph (int32 (B, N, k)) the
// caller found on x or on its knn_src; bn lists: the two layers'; fused_bwd: dgx.edgemlp.FUSED_BWD
std::tuple<Tensor, std::vector<Tensor>> edge_mlp2_forward(
    const Tensor& x_in, const Tensor& idx, int64_t k64, const Tensor& w1, const Tensor& g1, const Tensor& b1,
    const Tensor& w2, const Tensor& g2, const Tensor& b2, const c10::List<std::optional<Tensor>>& bn_t_l,
    std::vector<double> bn_f, std::vector<int64_t> bn_i, std::vector<std::string> groups, bool bf16, bool need_grad,
    bool fused_bwd) {
  TORCH_CHECK(x_in.is_cuda() && x_in.dim() == 3, "dgx edge MLP: (B, C, N) device input expected");
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(x_in.device());
  Dev d(x_in);
  Tensor x = x_in.to(at::kFloat);
  const int B = (int)x.size(0), C = (int)x.size(1), N = (int)x.size(2), k = (int)k64;
  const int64_t M = (int64_t)B * N, E = M * k;
  const int C1 = (int)w1.size(0), C2 = (int)w2.size(0);
  TORCH_CHECK(w1.numel() == (int64_t)C1 * 2 * C && w2.numel() == (int64_t)C2 * C1 && g1.numel() == C1 &&
                  b1.numel() == C1 && g2.numel() == C2 && b2.numel() == C2,
              "dgx edge MLP: conv / BatchNorm parameter shapes do not match the input");
  TORCH_CHECK(idx.scalar_type() == at::kInt && idx.is_contiguous() && idx.dim() == 3 && idx.size(0) == B &&
                  idx.size(1) == N && idx.size(2) == k,
              "dgx edge MLP: idx must be contiguous int32 (B, N, k)");
  auto bns = parse_bn(to_vec(bn_t_l), bn_f, bn_i, groups, 2, 6);
  const float slope1 = (float)bn_f[2], slope2 = (float)bn_f[5];
  const bool use1 = bns[0].use_batch(), use2 = bns[1].use_batch();
  Tensor X = x.permute({0, 2, 1}).reshape({M, C}).contiguous();   // B = 1 reshapes to a column-major view
  Tensor w1s = split_weight(w1, C, C1), PQ;
  if (C <= kSmallKMax) {   // raw coordinates (K = 3): exact fp32 in every mode
    PQ = at::empty({M, 2 * C1}, d.f32);
    check(dgx_gemm_smallk_f32(P(X), M > 1 ? X.stride(0) : C, P(w1s), (int)M, 2 * C1, C, P(PQ), 2 * C1, d.stream),
          "gemm small-k");
  } else {
    PQ = bf16 ? mm_xwt(d, X, w1s, nullptr) : mm32(d, X, w1s.t(), nullptr, false);
  }
  Tensor W2 = w2.reshape({C2, C1});
  // ---- conv1: BN1 statistics over all E edges
  Stats st1, st2;
  Tensor sumP1;
  if (use1) {
    Tensor ysel1 = at::empty({M, C1}, d.f32), arg1 = at::empty({M, C1}, d.u8);
    sumP1 = at::empty({M, C1}, d.f32);
    const int prow = dgx_edge_partials_rows(B, N, C1);
    Tensor part1 = at::empty({prow, 2, C1}, d.f32);
    check(dgx_edge_fwd_gather_f32(P(PQ), (int)PQ.stride(0), P<int32_t>(idx), B, N, k, C1, P(g1), P(ysel1),
                                  P<uint8_t>(arg1), P(sumP1), P(part1), prow, d.stream),
          "edge gather");
    st1 = batch_stats(d, part1, prow, (double)E, g1, b1, bns[0]);
  } else {
    st1 = running_stats(d, g1, b1, bns[0]);
    // sum_k P_j only enters the train-mode BN1 backward (c1 = 0 here)
    if (need_grad) sumP1 = at::zeros({M, C1}, d.f32);
  }
  Tensor H1, Z2, nt, tn;
  Tensor ysel = at::empty({M, C2}, d.f32), arg = at::empty({M, C2}, d.u8);
  if (bf16 && C1 == 64 && (C2 == 64 || C2 == 128) && k <= 64) {
    // h1 -> conv2 (MFMA) -> max over k + BN2 statistics in one kernel: z2 never reaches HBM;
    // h1 (bf16) is written only for the unfused backward's GEMMs (the fused backward rebuilds it)
    std::tie(nt, tn) = prep_weight(d, W2, C2, C1);
    Tensor dir2 = at::where(g2 < 0, -1.0, 1.0).to(at::kFloat).contiguous();
    Tensor W2d = (W2 * dir2.view({C2, 1})).to(at::kBFloat16).contiguous();
    if (need_grad && !emlp_fused_bwd_ok(fused_bwd, bf16, C1, C2, k)) H1 = at::empty({E, C1}, d.bf16);
    const int rows2 = dgx_edge_mlp_fused_rows(B, N);
    Tensor part2 = at::empty({rows2, 2, C2}, d.f32);
    check(dgx_edge_mlp_fused_fwd_bf16(P(PQ), 2 * C1, P<int32_t>(idx), B, N, k, C1, C2, P(st1.scale), P(st1.shift),
                                      slope1, W2d.data_ptr(), P(dir2), P(ysel), P<uint8_t>(arg), P(part2), rows2,
                                      H1.defined() ? H1.data_ptr() : nullptr, d.stream),
          "edge mlp fused forward");
    st2 = use2 ? batch_stats(d, part2, rows2, (double)E, g2, b2, bns[1]) : running_stats(d, g2, b2, bns[1]);
  } else {
    const bool h16 = bf16 && C1 % 64 == 0;
    H1 = at::empty({E, C1}, h16 ? d.bf16 : d.f32);
    check(dgx_edge_mlp_h1_f32(P(PQ), 2 * C1, P<int32_t>(idx), B, N, k, C1, P(st1.scale), P(st1.shift), slope1,
                              H1.data_ptr(), (int)h16, d.stream),
          "edge h1");
    // ---- conv2: one GEMM over the edge rows (+ BN2 column statistics)
    Tensor part2;
    if (h16) {
      std::tie(nt, tn) = prep_weight(d, W2, C2, C1);
      Z2 = use2 ? lds_xwt(d, H1, nt, &part2, true) : lds_xwt(d, H1, nt, nullptr, false);
    } else if (bf16) {
      Z2 = mm_xwt(d, H1, W2, use2 ? &part2 : nullptr);
    } else {
      Z2 = mm32(d, H1, W2.t(), nullptr, false);
      if (use2) {
        const int rows = dgx_colstats_rows(E);
        part2 = at::empty({rows, 2, C2}, d.f32);
        check(dgx_colstats_f32(P(Z2), C2, E, C2, P(part2), rows, d.stream), "colstats");
      }
    }
    st2 = use2 ? batch_stats(d, part2, (int)part2.size(0), (double)E, g2, b2, bns[1])
               : running_stats(d, g2, b2, bns[1]);
    // ---- max over k (layers.py:52) of LReLU(BN2(z2)): select, then apply
    check(dgx_edge_mlp_max_f32(Z2.data_ptr(), (int)is16(Z2), B, N, k, C2, P(st2.scale), P(ysel), P<uint8_t>(arg),
                               d.stream),
          "edge max");
  }
  // LReLU(BN2) of the selected values, written (B, C2, N) contiguous as the reference's max
  // over k returns it (LDS-transposed apply)
  Tensor out = at::empty({B, C2, N}, d.f32);
  check(dgx_pointconv_apply_f32(P(ysel), C2, B, N, C2, P(st2.scale), P(st2.shift), slope2, P(out), d.stream),
        "bn apply");
  auto e = [&](const Tensor& t) { return t.defined() ? t : at::empty({0}, d.f32); };
  return {out, {X, idx, PQ, e(sumP1), e(H1), e(Z2), ysel, arg, st1.scale, st1.shift, st1.mean, st1.invstd, st2.scale,
                st2.shift, st2.mean, st2.invstd, e(nt), e(tn)}};   // EmlpField order
}

// dgx_host::edge_mlp2_backward -> (dx or empty, dW1, dgamma1, dbeta1, dW2, dgamma2, dbeta2)
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor> edge_mlp2_backward(
    const Tensor& dout_in, std::vector<Tensor> S, const Tensor& w1, const Tensor& w2, std::vector<int64_t> shape,
    int64_t k64, std::vector<int64_t> eval, std::vector<std::string> groups, std::vector<double> slopes, bool bf16,
    bool x_needs_grad, int64_t opts) {
  TORCH_CHECK(S.size() == kNumEmlpFields && shape.size() == 3 && eval.size() == 2 && groups.size() == 2 &&
                  slopes.size() == 2,
              "dgx edge MLP backward: saved state does not match the stage");
  const Tensor &X = S[kEX], &idx = S[kEIdx], &PQ = S[kEPQ], &sumP1 = S[kESumP], &H1 = S[kEH1], &Z2 = S[kEZ2];
  const Tensor &ysel = S[kEYsel], &arg = S[kEArg], &nt = S[kENt], &tn = S[kETn];
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(X.device());
  Dev d(X);
  const Stats st1{S[kEScale1], S[kEShift1], S[kEMean1], S[kEInvstd1], groups[0], eval[0] != 0};
  const Stats st2{S[kEScale2], S[kEShift2], S[kEMean2], S[kEInvstd2], groups[1], eval[1] != 0};
  const int B = (int)shape[0], C = (int)shape[1], N = (int)shape[2], k = (int)k64;
  const int64_t M = (int64_t)B * N, E = M * k;
  const int C1 = (int)w1.size(0), C2 = (int)w2.size(0);
  TORCH_CHECK(X.size(0) == M && X.size(1) == C && idx.numel() == E && PQ.size(0) == M && PQ.size(1) == 2 * C1 &&
                  sumP1.numel() == M * C1 && ysel.numel() == M * C2 && arg.numel() == M * C2 &&
                  dout_in.numel() == M * C2 && dout_in.dim() == 3 && dout_in.size(1) == C2,
              "dgx edge MLP backward: saved state does not match the shapes");
  const float slope1 = (float)slopes[0], slope2 = (float)slopes[1];
  const bool fused = Z2.numel() == 0;                // fused forward: z2 was never stored
  const bool fused_bwd = fused && H1.numel() == 0;   // ... and h1 neither: the fused backward kernel
  const bool z16 = fused || is16(Z2);
  const bool have_prep = nt.numel() > 0;
  TORCH_CHECK(fused_bwd || (H1.size(0) == E && H1.size(1) == C1), "dgx edge MLP backward: h1 does not match");
  TORCH_CHECK(fused || (Z2.size(0) == E && Z2.size(1) == C2), "dgx edge MLP backward: z2 does not match");
  TORCH_CHECK(!fused || (have_prep && C1 == 64 && (!fused_bwd || C2 == 128)),
              "dgx edge MLP backward: the fused kernels' state expected");
  Tensor dout = dout_in.to(at::kFloat);
  Tensor dY_pm = dout.permute({0, 2, 1});   // (B, N, C2): point-major if the gradient came that way
  // ---- BN2 + LReLU backward at the selected edges, then dense over all edges
  Tensor dz = at::empty({M, C2}, d.f32), part;
  int nblk;
  if (dY_pm.is_contiguous()) {
    nblk = (int)std::max<int64_t>(1, std::min<int64_t>(1024, (M + 63) / 64));
    part = at::empty({nblk, 2, C2}, d.f32);
    check(dgx_edge_bwd_dz_f32(P(dY_pm), C2, P(ysel), (int)M, C2, P(st2.scale), P(st2.shift), P(st2.mean),
                              P(st2.invstd), slope2, P(dz), P(part), nblk, d.stream),
          "edge bwd dz");
  } else {   // (B, C2, N) gradient (a contiguous downstream): read channel-major, no transpose copy
    Tensor dcm = dout.contiguous();
    nblk = dgx_edge_bwd_dz_cm_rows(B, N);
    part = at::empty({nblk, 2, C2}, d.f32);
    check(dgx_edge_bwd_dz_cm_f32(P(dcm), P(ysel), B, N, C2, P(st2.scale), P(st2.shift), P(st2.mean), P(st2.invstd),
                                 slope2, P(dz), P(part), nblk, d.stream),
          "edge bwd dz");
  }
  auto c2 = backward_consts(d, part, nblk, (double)E, st2);   // dgamma2, dbeta2, c0, c1
  Tensor gw2, gE, part1;
  int rows, g16;
  if (fused_bwd) {
    // conv2 + LReLU/BN1 backward in one pass: gE, BN1 partials, dW2 slabs
    rows = dgx_edge_mlp_fused_bwd_rows(B, N);
    part1 = at::empty({rows, 2, C1}, d.f32);
    Tensor slab = at::empty({rows, C2, C1}, d.f32);
    gE = at::empty({E, C1}, d.bf16);
    Tensor consts = at::cat({c2[2], c2[3], st2.scale}).contiguous();
    check(dgx_edge_mlp_fused_bwd_bf16(P(PQ), 2 * C1, P<int32_t>(idx), B, N, k, C1, C2, P(st1.scale), P(st1.shift),
                                      P(st1.mean), P(st1.invstd), slope1, nt.data_ptr(), P(dz), P<uint8_t>(arg),
                                      P(consts), gE.data_ptr(), P(part1), P(slab), rows, d.stream),
          "edge mlp fused bwd");
    gw2 = at::empty({C2, C1}, d.f32);
    check(dgx_slab_reduce_f32(P(slab), rows, C2, C1, C2, P(gw2), C1, d.stream), "dW2 slab reduce");
    g16 = 1;
  } else {
    Tensor dZ2;
    if (fused) {
      // z2 recomputed from h1 on the MFMA, BN2 backward in the GEMM's epilogue:
      // dZ2 = c1 z2 + c0 + [slot] a2 dz, stored bf16 (z2 never reaches HBM)
      dZ2 = at::empty({E, C2}, d.bf16);
      Tensor consts = at::cat({c2[2], c2[3], st2.scale}).contiguous();
      check(dgx_gemm_dz2_bf16(H1.data_ptr(), nt.data_ptr(), (int)E, C2, C1, P(dz), P<uint8_t>(arg), P(consts), k,
                              dZ2.data_ptr(), d.stream),
            "edge dz2 gemm");
    } else {
      dZ2 = at::empty({E, C2}, Z2.options());
      check(dgx_edge_mlp_dz_f32(P(dz), P<uint8_t>(arg), Z2.data_ptr(), (int)z16, B, N, k, C2, P(st2.scale), P(c2[2]),
                                P(c2[3]), dZ2.data_ptr(), d.stream),
            "edge dz2");
    }
    // ---- conv2 GEMMs: dH1 = dZ2 W2, dW2 = dZ2^T H1; then LReLU + BN1 backward
    if (have_prep && z16 && C1 == 64) {
      gw2 = at::empty({C2, C1}, d.f32);
      // dH1 never leaves the GEMM tile: its epilogue forms g = dH1 LReLU'(z1) (bf16)
      // and the BN1-backward column partials
      lds_atb(d, dZ2, H1, gw2, 0, decode(opts).slab_cap_mb, nullptr);
      rows = dgx_gemm_h1bwd_rows((int)E);
      part1 = at::empty({rows, 2, C1}, d.f32);
      gE = at::empty({E, C1}, d.bf16);
      check(dgx_gemm_h1bwd_bf16(dZ2.data_ptr(), tn.data_ptr(), (int)E, C1, C2, P(PQ), 2 * C1, P<int32_t>(idx), N, k,
                                P(st1.scale), P(st1.shift), P(st1.mean), P(st1.invstd), slope1, gE.data_ptr(),
                                P(part1), rows, d.stream),
            "edge h1 bwd gemm");
      g16 = 1;
    } else {
      if (have_prep && z16) {
        gE = lds_xwt(d, dZ2, tn, nullptr, false);
        gw2 = at::empty({C2, C1}, d.f32);
        lds_atb(d, dZ2, H1, gw2, 0, decode(opts).slab_cap_mb, nullptr);
      } else {
        Tensor W2 = w2.reshape({C2, C1}), dZ2f = dZ2.to(at::kFloat), H1f = H1.to(at::kFloat);
        gE = bf16 ? mm16(d, dZ2f, W2) : mm32(d, dZ2f, W2, nullptr, false);
        gw2 = bf16 ? mm16(d, dZ2f.t(), H1f) : mm32(d, dZ2f.t(), H1f, nullptr, false);
      }
      rows = dgx_edge_mlp_h1_bwd_rows(B, N, k, C1);
      part1 = at::empty({rows, 2, C1}, d.f32);
      check(dgx_edge_mlp_h1_bwd_f32(P(gE), P(PQ), 2 * C1, P<int32_t>(idx), B, N, k, C1, P(st1.scale), P(st1.shift),
                                    P(st1.mean), P(st1.invstd), slope1, P(part1), rows, d.stream),
            "edge h1 bwd");
      g16 = 0;
    }
  }
  auto c1 = backward_consts(d, part1, rows, (double)E, st1);   // dgamma1, dbeta1, e0, e1
  // ---- dP / dQ over the graph
  Tensor rowptr = at::empty({M + 1}, d.i32), edges = at::empty({E}, d.i32);
  check(dgx_graph_reverse(P<int32_t>(idx), B, N, k, P<int32_t>(rowptr), P<int32_t>(edges), d.stream), "reverse graph");
  Tensor dPQ = at::empty({M, 2 * C1}, d.f32);
  check(dgx_edge_mlp_scatter_f32(gE.data_ptr(), g16, P(PQ), 2 * C1, P(sumP1), P<int32_t>(rowptr), P<int32_t>(edges), B,
                                 N, k, C1, P(st1.scale), P(c1[2]), P(c1[3]), P(dPQ), d.stream),
        "edge h1 scatter");
  // ---- conv1 (K = C, tiny): dW1 = [dP^T X | dQ^T X], dX = dP W1a + dQ W1b
  Tensor gw1, dx = at::empty({0}, d.f32);
  if (bf16) {   // the engine's GEMMs (split-K over the M rows, un-stacked in the slab sum)
    gw1 = at::empty({C1, 2 * C}, d.f32);
    mm_atb(d, dPQ, X, gw1, C1, nullptr);
    if (x_needs_grad) {
      Tensor dX = at::empty({M, C}, d.f32);
      mm_xw(d, dPQ, split_weight(w1, C, C1), dX, false);
      dx = dX.view({B, N, C}).permute({0, 2, 1});
    }
  } else {
    Tensor dwcat = mm32(d, dPQ.t(), X, nullptr, false);   // (2C1, C)
    gw1 = at::cat({dwcat.narrow(0, 0, C1), dwcat.narrow(0, C1, C1)}, 1);
    if (x_needs_grad) dx = mm32(d, dPQ, split_weight(w1, C, C1), nullptr, false).view({B, N, C}).permute({0, 2, 1});
  }
  return {dx, gw1.reshape(w1.sizes()), c1[0], c1[1], gw2.view(w2.sizes()), c2[0], c2[1]};
}

// dgx_host::bn_batch_stats -> [scale, shift, mean, invstd] of one layer (dgx.bn.batch_stats)
std::vector<Tensor> bn_batch_stats(const Tensor& partials, int64_t rows, double count, const Tensor& gamma,
                                   const Tensor& beta, const c10::List<std::optional<Tensor>>& bn_t_l,
                                   std::vector<double> bn_f, std::vector<int64_t> bn_i, std::string group) {
  TORCH_CHECK(partials.scalar_type() == at::kFloat && partials.is_contiguous() &&
                  partials.numel() >= rows * 2 * gamma.size(0),
              "dgx bn: contiguous fp32 (rows, 2, C) partials expected");
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(partials.device());
  Dev d(partials);
  Stats st = batch_stats(d, partials, (int)rows, count, gamma, beta, parse_bn(to_vec(bn_t_l), bn_f, bn_i, {group}, 1, 6)[0]);
  return {st.scale, st.shift, st.mean, st.invstd};
}

// dgx_host::bn_backward_consts -> [dgamma, dbeta, c0, c1] (dgx.bn.backward_consts)
std::vector<Tensor> bn_backward_consts(const Tensor& partials, int64_t rows, double count, const Tensor& scale,
                                       const Tensor& mean, const Tensor& invstd, bool eval, std::string group) {
  TORCH_CHECK(partials.scalar_type() == at::kFloat && partials.is_contiguous() &&
                  partials.numel() >= rows * 2 * scale.size(0),
              "dgx bn: contiguous fp32 (rows, 2, C) partials expected");
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(partials.device());
  Dev d(partials);
  auto r = backward_consts(d, partials, (int)rows, count, Stats{scale, Tensor(), mean, invstd, group, eval});
  return {r[0], r[1], r[2], r[3]};
}

// ---- the GEMM helpers above as ops (dgx.gemm binds them: tests and tools drive the schedule's own GEMMs) ----
Tensor out_or_none(const std::optional<Tensor>& t) { return t.has_value() ? *t : Tensor(); }

// dgx_host::gemm_xwt -> (out, BN column partials or empty): lds ? lds_xwt : mm_xwt
std::tuple<Tensor, Tensor> gemm_xwt(const Tensor& x, const Tensor& w, std::optional<Tensor> out, bool stats,
                                    bool out_bf16, const std::optional<Tensor>& addend, bool lds) {
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  Dev d(x);
  Tensor o = out_or_none(out), add = out_or_none(addend), part;
  Tensor r = lds ? lds_xwt(d, x, w, stats ? &part : nullptr, out_bf16, add.defined() ? &add : nullptr,
                           o.defined() ? &o : nullptr)
                 : mm_xwt(d, x, w, stats ? &part : nullptr, o.defined() ? &o : nullptr);
  return {r, stats ? part : at::empty({0}, d.f32)};
}

// dgx_host::gemm_xw -> out (+)= x w (mm_xw)
Tensor gemm_xw(const Tensor& x, const Tensor& w, std::optional<Tensor> out, bool accumulate) {
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  Dev d(x);
  TORCH_CHECK(out.has_value() || !accumulate, "dgx gemm: accumulate needs an output to accumulate into");
  Tensor o = out.has_value() ? *out : at::empty({x.size(0), w.size(1)}, d.f32);
  mm_xw(d, x, w, o, accumulate);
  return o;
}

// dgx_host::gemm_atb: out = a^T b, lds ? lds_atb (with the slab cap) : mm_atb
void gemm_atb(const Tensor& a, const Tensor& b, Tensor out, int64_t split_rows, bool lds, int64_t slab_cap_mb) {
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(a.device());
  Dev d(a);
  if (lds) lds_atb(d, a, b, out, (int)split_rows, slab_cap_mb, nullptr);
  else mm_atb(d, a, b, out, (int)split_rows, nullptr);
}

// dgx_host::gemm32 -> out (mm32)
Tensor gemm32(const Tensor& a, const Tensor& b, std::optional<Tensor> out, bool accumulate,
              const std::optional<Tensor>& addend) {
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(a.device());
  Dev d(a);
  TORCH_CHECK(out.has_value() || !accumulate, "dgx mm32: accumulate=True needs an output to accumulate into");
  Tensor o = out_or_none(out), add = out_or_none(addend);
  return mm32(d, a, b, o.defined() ? &o : nullptr, accumulate, add.defined() ? &add : nullptr);
}

bool gemm_edge_dz_ok(const Tensor& dpq16, int64_t cin) { return edge_dz_ok(dpq16, (int)cin); }

std::vector<PrepJob> prep_jobs(at::TensorList weights, const std::vector<int64_t>& rows, const std::vector<int64_t>& cols,
                               const c10::List<bool>& stacked, const c10::List<bool>& split) {
  const size_t n = rows.size();
  TORCH_CHECK(cols.size() == n && stacked.size() == n && split.size() == n && (weights.empty() || weights.size() == n),
              "dgx weight prep: per-job lists differ in length");
  std::vector<PrepJob> jobs(n);
  for (size_t j = 0; j < n; ++j)
    jobs[j] = PrepJob{weights.empty() ? Tensor() : weights[j], (int)rows[j], (int)cols[j], stacked.get(j), split.get(j)};
  return jobs;
}

// dgx_host::weight_prep -> the shared bf16 buffer of prep_weights (filled in place when given)
Tensor weight_prep(at::TensorList weights, std::vector<int64_t> rows, std::vector<int64_t> cols,
                   const c10::List<bool>& stacked, const c10::List<bool>& split, std::optional<Tensor> buf) {
  TORCH_CHECK(!weights.empty(), "dgx weight prep: no weights");
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(weights[0].device());
  Dev d(weights[0]);
  return prep_weights(d, prep_jobs(weights, rows, cols, stacked, split), out_or_none(buf)).first;
}

// dgx_host::weight_prep_one -> (nt, tn) of one weight by the single-weight kernel (prep_weight)
std::tuple<Tensor, Tensor> weight_prep_one(const Tensor& w, int64_t rows, int64_t cols, bool stacked) {
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(w.device());
  Dev d(w);
  auto r = prep_weight(d, w, (int)rows, (int)cols, stacked);
  return {r.first, r.second};
}

// dgx_host::weight_prep_layout (host only) -> total elements, then per job the offset and (rows, cols) of the nt
// and tn views prep_views cuts — read off views of a meta buffer, so these are the schedule's own views
std::tuple<int64_t, std::vector<int64_t>, std::vector<int64_t>, std::vector<int64_t>, std::vector<int64_t>>
weight_prep_layout(std::vector<int64_t> rows, std::vector<int64_t> cols, const c10::List<bool>& stacked,
                   const c10::List<bool>& split) {
  auto jobs = prep_jobs(at::TensorList(), rows, cols, stacked, split);
  int64_t total = 0;
  prep_views(Tensor(), jobs, &total);
  std::vector<int64_t> nt_off, nt_shape, tn_off, tn_shape;
  for (const auto& v : prep_views(at::empty({total}, at::device(at::kMeta).dtype(at::kBFloat16)), jobs)) {
    nt_off.push_back(v.first.storage_offset());
    nt_shape.insert(nt_shape.end(), v.first.sizes().begin(), v.first.sizes().end());
    tn_off.push_back(v.second.storage_offset());
    tn_shape.insert(tn_shape.end(), v.second.sizes().begin(), v.second.sizes().end());
  }
  return {total, nt_off, nt_shape, tn_off, tn_shape};
}

// DGCNN.forward (dgcnn.py:80-103) as one op: the EdgeConv chain + conv5 forward and,
// from a C++ autograd node, the whole backward. Every mode (bf16 / fp32, train / eval,
// SyncBatchNorm) runs the chain_* / pointconv_* schedule above.
// process-group names through the autograd context as one string
constexpr char kSep = '\x1f';
std::string join(const std::vector<std::string>& v) {
  std::string r;
  for (size_t i = 0; i < v.size(); ++i) r += (i ? std::string(1, kSep) : std::string()) + v[i];
  return r;
}
std::vector<std::string> split(const std::string& s, int n) {
  std::vector<std::string> r(1);
  for (char ch : s) {
    if (ch == kSep) r.emplace_back();
    else r.back() += ch;
  }
  TORCH_CHECK((int)r.size() == n, "dgx: process-group list does not match the layer count");
  return r;
}

struct Config {
  int64_t k;
  bool bf16;
  int64_t opts;
  std::vector<double> bn_f;
  std::vector<int64_t> bn_i;
  std::vector<std::string> groups;
};

std::vector<Layer> dgcnn_layers(at::TensorList params, const std::vector<std::optional<Tensor>>& bufs,
                                const Config& c, int L) {
  std::vector<Tensor> w, g, b;
  std::vector<double> slopes;
  for (int l = 0; l < L; ++l) {
    w.push_back(params[3 * l]);
    g.push_back(params[3 * l + 1]);
    b.push_back(params[3 * l + 2]);
    slopes.push_back(c.bn_f[3 * l + 2]);
  }
  return make_layers(w, g, b, parse_bn(bufs, c.bn_f, c.bn_i, c.groups, L, 3), slopes);
}

struct DgcnnRun {
  ChainOut chain;
  PcState pc;
  Tensor out;
};

DgcnnRun dgcnn_run(const Dev& d, const Tensor& x, std::vector<Layer>& all, const Config& c, const Tensor& idx0,
                   bool need_grad) {
  const int L = (int)all.size();
  std::vector<Layer> blocks(all.begin(), all.end() - 1);
  Layer& c5 = all.back();
  const int B = (int)x.size(0), N = (int)x.size(2);
  // one launch for every bf16 operand copy of the step (blocks 2.., conv5)
  std::vector<std::pair<Tensor, Tensor>> views;
  Tensor pbuf;
  std::vector<PrepJob> jobs;
  if (c.bf16) {
    jobs = chain_prep_jobs(blocks);
    jobs.push_back({c5.w.reshape({c5.w.size(0), c5.w.size(1)}), (int)c5.w.size(0), (int)c5.w.size(1), false, false});
    auto pw = prep_weights(d, jobs);
    pbuf = pw.first;
    views = pw.second;
  }
  DgcnnRun r;
  const Opts o = decode(c.opts);
  r.chain = chain_forward_impl(d, x, (int)c.k, blocks, c.bf16, need_grad, c.bf16 ? &views : nullptr, idx0, o);
  r.chain.prep = pbuf;
  Tensor nt5, tn5;
  if (c.bf16) {   // conv5's copies: the job after the blocks'
    nt5 = views[L - 2].first;
    tn5 = views[L - 2].second;
  }
  TORCH_CHECK(c5.w.size(1) == r.chain.xcat.size(1), "dgx dgcnn: conv5 takes the concat of the blocks");
  r.out = pointconv_forward_impl(d, r.chain.xcat, r.chain.have16 ? r.chain.xcat16 : Tensor(), B, N, c5, c.bf16, nt5,
                                 tn5, &r.pc, o.split32);
  return r;
}

class DgcnnFn : public torch::autograd::Function<DgcnnFn> {
 public:
  static variable_list forward(AutogradContext* ctx, Tensor x, at::TensorList params,
                               std::vector<std::optional<Tensor>> bufs, std::optional<Tensor> idx0, Config c) {
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
    Dev d(x);
    const int L = (int)params.size() / 3;
    auto all = dgcnn_layers(params, bufs, c, L);
    DgcnnRun r = dgcnn_run(d, x, all, c, defined_or_none(idx0), true);
    // x through save_for_backward: its version counter guards the point-major rows (a view of x)
    std::vector<Tensor> to_save{x};
    to_save.insert(to_save.end(), params.begin(), params.end());
    ctx->save_for_backward(to_save);
    std::vector<Tensor> state = r.chain.saved;
    state.push_back(r.chain.xcat);
    state.push_back(r.chain.xcat16);
    state.push_back(r.chain.prep.defined() ? r.chain.prep : at::empty({0}, d.bf16));
    auto pcs = r.pc.pack(d);
    state.insert(state.end(), pcs.begin(), pcs.end());
    ctx->saved_data["state"] = at::IValue(c10::List<Tensor>(state));
    ctx->saved_data["k"] = c.k;
    ctx->saved_data["bf16"] = c.bf16;
    ctx->saved_data["opts"] = c.opts;
    ctx->saved_data["bn_f"] = at::IValue(c.bn_f);
    std::vector<int64_t> eval;
    for (auto& s : r.chain.stats) eval.push_back(s.eval);
    eval.push_back(r.pc.st.eval);
    ctx->saved_data["eval"] = at::IValue(eval);
    ctx->saved_data["groups"] = join(c.groups);
    return {r.out};
  }

  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    auto sv = ctx->get_saved_variables();
    const Tensor& x = sv[0];
    std::vector<Tensor> params(sv.begin() + 1, sv.end());
    const int L = (int)params.size() / 3, n = L - 1;
    // one gradient per forward input: x, each parameter, then bufs / idx0 / config (none)
    variable_list flat(1 + params.size() + 3);
    Tensor dout = grads[0];
    if (!dout.defined()) return flat;
    auto sl = ctx->saved_data["state"].toTensorList();
    std::vector<Tensor> S(sl.begin(), sl.end());
    const int k = (int)ctx->saved_data["k"].toInt();
    const bool bf16 = ctx->saved_data["bf16"].toBool();
    const Opts o = decode(ctx->saved_data["opts"].toInt());
    auto bn_f = ctx->saved_data["bn_f"].toDoubleVector();
    auto eval = ctx->saved_data["eval"].toIntVector();
    std::vector<std::string> groups = split(ctx->saved_data["groups"].toStringRef(), L);
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
    Dev d(x);
    const int B = (int)x.size(0), C0 = (int)x.size(1), N = (int)x.size(2);
    const size_t nsaved = 1 + kPerLayer * n;
    std::vector<Tensor> saved(S.begin(), S.begin() + nsaved);
    const Tensor &xcat = S[nsaved], &xcat16 = S[nsaved + 1], &pbuf = S[nsaved + 2];
    TORCH_CHECK(S.size() == nsaved + 3 + kNumPcFields, "dgx dgcnn backward: saved state does not match the layer count");
    const Tensor& w5 = params[3 * n];
    PcState pc = PcState::unpack(&S[nsaved + 3], groups[n], eval[n] != 0, w5, bf16, B, N, bn_f[3 * n + 2]);
    std::vector<Layer> blocks(n);
    for (int l = 0; l < n; ++l) blocks[l] = weight_layer(params[3 * l], bn_f[3 * l + 2]);
    std::vector<std::pair<Tensor, Tensor>> views;
    if (pbuf.numel()) views = prep_views(pbuf, chain_prep_jobs(blocks));
    auto st = stats_from_saved(saved, n, eval, groups);
    SlabJobs slabs;   // every weight gradient's slab sum, as few launches as possible at the end
    auto pg = pointconv_backward_impl(d, dout, pc, &slabs);
    ChainGrads g = chain_backward_impl(d, pg[0], true, xcat, xcat16, saved, blocks, st, views, B, C0, N, k, bf16,
                                       ctx->needs_input_grad(0), o, &slabs);
    slabs.flush(d.stream);
    std::vector<Tensor> pgrads;
    for (int l = 0; l < n; ++l) pgrads.insert(pgrads.end(), {g.dw[l], g.dgamma[l], g.dbeta[l]});
    pgrads.insert(pgrads.end(), {pg[1].view(w5.sizes()), pg[2], pg[3]});
    flat[0] = g.dx;
    for (size_t j = 0; j < pgrads.size(); ++j) flat[1 + j] = pgrads[j];
    return flat;
  }
};

Tensor dgcnn(const Tensor& x, at::TensorList params, const c10::List<std::optional<Tensor>>& bufs_l,
             std::vector<double> bn_f, std::vector<int64_t> bn_i, std::vector<std::string> groups,
             const std::optional<Tensor>& idx0, int64_t k, bool bf16, int64_t opts) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kFloat && x.dim() == 3, "dgx dgcnn: fp32 (B,C,N) device cloud");
  TORCH_CHECK(params.size() % 3 == 0 && params.size() >= 6, "dgx dgcnn: (w, gamma, beta) per layer");
  auto bufs = to_vec(bufs_l);
  const int L = (int)params.size() / 3;
  TORCH_CHECK((int)bufs.size() == 3 * L && (int)bn_f.size() == 3 * L && (int)bn_i.size() == 2 * L &&
                  (int)groups.size() == L,
              "dgx dgcnn: per-layer BatchNorm lists do not match");
  for (const auto& p : params) TORCH_CHECK(p.scalar_type() == at::kFloat && p.is_cuda(), "dgx: fp32 device parameters");
  Config c{k, bf16, opts, std::move(bn_f), std::move(bn_i), std::move(groups)};
  bool need_grad = at::GradMode::is_enabled() && x.requires_grad();
  for (const auto& p : params) need_grad = need_grad || (at::GradMode::is_enabled() && p.requires_grad());
  if (!need_grad) {   // inference / no_grad: the forward only, nothing saved
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
    Dev d(x);
    auto all = dgcnn_layers(params, bufs, c, L);
    return dgcnn_run(d, x, all, c, defined_or_none(idx0), false).out;
  }
  return DgcnnFn::apply(x, params, bufs, idx0, c)[0];
}

// ---- kNN, reverse graphs and the graph feature as ops (dgx.ops binds them) ----
// dgx_host::knn -> [ids] or [ids, values] (knn above); xx / image: prepared operands
std::vector<Tensor> knn_op(const Tensor& x, int64_t k, int64_t order, at::ScalarType ids, bool values, bool generic,
                           const std::optional<Tensor>& xx, const std::optional<Tensor>& image) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 3 && x.scalar_type() == at::kFloat, "knn: a (B, C, N) fp32 device view expected");
  TORCH_CHECK(ids == at::kInt || ids == at::kLong, "knn: ids are int32 or int64");
  TORCH_CHECK(xx.has_value() == image.has_value() &&
                  (!xx.has_value() || (xx->options().type_equal(x.options()) && image->options().type_equal(x.options()) &&
                                       xx->device() == x.device() && image->device() == x.device())),
              "knn: prepared operands are |x|^2 and the image, fp32 buffers on the cloud's device");
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  Dev d(x);
  std::pair<Tensor, Tensor> prepared;
  if (xx.has_value()) prepared = {*xx, *image};
  auto r = knn(d, x, (int)std::clamp<int64_t>(k, 0, INT32_MAX), (int)order, ids, values, generic,
               xx.has_value() ? &prepared : nullptr);
  return values ? std::vector<Tensor>{r.first, r.second} : std::vector<Tensor>{r.first};
}

std::tuple<Tensor, Tensor> knn_image_buffers_op(int64_t B, int64_t C, int64_t N, at::Device dev) {
  auto r = knn_image_buffers(at::TensorOptions().device(dev).dtype(at::kFloat), (int)B, (int)C, (int)N);
  return {r.first, r.second};
}

void check_ids(const Tensor& idx) {
  TORCH_CHECK(idx.is_cuda() && idx.dim() == 3 && idx.scalar_type() == at::kInt && idx.is_contiguous(),
              "dgx: kNN ids must be contiguous int32 (B, N, k)");
}

// dgx_host::reverse_graphs -> the graphs' rowptr tensors, then their edges tensors
std::vector<Tensor> reverse_graphs_op(at::TensorList idxs) {
  TORCH_CHECK(!idxs.empty(), "dgx reverse graphs: no graphs");
  for (const auto& idx : idxs) {
    check_ids(idx);
    TORCH_CHECK(idx.sizes() == idxs[0].sizes() && idx.device() == idxs[0].device(),
                "dgx reverse graphs: graphs of one shape on one device expected");
  }
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(idxs[0].device());
  auto r = reverse_graphs(Dev(idxs[0]), idxs.vec(), (int)idxs[0].size(0), (int)idxs[0].size(1), (int)idxs[0].size(2));
  r.first.insert(r.first.end(), r.second.begin(), r.second.end());
  return r.first;
}

// dgx_host::graph_feature -> get_graph_feature's edge tensor (dgcnn.py:15-44), contiguous in the layout of `mode`
Tensor graph_feature(const Tensor& x, const Tensor& idx, int64_t mode) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 3 && x.scalar_type() == at::kFloat, "graph_feature: (B, C, N) fp32 expected");
  check_ids(idx);
  const int64_t B = x.size(0), C = x.size(1), N = x.size(2), k = idx.size(2);
  TORCH_CHECK(idx.size(0) == B && idx.size(1) == N && idx.device() == x.device(),
              "graph_feature: ids do not match the cloud");
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  Dev d(x);
  const std::vector<int64_t> shape = mode == DGX_GF_KNN_ONLY ? std::vector<int64_t>{B, N, k, C}
                                                             : std::vector<int64_t>{B, mode == DGX_GF_DISP ? C : 2 * C, N, k};
  Tensor out = at::empty(shape, d.f32);
  check(dgx_graph_feature_f32(P(x), x.stride(0), x.stride(1), x.stride(2), (int)B, (int)C, (int)N, P<int32_t>(idx),
                              (int)k, (int)mode, P(out), d.stream),
        "graph_feature");
  return out;
}

// dgx_host::graph_feature_backward -> dx (B, C, N): the deterministic CSR pull where it takes the shape, else atomics
Tensor graph_feature_backward(Tensor dout, const Tensor& idx, int64_t C, int64_t mode) {
  check_ids(idx);
  TORCH_CHECK(dout.device() == idx.device(), "graph_feature backward: gradient and ids on one device expected");
  const int B = (int)idx.size(0), N = (int)idx.size(1), k = (int)idx.size(2);
  TORCH_CHECK(C >= 1 && dout.numel() == idx.numel() * C * (mode == DGX_GF_CAT || mode == DGX_GF_DIFFCAT ? 2 : 1),
              "graph_feature backward: gradient does not match the edge tensor of mode ", mode);
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(dout.device());
  Dev d(dout);
  dout = dout.contiguous().to(at::kFloat);
  Tensor dx = at::zeros({B, C, N}, d.f32);
  if (k <= 64 && (int64_t)B * N < ((int64_t)1 << 25)) {
    const auto [rowptr, edges] = reverse_graphs(d, {idx}, B, N, k);
    check(dgx_graph_feature_bwd_csr_f32(P(dout), B, (int)C, N, k, (int)mode, P<int32_t>(rowptr[0]), P<int32_t>(edges[0]),
                                        P(dx), d.stream),
          "graph_feature backward");
  } else {
    check(dgx_graph_feature_bwd_f32(P(dout), B, (int)C, N, P<int32_t>(idx), k, (int)mode, P(dx), d.stream),
          "graph_feature backward");
  }
  return dx;
}

// dgx_host::vattn_forward -> agg (B*N, Dm): the fused kNN vector attention (attention.py:115-150, csrc/vattn.hip).
// weights: pos_mlp's and attn_mlp's (w1, b1, w2, b2), nn.Linear layout
Tensor vattn_forward(const Tensor& D, const Tensor& V, const Tensor& pos, const Tensor& idx, int64_t gather_stride,
                     at::TensorList weights, bool bf16) {
  check_ids(idx);
  const int64_t B = idx.size(0), N = idx.size(1), k = idx.size(2);
  auto dense = [&](const Tensor& t) {
    return t.is_cuda() && t.device() == idx.device() && t.scalar_type() == at::kFloat && t.is_contiguous();
  };
  TORCH_CHECK(dense(D) && dense(V) && D.dim() == 2 && D.sizes() == V.sizes(),
              "vattn: D and V are contiguous fp32 (rows, Dm) tables on the ids' device");
  TORCH_CHECK(dense(pos) && pos.dim() == 2 && pos.size(0) == B * N && pos.size(1) == 3,
              "vattn: pos is a contiguous fp32 (B*N, 3) table");
  TORCH_CHECK(weights.size() == 8, "vattn: pos_mlp and attn_mlp weights (w1, b1, w2, b2 each) expected");
  for (const auto& w : weights) TORCH_CHECK(dense(w), "vattn: weights are contiguous fp32 on the ids' device");
  const int64_t Dm = D.size(1), Hp = weights[0].size(0), H = weights[4].size(0);
  const std::vector<int64_t> want[8] = {{Hp, 3}, {Hp}, {Dm, Hp}, {Dm}, {H, Dm}, {H}, {Dm, H}, {Dm}};
  for (int j = 0; j < 8; ++j) TORCH_CHECK(weights[j].sizes() == want[j], "vattn: weight ", j, " has the wrong shape");
  TORCH_CHECK(gather_stride >= 0 && (B == 0 || (B - 1) * gather_stride + N <= D.size(0)),
              "vattn: gathered rows leave the tables");
  TORCH_CHECK(B * N < ((int64_t)1 << 31) && dgx_vattn_fused_shape((int)Dm, (int)H, (int)Hp, (int)k),
              "vattn: no fused kernel for Dm ", Dm, ", H ", H, ", Hp ", Hp, ", k ", k);
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(idx.device());
  Dev d(idx);
  Tensor agg = at::empty({B * N, Dm}, d.f32);
  check(dgx_vattn_fwd(P(D), P(V), D.size(0), P(pos), P<int32_t>(idx), (int)B, (int)N, (int)k, gather_stride,
                      P(weights[0]), P(weights[1]), P(weights[2]), P(weights[3]), P(weights[4]), P(weights[5]),
                      P(weights[6]), P(weights[7]), (int)Dm, (int)H, (int)Hp, bf16 ? 1 : 0, P(agg), d.stream),
        "vattn forward");
  return agg;
}

// dgx_host::knn_timing(on): on = true clears and starts recording this thread's kNN
// selection launches; on = false stops and returns [ms, flops, B, C, N, k] per launch
std::vector<double> knn_timing(bool on) {
  std::vector<double> out;
  if (on) {
    for (auto& r : t_knn_recs) {
      (void)hipEventDestroy(r.e0);
      (void)hipEventDestroy(r.e1);
    }
    t_knn_recs.clear();
    t_knn_timing = true;
    return out;
  }
  t_knn_timing = false;
  for (auto& r : t_knn_recs) {
    float ms = 0.f;
    (void)hipEventSynchronize(r.e1);
    (void)hipEventElapsedTime(&ms, r.e0, r.e1);
    out.insert(out.end(), {(double)ms, r.flops, (double)r.B, (double)r.C, (double)r.N, (double)r.k});
    (void)hipEventDestroy(r.e0);
    (void)hipEventDestroy(r.e1);
  }
  t_knn_recs.clear();
  return out;
}

// dgx_host::layout(): this file's name tables (dgx.schedule holds the same ones; a test compares them)
std::tuple<std::vector<std::string>, std::vector<std::string>, std::vector<std::string>, std::vector<std::string>>
layout() {
  return {{kChainNames, kChainNames + kPerLayer},
          {kPcNames, kPcNames + kNumPcFields},
          {kOptNames, kOptNames + kNumOptBits},
          {kEmlpNames, kEmlpNames + kNumEmlpFields}};
}

}  // namespace

TORCH_LIBRARY(dgx_host, m) {
  m.def("chain_forward(Tensor x, int k, Tensor[] weights, Tensor[] gammas, Tensor[] betas, Tensor?[] bn_t, "
        "float[] bn_f, int[] bn_i, str[] groups, float[] slopes, bool bf16, bool need_grad, Tensor? prep, "
        "Tensor? idx0, int opts) -> (Tensor, Tensor, Tensor[], Tensor)");
  m.def("chain_backward(Tensor dxcat, Tensor xcat, Tensor xcat16, Tensor[] saved, Tensor[] weights, Tensor? prep, "
        "int[] shape, int k, int[] eval, str[] groups, float[] slopes, bool bf16, bool x_needs_grad, int opts) "
        "-> (Tensor, Tensor[], Tensor[], Tensor[])");
  m.def("pointconv_forward(Tensor X, Tensor X16, int B, int N, Tensor weight, Tensor gamma, Tensor beta, "
        "Tensor?[] bn_t, float[] bn_f, int[] bn_i, str group, bool bf16, Tensor? nt, Tensor? tn, int opts) "
        "-> (Tensor, Tensor[])");
  m.def("pointconv_backward(Tensor dout, Tensor[] saved, Tensor weight, int B, int N, float slope, bool eval, "
        "str group, bool bf16, int opts) -> (Tensor, Tensor, Tensor, Tensor)");
  m.def("dgcnn(Tensor x, Tensor[] params, Tensor?[] bufs, float[] bn_f, int[] bn_i, str[] groups, Tensor? idx0, "
        "int k, bool bf16, int opts) -> Tensor");
  m.def("knn(Tensor x, int k, int order, ScalarType ids, bool values, bool generic, Tensor? xx, Tensor? image) "
        "-> Tensor[]");
  m.def("knn_image_buffers(int B, int C, int N, Device device) -> (Tensor, Tensor)", &knn_image_buffers_op);
  m.def("knn_timing(bool on) -> float[]", &knn_timing);
  m.def("reverse_graphs(Tensor[] idxs) -> Tensor[]");
  m.def("graph_feature(Tensor x, Tensor idx, int mode) -> Tensor");
  m.def("graph_feature_backward(Tensor dout, Tensor idx, int C, int mode) -> Tensor");
  m.def("vattn_forward(Tensor D, Tensor V, Tensor pos, Tensor idx, int gather_stride, Tensor[] weights, bool bf16) "
        "-> Tensor");
  m.def("edge_mlp2_forward(Tensor x, Tensor idx, int k, Tensor w1, Tensor g1, Tensor b1, Tensor w2, Tensor g2, "
        "Tensor b2, Tensor?[] bn_t, float[] bn_f, int[] bn_i, str[] groups, bool bf16, bool need_grad, "
        "bool fused_bwd) -> (Tensor, Tensor[])");
  m.def("edge_mlp2_backward(Tensor dout, Tensor[] saved, Tensor w1, Tensor w2, int[] shape, int k, int[] eval, "
        "str[] groups, float[] slopes, bool bf16, bool x_needs_grad, int opts) "
        "-> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)");
  m.def("bn_batch_stats(Tensor partials, int rows, float count, Tensor gamma, Tensor beta, Tensor?[] bn_t, "
        "float[] bn_f, int[] bn_i, str group) -> Tensor[]");
  m.def("bn_backward_consts(Tensor partials, int rows, float count, Tensor scale, Tensor mean, Tensor invstd, "
        "bool eval, str group) -> Tensor[]");
  m.def("gemm_xwt(Tensor x, Tensor w, Tensor(a!)? out, bool stats, bool out_bf16, Tensor? addend, bool lds) "
        "-> (Tensor(a), Tensor)");
  m.def("gemm_xw(Tensor x, Tensor w, Tensor(a!)? out, bool accumulate) -> Tensor(a)");
  m.def("gemm_atb(Tensor a, Tensor b, Tensor(c!) out, int split_rows, bool lds, int slab_cap_mb) -> ()");
  m.def("gemm32(Tensor a, Tensor b, Tensor(c!)? out, bool accumulate, Tensor? addend) -> Tensor(c)");
  m.def("gemm_edge_dz_ok(Tensor dpq16, int cin) -> bool");
  m.def("weight_prep(Tensor[] weights, int[] rows, int[] cols, bool[] stacked, bool[] split, Tensor(a!)? buf) "
        "-> Tensor(a)");
  m.def("weight_prep_one(Tensor w, int rows, int cols, bool stacked) -> (Tensor, Tensor)");
  m.def("weight_prep_layout(int[] rows, int[] cols, bool[] stacked, bool[] split) -> (int total, int[] nt_offset, "
        "int[] nt_shape, int[] tn_offset, int[] tn_shape)", &weight_prep_layout);
  m.def("layout() -> (str[] chain_fields, str[] pointconv_fields, str[] opts_bits, str[] edge_mlp_fields)", &layout);
}

TORCH_LIBRARY_IMPL(dgx_host, CompositeImplicitAutograd, m) {
  m.impl("dgcnn", dgcnn);
}

TORCH_LIBRARY_IMPL(dgx_host, CompositeExplicitAutograd, m) {
  m.impl("chain_forward", chain_forward);
  m.impl("chain_backward", chain_backward);
  m.impl("pointconv_forward", pointconv_forward);
  m.impl("pointconv_backward", pointconv_backward);
  m.impl("edge_mlp2_forward", edge_mlp2_forward);
  m.impl("edge_mlp2_backward", edge_mlp2_backward);
  m.impl("bn_batch_stats", bn_batch_stats);
  m.impl("bn_backward_consts", bn_backward_consts);
  m.impl("gemm_xwt", gemm_xwt);
  m.impl("gemm_xw", gemm_xw);
  m.impl("gemm_atb", gemm_atb);
  m.impl("gemm32", gemm32);
  m.impl("gemm_edge_dz_ok", gemm_edge_dz_ok);
  m.impl("weight_prep", weight_prep);
  m.impl("weight_prep_one", weight_prep_one);
  m.impl("knn", knn_op);
  m.impl("reverse_graphs", reverse_graphs_op);
  m.impl("graph_feature", graph_feature);
  m.impl("graph_feature_backward", graph_feature_backward);
  m.impl("vattn_forward", vattn_forward);
}
