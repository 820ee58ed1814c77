"""dgx.pointconv.pointconv_bn_lrelu (conv5 of reference models/dgcnn.py:74-78,
100-102, conv6 of model.DGCNN_semseg) against a plain torch float64 reference
written here — F.conv1d on the (B, K, N) view, F.batch_norm with the module's
flags, F.leaky_relu, .backward(gout) — on every route of pointconv_forward_impl
/ pointconv_backward_impl (csrc/dgx_torch.cpp) at a tile edge.

Route of each case of CASES (N from the kernel oracle's list; 682 / 683 put
B N on both sides of the fp32 weight gradient's split-K switch at 2048 rows):

  id            mode        forward GEMM / statistics            backward
  mm32-70       fp32        mm32, colstats, apply_T (Co % 4)     bwd_T, input_grad, mm32 x2
  mm32-1d       fp32        mm32, colstats, apply32_lt           bwd_T, input_grad, mm32 x2
  mm32-eval     fp32        mm32, running statistics             eval-mode affine, mm32 x2
  dw-2046       fp32        mm32                                 dW = mm32 unsplit (B N < 2048)
  dw-2049       fp32        mm32                                 dW = mm32 split-K (B N >= 2048)
  split-64      fp32_split  3-pass lds_xwt, colstats             bwd32_stats/split_lt, lds_atb_sum, lds_xwt x2
  split-128     fp32_split  3-pass lds_xwt, colstats             the same, two channel groups
  split-eval    fp32_split  3-pass lds_xwt, running statistics   the same, eval-mode constants
  split-no-96   fp32_split  refused (Co % 64): mm32              bwd_T, input_grad, mm32 x2
  split-no-45   fp32_split  refused (K % 64): mm32               the same
  xwt-45        bf16        mm_xwt + epilogue statistics (K 45)  bwd_T, input_grad bf16, mm_atb, mm_xw
  xwt-notwin    bf16        mm_xwt + epilogue statistics         the same (no twin)
  xwt-eval      bf16        mm_xwt, running statistics           eval-mode constants, mm_atb, mm_xw
                            (N 3 in bf16 mode only with running statistics, here and in a-70-eval: batch
                            statistics over 3 or 9 samples amplify the operand rounding by 1 / sigma of
                            the sample, without bound: B 1, N 3, Co 128 gives an output error of 0.10
                            against the unrounded reference, which is the reference's own sensitivity)
  lds-128       bf16, twin  lds_xwt, bf16 Z, bf16-store stats    bwd16_stats/dz_lt, lds_atb, lds_xwt
  lds-eval      bf16, twin  lds_xwt, fp32 Z, running statistics  bwd_T, input_grad bf16, lds_atb, lds_xwt
  a-96/68/70    bf16, twin  Co % 64 != 0: the backward's LDS GEMMs do not take dZ (inner dimension Co
                            for dX, Co rows for dW), so conv5 stays on mm_xwt / mm_atb / mm_xw. Before
                            this rule the forward took lds_xwt and .backward() raised "gemm lds nt
                            failed (-2)"; DGCNN(emb_dim=96) in bf16 mode is the model-level case.

LeakyReLU decisions: the fp64 reference cannot reproduce a sign taken from a
value that the engine computed with rounded operands, and one flipped sign
moves a whole row of dX by more than any bar. So the forward is compared with
the plain reference, the engine's signs are validated — they may differ from
the reference's only where |y| is below the mode's first-order error bound of
y itself, |gamma invstd| eps (|X| |W|^T) with eps = (K + 8) 2^-24 (fp32
accumulation), 2^-14 (three split-bf16 products of 2^-16 each) or 2^-7 (two
bf16 roundings of 2^-9 per product, doubled for the shift of the statistics)
— and the backward reference follows the validated signs.

BatchNorm conditioning (test_bn_conditioning_*): statistics are raw fp32
(sum z, sum z^2) block sums finalised as E[z^2] - E[z]^2, so the variance loses
about 2 r^2 2^-24 relative with r = |mean| / std. Constants c in
"relative variance error <= c (1 + r^2) 2^-24" measured on an MI355X over 5
seeds, Co 64 and 68 (profiles/bn_conditioning.log), variance / mean:
  colstats (fp32 mode)                       2.712 / 1.974   asserted at 8 / 8 (4x the simulated 2 r^2 2^-24)
  register-staged GEMM epilogue (bf16)       2.709 / 1.747   asserted at 4x
  LDS GEMM bf16-store epilogue (bf16, twin)  2.709 / 1.747   asserted at 4x (same tiles and sum order as above)
  EdgeConv gather partials (fp32 mode)       2.641 / 1.599   asserted at 4x
  torch F.batch_norm in fp32 on the same Z   2.80 / 6.5 at most, for the record
No producer exceeds 16x colstats. fp32-mode output error of the r = 64 channels
against the fp64 reference: 2.51e-4 at most (asserted at 4x); r <= 4: 1.2e-6;
r = 256: up to 4.3e-3, past the 1e-3 bar.
"""
import copy
import types

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err
from _pointconv_ref import U

SLOPE = 0.2
# id, mode, K, Co, B, N, twin, train, momentum, conv, route (route_of)
CASES = [
    ("mm32-70", "fp32", 45, 70, 1, 130, False, True, 0.1, "2d", "mm32"),
    ("mm32-1d", "fp32", 64, 128, 3, 257, False, True, None, "1d", "mm32"),
    ("mm32-eval", "fp32", 45, 68, 3, 3, False, False, 0.1, "1d", "mm32"),
    ("dw-2046", "fp32", 64, 68, 3, 682, False, True, 0.1, "2d", "mm32"),
    ("dw-2049", "fp32", 64, 68, 3, 683, False, True, 0.1, "2d", "mm32"),
    ("split-64", "fp32_split", 64, 64, 3, 257, False, True, 0.1, "2d", "split"),
    ("split-128", "fp32_split", 64, 128, 1, 384, False, True, None, "1d", "split"),
    ("split-eval", "fp32_split", 64, 64, 1, 130, False, False, 0.1, "2d", "split"),
    ("split-no-96", "fp32_split", 64, 96, 3, 130, False, True, 0.1, "2d", "mm32"),
    ("split-no-45", "fp32_split", 45, 64, 1, 257, False, True, None, "1d", "mm32"),
    ("xwt-45", "bf16", 45, 68, 3, 257, True, True, 0.1, "2d", "xwt"),
    ("xwt-notwin", "bf16", 64, 128, 3, 130, False, True, None, "1d", "xwt"),
    ("xwt-eval", "bf16", 64, 70, 1, 3, False, False, 0.1, "1d", "xwt"),
    ("lds-128", "bf16", 64, 128, 3, 130, True, True, 0.1, "2d", "lds16"),
    ("lds-128-1d", "bf16", 128, 128, 1, 257, True, True, None, "1d", "lds16"),
    ("lds-eval", "bf16", 64, 64, 1, 384, True, False, 0.1, "2d", "lds32"),
    ("a-96", "bf16", 64, 96, 3, 257, True, True, 0.1, "2d", "xwt"),
    ("a-68", "bf16", 64, 68, 1, 130, True, True, None, "1d", "xwt"),
    ("a-70", "bf16", 64, 70, 3, 384, True, True, 0.1, "2d", "xwt"),
    ("a-96-eval", "bf16", 64, 96, 1, 130, True, False, 0.1, "1d", "xwt"),
    ("a-70-eval", "bf16", 64, 70, 3, 3, True, False, 0.1, "2d", "xwt"),
]
IDS = [c[0] for c in CASES]
BAR = {"fp32": 1e-3, "fp32_split": 1e-3, "bf16": 2e-2}
NBT0 = 3   # batches already tracked: momentum=None then averages with factor 1 / 4


def decision_eps(mode, K):
    return {"fp32": (K + 8) * U, "fp32_split": 2.0 ** -14, "bf16": 2.0 ** -7}[mode]


def make_seq(K, Co, conv, momentum, seed):
    g = torch.Generator().manual_seed(seed)
    if conv == "2d":
        seq = torch.nn.Sequential(torch.nn.Conv2d(K, Co, 1, bias=False), torch.nn.BatchNorm2d(Co, momentum=momentum),
                                  torch.nn.LeakyReLU(SLOPE))
    else:
        seq = torch.nn.Sequential(torch.nn.Conv1d(K, Co, 1, bias=False), torch.nn.BatchNorm1d(Co, momentum=momentum),
                                  torch.nn.LeakyReLU(SLOPE))
    with torch.no_grad():
        seq[0].weight.copy_((torch.randn(Co, K, generator=g) / K ** 0.5).view_as(seq[0].weight))
        seq[1].weight.copy_(torch.randn(Co, generator=g))            # both signs
        seq[1].bias.copy_(0.3 * torch.randn(Co, generator=g))
        seq[1].running_mean.copy_(torch.linspace(-0.2, 0.2, Co))
        seq[1].running_var.copy_(torch.linspace(0.5, 2.0, Co))
        seq[1].num_batches_tracked.fill_(NBT0)
    return seq


def make_data(K, Co, B, N, seed):
    g = torch.Generator().manual_seed(seed + 1)
    return torch.randn(B * N, K, generator=g), torch.randn(B, Co, N, generator=g)


class Ref64:
    """The float64 reference of one call: forward at construction, ``backward``
    with the LeakyReLU signs to follow (None: its own)."""

    def __init__(self, X, seq, B, N, train, momentum, mode="fp32"):
        conv, bn = seq[0], seq[1]
        Co, K = conv.weight.shape[0], conv.weight.shape[1]
        self.x = X.detach().double().clone().requires_grad_(True)
        self.w = conv.weight.detach().double().reshape(Co, K, 1).clone().requires_grad_(True)
        self.gamma = bn.weight.detach().double().clone().requires_grad_(True)
        self.beta = bn.bias.detach().double().clone().requires_grad_(True)
        self.rm = bn.running_mean.detach().double().clone()
        self.rv = bn.running_var.detach().double().clone()
        self.nbt = int(bn.num_batches_tracked) + (1 if train else 0)
        factor = momentum if momentum is not None else 1.0 / self.nbt
        self.z = F.conv1d(self.x.view(B, N, K).permute(0, 2, 1), self.w)
        self.y = F.batch_norm(self.z, self.rm, self.rv, self.gamma, self.beta, train, factor, bn.eps)
        self.out = F.leaky_relu(self.y, SLOPE)
        with torch.no_grad():
            if train and mode == "bf16":
                # running statistics at 1e-5: of the product of the operands the mode uses (bf16-rounded)
                z16 = X.detach().bfloat16().double() @ conv.weight.detach().reshape(Co, K).bfloat16().double().t()
                n = z16.shape[0]
                self.rm = (1 - factor) * bn.running_mean.detach().double() + factor * z16.mean(0)
                self.rv = (1 - factor) * bn.running_var.detach().double() + factor * z16.var(0, unbiased=n > 1)
            if train:
                invstd = (self.z.var(dim=(0, 2), unbiased=False) + bn.eps).rsqrt()
            else:
                invstd = (bn.running_var.detach().double().to(self.z.device) + bn.eps).rsqrt()
            self.a = (self.gamma * invstd).abs()

    def check_signs(self, pos, mode):
        """engine signs ``pos`` (B, Co, N) may differ from the reference's only below the error bound of y"""
        with torch.no_grad():
            K = self.x.shape[1]
            B, Co, N = self.y.shape
            mag = (self.x.abs() @ self.w.abs().view(Co, K).t()).view(B, N, Co).permute(0, 2, 1)
            tol = self.a.view(1, Co, 1) * decision_eps(mode, K) * mag
            bad = pos != (self.y > 0)
            assert bool((self.y.abs()[bad] <= tol[bad]).all()), ("LeakyReLU sign", int(bad.sum()))
            return int(bad.sum())

    def backward(self, gout, pos=None):
        routed = self.out if pos is None else torch.where(pos, self.y, self.y * SLOPE)
        routed.backward(gout.double())
        return self.x.grad, self.w.grad, self.gamma.grad, self.beta.grad


def route_of(out, mode):
    """The route a forward took, read from the state its autograd node saved
    (dgx.schedule.PC_FIELDS): "split" keeps X's split planes, "lds16" a bf16 Z,
    "lds32" the bf16 weight copies of the LDS GEMMs, else the register-staged
    bf16 GEMM ("xwt") or the fp32 GEMM ("mm32")."""
    from dgx import schedule as S
    saved = S.PcSaved(*out.grad_fn.saved_tensors[1:])
    if saved.xhi.numel():
        return "split"
    if mode != "bf16":
        return "mm32"
    if saved.Z.dtype == torch.bfloat16:
        return "lds16"
    return "lds32" if saved.nt.numel() else "xwt"


def run_engine(cuda, seq, X, gout, B, N, mode, twin, train):
    from dgx import precision
    from dgx.pointconv import pointconv_bn_lrelu
    eng = copy.deepcopy(seq).to(cuda)
    eng.train(train)
    Xe = X.to(cuda).requires_grad_(True)
    X16 = Xe.detach().bfloat16() if twin else None
    with precision.mode(mode):
        out = pointconv_bn_lrelu(Xe, B, N, eng, X16=X16)
        eng.route = route_of(out, mode)
        out.backward(gout.to(cuda))
    torch.cuda.synchronize()
    return eng, Xe, out.detach()


def compare(eng, Xe, out, ref, grads, bar, train, seq):
    conv, bn = eng[0], eng[1]
    errs = {"out": rel_err(out.cpu(), ref.out.detach().cpu()),
            "dX": rel_err(Xe.grad.cpu(), grads[0].cpu()),
            "dW": rel_err(conv.weight.grad.reshape(grads[1].shape[:2]).cpu(), grads[1].reshape(grads[1].shape[:2]).cpu()),
            "dgamma": rel_err(bn.weight.grad.cpu(), grads[2].cpu()),
            "dbeta": rel_err(bn.bias.grad.cpu(), grads[3].cpu())}
    print("rel err:", {k: f"{v:.2e}" for k, v in errs.items()})
    for k, v in errs.items():
        assert v < bar, (k, v)
    if train:
        assert rel_err(bn.running_mean.cpu(), ref.rm.cpu()) < 1e-5
        assert rel_err(bn.running_var.cpu(), ref.rv.cpu()) < 1e-5
        assert int(bn.num_batches_tracked) == ref.nbt == NBT0 + 1
    else:   # eval: the running statistics are bit-unchanged (dgamma / dbeta above are the eval-mode formula's)
        assert torch.equal(bn.running_mean.cpu(), seq[1].running_mean)
        assert torch.equal(bn.running_var.cpu(), seq[1].running_var)
        assert int(bn.num_batches_tracked) == NBT0


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_pointconv_routes_vs_fp64(cuda, case):
    name, mode, K, Co, B, N, twin, train, momentum, conv, route = case
    seed = sum(map(ord, name))
    seq = make_seq(K, Co, conv, momentum, seed)
    X, gout = make_data(K, Co, B, N, seed)
    eng, Xe, out = run_engine(cuda, seq, X, gout, B, N, mode, twin, train)
    assert eng.route == route
    ref = Ref64(X.to(cuda), copy.deepcopy(seq).to(cuda), B, N, train, momentum, mode)
    flips = ref.check_signs(out > 0, mode)
    print("sign flips below the error bound:", flips)
    grads = ref.backward(gout.to(cuda), out > 0)
    compare(eng, Xe, out, ref, grads, BAR[mode], train, seq)


def _shapes():
    seen, r = set(), []
    for name, _, K, Co, B, N, _, train, momentum, conv, _ in CASES:
        key = (K, Co, B, N, train, momentum, conv)
        if key not in seen:
            seen.add(key)
            r.append((name,) + key)
    return r


@pytest.mark.parametrize("shape", _shapes(), ids=[s[0] for s in _shapes()])
def test_fp64_reference_matches_cpu_path(shape):
    """The reference above against dgx.cpu.pointconv_bn_lrelu (the torch modules
    themselves on the host) at the same shapes: 1e-5 in fp32."""
    from dgx import cpu
    name, K, Co, B, N, train, momentum, conv = shape
    seed = sum(map(ord, name))
    seq = make_seq(K, Co, conv, momentum, seed)
    X, gout = make_data(K, Co, B, N, seed)
    m = copy.deepcopy(seq)
    m.train(train)
    Xc = X.clone().requires_grad_(True)
    out = cpu.pointconv_bn_lrelu(Xc, B, N, m)
    assert tuple(out.shape) == (B, Co, N)
    out.backward(gout)
    ref = Ref64(X, seq, B, N, train, momentum)
    ref.check_signs(out.detach() > 0, "fp32")
    grads = ref.backward(gout, out.detach() > 0)
    compare(m, Xc, out.detach(), ref, grads, 1e-5, train, seq)


@pytest.mark.gpu
@pytest.mark.parametrize("mode,K,Co,B,N,twin", [("fp32", 45, 70, 3, 130, False), ("bf16", 64, 128, 3, 130, True),
                                                ("bf16", 64, 96, 3, 130, True), ("fp32_split", 64, 64, 3, 257, False)])
def test_library_op_equals_function(cuda, mode, K, Co, B, N, twin):
    """torch.ops.dgx.pointconv (what torch.compile / export trace) and the eager
    autograd Function run the same schedule: bit-equal outputs, gradients and
    updated running statistics."""
    from dgx import library, precision
    from dgx import schedule as S
    seq = make_seq(K, Co, "2d", 0.1, 11)
    X, gout = make_data(K, Co, B, N, 11)
    eng, Xe, out = run_engine(cuda, seq, X, gout, B, N, mode, twin, True)
    lib = copy.deepcopy(seq).to(cuda).train()
    conv, bn = lib[0], lib[1]
    Xl = X.to(cuda).requires_grad_(True)
    X16 = Xl.detach().bfloat16() if twin else torch.empty(0, dtype=torch.bfloat16, device=cuda)
    with precision.mode(mode):
        bf16, opts = S.decide()
        o, rm, rv, nb, _ = torch.ops.dgx.pointconv(Xl, X16, B, N, conv.weight, bn.weight, bn.bias,
                                                   *library._bn_args(bn, cuda), SLOPE, bf16, None, opts)
        o.backward(gout.to(cuda))
    torch.cuda.synchronize()
    assert torch.equal(o.detach(), out)
    assert torch.equal(Xl.grad, Xe.grad)
    for a, b in zip(lib.parameters(), eng.parameters()):
        assert torch.equal(a.grad, b.grad)
    assert torch.equal(rm, eng[1].running_mean) and torch.equal(rv, eng[1].running_var)
    assert int(nb) == int(eng[1].num_batches_tracked) == NBT0 + 1


@pytest.mark.gpu
def test_dgcnn_emb96_bf16_routed(cuda):
    """DGCNN(emb_dim=96) in bf16 mode (conv5 with Co % 64 != 0 and the bf16 twin
    of the concat buffer) on the small golden geometry (B 2, N 128, k 10):
    forward and backward complete, within SURVEY §8(c)'s bf16 bar (2e-2) of the
    fp64 oracle routed by the engine's validated decisions; the one-op host path
    gives the Function path's result bit for bit."""
    import dgx.edgeconv as E
    from conftest import validate_dgcnn_decisions
    from dgx import precision, synth
    from models.dgcnn import DGCNN
    from oracle import reference as R
    torch.manual_seed(96)
    emb, N, k, B = 96, 128, 10, 2
    base = DGCNN(types.SimpleNamespace(emb_dim=emb, k=k))
    init = {n: t.detach().clone() for n, t in base.state_dict().items()}
    x = torch.from_numpy(synth.cube_clouds(B, N, 7)).to(cuda).permute(0, 2, 1)
    gout = torch.from_numpy(synth.uniform(96, (B, emb, N)) - 0.5).float()
    runs = []
    with precision.mode("bf16"):
        for capture in (True, False):   # the autograd Functions (debug capture), then the one-op host path
            m = copy.deepcopy(base).to(cuda).train()
            if capture:
                E.set_debug_capture({})
                cap = E.debug_capture()
            try:
                y = m(x)
            finally:
                E.set_debug_capture(None)
            y.backward(gout.to(cuda))
            runs.append((y.detach(), {n: p.grad.clone() for n, p in m.named_parameters()}))
    torch.cuda.synchronize()
    y, grads = runs[0]
    assert torch.equal(y, runs[1][0])
    for n in grads:
        assert torch.equal(grads[n], runs[1][1][n]), n
    validate_dgcnn_decisions(cap, x, k, init, bf16=True)
    dec = [(i.long(), a, z) for (i, a, z) in (cap[("fwd", l)] for l in range(4))]
    params = {n: (t.to(cuda).double() if t.is_floating_point() else t.to(cuda)) for n, t in init.items()}
    for n, t in params.items():
        if t.is_floating_point() and "running" not in n:
            t.requires_grad_(True)
    ref = R.dgcnn_routed(x.double(), params, dec, y > 0)
    ref.backward(gout.to(cuda).double())
    assert rel_err(y.cpu(), ref.detach().cpu()) < 2e-2
    for n, g in grads.items():
        assert rel_err(g.cpu(), params[n].grad.cpu()) < 2e-2, n


# ------------------------------------------------- BatchNorm conditioning ----
LADDER = (0, 4, 16, 64, 256)
# producer -> (mode, twin); constants measured on an MI355X (profiles/bn_conditioning.log), see the module docstring
PRODUCERS = {"colstats": ("fp32", False), "gemm-epilogue": ("bf16", False), "lds-epilogue": ("bf16", True)}
MEASURED = {   # producer -> (variance constant, mean constant): largest over 5 seeds and Co in {64, 68}
    "gemm-epilogue": (2.709, 1.747),
    "lds-epilogue": (2.709, 1.747),
    "edge-gather": (2.641, 1.599),
}
MEASURED_OUT_R64 = 2.51e-4  # fp32 mode, rel_err of the r = 64 channels' output against the fp64 reference


def ladder_inputs(K, Co, B, N, seed):
    """X (B N, K) with a column of ones, W whose first column places channel o at
    mean r_o sigma_o, r_o = LADDER[o % 5] (sigma_o: the channel's std without the
    offset, in fp64)."""
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(B * N, K, generator=g)
    X[:, 0] = 1.0
    W = torch.randn(Co, K, generator=g) / K ** 0.5
    r = torch.tensor([float(LADDER[o % len(LADDER)]) for o in range(Co)], dtype=torch.float64)
    Z0 = X[:, 1:].double() @ W[:, 1:].double().t()
    W[:, 0] = (r * Z0.std(0, unbiased=False) - Z0.mean(0)).float()
    return X, W, r


def stat_constants(rm, rv, Z):
    """(variance constant, mean constant, r per channel) of running statistics
    (momentum 1: batch mean, unbiased batch variance) against the fp64 statistics
    of Z (rows, Co): relative variance error / ((1 + r^2) 2^-24), and mean error
    relative to rms(z) = sigma sqrt(1 + r^2) (a sum of n terms errs by at most
    depth u sum|z| <= depth u n rms(z)) / 2^-24."""
    mean, var = Z.mean(0), Z.var(0, unbiased=True)
    r = mean.abs() / var.sqrt()
    cv = ((rv.double() - var).abs() / var) / ((1 + r * r) * U)
    cm = ((rm.double() - mean).abs() / (var + mean * mean).sqrt()) / U
    return float(cv.max()), float(cm.max()), r


def run_ladder(cuda, producer, Co, seed, B=2, N=300, K=64):
    """One training forward of the public op with momentum 1 -> (constants of the
    engine, constants of torch's fp32 F.batch_norm on the same Z, output, fp64
    reference output, r per channel, route_of the forward)."""
    from dgx import precision
    from dgx.pointconv import pointconv_bn_lrelu
    mode, twin = PRODUCERS[producer]
    X, W, _ = ladder_inputs(K, Co, B, N, seed)
    seq = torch.nn.Sequential(torch.nn.Conv1d(K, Co, 1, bias=False), torch.nn.BatchNorm1d(Co, momentum=1.0),
                              torch.nn.LeakyReLU(SLOPE))
    with torch.no_grad():
        seq[0].weight.copy_(W.view(Co, K, 1))
        seq[1].weight.copy_(torch.where(torch.arange(Co) % 2 == 0, 1.0, -1.5))
        seq[1].bias.fill_(0.1)
    seq = seq.to(cuda).train()
    Xd = X.to(cuda)
    with precision.mode(mode):
        out = pointconv_bn_lrelu(Xd, B, N, seq, X16=Xd.bfloat16() if twin else None)
    route = route_of(out, mode)
    out = out.detach()
    torch.cuda.synchronize()
    Wd = W.to(cuda)
    if mode == "bf16":   # the operands the mode uses
        Z = Xd.bfloat16().double() @ Wd.bfloat16().double().t()
    else:
        Z = Xd.double() @ Wd.double().t()
    bn = seq[1]
    cv, cm, r = stat_constants(bn.running_mean, bn.running_var, Z)
    trm, trv = torch.zeros(Co, device=cuda), torch.ones(Co, device=cuda)
    F.batch_norm(Z.float(), trm, trv, None, None, True, 1.0, bn.eps)
    tcv, tcm, _ = stat_constants(trm, trv, Z)
    y = F.batch_norm(Z, None, None, bn.weight.detach().double(), bn.bias.detach().double(), True, 0.0, bn.eps)
    ref = F.leaky_relu(y, SLOPE).view(B, N, Co).permute(0, 2, 1)
    return (cv, cm), (tcv, tcm), out, ref, r, route


def run_edge_ladder(cuda, seed, B=2, N=300, C=4, Co=64, k=10):
    """The same ladder through one EdgeConv block (dgx_edge_fwd_gather's
    partials): x with a channel of ones, the offset on the x_i half of the
    weight. -> (constants of the engine, constants of torch's fp32 batch_norm)."""
    import dgx.edgeconv as E
    from oracle import reference as R
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, N, generator=g)
    x[:, C - 1] = 1.0
    w = torch.randn(Co, 2 * C, generator=g) / (2 * C) ** 0.5
    w[:, C - 1] = 0.0
    w[:, 2 * C - 1] = 0.0
    blk = torch.nn.Sequential(torch.nn.Conv2d(2 * C, Co, 1, bias=False), torch.nn.BatchNorm2d(Co, momentum=1.0),
                              torch.nn.LeakyReLU(SLOPE)).to(cuda).train()
    xd = x.to(cuda)
    r = torch.tensor([float(LADDER[o % len(LADDER)]) for o in range(Co)], dtype=torch.float64, device=cuda)

    def forward():
        with torch.no_grad():
            blk[0].weight.copy_(w.view(Co, 2 * C, 1, 1))
        E.set_debug_capture({})
        try:
            E.edgeconv_stack(xd, k, [blk], True)
            idx = E.debug_capture()[("fwd", 0)][0]
        finally:
            E.set_debug_capture(None)
        e = R.graph_feature(xd.double(), k, idx=idx.long().view(B, N, k))
        return F.conv2d(e, w.to(cuda).double().view(Co, 2 * C, 1, 1)).permute(0, 2, 3, 1).reshape(-1, Co)

    Z0 = forward()   # the kNN graph does not depend on the weight; sigma_o without the offset
    w[:, 2 * C - 1] = (r * Z0.std(0, unbiased=False) - Z0.mean(0)).float().cpu()
    Z = forward()
    torch.cuda.synchronize()
    bn = blk[1]
    cv, cm, _ = stat_constants(bn.running_mean, bn.running_var, Z)
    trm, trv = torch.zeros(Co, device=cuda), torch.ones(Co, device=cuda)
    F.batch_norm(Z.float(), trm, trv, None, None, True, 1.0, bn.eps)
    tcv, tcm, _ = stat_constants(trm, trv, Z)
    return (cv, cm), (tcv, tcm)


def _group_err(out, ref, r, lo, hi):
    sel = ((r >= lo) & (r <= hi)).nonzero().flatten()
    return rel_err(out[:, sel].cpu(), ref[:, sel].cpu())


@pytest.mark.gpu
@pytest.mark.parametrize("Co", [64, 68])
def test_bn_conditioning_colstats(cuda, Co):
    """fp32 mode (colstats_kernel): relative variance error <= 8 (1 + r^2) 2^-24 —
    4x the 2 r^2 2^-24 of raw fp32 sums —, mean error <= 8 2^-24 rms(z); the
    output holds 1e-3 for r <= 4 and, at r = 64, 4x the error measured there."""
    (cv, cm), torch_c, out, ref, r, route = run_ladder(cuda, "colstats", Co, 0)
    assert route == "mm32"
    print(f"colstats Co {Co}: variance constant {cv:.3f}, mean constant {cm:.3f}; torch fp32 {torch_c}")
    assert cv <= 8.0 and cm <= 8.0
    e4, e64 = _group_err(out, ref, r, 0, 5), _group_err(out, ref, r, 60, 70)
    print(f"output rel err: r <= 4 {e4:.2e}, r = 64 {e64:.2e}")
    assert e4 < 1e-3
    assert e64 <= 4 * MEASURED_OUT_R64


@pytest.mark.gpu
@pytest.mark.parametrize("Co", [64, 68])
@pytest.mark.parametrize("producer", ["gemm-epilogue", "lds-epilogue"])
def test_bn_conditioning_gemm_epilogues(cuda, producer, Co):
    """bf16 mode: the register-staged GEMM's statistics epilogue (no twin) and the
    LDS GEMM's bf16-store epilogue (twin; Co 68 is refused by the LDS route and
    takes the register-staged GEMM) against the fp64 statistics of the
    bf16-rounded operands' product: 4x the measured constants."""
    (cv, cm), torch_c, _, _, _, route = run_ladder(cuda, producer, Co, 0)
    assert route == ("lds16" if producer == "lds-epilogue" and Co == 64 else "xwt")
    print(f"{producer} Co {Co}: variance constant {cv:.3f}, mean constant {cm:.3f}; torch fp32 {torch_c}")
    assert cv <= 4 * MEASURED[producer][0] and cm <= 4 * MEASURED[producer][1]


@pytest.mark.gpu
def test_bn_conditioning_edge_gather(cuda):
    """One EdgeConv block (dgx_edge_fwd_gather's partials over the B N k edges)."""
    (cv, cm), torch_c = run_edge_ladder(cuda, 0)
    print(f"edge-gather: variance constant {cv:.3f}, mean constant {cm:.3f}; torch fp32 {torch_c}")
    assert cv <= 4 * MEASURED["edge-gather"][0] and cm <= 4 * MEASURED["edge-gather"][1]
