"""Kernel-level oracle tests of the EdgeConv BatchNorm arithmetic (csrc/edgeconv.hip:
bn_finalize, eval affine, BN + LeakyReLU apply, dz / packed dz / channel-major dz,
backward finalize; the schedule's batch_stats / running_stats / backward_consts /
compact of csrc/dgx_torch.cpp; reference models/dgcnn.py:54-98): every C entry is
called with given data and compared with the fp64 restatement of
tests/_edgebn_ref.py, whose docstring derives the lattice constructions (bit
equality) and every bound of the random cases (none comes from a run). apply, dz
and the packed words are bit-equal on random data too; the random tests print
their worst got / bound ratio.

Buffer hygiene: every output is pre-filled with a sentinel; matrices end in a
canary row and keep their columns beyond Co, per-channel vectors end in four
canary elements; inputs a kernel indexes by row end in a NaN row. Nothing here
can fault: all shapes are the real ones of the buffers handed over."""
import pytest
import torch

import _edgebn_ref as R
from dgx import _native as nat
from dgx import bn as bn_

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
F64 = torch.float64
EINVAL = -1
NBT_SENT = -77
FIN_NAMES = ("scale", "shift", "mean", "invstd", "rm", "rv")
BWD_NAMES = ("dgamma", "dbeta", "c0", "c1")


def _ids(grid):
    return ["-".join(str(int(v) if isinstance(v, bool) else v) for v in case) for case in grid]


def _vec(Co, cuda, init=None):
    """(Co + 4 canary elements, view of the Co)"""
    full = torch.full((Co + 4,), R.SENT, device=cuda)
    if init is not None:
        full[:Co] = init.to(cuda)
    return full, full[:Co]


def _tails_intact(o):
    return all(bool((full[-4:] == R.SENT).all()) for full in o.fulls)


def _untouched(o):
    return all(bool((full == R.SENT).all()) for full in o.fulls)


def _compare(kind, got, ref, names, worst):
    """lattice: bit equality; random: within the derived bound, worst ratio recorded"""
    for name in names:
        g, want = getattr(got, name, None), getattr(ref, name)
        if g is None or want is None:
            continue
        g = g.detach().double().cpu()
        if kind == "lattice":
            assert torch.equal(g, want), (name, g, want)
        else:
            ratio = R.worst(g, want, getattr(ref, name + "_b"))
            worst[name] = max(worst.get(name, 0.0), ratio)
            assert ratio <= 1.0, (name, ratio)


def _report(what, worst):
    if worst:
        print(f"[edgebn] {what}: worst got/bound " + ", ".join(f"{n} {v:.3f}" for n, v in worst.items()))


# ---- dgx_bn_finalize[_out]_f32 / _f64 -----------------------------------------------

def _finalize(cuda, c, f64, form, running, nbt, momentum, affine=True, stats=True, devcount=False, drop=()):
    """One call. form "out" / "inplace"; running: hand over running statistics;
    nbt: the counter's value or None; drop: `_new` targets withheld (error cases).
    -> Case: rc, the outputs (None where not asked for), fulls (every output
    buffer with its canaries), nbt (the counter afterwards)"""
    L = nat.lib()
    Co = c.Co
    p = c.partials.double() if f64 else c.partials.float()
    buf = (R.with_count(p, c.count) if devcount else p.reshape(-1)).to(cuda)
    count = -1.0 if devcount else c.count
    gamma, beta = (c.gamma.to(cuda), c.beta.to(cuda)) if affine else (None, None)
    o = R.Case()
    o.fulls = []

    def out():
        full, v = _vec(Co, cuda)
        o.fulls.append(full)
        return v

    o.scale, o.shift = out(), out()
    o.mean, o.invstd = (out(), out()) if stats else (None, None)
    o.rm = o.rv = o.nbt = None
    nb = torch.tensor([nbt, NBT_SENT], dtype=torch.int64, device=cuda) if nbt is not None else None
    st = nat.stream_of(buf)
    P = nat.ptr
    if form == "out":
        rm, rv = (c.rm.to(cuda), c.rv.to(cuda)) if running else (None, None)
        o.rm, o.rv = (out(), out()) if running else (None, None)
        nb_new = torch.full((2,), NBT_SENT, dtype=torch.int64, device=cuda) if nbt is not None else None
        tgt = {"rm": o.rm, "rv": o.rv, "nbt": nb_new}
        for name in drop:
            tgt[name] = None
        fn = L.dgx_bn_finalize_out_f64 if f64 else L.dgx_bn_finalize_out_f32
        o.rc = fn(P(buf), c.nrows, Co, count, P(gamma), P(beta), P(rm), P(rv), momentum, c.eps, P(o.scale), P(o.shift),
                  P(o.mean), P(o.invstd), P(nb), P(tgt["rm"]), P(tgt["rv"]), P(tgt["nbt"]), st)
        torch.cuda.synchronize()
        if running:   # the inputs are only read
            assert torch.equal(rm.cpu(), c.rm) and torch.equal(rv.cpu(), c.rv)
        if nbt is not None:
            assert nb.tolist() == [nbt, NBT_SENT] and int(nb_new[1]) == NBT_SENT
            o.nbt = int(nb_new[0])
    else:
        if running:
            (rm_f, o.rm), (rv_f, o.rv) = _vec(Co, cuda, c.rm), _vec(Co, cuda, c.rv)
        fn = L.dgx_bn_finalize_f64 if f64 else L.dgx_bn_finalize_f32
        o.rc = fn(P(buf), c.nrows, Co, count, P(gamma), P(beta), P(o.rm), P(o.rv), momentum, c.eps, P(o.scale),
                  P(o.shift), P(o.mean), P(o.invstd), P(nb), st)
        torch.cuda.synchronize()
        if running:
            assert bool((rm_f[-4:] == R.SENT).all()) and bool((rv_f[-4:] == R.SENT).all())
        if nbt is not None:
            assert int(nb[1]) == NBT_SENT
            o.nbt = int(nb[0])
    return o


def _finalize_variants(t, f64):
    """(form, running, nbt, cumulative, affine, stats, devcount) of geometry t"""
    v = [("inplace", False, None, False, False, False, False),     # null gamma / beta / mean / invstd outputs
         ("out", True, None, False, True, True, False),
         ("out", True, (0, 1, 3)[t % 3], True, True, True, False),  # cumulative momentum through nbt
         ("out", True, None, True, True, True, False),              # cumulative without a counter: factor 0
         ("inplace", True, 5, False, True, True, False)]
    if f64:
        v.append(("out", True, (3, 0, 1)[t % 3], True, True, True, True))   # the count follows the sums on the device
        v.append(("inplace", False, None, False, True, True, True))
    return v


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("kind", ["lattice", "random"])
@pytest.mark.parametrize("Co,nrows", R.FIN_GRID, ids=_ids(R.FIN_GRID))
def test_finalize(cuda, kind, f64, Co, nrows):
    t = R.FIN_GRID.index((Co, nrows))
    c = R.make_finalize_case(kind, Co, nrows, (4, 2, 1)[t % 3], seed=10 + t, f64=f64)
    worst = {}
    for form, running, nbt, cumulative, affine, stats, devcount in _finalize_variants(t, f64):
        momentum = -1.0 if cumulative else c.momentum
        o = _finalize(cuda, c, f64, form, running, nbt, momentum, affine, stats, devcount)
        assert o.rc == 0 and _tails_intact(o)
        buf = R.with_count(c.partials, c.count) if devcount else c.partials
        r = R.finalize(buf, -1.0 if devcount else c.count, c.gamma if affine else None, c.beta if affine else None,
                       c.rm if running else None, c.rv if running else None, momentum, c.eps, nbt, co=Co)
        if kind == "lattice":
            assert R.fits_f32(r.scale, r.shift, r.mean, r.invstd, r.rm, r.rv)
        _compare(kind, o, r, FIN_NAMES, worst)
        assert o.nbt == r.nbt
        cc = R.clamp_channel(Co)   # S2 / count - mean^2 < 0 there: var = 0
        if stats:
            assert float(r.var[cc]) == 0.0
            if kind == "lattice":
                assert float(o.invstd[cc]) == 2.0
    _report(f"finalize {'f64' if f64 else 'f32'} Co {Co} nrows {nrows}", worst)


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("kind", ["lattice", "random"])
def test_finalize_count_one(cuda, kind, f64):
    """One element per channel: var = 0 (lattice) or the rounding error of the
    given y^2 (random), and the running variance takes the biased value."""
    Co = 5
    c = R.make_finalize_case("lattice", Co, 1, 1, seed=3, f64=f64)
    if kind == "random":
        g = torch.Generator().manual_seed(4)
        y = torch.randn(Co, generator=g)
        p = torch.stack([y.double(), y.double() ** 2]).view(1, 2, Co)
        c.partials = p if f64 else p.float()
        c.eps, c.momentum = R.EPS_RANDOM, 0.1
        c.gamma, c.beta = torch.randn(Co, generator=g), torch.randn(Co, generator=g)
    worst = {}
    for form in ("out", "inplace"):
        o = _finalize(cuda, c, f64, form, True, 2, c.momentum)
        assert o.rc == 0 and _tails_intact(o)
        r = R.finalize(c.partials, 1.0, c.gamma, c.beta, c.rm, c.rv, c.momentum, c.eps, 2)
        _compare(kind, o, r, FIN_NAMES, worst)
        assert o.nbt == 3
        # the documented rule, stated on its own: the biased variance enters the running one
        m = c.momentum
        want = (1 - m) * c.rv.double() + m * r.var
        assert R.within(o.rv.cpu(), want, r.rv_b)
    _report(f"finalize count 1 {'f64' if f64 else 'f32'}", worst)


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_finalize_error_codes_write_nothing(cuda, f64):
    c = R.make_finalize_case("lattice", 5, 3, 4, seed=1, f64=f64)
    for kw in (dict(form="out", running=True, nbt=None, momentum=0.25, drop=("rm",)),
               dict(form="out", running=True, nbt=None, momentum=0.25, drop=("rv",)),
               dict(form="out", running=True, nbt=1, momentum=0.25, drop=("nbt",)),
               dict(form="inplace", running=True, nbt=1, momentum=-1.0)):   # cumulative: the counter may not alias
        o = _finalize(cuda, c, f64, **kw)
        assert o.rc == EINVAL, (kw, o.rc)
        if kw["form"] == "out":
            assert _untouched(o), kw
            assert o.nbt is None or o.nbt == NBT_SENT
        else:
            assert all(bool((full == R.SENT).all()) for full in o.fulls), kw
            assert torch.equal(o.rm.cpu(), c.rm) and torch.equal(o.rv.cpu(), c.rv) and o.nbt == 1


# ---- dgx_bn_eval_affine_f32 -----------------------------------------------------------

@pytest.mark.parametrize("kind", ["lattice", "random"])
@pytest.mark.parametrize("Co", [1, 3, 255, 256, 257])
def test_eval_affine(cuda, kind, Co):
    L = nat.lib()
    c = R.make_finalize_case(kind, Co, 1, 4, seed=Co)
    if kind == "lattice":
        c.rv = torch.tensor([R.VARS[o % 3] for o in range(Co)])    # rv + eps in {1, 4, 16}
    worst = {}
    for affine in (True, False):
        gamma, beta = (c.gamma.to(cuda), c.beta.to(cuda)) if affine else (None, None)
        rm, rv = c.rm.to(cuda), c.rv.to(cuda)
        (sf, scale), (hf, shift) = _vec(Co, cuda), _vec(Co, cuda)
        nat.check(L.dgx_bn_eval_affine_f32(Co, nat.ptr(gamma), nat.ptr(beta), nat.ptr(rm), nat.ptr(rv), c.eps,
                                           nat.ptr(scale), nat.ptr(shift), nat.stream_of(rm)), "eval affine")
        torch.cuda.synchronize()
        assert bool((sf[-4:] == R.SENT).all()) and bool((hf[-4:] == R.SENT).all())
        r = R.eval_affine(c.gamma if affine else None, c.beta if affine else None, c.rm, c.rv, c.eps)
        o = R.Case()
        o.scale, o.shift = scale, shift
        _compare(kind, o, r, ("scale", "shift"), worst)
    _report(f"eval affine Co {Co}", worst)


# ---- through the binding: dgx.bn.batch_stats / the schedule's compact ---------------------

def _bn_module(c, cuda, momentum, train=True, nbt=0):
    bn = torch.nn.BatchNorm2d(c.Co, eps=c.eps, momentum=momentum).to(cuda)
    with torch.no_grad():
        bn.running_mean.copy_(c.rm)
        bn.running_var.copy_(c.rv)
        bn.num_batches_tracked.fill_(nbt)
    return bn.train() if train else bn.eval()


@pytest.mark.parametrize("kind", ["lattice", "random"])
@pytest.mark.parametrize("rows", R.COMPACT_ROWS)
def test_batch_stats_binding(cuda, kind, rows):
    """dgx.bn.batch_stats with Co = 5: no pre-reduce (1024 rows), compact with 1,
    127 and 0 leftover rows; a train-mode module updated in place (momentum and
    cumulative), a `stats_out` target, and an eval-mode module (no update)."""
    Co = 5
    c = R.make_finalize_case(kind, Co, rows, 4, seed=rows)
    partials = c.partials.to(cuda).contiguous()
    gamma, beta = c.gamma.to(cuda), c.beta.to(cuda)
    slabs = R.compact_slabs(rows)
    worst = {}

    def check(st, r, rm, rv, nbt):
        o = R.Case()
        o.scale, o.shift, o.mean, o.invstd, o.rm, o.rv = st.scale, st.shift, st.mean, st.invstd, rm, rv
        _compare(kind, o, r, FIN_NAMES, worst)
        assert int(nbt) == r.nbt
        assert not st.eval and st.group is None

    # train mode, momentum, in place
    bn = _bn_module(c, cuda, c.momentum, nbt=4)
    st = bn_.batch_stats(partials, rows, c.count, bn, gamma, beta)
    r = R.finalize(c.partials, c.count, c.gamma, c.beta, c.rm, c.rv, c.momentum, c.eps, 4, slabs=slabs)
    check(st, r, bn.running_mean, bn.running_var, bn.num_batches_tracked)
    # train mode, momentum=None: the cumulative average, counter 1 -> factor 1/2
    bn = _bn_module(c, cuda, None, nbt=1)
    st = bn_.batch_stats(partials, rows, c.count, bn, gamma, beta)
    r = R.finalize(c.partials, c.count, c.gamma, c.beta, c.rm, c.rv, -1.0, c.eps, 1, slabs=slabs)
    check(st, r, bn.running_mean, bn.running_var, bn.num_batches_tracked)
    # a functional caller's targets: the module's buffers are only read
    bn = _bn_module(c, cuda, c.momentum, nbt=7)
    bn.stats_out = (torch.full((Co,), R.SENT, device=cuda), torch.full((Co,), R.SENT, device=cuda),
                    torch.full((), NBT_SENT, dtype=torch.int64, device=cuda))
    st = bn_.batch_stats(partials, rows, c.count, bn, gamma, beta)
    r = R.finalize(c.partials, c.count, c.gamma, c.beta, c.rm, c.rv, c.momentum, c.eps, 7, slabs=slabs)
    check(st, r, bn.stats_out[0], bn.stats_out[1], bn.stats_out[2])
    assert torch.equal(bn.running_mean.cpu(), c.rm) and torch.equal(bn.running_var.cpu(), c.rv)
    assert int(bn.num_batches_tracked) == 7
    # eval mode: batch statistics asked for explicitly, nothing is updated
    bn = _bn_module(c, cuda, c.momentum, train=False, nbt=7)
    st = bn_.batch_stats(partials, rows, c.count, bn, gamma, beta)
    r = R.finalize(c.partials, c.count, c.gamma, c.beta, None, None, c.momentum, c.eps, None, slabs=slabs)
    o = R.Case()
    o.scale, o.shift, o.mean, o.invstd = st.scale, st.shift, st.mean, st.invstd
    _compare(kind, o, r, FIN_NAMES[:4], worst)
    assert torch.equal(bn.running_mean.cpu(), c.rm) and torch.equal(bn.running_var.cpu(), c.rv)
    assert int(bn.num_batches_tracked) == 7
    _report(f"batch_stats rows {rows}", worst)


def test_frozen_eval_module_takes_the_running_statistics(cuda):
    """A BN layer frozen in eval() inside a training model: the schedule's
    running_stats (reached through the pointwise conv op, which keeps the layer's
    per-channel state for its backward) must hold the eval affine of the running
    statistics, mean = running_mean, invstd = rsqrt(running_var + eps), and
    leave the buffers alone."""
    from dgx import schedule as S
    from dgx.pointconv import pointconv_bn_lrelu
    B, N, K, Co = 2, 5, 8, 5
    c = R.make_finalize_case("random", Co, 1, 4, seed=9)
    g = torch.Generator().manual_seed(9)
    seq = torch.nn.Sequential(torch.nn.Conv1d(K, Co, 1, bias=False), torch.nn.BatchNorm1d(Co, eps=c.eps),
                              torch.nn.LeakyReLU(0.2)).to(cuda).train()
    bn = seq[1]
    with torch.no_grad():
        bn.weight.copy_(c.gamma)
        bn.bias.copy_(c.beta)
        bn.running_mean.copy_(c.rm)
        bn.running_var.copy_(c.rv)
        bn.num_batches_tracked.fill_(3)
    bn.eval()
    X = torch.randn(B * N, K, generator=g).to(cuda)
    out = pointconv_bn_lrelu(X, B, N, seq)
    sv = S.PcSaved(*out.grad_fn.saved_tensors[1:])
    torch.cuda.synchronize()
    r = R.eval_affine(c.gamma, c.beta, c.rm, c.rv, c.eps)
    worst = {}
    _compare("random", sv, r, ("scale", "shift", "invstd"), worst)
    assert torch.equal(sv.mean.cpu(), c.rm)
    assert torch.equal(bn.running_mean.cpu(), c.rm) and torch.equal(bn.running_var.cpu(), c.rv)
    assert int(bn.num_batches_tracked) == 3
    # and the op's output is that affine applied to Z = X W^T
    Z = X.double() @ seq[0].weight.detach().double().view(Co, K).t()
    z = Z * sv.scale.double() + sv.shift.double()
    want = torch.where(z > 0, z, 0.2 * z).view(B, N, Co).permute(0, 2, 1)
    assert float((out.detach().double() - want).abs().max()) < 1e-4 * float(want.abs().max())
    _report("frozen eval (running_stats)", worst)


# ---- dgx_bn_lrelu_apply_f32 --------------------------------------------------------------

def _apply(cuda, c, M, Co, ldo, twin, oo=0, oy=0, ot=0):
    """-> (rc, out buffer, expected out buffer, twin buffer, expected twin buffer),
    buffers whole: offsets, guard columns, canary row and tail included"""
    L = nat.lib()
    n = (M + 1) * ldo + 8
    ybuf = torch.zeros(M * Co + 8, device=cuda)
    ybuf[oy:oy + M * Co] = c.ysel.to(cuda).view(-1)
    ysel = ybuf[oy:oy + M * Co].view(M, Co)
    out_f = torch.full((n,), R.SENT, device=cuda)
    tw_f = torch.full((n,), R.SENT, dtype=BF, device=cuda) if twin else None
    scale, shift = c.scale.to(cuda), c.shift.to(cuda)
    rc = L.dgx_bn_lrelu_apply_f32(nat.ptr(ybuf[oy:]), M, Co, nat.ptr(scale), nat.ptr(shift), c.slope, nat.ptr(out_f[oo:]),
                                  ldo, nat.ptr(tw_f[ot:]) if twin else None, nat.stream_of(ybuf))
    torch.cuda.synchronize()
    want, want16, zero = R.apply(ysel, scale, shift, c.slope)
    exp_f = torch.full((n,), R.SENT, device=cuda)
    exp_f[oo:oo + (M + 1) * ldo].view(M + 1, ldo)[:M, :Co] = want.float()
    exp16 = None
    if twin:
        exp16 = torch.full((n,), R.SENT, dtype=BF, device=cuda)
        exp16[ot:ot + (M + 1) * ldo].view(M + 1, ldo)[:M, :Co] = want16.to(BF)
    return rc, out_f, exp_f, tw_f, exp16, zero


@pytest.mark.parametrize("kind", ["lattice", "random"])
@pytest.mark.parametrize("M,Co,ldo,twin,oo,oy,ot,v4", R.APPLY_GRID, ids=_ids(R.APPLY_GRID))
def test_apply(cuda, kind, M, Co, ldo, twin, oo, oy, ot, v4):
    """Scalar kernel (Co 1, 3, 65), 4-wide kernel (Co 4, 64, 68) and the forced
    scalar fallbacks of Co % 4 == 0 (ldo odd; out, ysel or the bf16 twin off the
    vector alignment by one element); ldo > Co keeps its guard columns. v4 (which
    kernel the documented rule picks) is checked on the CPU, the values here."""
    c = R.make_edge_case(kind, M, Co, seed=M + Co + ldo)
    rc, out_f, exp_f, tw_f, exp16, zero = _apply(cuda, c, M, Co, ldo, twin, oo, oy, ot)
    assert rc == 0
    if kind == "lattice":
        assert bool(zero.any())                 # exact zeros of z: `>` and `>=` differ in sign handling only there
    assert torch.equal(out_f, exp_f)
    if twin:
        assert torch.equal(tw_f, exp16)


@pytest.mark.parametrize("M,Co,ldo,twin", R.APPLY_STRIDE_GRID, ids=_ids(R.APPLY_STRIDE_GRID))
def test_apply_grid_stride_loop(cuda, M, Co, ldo, twin):
    """Just past the 8192 x 256-thread grid cap (scalar: one element a thread,
    4-wide: four): some threads take a second element. Random data, every
    element, guard columns and twin compared."""
    c = R.make_edge_case("random", M, Co, seed=M)
    rc, out_f, exp_f, tw_f, exp16, _ = _apply(cuda, c, M, Co, ldo, twin)
    assert rc == 0
    assert torch.equal(out_f, exp_f) and torch.equal(tw_f, exp16)


def test_apply_of_nothing_writes_nothing(cuda):
    c = R.make_edge_case("lattice", 0, 8, seed=1)
    rc, out_f, exp_f, tw_f, exp16, _ = _apply(cuda, c, 0, 8, 8, 1)
    assert rc == 0
    assert bool((out_f == R.SENT).all()) and bool((tw_f.float() == R.SENT).all())


# ---- dgx_edge_bwd_dz_f32 / dgx_edge_bwd_dz_packed_f32 ---------------------------------------

def _dz_inputs(cuda, c):
    M, Co = c.M, c.Co
    t = R.Case()
    nan_row = torch.full((1, Co), float("nan"))
    t.ysel = torch.cat([c.ysel, nan_row]).to(cuda)
    t.arg = torch.cat([c.arg, torch.full((1, Co), 255, dtype=torch.uint8)]).to(cuda)
    t.scale, t.shift, t.mean, t.invstd = (v.to(cuda) for v in (c.scale, c.shift, c.mean, c.invstd))
    return t


def _assert_partials(kind, got, part, bound, what, worst):
    assert not bool((got == R.SENT).any()), f"{what}: a partial row was left unwritten"
    if kind == "lattice":
        assert torch.equal(got.double(), part), what
    else:
        ratio = R.worst(got, part, bound)
        worst[what] = max(worst.get(what, 0.0), ratio)
        assert ratio <= 1.0, (what, ratio)


@pytest.mark.parametrize("kind", ["lattice", "random"])
@pytest.mark.parametrize("M,nrows,Co,pad", R.DZ_GRID, ids=_ids(R.DZ_GRID))
def test_dz_and_packed_dz(cuda, kind, M, nrows, Co, pad):
    L = nat.lib()
    c = R.make_edge_case(kind, M, Co, seed=M + Co)
    t = _dz_inputs(cuda, c)
    lddy, off = Co + pad, pad // 2
    wide = torch.full((M + 1, lddy), float("nan"), device=cuda)     # dY: a column slice of a wider buffer
    wide[:M, off:off + Co] = c.dY.to(cuda)
    dY = wide[:, off:off + Co]
    st = nat.stream_of(wide)
    d, _, zero = R.dz(c.dY.to(cuda), t.ysel[:M], t.scale, t.shift, c.slope)
    part, bound, mag = R.dz_partials(d, t.ysel[:M], t.mean, t.invstd, R.row_blocks(M, nrows), nrows)
    if kind == "lattice":
        assert bool(zero.any())
        R.assert_dz_exact(mag)
    assert bool((part[-(-M // -(-M // nrows)):] == 0).all())         # blocks past M hold exactly 0
    worst = {}
    dz_f, dz = R.guarded(M, Co, cuda)
    p_f, p = R.guarded(nrows, 2 * Co, cuda)
    tail = (M, Co, nat.ptr(t.scale), nat.ptr(t.shift), nat.ptr(t.mean), nat.ptr(t.invstd), c.slope)
    nat.check(L.dgx_edge_bwd_dz_f32(nat.ptr(dY), lddy, nat.ptr(t.ysel), *tail, nat.ptr(dz), nat.ptr(p), nrows, st), "dz")
    torch.cuda.synchronize()
    assert R.guard_intact(dz_f) and R.guard_intact(p_f)
    assert torch.equal(dz.double(), d), "dz is the fp32 product: bit-equal on any data"
    _assert_partials(kind, p.view(nrows, 2, Co), part, bound, "partials", worst)
    # packed: the slot in the low 6 mantissa bits, the partials those of the unpacked dz
    w_f, w = R.guarded(M, Co, cuda)
    q_f, q = R.guarded(nrows, 2 * Co, cuda)
    nat.check(L.dgx_edge_bwd_dz_packed_f32(nat.ptr(dY), lddy, nat.ptr(t.ysel), nat.ptr(t.arg), *tail, nat.ptr(w),
                                           nat.ptr(q), nrows, st), "dz packed")
    torch.cuda.synchronize()
    assert R.guard_intact(w_f) and R.guard_intact(q_f)
    assert torch.equal(w.contiguous().view(torch.int32), R.packed(d, t.arg[:M]))
    assert torch.equal(q, p), "packed partials equal the unpacked ones bit for bit"
    if M * Co >= 64:
        assert int(t.arg[:M].max()) == 63 and int(t.arg[:M].min()) == 0
    _report(f"dz M {M} nrows {nrows} Co {Co}", worst)


def test_dz_error_codes_write_nothing(cuda):
    L = nat.lib()
    c = R.make_edge_case("lattice", 5, 8, seed=1)
    t = _dz_inputs(cuda, c)
    dY = c.dY.to(cuda)
    for M, Co, lddy, nrows in ((0, 8, 8, 2), (5, 0, 8, 2), (5, 8, 7, 2), (5, 8, 8, 0)):
        dz_f, dz = R.guarded(5, 8, cuda)
        p_f, p = R.guarded(2, 16, cuda)
        rc = L.dgx_edge_bwd_dz_f32(nat.ptr(dY), lddy, nat.ptr(t.ysel), M, Co, nat.ptr(t.scale), nat.ptr(t.shift),
                                   nat.ptr(t.mean), nat.ptr(t.invstd), c.slope, nat.ptr(dz), nat.ptr(p), nrows,
                                   nat.stream_of(dY))
        torch.cuda.synchronize()
        assert rc == EINVAL
        assert bool((dz_f == R.SENT).all()) and bool((p_f == R.SENT).all())


# ---- dgx_edge_bwd_dz_cm_f32 (channel-major dY) ----------------------------------------------

def _dz_cm(cuda, c, t, B, N, Co, nrows):
    L = nat.lib()
    M = B * N
    dYcm = torch.full((M * Co + 64,), float("nan"), device=cuda)      # (B, Co, N), NaN behind it
    dYcm[:M * Co] = c.dY.view(B, N, Co).permute(0, 2, 1).contiguous().view(-1).to(cuda)
    rows = max(nrows, L.dgx_edge_bwd_dz_cm_rows(B, N))
    dz_f, dz = R.guarded(M, Co, cuda)
    p_f, p = R.guarded(rows, 2 * Co, cuda)
    rc = L.dgx_edge_bwd_dz_cm_f32(nat.ptr(dYcm), nat.ptr(t.ysel), B, N, Co, nat.ptr(t.scale), nat.ptr(t.shift),
                                  nat.ptr(t.mean), nat.ptr(t.invstd), c.slope, nat.ptr(dz), nat.ptr(p), nrows,
                                  nat.stream_of(dYcm))
    torch.cuda.synchronize()
    return rc, dz_f, dz, p_f, p


@pytest.mark.parametrize("kind", ["lattice", "random"])
@pytest.mark.parametrize("B,N,Co", R.CM_GRID, ids=_ids(R.CM_GRID))
def test_dz_channel_major(cuda, kind, B, N, Co):
    L = nat.lib()
    M = B * N
    c = R.make_edge_case(kind, M, Co, seed=N + Co)
    t = _dz_inputs(cuda, c)
    blocks, nrows = R.cm_blocks(B, N)
    assert L.dgx_edge_bwd_dz_cm_rows(B, N) == nrows
    d, _, zero = R.dz(c.dY.to(cuda), t.ysel[:M], t.scale, t.shift, c.slope)      # the reference on the transposed dY
    part, bound, mag = R.dz_partials(d, t.ysel[:M], t.mean, t.invstd, blocks, nrows)
    if kind == "lattice":
        assert bool(zero.any())
        R.assert_dz_exact(mag)
    rc, dz_f, dz, p_f, p = _dz_cm(cuda, c, t, B, N, Co, nrows)
    assert rc == 0 and R.guard_intact(dz_f) and R.guard_intact(p_f)
    assert torch.equal(dz.double(), d)
    worst = {}
    _assert_partials(kind, p.view(nrows, 2, Co), part, bound, "partials", worst)   # row b ceil(N / 64) + tile
    _report(f"dz cm B {B} N {N} Co {Co}", worst)
    for wrong in (nrows + 1, nrows - 1):
        rc, dz_f, dz, p_f, p = _dz_cm(cuda, c, t, B, N, Co, wrong)
        assert rc == EINVAL and bool((dz_f == R.SENT).all()) and bool((p_f == R.SENT).all())


# ---- dgx_bn_bwd_finalize_f32 / _f64 ------------------------------------------------------

def _bwd_finalize(cuda, c, f64, accumulate, grads=True, devcount=False):
    L = nat.lib()
    Co = c.Co
    p = c.partials.double() if f64 else c.partials.float()
    buf = (R.with_count(p, c.count) if devcount else p.reshape(-1)).to(cuda)
    scale, mean, invstd = c.scale.to(cuda), c.mean.to(cuda), c.invstd.to(cuda)
    o = R.Case()
    o.fulls = []
    o.dgamma = o.dbeta = None
    if grads:
        (gf, o.dgamma), (bf, o.dbeta) = _vec(Co, cuda, c.prev[0]), _vec(Co, cuda, c.prev[1])
        o.fulls += [gf, bf]
    (c0f, o.c0), (c1f, o.c1) = _vec(Co, cuda), _vec(Co, cuda)
    o.fulls += [c0f, c1f]
    fn = L.dgx_bn_bwd_finalize_f64 if f64 else L.dgx_bn_bwd_finalize_f32
    o.rc = fn(nat.ptr(buf), c.nrows, Co, -1.0 if devcount else c.count, nat.ptr(scale), nat.ptr(mean), nat.ptr(invstd),
              nat.ptr(o.dgamma), nat.ptr(o.dbeta), nat.ptr(o.c0), nat.ptr(o.c1), accumulate, nat.stream_of(buf))
    torch.cuda.synchronize()
    return o


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("kind", ["lattice", "random"])
@pytest.mark.parametrize("Co,nrows", R.FIN_GRID, ids=_ids(R.FIN_GRID))
def test_bwd_finalize(cuda, kind, f64, Co, nrows):
    t = R.FIN_GRID.index((Co, nrows))
    c = R.make_bwdfin_case(kind, Co, nrows, seed=40 + t, f64=f64)
    worst = {}
    variants = [(0, True, False), (1, True, False), (t % 2, False, False)]        # (accumulate, dgamma / dbeta, count on device)
    if f64:
        variants += [(1 - t % 2, True, True)]
    for accumulate, grads, devcount in variants:
        o = _bwd_finalize(cuda, c, f64, accumulate, grads, devcount)
        assert o.rc == 0 and _tails_intact(o)
        buf = R.with_count(c.partials, c.count) if devcount else c.partials
        r = R.bwd_consts(buf, -1.0 if devcount else c.count, c.scale, c.mean, c.invstd, accumulate, c.prev, co=Co)
        if kind == "lattice":
            assert R.fits_f32(r.dgamma, r.dbeta, r.c0, r.c1)
        _compare(kind, o, r, BWD_NAMES, worst)
    _report(f"bwd finalize {'f64' if f64 else 'f32'} Co {Co} nrows {nrows}", worst)


@pytest.mark.parametrize("kind", ["lattice", "random"])
@pytest.mark.parametrize("rows", [64, 1025, 1152])
def test_backward_consts_binding(cuda, kind, rows):
    """dgx.bn.backward_consts: the train form, and the eval form with c0 = c1 = 0
    exactly while dgamma / dbeta are still computed; more than 1024 rows go
    through the schedule's compact."""
    Co = 5
    c = R.make_bwdfin_case(kind, Co, rows, seed=rows)
    partials = c.partials.to(cuda).contiguous()
    slabs = R.compact_slabs(rows)
    worst = {}
    for ev in (False, True):
        st = bn_.Stats(c.scale.to(cuda), None, c.mean.to(cuda), c.invstd.to(cuda), None, ev)
        got = bn_.backward_consts(partials, rows, c.count, st)
        torch.cuda.synchronize()
        o = R.Case()
        o.dgamma, o.dbeta, o.c0, o.c1 = got
        r = R.bwd_consts(c.partials, c.count, c.scale, c.mean, c.invstd, 0, slabs=slabs, eval=ev)
        _compare(kind, o, r, BWD_NAMES, worst)
        if ev:
            assert float(o.c0.abs().max()) == 0.0 and float(o.c1.abs().max()) == 0.0
            assert float(o.dgamma.abs().max()) > 0.0 and float(o.dbeta.abs().max()) > 0.0
    _report(f"backward_consts rows {rows}", worst)


# ---- composition: gather -> batch_stats -> apply -> dz -> backward_consts ---------------------

def test_block_composition_against_the_fp64_module_chain(cuda):
    """One EdgeConv block's BatchNorm path at B 2, N 65, k 7, Co 65, gamma of mixed
    sign: dgx.edgeconv.edge_select, dgx.bn.batch_stats, the apply, the dz kernel and
    dgx.bn.backward_consts, against nn.BatchNorm2d (double) -> LeakyReLU(0.2) ->
    max(dim=-1) on the same PQ and idx. The forward and the per-edge input
    gradient a dz [selected] + c0 + c1 y must lie within the bounds summed along
    the chain (u = 2^-24, E = B N k edges, every sum in any order):
      y = fl(P_j + Q_i): u |y|;   sums of E terms: (E + 64) u sum|term| on top of the terms' own;
      mean, var, invstd, a, b: _edgebn_ref's first-order propagation of those sum errors + 2u of each;
      z = fma(a, ysel, b): da |y| + |a| u |y| + db + u |z|, LeakyReLU 1-Lipschitz, + u |out|;
      dz = dY LReLU'(z): u |dz|, + (1 - slope) |dY| where |z| is below its bound (the sign may differ);
      yhat: invstd (u |y| + dmean + u |y - mean|) + |y - mean| dinvstd + 2u |yhat|;
      dbeta, dgamma: the summed term bounds + (M + 64) u sum|term|;
      c1 = -a g2 invstd, c0 = -a g1 - c1 mean (g = sums / E): first order in every factor + 4u of each product;
      gradient: |dz| da + |a| dz_b + c0_b + c1_b |y|."""
    from dgx import edgeconv as E
    L = nat.lib()
    B, N, k, Co, slope = 2, 65, 7, 65, R.f32_value(0.2)
    M, Ed, U = B * N, B * N * k, R.U
    g = torch.Generator().manual_seed(11)
    PQ = torch.randn(M, 2 * Co, generator=g)
    idx = torch.stack([torch.randperm(N, generator=g)[:k] for _ in range(M)]).int().view(B, N, k)   # no duplicate neighbours
    gamma = torch.randn(Co, generator=g)
    gamma[0], gamma[-1] = gamma[0].abs(), -gamma[-1].abs()
    beta = 0.3 * torch.randn(Co, generator=g)
    dY = torch.randn(M, Co, generator=g)
    eps = 1e-5
    # the fp64 module chain
    i = torch.arange(M).repeat_interleave(k)
    j = (i // N) * N + idx.view(-1).long()
    y = (PQ[:, :Co].double()[j] + PQ[:, Co:].double()[i]).view(B, N, k, Co).permute(0, 3, 1, 2).contiguous()
    y.requires_grad_(True)
    bn = torch.nn.BatchNorm2d(Co, eps=eps).double().train()
    with torch.no_grad():
        bn.weight.copy_(gamma.double())
        bn.bias.copy_(beta.double())
    want, want_arg = torch.nn.functional.leaky_relu(bn(y), slope).max(dim=-1)
    want.backward(dY.double().view(B, N, Co).permute(0, 2, 1))
    # the engine
    dPQ, didx, dgam, dbet = PQ.to(cuda), idx.to(cuda), gamma.to(cuda), beta.to(cuda)
    st_ = nat.stream_of(dPQ)
    ysel, arg, sumP, part, prow = E.edge_select(dPQ, didx, B, N, k, Co, dgam, st_)
    mod = torch.nn.BatchNorm2d(Co, eps=eps).to(cuda).train()
    st = bn_.batch_stats(part, prow, float(Ed), mod, dgam, dbet)
    out = torch.empty(M, Co, device=cuda)
    nat.check(L.dgx_bn_lrelu_apply_f32(nat.ptr(ysel), M, Co, nat.ptr(st.scale), nat.ptr(st.shift), slope, nat.ptr(out),
                                       Co, None, st_), "apply")
    nblk = 3
    dz = torch.empty(M, Co, device=cuda)
    bpart = torch.empty(nblk, 2, Co, device=cuda)
    ddY = dY.to(cuda)
    nat.check(L.dgx_edge_bwd_dz_f32(nat.ptr(ddY), Co, nat.ptr(ysel), M, Co, nat.ptr(st.scale), nat.ptr(st.shift),
                                    nat.ptr(st.mean), nat.ptr(st.invstd), slope, nat.ptr(dz), nat.ptr(bpart), nblk, st_),
              "dz")
    dgamma, dbeta, c0, c1 = bn_.backward_consts(bpart, nblk, float(Ed), st)
    torch.cuda.synchronize()
    D = lambda v: v.detach().double().cpu()
    # bounds along the chain
    ye = y.detach().permute(0, 2, 3, 1).reshape(Ed, Co)                    # edge-major (E, Co)
    mean, var = ye.mean(0), ye.var(0, unbiased=False)
    e1 = (Ed + 64) * U * ye.abs().sum(0)
    e2 = (Ed + 64 + 3) * U * (ye * ye).sum(0)
    dmean = e1 / Ed
    dvar = e2 / Ed + 2 * mean.abs() * dmean
    invstd = (var + eps).rsqrt()
    dinv = 0.5 * invstd ** 3 * dvar + 2 * U * invstd
    gm, bt = gamma.double(), beta.double()
    a = gm * invstd
    da = gm.abs() * dinv + 2 * U * a.abs()
    sh = bt - mean * a
    dsh = a.abs() * dmean + mean.abs() * da + 2 * U * (sh.abs() + (mean * a).abs())
    pm = lambda v: v.permute(0, 2, 1).reshape(M, Co)
    sel = torch.zeros(B, Co, N, k, dtype=F64).scatter_(3, want_arg.unsqueeze(-1), 1.0)
    ys = pm((y.detach() * sel).sum(-1))                                   # the selected pre-BN value (M, Co)
    z = a * ys + sh
    z_b = da * ys.abs() + a.abs() * U * ys.abs() + dsh + U * z.abs()
    out_ref = pm(want.detach())
    out_b = z_b + U * out_ref.abs()
    ratio = {"out": R.worst(D(out), out_ref, out_b),
             "scale": R.worst(D(st.scale), a, da), "shift": R.worst(D(st.shift), sh, dsh)}
    assert torch.equal(D(arg).long(), pm(want_arg)), "no duplicate neighbours: the selected slot is autograd's"
    go = dY.double()
    dz_ref = go * R.lrelu_grad(z > 0, slope)
    dz_b = U * dz_ref.abs() + (z.abs() <= z_b).double() * go.abs() * (1 - slope)
    yh = (ys - mean) * invstd
    yh_b = invstd * (U * ys.abs() + dmean + U * (ys - mean).abs()) + (ys - mean).abs() * dinv + 2 * U * yh.abs()
    t2 = dz_ref * yh
    db_ref, dg_ref = dz_ref.sum(0), t2.sum(0)
    db_b = dz_b.sum(0) + (M + 64) * U * dz_ref.abs().sum(0)
    dg_b = (dz_b * yh.abs() + dz_ref.abs() * yh_b + dz_b * yh_b + U * t2.abs()).sum(0) + (M + 64) * U * t2.abs().sum(0)
    ratio["dbeta"], ratio["dgamma"] = R.worst(D(dbeta), db_ref, db_b), R.worst(D(dgamma), dg_ref, dg_b)
    assert _rel(db_ref, bn.bias.grad) < 1e-12 and _rel(dg_ref, bn.weight.grad) < 1e-12
    g1, g2 = db_ref / Ed, dg_ref / Ed
    c1_ref = -a * g2 * invstd
    c1_b = (g2 * invstd).abs() * da + (a * invstd).abs() * dg_b / Ed + (a * g2).abs() * dinv + 4 * U * c1_ref.abs()
    c0_ref = -a * g1 - c1_ref * mean
    c0_b = g1.abs() * da + a.abs() * db_b / Ed + c1_b * mean.abs() + c1_ref.abs() * dmean \
        + 4 * U * ((a * g1).abs() + (c1_ref * mean).abs())
    ratio["c0"], ratio["c1"] = R.worst(D(c0), c0_ref, c0_b), R.worst(D(c1), c1_ref, c1_b)
    # the per-edge input gradient from the engine's a, dz, c0, c1 and the fp64 y
    v = lambda t: t.view(1, Co, 1, 1)
    spread = lambda t: t.view(B, N, Co).permute(0, 2, 1).unsqueeze(-1)      # (M, Co) -> (B, Co, N, 1)
    got_dy = spread(D(st.scale) * D(dz)) * sel + v(D(c0)) + v(D(c1)) * y.detach()
    dy_b = spread(dz_ref.abs() * da + (a.abs() + da) * dz_b) * sel + v(c0_b) + v(c1_b) * y.detach().abs()
    ratio["dy"] = R.worst(got_dy, y.grad, dy_b)
    print("[edgebn] composition: worst got/bound " + ", ".join(f"{n} {r:.3f}" for n, r in ratio.items()))
    assert all(r <= 1.0 for r in ratio.values()), ratio


def _rel(got, want):
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-300))
