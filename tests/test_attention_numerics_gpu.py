"""f2 numerics: the attention kernels (csrc/attention.hip via dgx.attention)
where `torch.randn` operands cannot reach: structured softmax rows, every tile
edge, operand and dO layouts through the backward, the module's separate
projection weights, the dropout mask read out of each kernel, and the
magnitude of dO.

Every reference is the fp64 restatement of test_attention_gpu (`_ref`) on the
same 16-bit-rounded operands (the fp32 operands themselves in the split-fp32
mode); bars are that file's TOL_FWD / TOL_BWD, normwise. Where the scores are
large the bar grows by what the score arithmetic itself allows, derived from
the operands in the test (`_eps_s`): a score is a D-term fp32 sum (16-bit
types: relative error u = D * 2^-24 of sum |q_d k_d|) or a split-plane sum
that drops lo*lo (u = 2^-16), so each softmax weight is off by at most a
factor exp(2 eps_s), eps_s = u * max_ij sum_d |q_id k_jd| * scale.

All random operands come from seeded generators of their own: the host RNG
state is not touched.
"""
import copy
import functools
import math

import pytest
import torch

from test_attention_gpu import TOL_BWD, TOL_FWD, _nerr, _ref

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16, torch.float32]
LOG2E = 1.4426950408889634
NAMES = ("dq", "dk", "dv")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(shape, g, dt=torch.float32):
    return torch.randn(shape, generator=g).to(dt)


def _heads(t, H):
    B, N, E = t.shape
    return t.detach().double().cpu().contiguous().view(B, N, H, E // H).transpose(1, 2)   # (B, H, N, D)


def _ref_run(q, k, v, H, go=None, mask=None, p=0.0):
    """fp64 on the host: o (B, Nq, E), lse (B*H*Nq, log2 domain of the scaled
    scores, as the forward keeps it), (dq, dk, dv) for the output gradient go."""
    scale = 1.0 / math.sqrt(q.shape[2] // H)
    qr, kr, vr = (t.detach().double().cpu().contiguous().requires_grad_(True) for t in (q, k, v))
    o = _ref(qr, kr, vr, H, scale, mask=None if mask is None else mask.cpu(), p=p)
    with torch.no_grad():
        s = _heads(q, H) @ _heads(k, H).transpose(-1, -2) * scale
        lse = (torch.logsumexp(s, -1) * LOG2E).reshape(-1)
    grads = None
    if go is not None:
        o.backward(go.detach().double().cpu())
        grads = (qr.grad, kr.grad, vr.grad)
    return o.detach(), lse, grads


def _eng_run(q, k, v, H, go=None, p=0.0):
    """The engine on device operands as given (views keep their strides):
    o, (dq, dk, dv) for go; go = "sum" runs o.sum().backward()."""
    from dgx.attention import attention
    qe, ke, ve = (t.detach().requires_grad_(True) for t in (q, k, v))
    o = attention(qe, ke, ve, H, dropout_p=p)
    grads = None
    if go is not None:
        if isinstance(go, str):
            o.sum().backward()
        else:
            o.backward(go)
        grads = (qe.grad, ke.grad, ve.grad)
    return o.detach(), grads


def _eng_lse(q, k, v, H):
    import dgx.attention as A
    scale = 1.0 / math.sqrt(q.shape[2] // H)
    return A.attn_forward(q, k, v, H, 0.0, scale, A.compute_dtype(q), None)[1]


def _eps_s(q, k, H, dt):
    """Bound on the absolute error of a scaled score (natural units), from the
    operands: u * max_ij sum_d |q_id k_jd| * scale (module docstring)."""
    D = q.shape[2] // H
    m = float((_heads(q, H).abs() @ _heads(k, H).abs().transpose(-1, -2)).max()) / math.sqrt(D)
    return (2.0 ** -16 if dt == torch.float32 else D * 2.0 ** -24) * m


def _ulp32(x):
    return math.ldexp(1.0, math.frexp(float(x))[1] - 24)


def _check_lse(got, want, eps, what):
    bar = LOG2E * eps + 4 * _ulp32(want.abs().max())
    err = float((got.double().cpu() - want).abs().max())
    print(what, "lse err", err, "bar", bar, "eps_s", eps)
    assert err <= bar, (what, "lse", err, bar, eps)


def _check_grads(got, want, bar, what):
    for n, g, w in zip(NAMES, got, want):
        e = _nerr(g, w)
        print(what, n, e, "bar", bar)
        assert e < bar, (what, n, e, bar)


# ------------------------------------------------- A. structured softmax ----
SB, SH, SNQ, SNK = 1, 2, 77, 130   # ragged in both query tiles and in the third key tile


def _onehot_qk(D, dt, g):
    """k = randn, q_i = 12 k[pi(i)], pi(i) = 53 i mod Nk: one target per row, in
    every key tile (63, 64 and 128 among them); the target's score is 55 to 200
    natural units (past 128 in the exp2 domain) and every other score at least
    30 below it, so each weight is 1 or below 2^-43: o = v[pi] exactly."""
    k = _randn((SB, SNK, SH * D), g, dt)
    pi = (53 * torch.arange(SNQ)) % SNK
    q = (12 * k[:, pi].float()).to(dt)
    return q, k, pi


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dt", DTYPES)
def test_onehot_rows_forward(cuda, dt, D):
    g = _gen(100 + D)
    q, k, pi = _onehot_qk(D, dt, g)
    v = _randn((SB, SNK, SH * D), g, dt)
    ref, lse, _ = _ref_run(q, k, v, SH)
    # the construction itself: the runner-up of every row is at least 30 natural units down
    s = _heads(q, SH) @ _heads(k, SH).transpose(-1, -2) / math.sqrt(D)
    top2 = s.topk(2, -1)[0]
    assert float((top2[..., 0] - top2[..., 1]).min()) > 30 and float(top2[..., 0].max()) * LOG2E > 128
    assert torch.equal(s.argmax(-1), pi.expand(SB, SH, SNQ))
    q, k, v = (t.to(cuda) for t in (q, k, v))
    o, _ = _eng_run(q, k, v, SH)
    if dt == torch.float32:
        assert _nerr(o, ref) < TOL_FWD[dt], _nerr(o, ref)
    else:
        for h in range(SH):
            sl = slice(h * D, (h + 1) * D)
            assert torch.equal(o[..., sl], v[:, pi.to(cuda)][..., sl]), h
    _check_lse(_eng_lse(q, k, v, SH), lse, _eps_s(q, k, SH, dt), "one-hot")


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dt", DTYPES)
def test_onehot_rows_backward(cuda, dt, D):
    """Even rows one-hot, odd rows randn: the diffuse rows set max|grad_ref|,
    and the peaked rows' dq (dS = 0) must vanish under the same normwise bar."""
    g = _gen(200 + D)
    q, k, _ = _onehot_qk(D, dt, g)
    q[:, 1::2] = _randn(q[:, 1::2].shape, g, dt)
    v = _randn((SB, SNK, SH * D), g, dt)
    go = _randn((SB, SNQ, SH * D), g, dt)
    ref, _, want = _ref_run(q, k, v, SH, go)
    assert float(want[0][:, 0::2].abs().max()) < 1e-9 * float(want[0].abs().max())
    o, got = _eng_run(*(t.to(cuda) for t in (q, k, v)), SH, go.to(cuda))
    assert _nerr(o, ref) < TOL_FWD[dt], _nerr(o, ref)
    _check_grads(got, want, TOL_BWD[dt], "one-hot/randn rows")


def _moving_qk(kind, D, dt, g):
    """Scores that move along the key axis. ascending / descending: q = 4 +
    randn, k_j = level_j (7.5 / sqrt(D)) + 0.3 randn with level = -1, 0, +1 on
    the three 64-key tiles (reversed for descending): the scores are a
    staircase of 30 natural units per tile under noise of about 1.3, so every
    row stays spread over the keys of its top tile. ascending replaces the
    running max in every tile (alpha = exp2(m - mx) about 2^-43 each time);
    descending never replaces it after tile 0 (alpha exactly 1). Two choices
    keep the comparison about the softmax and not about the data: the large
    component sits in q, not in k (dq = sum_j dS_ij k_j has sum_j dS_ij = 0, so
    a large common part of k makes dq a difference of large terms), and the
    rows are not nearly one-hot (delta = rowsum(dO . O) reads the 16-bit
    rounded O, an absolute error in dS that a row with almost no gradient of
    its own cannot hide; exactly one-hot rows, where O = v[target] is exact,
    have their own test above). offset: q, k = 2.6 (1.5 + 0.5 randn), every key
    shares a large component with every query: scores above 90."""
    E = SH * D
    if kind == "offset":
        q = 2.6 * (1.5 + 0.5 * _randn((SB, SNQ, E), g))
        k = 2.6 * (1.5 + 0.5 * _randn((SB, SNK, E), g))
    else:
        level = (torch.arange(SNK) // 64 - 1).float()
        if kind == "descending":
            level = -level
        q = 4.0 + _randn((SB, SNQ, E), g)
        k = level.view(1, SNK, 1) * (7.5 / math.sqrt(D)) + 0.3 * _randn((SB, SNK, E), g)
    return q.to(dt), k.to(dt)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("kind", ["ascending", "descending", "offset"])
@pytest.mark.parametrize("dt", DTYPES)
def test_moving_scores(cuda, dt, kind, D):
    g = _gen(300 + D)
    q, k = _moving_qk(kind, D, dt, g)
    v = _randn((SB, SNK, SH * D), g, dt)
    go = _randn((SB, SNQ, SH * D), g, dt)
    ref, lse, want = _ref_run(q, k, v, SH, go)
    s = _heads(q, SH) @ _heads(k, SH).transpose(-1, -2) / math.sqrt(D)
    tiles = [s[..., :64].amax(-1), s[..., 64:128].amax(-1), s[..., 128:].amax(-1)]   # per 64-key tile
    if kind == "ascending":      # every tile raises every row's max
        assert bool((tiles[1] > tiles[0] + 10).all()) and bool((tiles[2] > tiles[1] + 10).all())
    elif kind == "descending":   # no later tile reaches the first tile's max
        assert bool((tiles[0] > tiles[1] + 10).all()) and bool((tiles[1] > tiles[2] + 10).all())
    else:
        assert float(s.min()) > 90
    eps = _eps_s(q, k, SH, dt)
    widen = math.expm1(2 * eps)
    q, k, v = (t.to(cuda) for t in (q, k, v))
    o, got = _eng_run(q, k, v, SH, go.to(cuda))
    e = _nerr(o, ref)
    print(kind, "fwd", e, "bar", TOL_FWD[dt] + widen, "eps_s", eps)
    assert e < TOL_FWD[dt] + widen, (kind, e, TOL_FWD[dt] + widen, eps)
    _check_lse(_eng_lse(q, k, v, SH), lse, eps, kind)
    _check_grads(got, want, TOL_BWD[dt] + widen, f"{kind} eps_s {eps:.3g}")


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dt", DTYPES)
def test_uniform_rows(cuda, dt, D):
    """q = 0: every weight is 1 / Nk, o the column mean of v, lse = log2(Nk),
    dk exactly 0 (dk = dS^T q), dq and dv their references."""
    Nk = 300
    g = _gen(400 + D)
    q = torch.zeros((SB, SNQ, SH * D), dtype=dt)
    k = _randn((SB, Nk, SH * D), g, dt)
    v = _randn((SB, Nk, SH * D), g, dt)
    go = _randn((SB, SNQ, SH * D), g, dt)
    ref, lse, want = _ref_run(q, k, v, SH, go)
    assert float((ref - v.double().mean(1, keepdim=True)).abs().max()) < 1e-12
    q, k, v = (t.to(cuda) for t in (q, k, v))
    o, got = _eng_run(q, k, v, SH, go.to(cuda))
    assert _nerr(o, ref) < TOL_FWD[dt], _nerr(o, ref)
    got_lse = _eng_lse(q, k, v, SH).double().cpu()
    assert float((got_lse - math.log2(Nk)).abs().max()) <= 4 * _ulp32(math.log2(Nk))
    _check_lse(got_lse, lse, 0.0, "uniform")
    assert not bool(got[1].any()), "dk with q = 0"
    for i in (0, 2):
        assert _nerr(got[i], want[i]) < TOL_BWD[dt], (NAMES[i], _nerr(got[i], want[i]))


# ------------------------------------------------------- B. tile edges ------
# 16 (MFMA tile, keys per wave of the dK/dV pass), 32 (queries per wave), 64
# (K/V and Q/dO tiles), 128 (queries per block): N = tile, tile +- 1, Nk = 1
EDGES = [(1, 1, 64), (17, 1, 64), (15, 17, 64), (16, 16, 64), (33, 63, 64), (32, 64, 64), (31, 65, 64),
         (127, 129, 64), (128, 128, 64), (129, 127, 64), (127, 129, 128), (128, 128, 128), (129, 127, 128)]
# head padding: D < 64 -> 64, 64 < D < 128 -> 128, D not a multiple of 8
EDGES += [(33, 65, D) for D in (8, 20, 40, 72, 96, 120)]


@pytest.mark.parametrize("Nq,Nk,D", EDGES)
@pytest.mark.parametrize("dt", DTYPES)
def test_tile_edges(cuda, dt, Nq, Nk, D):
    B, H = 1, 2
    g = _gen(1000 * Nq + 10 * Nk + D)
    q = _randn((B, Nq, H * D), g, dt)
    k = _randn((B, Nk, H * D), g, dt)
    v = _randn((B, Nk, H * D), g, dt)
    go = _randn((B, Nq, H * D), g, dt)
    ref, _, want = _ref_run(q, k, v, H, go)
    o, got = _eng_run(*(t.to(cuda) for t in (q, k, v)), H, go.to(cuda))
    assert o.shape == ref.shape and o.dtype == dt
    assert _nerr(o, ref) < TOL_FWD[dt], _nerr(o, ref)
    for i, n in enumerate(NAMES):
        if Nk == 1 and n != "dv":
            # one key: P = 1, dS = dP - delta = 0, the true dq and dk are identically zero;
            # the kernels form dS from two differently ordered sums, so bound the absolute error
            dp = float((_heads(go, H) @ _heads(v, H).transpose(-1, -2)).abs().max())
            other = float((k if n == "dq" else q).double().abs().max())
            bar = TOL_BWD[dt] / math.sqrt(D) * dp * other
            assert float(want[i].abs().max()) <= 1e-12
            e = float(got[i].double().abs().max())
            assert e <= bar, (n, e, bar)
        else:
            e = _nerr(got[i], want[i])
            assert e < TOL_BWD[dt], (n, e)


# ------------------------------------------- C. layouts through the backward --
LAYOUTS = ["qkv_slices", "kv_slices", "seq_first", "misaligned", "dout_transposed", "dout_expanded"]


def _layout_case(layout, dt, dev):
    """(q, k, v, go) on the device as the named views; go may be "sum"."""
    B, H, D, N, M = 2, 2, 64, 96, 80
    E = H * D
    g = _gen(500 + LAYOUTS.index(layout))
    go = _randn((B, N, E), g, dt).to(dev)
    if layout == "qkv_slices":       # one (B, N, 3E) in-projection (self-attention)
        qkv = _randn((B, N, 3 * E), g, dt).to(dev)
        return qkv[..., :E], qkv[..., E:2 * E], qkv[..., 2 * E:], go
    q = _randn((B, N, E), g, dt).to(dev)
    if layout == "kv_slices":        # cross-attention over one memory: (B, M, 2E)
        kv = _randn((B, M, 2 * E), g, dt).to(dev)
        return q, kv[..., :E], kv[..., E:], go
    if layout == "seq_first":        # batch_first=False: (N, B, E) transposed
        q, k, v = (_randn((n, B, E), g, dt).to(dev).transpose(0, 1) for n in (N, M, M))
        return q, k, v, go
    if layout == "misaligned":       # 8 bytes into a row: not 16-byte aligned, the copy branch of _operand
        q, k, v = (_randn((B, n, E + 8), g, dt).to(dev)[..., 4:4 + E] for n in (N, M, M))
        assert q.data_ptr() % 16 == 8 and all(s % 8 == 0 for s in q.stride()[:2])
        return q, k, v, go
    k = _randn((B, M, E), g, dt).to(dev)
    v = _randn((B, M, E), g, dt).to(dev)
    if layout == "dout_transposed":
        return q, k, v, _randn((N, B, E), g, dt).to(dev).transpose(0, 1)
    return q, k, v, "sum"            # o.sum().backward(): dO is a stride-0 expansion of one 1


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
def test_layouts_backward(cuda, dt, layout):
    q, k, v, go = _layout_case(layout, dt, cuda)
    if layout not in ("dout_transposed", "dout_expanded"):
        assert not (q.is_contiguous() and k.is_contiguous() and v.is_contiguous())
    dense = torch.ones((q.shape[0], q.shape[1], q.shape[2]), dtype=dt, device=cuda) if isinstance(go, str) \
        else go.contiguous()
    ref, _, want = _ref_run(q, k, v, 2, dense)
    o, got = _eng_run(q, k, v, 2, go)
    assert _nerr(o, ref) < TOL_FWD[dt], _nerr(o, ref)
    _check_grads(got, want, TOL_BWD[dt], layout)
    o2, got2 = _eng_run(q.contiguous(), k.contiguous(), v.contiguous(), 2, dense)
    assert torch.equal(o, o2)
    for n, a, b in zip(NAMES, got, got2):
        assert torch.equal(a, b), (layout, n)


# -------------------------------------------------- D. module parity --------
@pytest.mark.parametrize("form", ["self", "cross", "separate", "kvdim"])
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("batch_first", [True, False])
def test_module_matches_torch_mha_fp64(cuda, batch_first, bias, form):
    """EngineMultiheadAttention (eval, fp32 parity mode) against stock
    nn.MultiheadAttention in fp64 on the host with the same weights: output,
    every parameter's gradient, every input's gradient. "kvdim" is kdim = 96,
    vdim = 72: the separate q/k/v_proj_weight branch."""
    from dgx import precision as prec
    from dgx.attention import EngineMultiheadAttention, use_engine_attention
    E, H, B, N, M = 128, 2, 2, 48, 40
    kd, vd = (96, 72) if form == "kvdim" else (None, None)
    with torch.random.fork_rng(devices=[]):   # the constructor's init draws from the host generator
        ref = torch.nn.MultiheadAttention(E, H, bias=bias, batch_first=batch_first, kdim=kd, vdim=vd)
    assert ref._qkv_same_embed_dim == (form != "kvdim")
    g = _gen(600)
    with torch.no_grad():
        for p in ref.parameters():
            p.copy_(_randn(p.shape, g) * (0.3 if p.dim() == 1 else 1.0 / math.sqrt(p.shape[-1])))
    eng = use_engine_attention(copy.deepcopy(ref).to(cuda)).eval()
    assert type(eng) is EngineMultiheadAttention
    ref = ref.double().eval()

    def seq(n, width):
        t = _randn((B, n, width), g)
        return t if batch_first else t.transpose(0, 1).contiguous()
    x = seq(N, E)
    if form == "self":
        ins = [x]
        pick = (0, 0, 0)
    elif form == "cross":
        ins = [x, seq(M, E)]
        pick = (0, 1, 1)
    else:
        ins = [x, seq(M, kd or E), seq(M, vd or E)]
        pick = (0, 1, 2)
    go = seq(N, E)
    rin = [t.double().requires_grad_(True) for t in ins]
    ein = [t.to(cuda).requires_grad_(True) for t in ins]
    want, _ = ref(*(rin[i] for i in pick), need_weights=False)
    want.backward(go.double())
    with prec.mode("fp32"):
        got, none = eng(*(ein[i] for i in pick), need_weights=False)
        got.backward(go.to(cuda))
    assert none is None and got.dtype == torch.float32 and got.shape == want.shape
    assert _nerr(got, want) < TOL_FWD[torch.float32], _nerr(got, want)
    bar = TOL_BWD[torch.float32]
    names = [n for n, _ in ref.named_parameters()]
    assert names == [n for n, _ in eng.named_parameters()]
    assert ("q_proj_weight" in names) == (form == "kvdim")
    for (n, pr), pe in zip(ref.named_parameters(), eng.parameters()):
        assert pe.grad is not None and _nerr(pe.grad, pr.grad) < bar, (n, _nerr(pe.grad, pr.grad))
    for i, (r, e) in enumerate(zip(rin, ein)):
        assert _nerr(e.grad, r.grad) < bar, (i, _nerr(e.grad, r.grad))


# ------------------------------------------------- E. dropout masks ---------
SEED = 0x1234_5678_9ABC


def _fix_seed(monkeypatch):
    import dgx.attention as A
    monkeypatch.setattr(A, "new_seed", lambda dev: torch.tensor([SEED], dtype=torch.int64, device=dev))
    return A


@pytest.mark.parametrize("p", [0.1, 0.5, 0.9])
@pytest.mark.parametrize("D,Nk", [(64, 50), (128, 100)])
@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
def test_dropout_mask_read_out_of_kernels(cuda, monkeypatch, dt, D, Nk, p):
    """q = 0 (weights exactly 1 / Nk) and v[j] = e_j: o[q, j] is keep(q, j) /
    (Nk (1 - p)), the forward's mask; with dO rows e_c, dv[j, c] is the dK/dV
    pass's keep(q_c, j) / (Nk (1 - p)). Both equal dropout_mask bit for bit."""
    A = _fix_seed(monkeypatch)
    B, H, Nq = 2, 3, 150
    E = H * D
    assert Nk <= D
    g = _gen(700 + D)
    q = torch.zeros((B, Nq, E), dtype=dt, device=cuda)
    k = _randn((B, Nk, E), g, dt).to(cuda)
    v4 = torch.zeros((B, Nk, H, D), dtype=dt)
    j = torch.arange(Nk)
    v4[:, j, :, j] = 1
    v = v4.view(B, Nk, E).to(cuda)
    mask = A.dropout_mask(B * H * Nq, Nk, p, SEED, cuda).view(B, H, Nq, Nk).bool()
    ve = v.clone().requires_grad_(True)
    o = A.attention(q, k, ve, H, dropout_p=p)
    oh = o.detach().view(B, Nq, H, D).permute(0, 2, 1, 3)          # (B, H, Nq, D)
    assert torch.equal(oh[..., :Nk] != 0, mask), "forward mask"
    assert not bool(oh[..., Nk:].any())
    val = 1.0 / (Nk * (1.0 - p))
    half_ulp = 2.0 ** (-9 if dt == torch.bfloat16 else -12)
    assert float((oh[..., :Nk][mask].double() - val).abs().max()) <= 2 * half_ulp * val
    for c0 in range(0, Nq, D):
        n = min(D, Nq - c0)
        go = torch.zeros((B, Nq, H, D), dtype=dt)
        c = torch.arange(n)
        go[:, c0 + c, :, c] = 1
        dv, = torch.autograd.grad(o, ve, go.view(B, Nq, E).to(cuda), retain_graph=True)
        dvh = dv.view(B, Nk, H, D).permute(0, 2, 3, 1)             # (B, H, channel = query - c0, key)
        assert torch.equal(dvh[:, :, :n] != 0, mask[:, :, c0:c0 + n]), ("dK/dV mask", c0)
        assert not bool(dvh[:, :, n:].any())
        assert float((dvh[:, :, :n][mask[:, :, c0:c0 + n]].double() - val).abs().max()) <= 4 * half_ulp * val


@pytest.mark.parametrize("dt,Nq,Nk,D", [(torch.bfloat16, 77, 130, 128),
                                        (torch.float16, 150, 50, 64), (torch.bfloat16, 150, 50, 64),
                                        (torch.float16, 150, 100, 128), (torch.bfloat16, 150, 100, 128)])
def test_dropout_masked_reference_ragged(cuda, monkeypatch, dt, Nq, Nk, D):
    """Forward and backward with dropout against the fp64 reference that
    applies dropout_mask to the softmax weights, at ragged Nq != Nk, H = 3:
    dq here reads the dQ pass's regenerated mask (dq does not depend on the
    mask when q = 0, so the read-out test above cannot see it)."""
    A = _fix_seed(monkeypatch)
    B, H, p = 2, 3, 0.5
    g = _gen(800 + D + Nk)
    q = _randn((B, Nq, H * D), g, dt)
    k = _randn((B, Nk, H * D), g, dt)
    v = _randn((B, Nk, H * D), g, dt)
    go = _randn((B, Nq, H * D), g, dt)
    mask = A.dropout_mask(B * H * Nq, Nk, p, SEED, cuda)
    ref, _, want = _ref_run(q, k, v, H, go, mask=mask, p=p)
    o, got = _eng_run(*(t.to(cuda) for t in (q, k, v)), H, go.to(cuda), p=p)
    assert _nerr(o, ref) < TOL_FWD[dt], _nerr(o, ref)
    _check_grads(got, want, TOL_BWD[dt], "dropout")


# ------------------------------------------------- F. gradient range --------
# (B, H, Nq, Nk, D) and the randn operands of test_nonfinite_gpu's attention case
RB, RH, RNQ, RNK, RD = 1, 2, 77, 130, 64
RANGE_J = ([(torch.float16, j) for j in (-12, -6, 0, 4, 8, 11, "top")]
           + [(dt, j) for dt in (torch.bfloat16, torch.float32) for j in (-40, 0, 40)])


@functools.lru_cache(maxsize=None)
def _range_case(dt):
    g = _gen(5)
    q, k, v = (_randn((RB, n, RH * RD), g, dt) for n in (RNQ, RNK, RNK))
    go = _randn((RB, RNQ, RH * RD), g, dt)
    _, _, want = _ref_run(q, k, v, RH, go)
    qh, kh, vh, gh = (_heads(t, RH) for t in (q, k, v, go))
    P = torch.softmax(qh @ kh.transpose(-1, -2) / math.sqrt(RD), -1)
    dS = P * (gh @ vh.transpose(-1, -2) - (gh * (P @ vh)).sum(-1, keepdim=True))
    top = max(float(t.abs().max()) for t in (go.double(), dS) + tuple(want))
    # the largest j with 2^j max|dO|, 2^j max|dS_ref| and every 2^j max|grad_ref| below 2^15 (half of
    # fp16's maximum: the margin for rounding). Here max|dO| = 3.58, max|dS| = 1.59, the gradients 0.7-0.9:
    # j_top = 13 (and dO * 2^14 already overflows fp16).
    j_top = math.ceil(15 - math.log2(top)) - 1
    return q, k, v, go, want, j_top


def _range_engine(dt, dev):
    """One forward; returns f(j) -> (dq, dk, dv) for dO * 2^j, and dO * 2^j itself."""
    from dgx.attention import attention
    q, k, v, go, want, j_top = _range_case(dt)
    leaves = [t.to(dev).requires_grad_(True) for t in (q, k, v)]
    o = attention(*leaves, RH)

    def run(j):
        go_j = (go.double() * 2.0 ** j).to(dt)
        return torch.autograd.grad(o, leaves, go_j.to(dev), retain_graph=True), go_j
    return run, go, want, j_top


@pytest.mark.parametrize("dt,j", RANGE_J)
def test_gradient_range(cuda, dt, j):
    """The backward on dO * 2^j against 2^j * (fp64 gradients for dO): the dS
    scale follows max|dO|, so the error does not depend on j. A fixed 2^8 scale
    (before this test) returned inf / NaN for fp16 at j >= 8. Measured on
    gfx950, fp16: dq / dk / dv errors 3.7e-4 / 2.6e-4 / 3.0e-4 at every j from
    -12 to 14; the fp16 MFMA keeps subnormal operands, and below -12 the error
    doubles per step (dO * 2^j itself is rounded), first over 5e-3 at j = -17."""
    run, go, want, j_top = _range_engine(dt, cuda)
    if dt == torch.float16:
        assert j_top == 13
    if j == "top":
        j = j_top
    got, _ = run(j)
    _check_grads(got, [w * 2.0 ** j for w in want], TOL_BWD[dt], f"{dt} j={j}")


@pytest.mark.parametrize("dt", DTYPES)
def test_gradient_range_every_j_and_scale_invariance(cuda, dt):
    """fp16: every j from the floor to j_top meets the bar. All types: where
    dO * 2^j is exact, the gradients for j and for 0 are bitwise equal after
    the exact rescaling wherever both outputs are normal numbers (the packed
    dS does not depend on j)."""
    run, go, want, j_top = _range_engine(dt, cuda)
    js = list(range(-12, j_top + 1)) if dt == torch.float16 else [-40, 0, 40]
    base, _ = run(0)
    tiny = torch.finfo(dt).tiny
    for j in js:
        got, go_j = run(j)
        _check_grads(got, [w * 2.0 ** j for w in want], TOL_BWD[dt], f"{dt} j={j}")
        if not torch.equal(go_j.double(), go.double() * 2.0 ** j):
            continue   # dO * 2^j was rounded (fp16 subnormals): another input
        for n, a, b in zip(NAMES, got, base):
            a, b = a.double(), b.double() * 2.0 ** j
            normal = (a.abs() >= tiny) & (b.abs() >= tiny * 2.0 ** j) & torch.isfinite(a)
            assert bool(normal.any()) and torch.equal(a[normal], b[normal]), (n, j)


def test_gradient_range_never_finite_and_wrong(cuda):
    """fp16 above j_top, through the j at which dO itself overflows: every
    returned gradient either meets the bar or holds a non-finite value (which
    GradScaler sees and skips the step for); never finite and wrong."""
    dt = torch.float16
    run, go, want, j_top = _range_engine(dt, cuda)
    seen_overflow = False
    for j in range(j_top + 1, j_top + 5):
        got, go_j = run(j)
        seen_overflow |= not bool(torch.isfinite(go_j).all())
        for n, a, w in zip(NAMES, got, want):
            e = _nerr(a, w * 2.0 ** j) if bool(torch.isfinite(a).all()) else None
            print(n, j, e)
            assert e is None or e < TOL_BWD[dt], (n, j, e)
    assert seen_overflow
