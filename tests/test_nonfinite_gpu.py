"""Non-finite values through the engine (DESIGN "Non-finite values").

The training loop's GradScaler skips a step when a gradient is non-finite, and
the loss head answers a bad row with NaN so that it does. Both only work if an
inf or NaN that enters an engine kernel comes out non-finite at the other end
and no kernel turns one into an address. Every check here is a predicate (an
id is in range, a value is finite or not, two buffers are bitwise equal); the
reference is its own op sequence in stock PyTorch on the same inputs.

Section (a), the kNN kernels, launches nothing that consumes an id: a bad id
is a failed assertion on the host.
"""
import types

import numpy as np
import pytest
import torch

from dgx import synth

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")


# ------------------------------------------------------------------ (a) kNN --
# one shape per selection kernel dgx_knn_kernel_name tells apart (C, k, N)
KNN_SHAPES = [(3, 20, 250), (3, 40, 2048), (64, 20, 512), (128, 16, 300), (9, 64, 300)]
# (C, k, N) outside the fused kernel: C > 128, and k > 64
KNN_GENERIC_SHAPES = [(160, 20, 333), (64, 65, 300)]


def _bad_patterns(N):
    """name -> {point: {channel or None (= all): value}} written into cloud 0."""
    j = N // 2 + 1
    return {
        "nan_point": {j: {None: NAN}},
        "nan_coordinate": {j: {1: NAN}},
        "inf_minus_inf": {j: {0: INF, 1: -INF}},
        "several": {1: {None: NAN}, 17: {2: NAN}, N // 3: {0: INF, 1: -INF}, N - 2: {0: INF}},
        "first": {0: {None: NAN}},
        "last": {N - 1: {2: NAN}},
        "every_point": {p: {p % 3: NAN} for p in range(N)},
    }


def _cloud_pair(C, N, seed):
    pts = synth.cube_clouds(2, N, seed) if C == 3 else synth.relu_normal(seed, (2, N, C)) - np.float32(0.25)
    return np.ascontiguousarray(pts, dtype=np.float32)


def _poison(pts, pattern):
    out = pts.copy()
    for p, chans in pattern.items():
        for c, v in chans.items():
            if c is None:
                out[0, p, :] = v
            else:
                out[0, p, c] = v
    return out


def _knn_view(pts, layout, dev):
    t = torch.from_numpy(pts).to(dev)
    return t.permute(0, 2, 1) if layout == "perm" else t.permute(0, 2, 1).contiguous()


def _run_fused(x, k):
    """dgx_knn_prepare_f32 + dgx_knn_select_f32 (int64 ids, values) and
    dgx_knn_f32 (int32 ids) into caller buffers pre-filled with -1."""
    from dgx import _native as nat
    from dgx.ops import reduction_order
    L = nat.lib()
    B, C, N = x.shape
    sB, sC, sN = x.stride()
    order, s, dev = reduction_order(x), nat.stream_of(x), x.device
    idx64 = torch.full((B, N, k), -1, dtype=torch.int64, device=dev)
    idx32 = torch.full((B, N, k), -1, dtype=torch.int32, device=dev)
    vals = torch.full((B, N, k), -1.0, dtype=torch.float32, device=dev)
    xx = torch.empty(B * N, dtype=torch.float32, device=dev)
    nb = L.dgx_knn_image_bytes(B, C, N)
    img = torch.empty((nb + 3) // 4, dtype=torch.float32, device=dev)
    nat.check(L.dgx_knn_prepare_f32(nat.f32(x), sB, sC, sN, B, C, N, order, nat.f32(xx), nat.f32(img), nb, s),
              "prepare")
    nat.check(L.dgx_knn_select_f32(nat.f32(x), sB, sC, sN, nat.f32(xx), B, C, N, k, nat.ptr(idx64, torch.int64), None,
                                   nat.f32(vals), nat.f32(img), nb, s), "select")
    wb = L.dgx_knn_workspace_bytes(B, C, N)
    ws = torch.empty((wb + 3) // 4, dtype=torch.float32, device=dev)
    nat.check(L.dgx_knn_f32(nat.f32(x), sB, sC, sN, B, C, N, k, order, None, nat.i32(idx32), nat.f32(ws), wb, s), "knn")
    torch.cuda.synchronize()
    return idx64.cpu(), vals.cpu(), idx32.cpu()


def _run_generic(x, k):
    from dgx import _native as nat
    from dgx.ops import reduction_order
    L = nat.lib()
    B, C, N = x.shape
    sB, sC, sN = x.stride()
    dev = x.device
    idx64 = torch.full((B, N, k), -1, dtype=torch.int64, device=dev)
    vals = torch.full((B, N, k), -1.0, dtype=torch.float32, device=dev)
    wb = L.dgx_knn_generic_workspace_bytes(B, C, N)
    ws = torch.empty((wb + 3) // 4, dtype=torch.float32, device=dev)
    nat.check(L.dgx_knn_generic_f32(nat.f32(x), sB, sC, sN, B, C, N, k, reduction_order(x),
                                    nat.ptr(idx64, torch.int64), None, nat.f32(vals), nat.f32(ws), wb,
                                    nat.stream_of(x)), "knn (generic)")
    torch.cuda.synchronize()
    return idx64.cpu(), vals.cpu(), None


def _reference_nan_scores(pts0):
    """Where the reference's pairwise score (models/dgcnn.py:7-9) of cloud 0 is
    NaN: (N, N) bool, row = query. NaN-ness does not depend on summation order
    (no finite product overflows here)."""
    x = torch.from_numpy(pts0).t().unsqueeze(0)                 # (1, C, N)
    inner = -2 * torch.matmul(x.transpose(2, 1), x)
    xx = torch.sum(x ** 2, dim=1, keepdim=True)
    pd = -xx - inner - xx.transpose(2, 1)
    return torch.isnan(pd[0])


def _check_knn(run, C, k, N, layout, dev):
    clean_pts = _cloud_pair(C, N, seed=C + k + N)
    clean = run(_knn_view(clean_pts, layout, dev), k)
    assert bool(((clean[0] >= 0) & (clean[0] < N)).all())
    for name, pattern in _bad_patterns(N).items():
        pts = _poison(clean_pts, pattern)
        idx64, vals, idx32 = run(_knn_view(pts, layout, dev), k)
        for ids in (idx64, idx32):
            if ids is None:
                continue
            unwritten = int((ids == -1).sum())
            assert unwritten == 0, (name, "ranks left unwritten", unwritten)
            lo, hi = int(ids.min()), int(ids.max())
            assert 0 <= lo and hi < N, (name, "id out of range", lo, hi)
            # the clean cloud does not see its neighbour's values
            assert torch.equal(ids[1], clean[0][1].to(ids.dtype)), (name, "cloud 1 ids changed")
        assert torch.equal(vals[1].view(torch.int32), clean[1][1].view(torch.int32)), (name, "cloud 1 values changed")
        if idx32 is not None:
            # both entry points rank the same scores; NaN ties are not ordered
            assert torch.equal(idx32[1].long(), idx64[1])
        # torch.topk ranks NaN first: a candidate whose score is NaN for a finite
        # row is that row's neighbour (as long as k of them fit), so the NaN
        # spreads through the gather as it does in the reference
        nan_score = _reference_nan_scores(pts[0])
        finite_row = torch.from_numpy(np.isfinite(pts[0]).all(axis=1))
        member = torch.zeros(N, N, dtype=torch.bool)
        member.scatter_(1, idx64[0], True)
        rows = finite_row & (nan_score.sum(1) <= k)
        missing = (nan_score & ~member)[rows]
        assert not bool(missing.any()), (name, "NaN-score candidates not selected", int(missing.sum()))
        # and each row's ids are k distinct points
        assert bool((member.sum(1) == k).all()), (name, "repeated ids in a row")


@pytest.mark.parametrize("layout", ["bcn", "perm"])
@pytest.mark.parametrize("C,k,N", KNN_SHAPES)
def test_knn_ids_valid_for_nonfinite_input(cuda, C, k, N, layout):
    _check_knn(_run_fused, C, k, N, layout, cuda)


def test_knn_shapes_cover_distinct_kernels(cuda):
    from dgx import _native as nat
    names = {nat.lib().dgx_knn_kernel_name(C, k, N) for C, k, N in KNN_SHAPES}
    assert len(names) == len(KNN_SHAPES) and b"" not in names


@pytest.mark.parametrize("layout", ["bcn", "perm"])
@pytest.mark.parametrize("C,k,N", KNN_GENERIC_SHAPES)
def test_knn_generic_ids_valid_for_nonfinite_input(cuda, C, k, N, layout):
    from dgx import ops
    assert not ops.fast_shape(C, k, N)
    _check_knn(_run_generic, C, k, N, layout, cuda)


def test_knn_two_group_kernel_nonfinite(cuda):
    """The two-query-groups-per-wave kernel (C = 128 on a grid of at least 512
    workgroups: 52 clouds of 300 points): cloud 0 bad, the rest bitwise clean."""
    from dgx import _native as nat
    C, k, N, B = 128, 16, 300, 52
    # the route: the kernel of this (C, k, N) is the two-group one, and the grid is
    # not "small" (csrc/knn.hip knn_small: fewer than 512 workgroups of 32 queries)
    assert nat.lib().dgx_knn_kernel_name(C, k, N) == b"knn_kernel<32, 16, 2>"
    assert B * ((N + 31) // 32) >= 512
    pts = synth.relu_normal(5, (B, N, C)) - np.float32(0.25)
    x = _knn_view(pts, "bcn", cuda)
    clean = _run_fused(x, k)
    bad = pts.copy()
    bad[0, 7, :] = NAN
    bad[0, N - 1, 3] = INF
    idx64, vals, idx32 = _run_fused(_knn_view(bad, "bcn", cuda), k)
    for ids in (idx64, idx32):
        assert int((ids == -1).sum()) == 0
        assert 0 <= int(ids.min()) and int(ids.max()) < N
        assert torch.equal(ids[1:], clean[0][1:].to(ids.dtype))
    assert torch.equal(vals[1:].view(torch.int32), clean[1][1:].view(torch.int32))
    finite_rows = [i for i in range(N) if i not in (7, N - 1)]
    assert bool((idx64[0][finite_rows] == 7).any(1).all())


# ------------------------------------------------------- (b) / (c) helpers --
def _rows(t):
    """(..., n) -> which rows hold a non-finite element."""
    return ~torch.isfinite(t.detach().float().cpu()).all(-1)


def _any(t):
    return bool((~torch.isfinite(t.detach().float().cpu())).any())


def _no_laundering(ref_rows, got_rows, what):
    laundered = ref_rows & ~got_rows
    assert not bool(laundered.any()), (what, "finite where the reference is not", int(laundered.sum()))


def _edge_blocks(widths, seed):
    """Reference blocks Conv2d(2C, Co, 1) -> BatchNorm2d -> LeakyReLU (models/dgcnn.py:54-73)
    with gammas of both signs; returns the host modules (the reference's)."""
    torch.manual_seed(seed)
    blocks = []
    for cin, co in zip(widths[:-1], widths[1:]):
        blk = torch.nn.Sequential(torch.nn.Conv2d(2 * cin, co, 1, bias=False), torch.nn.BatchNorm2d(co),
                                  torch.nn.LeakyReLU(0.2))
        with torch.no_grad():
            blk[1].weight.copy_(torch.randn(co))
            blk[1].bias.copy_(0.1 * torch.randn(co))
            blk[1].running_mean.copy_(0.1 * torch.randn(co))
            blk[1].running_var.copy_(torch.rand(co) + 0.5)
        blocks.append(blk)
    return blocks


def _reference_chain(blocks, x, k):
    """models/dgcnn.py:84-100 in stock PyTorch: (B, sum Co, N)."""
    from oracle import reference as R
    outs = []
    for blk in blocks:
        x = blk(R.graph_feature(x, k)).max(dim=-1)[0]
        outs.append(x)
    return torch.cat(outs, 1)


def _engine_chain(blocks, x, k):
    from dgx.edgeconv import edgeconv_stack
    B, _, N = x.shape
    return edgeconv_stack(x, k, blocks).view(B, N, -1).permute(0, 2, 1)


class _Variant:
    """How one engine route is entered: precision mode, BatchNorm mode, schedule
    switches, cloud layout; ``flags`` is what dgx.schedule.decide() must report
    inside it, so a route that was not taken fails instead of passing."""

    def __init__(self, mode="fp32", train=True, switches=(), widths=(64, 64), B=2, flags=None):
        self.mode, self.train, self.switches, self.widths, self.B = mode, train, dict(switches), widths, B
        self.flags = flags

    def enter(self, monkeypatch):
        import dgx.edgeconv as E
        from dgx import precision as prec
        from dgx import schedule as S
        for name, val in self.switches.items():
            monkeypatch.setattr(E, name, val)
        ctx = prec.mode(self.mode)
        ctx.__enter__()
        d = S.decide()
        seen = (bool(d.bf16),) + tuple(name for i, name in enumerate(S.OPT_BITS) if (d.opts >> i) & 1)
        return ctx, seen


_DEFAULT_ON = ("SCATTER_PACKED", "FOLD_BN_BWD", "FUSE_KNN_IMAGE", "FUSE_EDGE_DZ", "SPLIT32_EDGE")


def _flags(bf16, add=(), drop=()):
    from dgx import schedule as S
    on = (set(_DEFAULT_ON) | set(add)) - set(drop)
    return (bf16,) + tuple(n for n in S.OPT_BITS if n in on)


# name -> variant. The schedule (csrc/dgx_torch.cpp chain_backward) picks the
# kernels from these flags alone: fp32 -> dgx_edge_bwd_dz_f32 + the pull
# scatter with dz and slot bytes (fp32 dPQ); bf16 / split -> packed dz|slot
# words, bf16 / split-plane dPQ; FOLD_BN_BWD -> dgx_edge_bwd_scatter_fin_f32,
# else the separate finalize + dgx_edge_bwd_scatter[_packed]_f32; two bf16
# blocks -> dgx_gemm_edge_dz_bf16 writes block 1's packed dz (its further conditions: _gemm_dz_route). One
# cloud stored channel-major takes the same kernels: its point-major rows are a
# column-major view (tests/test_batch1_gpu.py), which the GEMMs must still read
# as rows. (dgx_edge_bwd_dz_cm_f32 is the edge MLP's: see its backward test.)
EDGE_VARIANTS = {
    "fp32_fin": _Variant("fp32", flags=(False, (), ())),
    "fp32_unfolded": _Variant("fp32", switches={"FOLD_BN_BWD": False}, flags=(False, (), ("FOLD_BN_BWD",))),
    "fp32_split_planes": _Variant("fp32_split", flags=(False, ("SPLIT32",), ())),
    "bf16_packed_fin": _Variant("bf16", flags=(True, (), ())),
    "bf16_packed_unfolded": _Variant("bf16", switches={"FOLD_BN_BWD": False}, flags=(True, (), ("FOLD_BN_BWD",))),
    "bf16_slot_bytes": _Variant("bf16", switches={"SCATTER_PACKED": False}, flags=(True, (), ("SCATTER_PACKED",))),
    "bf16_two_blocks_gemm_dz": _Variant("bf16", widths=(64, 64, 128), flags=(True, (), ())),
    "eval_fp32": _Variant("fp32", train=False, flags=(False, (), ())),
    "eval_bf16": _Variant("bf16", train=False, flags=(True, (), ())),
    "one_cloud_channel_major": _Variant("fp32", B=1, flags=(False, (), ())),
}
FORWARD_VARIANTS = ["fp32_fin", "bf16_packed_fin", "eval_fp32", "eval_bf16", "one_cloud_channel_major"]
N_PTS, K_NB = 130, 10


def _gemm_dz_route(widths, B, N, cuda):
    """The conditions under which chain_backward hands block l's dX GEMM the
    epilogue that writes block l-1's packed dz (csrc/dgx_torch.cpp:
    block_uses_prep, lds_ok, edge_dz_ok, besides bf16 + FUSE_EDGE_DZ +
    SCATTER_PACKED in the flags), for the last block of ``widths``."""
    from dgx import gemm as G
    cin, co, total = widths[-2], widths[-1], sum(widths[1:])
    off_in = sum(widths[1:-2])
    dpq16 = torch.empty(B * N, 2 * co, dtype=torch.bfloat16, device=cuda)
    x16 = torch.empty(B * N, total, dtype=torch.bfloat16, device=cuda)[:, off_in:off_in + cin]
    return (cin % 64 == 0 and total % 8 == 0 and off_in % 8 == 0 and x16.stride(0) % 8 == 0
            and x16.data_ptr() % 16 == 0 and bool(G.edge_dz_ok(dpq16, cin)))


def _run_variant(v, monkeypatch, cuda, x, gout=None):
    """Reference and engine forward (and backward with ``gout``) of the
    variant's blocks: (ref out, engine out, ref modules, engine modules, ref x, engine x)."""
    import copy
    ref_blocks = _edge_blocks(v.widths, seed=len(v.widths) + v.B)
    eng_blocks = [copy.deepcopy(b).to(cuda) for b in ref_blocks]
    for b in ref_blocks + eng_blocks:
        b.train(v.train)
    xr = x.clone().requires_grad_(True)
    xe = x.clone().to(cuda).requires_grad_(True)
    ref = _reference_chain(ref_blocks, xr, K_NB)
    ctx, seen = v.enter(monkeypatch)
    try:
        out = _engine_chain(eng_blocks, xe, K_NB)
        if gout is not None:
            ref.backward(gout)
            out.backward(gout.to(cuda))
            torch.cuda.synchronize()
    finally:
        ctx.__exit__(None, None, None)
    assert seen == _flags(*v.flags), ("route not taken", seen, _flags(*v.flags))
    if len(v.widths) > 2:
        assert _gemm_dz_route(v.widths, v.B, x.shape[2], cuda), "dgx_gemm_edge_dz_bf16 not reached"
    return ref, out, ref_blocks, eng_blocks, xr, xe


# ------------------------------------------------- (b) forward: no laundering --
@pytest.mark.parametrize("bad", [NAN, INF])
@pytest.mark.parametrize("name", FORWARD_VARIANTS)
def test_edgeconv_forward_keeps_nonfinite(cuda, monkeypatch, name, bad):
    """One NaN / inf in cloud 0's input: every (cloud, channel) row that is
    non-finite in the reference is non-finite in the engine's output, and the
    running statistics are non-finite exactly where the reference's are.
    (Training BatchNorm spreads it over the whole channel on both sides; in eval
    mode the gather's ordered maximum would pass over a NaN neighbour, so the
    kernel restores it from the slot sum.)"""
    v = EDGE_VARIANTS[name]
    torch.manual_seed(11)
    x = torch.randn(v.B, v.widths[0], N_PTS)
    x[0, 5, 33] = bad
    with torch.no_grad():
        ref, out, ref_blocks, eng_blocks, _, _ = _run_variant(v, monkeypatch, cuda, x)
    assert bool(_rows(ref).any())
    _no_laundering(_rows(ref), _rows(out), name)
    if not v.train:
        # eval: no BatchNorm sum spreads the value, so compare element by element.
        # The bad point is a neighbour of finite centres (all of them for a NaN:
        # topk's NaN-first order), whose own terms are finite: there only the
        # gather's maximum carries it. The engine may be non-finite where the
        # reference is finite (a -inf neighbour that max ignores), never the reverse.
        ref_bad = ~torch.isfinite(ref)
        others = torch.ones(N_PTS, dtype=torch.bool)
        others[33] = False
        assert bool(ref_bad[0][:, others].any()), "no finite centre sees the bad point"
        _no_laundering(ref_bad, ~torch.isfinite(out.cpu()), name + " per element")
    for rb, eb in zip(ref_blocks, eng_blocks):
        for stat in ("running_mean", "running_var"):
            assert torch.equal(torch.isfinite(getattr(rb[1], stat)), torch.isfinite(getattr(eb[1], stat).cpu())), stat


def _mlp_convs(seed):
    torch.manual_seed(seed)
    c1 = torch.nn.Sequential(torch.nn.Conv2d(6, 64, 1, bias=False), torch.nn.BatchNorm2d(64), torch.nn.LeakyReLU(0.2))
    c2 = torch.nn.Sequential(torch.nn.Conv2d(64, 128, 1, bias=False), torch.nn.BatchNorm2d(128),
                             torch.nn.LeakyReLU(0.2))
    with torch.no_grad():
        c1[1].weight.copy_(torch.randn(64))
        c2[1].weight.copy_(torch.randn(128))
    return c1, c2


def _run_edge_mlp(mode, cuda, x, gout=None, train=True):
    """PositionEmbedding's edge stage (models/layers.py:45-52): reference and
    engine. bf16 must take the fused forward kernel, fp32 the unfused ones (the
    stage's debug capture says which ran)."""
    import copy
    import dgx.edgeconv as E
    from dgx import precision as prec
    from dgx.edgemlp import edge_mlp2
    from oracle import reference as R
    r1, r2 = _mlp_convs(4)
    e1, e2 = copy.deepcopy(r1).to(cuda), copy.deepcopy(r2).to(cuda)
    for m in (r1, r2, e1, e2):
        m.train(train)
    xr = x.clone().requires_grad_(True)
    xe = x.clone().to(cuda).requires_grad_(True)
    ref = r2(r1(R.graph_feature(xr, K_NB))).max(dim=-1)[0]
    E.set_debug_capture({})
    try:
        with prec.mode(mode):
            out = edge_mlp2(xe, K_NB, e1, e2)
            if gout is not None:
                ref.backward(gout)
                out.backward(gout.to(cuda))
                torch.cuda.synchronize()
        cap = E.debug_capture()["emlp"]
    finally:
        E.set_debug_capture(None)
    assert cap["fused"] == (mode == "bf16") and cap["bf16"] == (mode == "bf16"), "edge MLP forward route not taken"
    return ref, out, (r1, r2), (e1, e2), xr, xe


@pytest.mark.parametrize("bad", [NAN, INF])
@pytest.mark.parametrize("mode", ["fp32", "bf16"])   # unfused fp32 kernels / the fused bf16 kernel
def test_edge_mlp_forward_keeps_nonfinite(cuda, mode, bad):
    x = torch.from_numpy(synth.cube_clouds(2, N_PTS, 3)).permute(0, 2, 1).contiguous()
    x[0, 1, 40] = bad
    with torch.no_grad():
        ref, out, rs, es, _, _ = _run_edge_mlp(mode, cuda, x)
    assert bool(_rows(ref).any())
    _no_laundering(_rows(ref), _rows(out), mode)
    for rb, eb in zip(rs, es):
        for stat in ("running_mean", "running_var"):
            assert torch.equal(torch.isfinite(getattr(rb[1], stat)), torch.isfinite(getattr(eb[1], stat).cpu())), stat


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_edge_mlp_eval_nan_point_documented(cuda, mode):
    """A deliberate difference (DESIGN "Non-finite values"): with running
    statistics the edge MLP's maximum over k (mlp_max_kernel, the fused
    kernel's epilogue) compares ordered and passes over a NaN edge, where the
    reference's max returns it. What the engine guarantees instead: the bad
    point's own column is non-finite in every channel (all its edges are NaN),
    so the loss still is; the clean cloud is untouched."""
    x = torch.from_numpy(synth.cube_clouds(2, N_PTS, 3)).permute(0, 2, 1).contiguous()
    x[0, :, 40] = NAN
    with torch.no_grad():
        ref, out, _, _, _, _ = _run_edge_mlp(mode, cuda, x, train=False)
    out = out.cpu()
    assert not bool(torch.isfinite(ref[0, :, 40]).any())
    assert not bool(torch.isfinite(out[0, :, 40]).any())
    assert not bool(torch.isfinite(out.sum()))
    assert bool(torch.isfinite(out[1]).all()) and bool(torch.isfinite(ref[1]).all())


# ------------------------------------------------ (c) backward: no laundering --
def _grads_not_laundered(pairs, what):
    """pairs: (name, reference gradient, engine gradient)."""
    some = False
    for name, want, got in pairs:
        if _any(want):
            some = True
            assert _any(got), (what, name, "gradient finite where the reference's is not")
    assert some, (what, "the reference's gradients stayed finite: the case checks nothing")


def _block_grad_pairs(ref_blocks, eng_blocks, xr, xe):
    pairs = [("dx", xr.grad, xe.grad)]
    for i, (rb, eb) in enumerate(zip(ref_blocks, eng_blocks)):
        pairs += [(f"block{i}.weight", rb[0].weight.grad, eb[0].weight.grad),
                  (f"block{i}.gamma", rb[1].weight.grad, eb[1].weight.grad),
                  (f"block{i}.beta", rb[1].bias.grad, eb[1].bias.grad)]
    return pairs


@pytest.mark.parametrize("bad", [INF, NAN])
@pytest.mark.parametrize("name", list(EDGE_VARIANTS))
def test_edgeconv_backward_keeps_nonfinite(cuda, monkeypatch, name, bad):
    v = EDGE_VARIANTS[name]
    torch.manual_seed(12)
    x = torch.randn(v.B, v.widths[0], N_PTS)
    gout = torch.randn(v.B, sum(v.widths[1:]), N_PTS)
    gout[0, sum(v.widths[1:]) - 3, 77] = bad     # in the last block's slice: flows through every block
    _, _, ref_blocks, eng_blocks, xr, xe = _run_variant(v, monkeypatch, cuda, x, gout)
    _grads_not_laundered(_block_grad_pairs(ref_blocks, eng_blocks, xr, xe), name)


@pytest.mark.parametrize("bad", [INF, NAN])
@pytest.mark.parametrize("layout", ["channel_major", "point_major"])
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_edge_mlp_backward_keeps_nonfinite(cuda, mode, layout, bad):
    """The stage's backward picks its dz kernel by the incoming gradient's
    layout (dgx/edgemlp.py _backward): (B, C2, N)-contiguous, what a module
    downstream hands back, -> dgx_edge_bwd_dz_cm_f32; point-major ->
    dgx_edge_bwd_dz_f32. Both are driven, and the layout that selects is asserted."""
    from dgx import edgemlp
    torch.manual_seed(31)
    x = torch.from_numpy(synth.cube_clouds(2, N_PTS, 3)).permute(0, 2, 1).contiguous()
    gout = torch.randn(2, 128, N_PTS) if layout == "channel_major" else torch.randn(2, N_PTS, 128).permute(0, 2, 1)
    assert gout.permute(0, 2, 1).is_contiguous() == (layout == "point_major")   # the route's condition
    assert gout.to(cuda).stride() == gout.stride()
    gout[0, 17, 5] = bad
    assert edgemlp._fused_bwd_ok(mode == "bf16", 64, 128, K_NB) == (mode == "bf16")   # the backward that runs
    _, _, rs, es, xr, xe = _run_edge_mlp(mode, cuda, x, gout)
    _grads_not_laundered(_block_grad_pairs(rs, es, xr, xe), (mode, layout))


def _scatter_out_nonfinite(out, S, row, ch):
    """dQ of the poisoned (row, channel) and dP of that channel in the row's cloud."""
    Co, N = S["Co"], S["N"]
    out = out.float()
    b = row // N
    assert not bool(torch.isfinite(out[row, Co + ch])), "dQ laundered"
    assert bool((~torch.isfinite(out[b * N:(b + 1) * N, ch])).any()), "dP laundered"


@pytest.mark.parametrize("packed", [False, True])
def test_scatter_entries_keep_nonfinite_dz(cuda, packed):
    """Every backward-scatter entry of the C ABI on a dz with one inf (slot bits
    kept in a packed word): c0 / c1 given (fp32, bf16, split planes 2 / 3) and
    finalized in the prologue (fp32, bf16)."""
    import test_scatter_gpu as SP
    from dgx import _native as nat
    S = SP._setup(cuda, 2, 300, 11, 20, seed=9, packed=packed)
    L, st, M, Co = S["L"], S["st"], S["M"], S["Co"]
    row, ch = 301, 7
    w = S["dz"].view(torch.int32)
    w[row, ch] = 0x7F800000 | (int(w[row, ch]) & 63 if packed else 0)
    reached = []
    _scatter_out_nonfinite(SP._pull(S, packed), S, row, ch)
    reached.append("pull_f32")
    for mode in (1, 2, 3):
        planes = torch.zeros(3, M, 2 * Co, device=cuda, dtype=torch.bfloat16)
        common = (S["B"], S["N"], S["k"], Co, nat.f32(st.scale), nat.f32(S["c0"]), nat.f32(S["c1"]),
                  nat.ptr(planes, nat.BF16), mode, S["stream"])
        if packed:
            nat.check(L.dgx_edge_bwd_scatter_packed_f32(nat.f32(S["PQ"]), 2 * Co, nat.i32(S["rowptr"]),
                                                        nat.i32(S["edges"]), nat.f32(S["dz"]), nat.f32(S["sumP"]),
                                                        *common), "scatter")
        else:
            nat.check(L.dgx_edge_bwd_scatter_f32(nat.f32(S["PQ"]), 2 * Co, nat.i32(S["rowptr"]), nat.i32(S["edges"]),
                                                 nat.f32(S["dz"]), nat.u8(S["arg"]), nat.f32(S["sumP"]), *common),
                      "scatter")
        _scatter_out_nonfinite(planes[0], S, row, ch)          # the hi plane (mode 1: the bf16 output)
        reached.append(f"pull_mode{mode}")
    for mode in (0, 1):
        out = torch.zeros(M, 2 * Co, device=cuda, dtype=torch.bfloat16 if mode else torch.float32)
        o = [torch.empty(Co, device=cuda) for _ in range(4)]
        nat.check(L.dgx_edge_bwd_scatter_fin_f32(
            nat.f32(S["PQ"]), 2 * Co, nat.i32(S["rowptr"]), nat.i32(S["edges"]), nat.f32(S["dz"]),
            None if packed else nat.u8(S["arg"]), nat.f32(S["sumP"]), S["B"], S["N"], S["k"], Co,
            nat.f32(S["partials"]), S["nblk"], float(M * S["k"]), nat.f32(st.scale), nat.f32(st.mean),
            nat.f32(st.invstd), 0, *(nat.f32(t) for t in o), nat.ptr(out, nat.F32, nat.BF16), mode, int(packed),
            S["stream"]), "scatter fin")
        _scatter_out_nonfinite(out, S, row, ch)
        reached.append(f"fin_mode{mode}")
    torch.cuda.synchronize()
    assert reached == ["pull_f32", "pull_mode1", "pull_mode2", "pull_mode3", "fin_mode0", "fin_mode1"]


@pytest.mark.parametrize("bad", [INF, NAN])
def test_dz_kernels_keep_nonfinite_gradient(cuda, bad):
    """dgx_edge_bwd_dz_f32 / _packed_f32 / _cm_f32 (channel-major dY): a non-
    finite dY element gives a non-finite dz (also after the packed word's slot
    bits are masked off) and non-finite BN partial sums of its channel; the
    other channels stay finite."""
    from dgx import _native as nat
    B, N, Co, k = 2, 150, 24, 11
    M = B * N
    L = nat.lib()
    g = torch.Generator(device="cpu").manual_seed(6)
    ysel = torch.randn(M, Co, generator=g).to(cuda)
    arg = torch.randint(0, k, (M, Co), generator=g, dtype=torch.uint8).to(cuda)
    dY = torch.randn(M, Co, generator=g)
    dY[200, 9] = bad
    dY = dY.to(cuda)
    sc, sh, mu = (torch.randn(Co, generator=g).to(cuda) for _ in range(3))
    ist = (torch.rand(Co, generator=g) + 0.5).to(cuda)
    for packed in (False, True, "cm"):
        dz = torch.empty(M, Co, device=cuda)
        nrows = L.dgx_edge_bwd_dz_cm_rows(B, N) if packed == "cm" else 16
        part = torch.empty(nrows, 2, Co, device=cuda)
        a = (M, Co, nat.f32(sc), nat.f32(sh), nat.f32(mu), nat.f32(ist), 0.2, nat.f32(dz), nat.f32(part), nrows,
             nat.stream_of(dz))
        if packed == "cm":
            dcm = dY.view(B, N, Co).permute(0, 2, 1).contiguous()             # (B, Co, N)
            nat.check(L.dgx_edge_bwd_dz_cm_f32(nat.f32(dcm), nat.f32(ysel), B, N, *a[1:]), "dz cm")
        elif packed:
            nat.check(L.dgx_edge_bwd_dz_packed_f32(nat.f32(dY), Co, nat.f32(ysel), nat.u8(arg), *a), "dz packed")
            dz = (dz.view(torch.int32) & ~63).view(torch.float32)
        else:
            nat.check(L.dgx_edge_bwd_dz_f32(nat.f32(dY), Co, nat.f32(ysel), *a), "dz")
        torch.cuda.synchronize()
        assert not bool(torch.isfinite(dz[200, 9])), packed
        bad_ch = ~torch.isfinite(part).all(0)                      # (2, Co)
        assert bool(bad_ch[:, 9].all()), packed
        keep = torch.ones(Co, dtype=torch.bool)
        keep[9] = False
        assert bool(torch.isfinite(part[:, :, keep]).all()) and bool(torch.isfinite(dz[:, keep]).all())


@pytest.mark.parametrize("bad", [INF, NAN])
@pytest.mark.parametrize("k,form", [(10, "csr"), (65, "atomic")])
def test_graph_feature_backward_keeps_nonfinite(cuda, k, form, bad):
    """get_graph_feature's backward: the reverse-graph pull (k <= 64) and the
    atomic form (k > 64, which also takes the generic kNN)."""
    from models.dgcnn import get_graph_feature
    from oracle import reference as R
    assert (k <= 64) == (form == "csr")
    torch.manual_seed(k)
    x = torch.randn(2, 8, N_PTS)
    xr, xe = x.clone().requires_grad_(True), x.clone().to(cuda).requires_grad_(True)
    gout = torch.randn(2, 16, N_PTS, k)
    gout[0, 3, 50, k - 1] = bad
    gout[1, 11, 9, 0] = bad
    R.graph_feature(xr, k).backward(gout)
    get_graph_feature(xe, k=k).backward(gout.to(cuda))
    _no_laundering(_rows(xr.grad), _rows(xe.grad), form)
    assert bool(_rows(xr.grad).any())


@pytest.mark.parametrize("bad", [INF, NAN])
@pytest.mark.parametrize("mode", ["fp32", "bf16", "fp32_split"])
def test_pointconv_backward_keeps_nonfinite(cuda, mode, bad):
    """conv5 (models/dgcnn.py:74-78, 101): Conv1x1 -> BatchNorm -> LeakyReLU on the point-major rows."""
    import copy
    from dgx import precision as prec
    from dgx.pointconv import pointconv_bn_lrelu
    torch.manual_seed(21)
    B, N, K, Co = 2, N_PTS, 68, 96
    seq = torch.nn.Sequential(torch.nn.Conv2d(K, Co, 1, bias=False), torch.nn.BatchNorm2d(Co), torch.nn.LeakyReLU(0.2))
    with torch.no_grad():
        seq[1].weight.copy_(torch.randn(Co))
    eng = copy.deepcopy(seq).to(cuda)
    X = torch.randn(B * N, K)
    Xr, Xe = X.clone().requires_grad_(True), X.clone().to(cuda).requires_grad_(True)
    gout = torch.randn(B, Co, N)
    gout[1, 40, 3] = bad
    seq(Xr.view(B, N, K).permute(0, 2, 1).unsqueeze(-1)).squeeze(-1).backward(gout)
    with prec.mode(mode):
        pointconv_bn_lrelu(Xe, B, N, eng).backward(gout.to(cuda))
    _grads_not_laundered(_block_grad_pairs([seq], [eng], Xr, Xe), mode)


@pytest.mark.parametrize("bad", [INF, NAN])
@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16, torch.float32])
def test_attention_backward_keeps_nonfinite(cuda, dt, bad):
    """dgx.attention.attention against scaled_dot_product_attention, the op
    nn.MultiheadAttention runs, at (B, H, Nq, Nk, D) = (1, 2, 77, 130, 64)."""
    from dgx.attention import attention
    B, H, Nq, Nk, D = 1, 2, 77, 130, 64
    g = torch.Generator().manual_seed(5)
    q, k, v = (torch.randn(B, n, H * D, generator=g).to(dt) for n in (Nq, Nk, Nk))
    go = torch.randn(B, Nq, H * D, generator=g).to(dt)
    go[0, 31, 70] = bad
    ref_in = [t.detach().clone().float().requires_grad_(True) for t in (q, k, v)]
    heads = [t.view(B, -1, H, D).transpose(1, 2) for t in ref_in]
    ref = torch.nn.functional.scaled_dot_product_attention(*heads).transpose(1, 2).reshape(B, Nq, H * D)
    ref.backward(go.float())
    eng_in = [t.detach().clone().to(cuda).requires_grad_(True) for t in (q, k, v)]
    attention(*eng_in, H).backward(go.to(cuda))
    _grads_not_laundered([(n, r.grad, e.grad) for n, r, e in zip(("dq", "dk", "dv"), ref_in, eng_in)], str(dt))
    for n, r, e in zip(("dq", "dk", "dv"), ref_in, eng_in):
        _no_laundering(_rows(r.grad), _rows(e.grad), n)


# ------------------------------------------------ (d) the step is skipped ----
def _dgcnn_case(cuda):
    from models.dgcnn import DGCNN
    torch.manual_seed(0)
    model = DGCNN(types.SimpleNamespace(emb_dim=64, k=10)).to(cuda).train()
    x = torch.from_numpy(synth.cube_clouds(2, 128, 7)).to(cuda).permute(0, 2, 1)

    def run(xin):
        out = model(xin)
        return out, out.float().pow(2).mean()
    return model, x, run


def _net_case(cuda):
    """Net at the size of test_amp_bn_gpu.test_net_autocast_grad_scaler."""
    from models.model_partseg import Net
    torch.manual_seed(3)
    args = types.SimpleNamespace(k=20, emb_dim=64, n_heads=4, n_blocks=1, ff_dims=128, dropout=0.0, nclasses=50)
    model = Net(args).to(cuda).train()
    x = torch.from_numpy(synth.cube_clouds(2, 256, 12)).to(cuda).permute(0, 2, 1).contiguous()
    lbl = torch.nn.functional.one_hot(torch.tensor([3, 7]), 16).float().to(cuda)
    target = torch.randint(0, 50, (2, 256), generator=torch.Generator().manual_seed(1)).to(cuda)

    def run(xin):
        out = model(xin, lbl)
        return out, torch.nn.functional.cross_entropy(out.float(), target)
    return model, x, run


MODEL_CASES = {"dgcnn": _dgcnn_case, "net": _net_case}


def _bits(t):
    return t.detach().clone()


def _opt_state(model, opt):
    """Every parameter and every optimizer state tensor (momentum / exp_avg /
    exp_avg_sq buffers, device step counts), cloned."""
    snap = [_bits(p) for p in model.parameters()]
    for p in model.parameters():
        for key, val in sorted(opt.state.get(p, {}).items()):
            if isinstance(val, torch.Tensor):
                snap.append(_bits(val))
    return snap


def _same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and torch.equal(x, y) and
                                    torch.equal(torch.isnan(x), torch.isnan(y)) for x, y in zip(a, b))


def _scaled_steps(model, x, run, opt, scaler, poison_at):
    """Three fp16-autocast steps; in step ``poison_at`` a hook multiplies one
    element of the model output's gradient by inf. Returns per step
    (state unchanged, scale before, scale after)."""
    rec = []
    for s in range(3):
        opt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.float16):
            out, loss = run(x)
        if s == poison_at:
            def hook(g):
                g = g.contiguous().clone()
                g.view(-1)[7] *= INF
                return g
            out.register_hook(hook)
        before, scale_before = _opt_state(model, opt), scaler.get_scale()
        scaler.scale(loss).backward()
        scaler.step(opt)
        scaler.update()
        after = _opt_state(model, opt)
        # state tensors created by a step count as changed unless they are all zero
        unchanged = _same(before, after[:len(before)]) and not any(bool(t.any()) for t in after[len(before):]) \
            and len(before) == len(after)
        rec.append((unchanged, scale_before, scaler.get_scale()))
    return rec


@pytest.mark.parametrize("which", ["SGD", "Adam", "AdamW"])
@pytest.mark.parametrize("case", list(MODEL_CASES))
def test_nonfinite_gradient_skips_the_step(cuda, case, which):
    """A clean step, a step whose output gradient holds an inf, a clean step:
    the middle one leaves every parameter, optimizer buffer and device step
    count bitwise unchanged and multiplies the scale by backoff_factor; the
    others update. torch.optim.SGD under torch.amp.GradScaler on the same
    engine model skips the same steps."""
    import dgx.optim as O
    skipped = {}
    for flavour in ("dgx", "torch"):
        model, x, run = MODEL_CASES[case](cuda)
        if flavour == "dgx":
            kw = dict(lr=0.01, momentum=0.9) if which == "SGD" else dict(lr=1e-3)
            opt, scaler = getattr(O, which)(model.parameters(), **kw), O.GradScaler("cuda", init_scale=1024.0)
        else:
            opt = torch.optim.SGD(model.parameters(), lr=0.01, momentum=0.9)
            scaler = torch.amp.GradScaler("cuda", init_scale=1024.0)
        rec = _scaled_steps(model, x, run, opt, scaler, poison_at=1)
        skipped[flavour] = [r[0] for r in rec]
        if flavour == "dgx":
            assert skipped["dgx"] == [False, True, False], skipped
            assert rec[0][2] == rec[0][1] and rec[2][2] == rec[2][1]
            assert rec[1][2] == rec[1][1] * scaler.get_backoff_factor()
    assert skipped["torch"] == skipped["dgx"], skipped


# ------------------------------------------------ (e) NaN input end to end ----
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("case", list(MODEL_CASES))
def test_nan_point_end_to_end(cuda, case, mode):
    """One NaN point in cloud 0: the model runs to completion in eval and train
    mode with a non-finite loss; a clean eval forward afterwards is bitwise what
    it was before (no scratch or cache keeps the NaN). The train pass poisons
    the BatchNorm running statistics, as the reference's does; with the buffers
    restored the clean forward is again unchanged."""
    from dgx import precision as prec
    model, x, run = MODEL_CASES[case](cuda)
    bad = x.clone()
    bad[0, :, 5] = NAN
    with prec.mode(mode):
        model.eval()
        with torch.no_grad():
            y0 = run(x)[0].clone()
            assert bool(torch.isfinite(y0).all())
            out, loss = run(bad)
            assert not bool(torch.isfinite(loss)) and not bool(torch.isfinite(out[0]).all())
            assert torch.equal(run(x)[0], y0)
        state = {n: t.detach().clone() for n, t in model.state_dict().items()}
        model.train()
        out, loss = run(bad)
        loss.backward()
        torch.cuda.synchronize()
        assert not bool(torch.isfinite(loss))
        poisoned = [n for n, t in model.state_dict().items() if t.is_floating_point() and not torch.isfinite(t).all()]
        assert poisoned and all("running_" in n for n in poisoned), poisoned
        model.load_state_dict(state)
        model.eval()
        with torch.no_grad():
            assert torch.equal(run(x)[0], y0)
