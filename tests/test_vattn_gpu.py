"""The fused kNN vector attention (csrc/vattn.hip, dgx.vattn) on the device
against the fp64 restatement tests/_vattn_ref.py (pinned to the reference by
tests/test_vattn_cpu.py), at every tile edge of the kernel, in both operand
modes, with the recompute backward, and through the modules.

Bars (rel_err = max|a - b| / max|b|):
  fp32 mode forward           <= 1e-5 of fp64
  bf16 mode forward           err(kernel, fp64) <= 2 x err(bf16-rounded restatement, fp64), same inputs
  gradients (both modes)      inputs 1e-5, parameters 2e-4 of fp64 autograd of the restatement
  bf16-mode gradients         bit-equal to fp32-mode gradients
"""
import types

import numpy as np
import pytest
import torch

import _vattn_ref as VR
from conftest import load_golden, rel_err

pytestmark = pytest.mark.gpu
DM, H, HP = 64, 256, 64


def _ppb():
    from dgx import vattn
    return vattn.fwd_points()


def _shapes():
    P = _ppb()
    return [(1, 1, 1), (1, 5, 1), (2, P - 1, 17), (2, P + 1, 16), (3, 2 * P, 20), (1, 40, 32), (2, 33, 33), (1, 70, 64)]


def _mlps(dev, seed=0):
    """pos_mlp, attn_mlp at the reference's default init (attention.py:93-105)."""
    torch.manual_seed(seed)
    pos = torch.nn.Sequential(torch.nn.Linear(3, HP), torch.nn.ReLU(), torch.nn.Linear(HP, DM))
    att = torch.nn.Sequential(torch.nn.Linear(DM, H), torch.nn.ReLU(), torch.nn.Linear(H, DM))
    return pos.to(dev), att.to(dev)


def _inputs(dev, B, N, k, seed=1):
    g = torch.Generator().manual_seed(seed + 1000 * B + 10 * N + k)
    D = torch.randn(B * N, DM, generator=g)
    V = torch.randn(B * N, DM, generator=g)
    pos = torch.rand(B * N, 3, generator=g) * 2 - 1
    idx = torch.randint(0, N, (B, N, k), generator=g, dtype=torch.int32)
    gout = torch.randn(B * N, DM, generator=g)
    return tuple(t.to(dev) for t in (D, V, pos, idx, gout))


def _params(pos_mlp, attn_mlp):
    from dgx import cpu
    return cpu.vattn_params(pos_mlp, attn_mlp)


def _fused(D, V, pos, idx, mlps, gs, mode):
    from dgx import precision as prec, vattn
    with prec.mode(mode):
        return vattn.vector_attention(D, V, pos, idx, mlps[0], mlps[1], gs)


def _np(t):
    return t.detach().cpu().numpy()


# ------------------------------------------------------------------ forward ----
@pytest.mark.parametrize("local", [False, True])
@pytest.mark.parametrize("case", range(8))
def test_forward_fp32_and_bf16(cuda, case, local):
    """Observed on MI355X over the 16 cases: fp32 mode 5.2e-8 .. 1.7e-7; bf16 mode
    equal to the bf16-rounded restatement to three digits in every case (kernel,
    yardstick) = (1.97e-4, 1.97e-4) at (1,1,1) .. (1.52e-3, 1.52e-3) at (2,33,33)."""
    B, N, k = _shapes()[case]
    gs = N if local else 0
    mlps = _mlps(cuda)
    D, V, pos, idx, _ = _inputs(cuda, B, N, k)
    want = VR.vattn(D, V, pos, idx, _params(*mlps), gs)
    e32 = rel_err(_np(_fused(D, V, pos, idx, mlps, gs, "fp32")), _np(want))
    yard = rel_err(_np(VR.vattn(D, V, pos, idx, _params(*mlps), gs, bf16=True)), _np(want))
    e16 = rel_err(_np(_fused(D, V, pos, idx, mlps, gs, "bf16")), _np(want))
    print(f"vattn fwd (B,N,k)=({B},{N},{k}) gs={gs}: fp32 {e32:.2e}  bf16 {e16:.2e}  yardstick {yard:.2e}")
    assert e32 <= 1e-5
    assert e16 <= 2 * yard
    # fp32_split is never narrower than asked: the fp32 kernel
    assert torch.equal(_fused(D, V, pos, idx, mlps, gs, "fp32_split"), _fused(D, V, pos, idx, mlps, gs, "fp32"))


def test_equal_neighbours_give_inverse_sqrt_k(cuda):
    """All k ids of a row equal: a is the same in every slot, so t = 1 / sqrt(k)
    and agg = sqrt(k) a (V_j + r) per channel."""
    B, N, k = 1, 6, 9
    mlps = _mlps(cuda)
    D, V, pos, idx, _ = _inputs(cuda, B, N, k)
    idx = idx[:, :, :1].expand(B, N, k).contiguous()
    got = _fused(D, V, pos, idx, mlps, 0, "fp32")
    want = VR.vattn(D, V, pos, idx, _params(*mlps), 0)
    one = VR.vattn(D, V, pos, idx[:, :, :1].contiguous(), _params(*mlps), 0)   # k = 1: t = 1
    assert rel_err(_np(want), _np(one) * np.sqrt(k)) <= 1e-12
    assert rel_err(_np(got), _np(want)) <= 1e-5


def test_wide_logits_need_the_row_maximum(cuda):
    """Logits spread over about 30 within a row (attn_mlp's last layer scaled
    up): the softmax weights span 13 decades, the small ones are only right
    relative to the row maximum, and a^2 stays a normal fp32 number (fp64 does
    not underflow where fp32 does: no further)."""
    B, N, k = 1, 37, 20
    mlps = _mlps(cuda)
    D, V, pos, idx, _ = _inputs(cuda, B, N, k)
    with torch.no_grad():
        s = mlps[1](D[:N])   # logits of about the attention's own scale (u = D_j + r, |r| << |D|)
        spread = float((s.max(dim=-1)[0] - s.min(dim=-1)[0]).max())
        mlps[1][2].weight.mul_(30.0 / spread)
        mlps[1][2].bias.mul_(30.0 / spread)
    got = _fused(D, V, pos, idx, mlps, 0, "fp32")
    want = VR.vattn(D, V, pos, idx, _params(*mlps), 0)
    assert torch.isfinite(got).all()
    assert rel_err(_np(got), _np(want)) <= 1e-5


# ---------------------------------------------------------------- gradients ----
def _grads(fn, D, V, mlps, gout):
    Dl, Vl = D.clone().requires_grad_(True), V.clone().requires_grad_(True)
    for m in mlps:
        m.zero_grad(set_to_none=True)
    out = fn(Dl, Vl)
    out.backward(gout.to(out.dtype))
    return [Dl.grad, Vl.grad] + [p.grad.clone() for p in _params(*mlps)]


def _ref_grads(D, V, pos, idx, mlps, gs, gout):
    leaves = [t.detach().double().requires_grad_(True) for t in [D, V] + _params(*mlps)]
    out = VR.vattn(leaves[0], leaves[1], pos, idx, leaves[2:], gs)
    return torch.autograd.grad(out, leaves, gout.double())


@pytest.mark.parametrize("local", [False, True])
@pytest.mark.parametrize("case", [1, 2, 4, 6, 7])
def test_backward_both_modes(cuda, case, local):
    B, N, k = _shapes()[case]
    gs = N if local else 0
    mlps = _mlps(cuda)
    D, V, pos, idx, gout = _inputs(cuda, B, N, k)
    want = _ref_grads(D, V, pos, idx, mlps, gs, gout)
    g32 = _grads(lambda d, v: _fused(d, v, pos, idx, mlps, gs, "fp32"), D, V, mlps, gout)
    g16 = _grads(lambda d, v: _fused(d, v, pos, idx, mlps, gs, "bf16"), D, V, mlps, gout)
    # with k = 1, t = a / |a| = 1: agg = V_j + r whatever the logits, so dD and attn_mlp's gradients are
    # exactly 0 in real arithmetic and both sides hold rounding noise, which has no relative error;
    # it must vanish at the same bar relative to the largest gradient of its kind (inputs / parameters)
    scales = [max(float(w.abs().max()) for w in want[:2])] * 2 + [max(float(w.abs().max()) for w in want[2:])] * 8
    for j, (a, b, w, sc) in enumerate(zip(g32, g16, want, scales)):
        tol = 1e-5 if j < 2 else 2e-4
        if float(w.abs().max()) <= 1e-9 * sc:
            assert k == 1 and j in (0, 6, 7, 8, 9), j
            assert float(a.abs().max()) <= tol * sc, j
        else:
            e = rel_err(_np(a), _np(w))
            print(f"vattn bwd (B,N,k)=({B},{N},{k}) gs={gs} grad {j}: {e:.2e}")
            assert e <= tol, j
        assert torch.equal(a, b), j   # the backward is the same in both modes


def test_backward_chunking(cuda, monkeypatch):
    """One point per backward chunk against a single chunk."""
    from dgx import vattn
    B, N, k = 2, 19, 7
    mlps = _mlps(cuda)
    D, V, pos, idx, gout = _inputs(cuda, B, N, k)
    run = lambda: _grads(lambda d, v: _fused(d, v, pos, idx, mlps, N, "fp32"), D, V, mlps, gout)   # noqa: E731
    whole = run()
    monkeypatch.setattr(vattn, "BWD_CHUNK_MB", 0)
    assert vattn._chunk_points(k, DM, H, HP) == 1
    for a, b in zip(run(), whole):
        assert rel_err(_np(a), _np(b)) <= 1e-5


def test_two_runs_bit_equal(cuda):
    B, N, k = 3, 45, 20
    mlps = _mlps(cuda)
    D, V, pos, idx, gout = _inputs(cuda, B, N, k)
    for mode in ("fp32", "bf16"):
        a = _grads(lambda d, v: _fused(d, v, pos, idx, mlps, 0, mode), D, V, mlps, gout)
        b = _grads(lambda d, v: _fused(d, v, pos, idx, mlps, 0, mode), D, V, mlps, gout)
        assert torch.equal(_fused(D, V, pos, idx, mlps, 0, mode), _fused(D, V, pos, idx, mlps, 0, mode))
        assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_graph_capture_replays_bit_equal(cuda):
    """Forward + backward captured in a HIP graph against the eager run."""
    from dgx import precision as prec, vattn
    B, N, k = 2, 40, 12
    mlps = _mlps(cuda)
    D, V, pos, idx, gout = _inputs(cuda, B, N, k)
    params = _params(*mlps)

    def step(Dl, Vl):
        out = vattn.vector_attention(Dl, Vl, pos, idx, mlps[0], mlps[1], N)
        return (out,) + torch.autograd.grad(out, [Dl, Vl] + params, gout)

    # The leaves first meet autograd in the side-stream warm-up (as in every capture test of
    # this suite): a leaf first used on the default stream binds its gradient accumulator to the
    # legacy stream, which the engine would then touch during the capture.
    Ds, Vs = D.clone().requires_grad_(True), V.clone().requires_grad_(True)
    with prec.mode("fp32"):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            step(Ds, Vs)   # eager warm-up
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = step(Ds, Vs)
        graph.replay()
        torch.cuda.synchronize()
        eager = step(D.clone().requires_grad_(True), V.clone().requires_grad_(True))
    for a, b in zip(captured, eager):
        assert torch.equal(a, b)


def test_nan_reaches_exactly_its_neighbourhoods(cuda):
    B, N, k = 2, 50, 20
    mlps = _mlps(cuda)
    D, V, pos, idx, _ = _inputs(cuda, B, N, k)
    bad = N + 7                                   # a row of cloud 1
    D = D.clone()
    D[bad, 3] = float("nan")
    for mode in ("fp32", "bf16"):
        out = _fused(D, V, pos, idx, mlps, N, mode)
        hit = (idx.long() + torch.arange(B, device=cuda).view(B, 1, 1) * N == bad).any(dim=-1).view(-1)
        assert hit.any() and not hit.all()
        assert torch.isnan(out[hit]).all() and torch.isfinite(out[~hit]).all()


def test_non_fused_shape_takes_the_composed_path(cuda):
    """d_qkv 32: no fused kernel; the composed device path, against fp64."""
    from dgx import vattn
    torch.manual_seed(5)
    pos_mlp = torch.nn.Sequential(torch.nn.Linear(3, 64), torch.nn.ReLU(), torch.nn.Linear(64, 32)).to(cuda)
    att = torch.nn.Sequential(torch.nn.Linear(32, 128), torch.nn.ReLU(), torch.nn.Linear(128, 32)).to(cuda)
    assert not vattn.fused_shape(32, 128, 64, 8)
    B, N, k = 2, 30, 8
    D, V = torch.randn(B * N, 32, device=cuda), torch.randn(B * N, 32, device=cuda)
    pos = torch.rand(B * N, 3, device=cuda)
    idx = torch.randint(0, N, (B, N, k), device=cuda)
    got = vattn.vector_attention(D, V, pos, idx, pos_mlp, att, 0)
    want = VR.vattn(D, V, pos, idx, _params(pos_mlp, att), 0)
    assert rel_err(_np(got), _np(want)) <= 1e-5


def test_ids_are_range_checked(cuda):
    from dgx import vattn
    mlps = _mlps(cuda)
    D, V, pos, idx, _ = _inputs(cuda, 1, 10, 4)
    idx = idx.clone()
    idx[0, 3, 1] = 10
    with pytest.raises(IndexError):
        vattn.vector_attention(D, V, pos, idx, mlps[0], mlps[1], 0)


# ------------------------------------------------------------------ modules ----
def _args(**kw):
    return types.SimpleNamespace(**kw)


def _golden_module(cuda):
    from models.attention import VectorAttention
    z = load_golden("vattn_small.npz")
    m = VectorAttention(_args(emb_dim=32, d_qkv=64, k=10)).train()
    m.load_state_dict({k: torch.from_numpy(z["w_" + k].copy()) for k in m.state_dict()})
    ins = [torch.from_numpy(z["in_" + n].copy()).to(cuda) for n in ("query", "key", "value", "canonical")]
    return z, m.to(cuda), ins


def test_vector_attention_module_matches_reference(cuda):
    from dgx import precision as prec
    z, m, ins = _golden_module(cuda)
    leaves = [t.clone().requires_grad_(True) for t in ins[:3]]
    with prec.mode("fp32"):
        y = m(*leaves, ins[3])
        y.backward(torch.from_numpy(z["g"].copy()).to(cuda))
    assert rel_err(_np(y), z["out"]) <= 1e-4
    for name, p in m.named_parameters():
        assert rel_err(_np(p.grad), z["grad_" + name]) <= 2e-4, name
    for n, t in zip(("query", "key", "value"), leaves):
        assert rel_err(_np(t.grad), z["gin_" + n]) <= 2e-4, n


def test_vector_attention_compiles_fullgraph(cuda):
    from dgx import precision as prec
    _, m, ins = _golden_module(cuda)
    with prec.mode("fp32"):
        eager = m(*ins)
        compiled = torch.compile(m, backend="aot_eager", fullgraph=True)(*ins)
    assert torch.equal(compiled, eager)


def test_transformer_against_fp64_and_shares_one_knn(cuda):
    """Transformer (d_qkv 64: every attention fused) forward + backward against
    a float64 copy of itself whose attentions run the fp64 restatement; the 6
    attention calls of a forward search the cloud once."""
    import copy
    from dgx import ops, precision as prec
    import models.attention as MA
    from models.transformer import Transformer
    torch.manual_seed(7)
    args = _args(emb_dim=32, d_qkv=64, ff_dims=64, n_blocks=1, dropout=0.0, k=10, n_heads=4)
    m = Transformer(args).to(cuda).train()
    ref = copy.deepcopy(m).double()
    B, N = 2, 128
    src, tgt = torch.randn(B, 32, N, device=cuda), torch.randn(B, 32, N, device=cuda)
    pts = torch.rand(B, 3, N, device=cuda)
    g0, g1 = torch.randn(B, 32, N, device=cuda), torch.randn(B, 32, N, device=cuda)
    launches = []
    ops.set_knn_timing(launches)
    with prec.mode("fp32"):
        y0, y1 = m(src, tgt, pts)
    ops.set_knn_timing(None)
    assert len(launches) == 1
    torch.autograd.backward([y0, y1], [g0, g1])

    idx = MA.knn(pts, k=10)

    def ref_forward(self, query, key, value, canonical, mask=None):
        return VR.module(self.state_dict(keep_vars=True), query, key, value, canonical, idx)

    for mod in ref.modules():
        if isinstance(mod, MA.VectorAttention):
            mod.forward = types.MethodType(ref_forward, mod)
    r0, r1 = ref(src.double(), tgt.double(), pts.double())
    torch.autograd.backward([r0, r1], [g0.double(), g1.double()])
    assert rel_err(_np(y0), _np(r0)) <= 1e-4 and rel_err(_np(y1), _np(r1)) <= 1e-4
    scale = max(float(p.grad.abs().max()) for p in ref.parameters())
    for (name, p), q in zip(m.named_parameters(), ref.parameters()):
        if float(q.grad.abs().max()) <= 1e-9 * scale:   # exactly 0 in real arithmetic (a bias before a BatchNorm)
            assert float(p.grad.abs().max()) <= 2e-4 * scale, name
        else:
            assert rel_err(_np(p.grad), _np(q.grad)) <= 2e-4, name
