"""SURVEY §8(b) torch op layer: the engine as torch.ops.dgx custom ops (dgx.library).

* every op's result equals the engine's autograd-Function path bit for bit
  (the op's device kernel runs the same code);
* torch.compile(DGCNN, fullgraph=True) traces the train step with no graph
  break (the ops' fake kernels describe every output) and its forward,
  backward and BatchNorm buffer updates equal the eager engine's bit for bit;
* torch.export captures the eval forward.
The compiled runs use AOTAutograd's eager backend: the point is the graph
capture of the engine's ops, not a code generator for the glue around them.
"""
import copy
import types

import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu


def _model(emb=128, k=20, seed=0):
    from models.dgcnn import DGCNN
    torch.manual_seed(seed)
    return DGCNN(types.SimpleNamespace(emb_dim=emb, k=k))


def _cloud(cuda, B=4, N=512, seed=5):
    from dgx import synth
    return torch.from_numpy(synth.cube_clouds(B, N, seed)).to(cuda).permute(0, 2, 1)


def _step(m, x, gout, call=None):
    """One train step; ``call``: the callable to run (e.g. the compiled module), m its parameters' owner."""
    m.zero_grad(set_to_none=True)
    y = (call if call is not None else m)(x)
    y.backward(gout)
    return (y.detach().clone(), {n: p.grad.clone() for n, p in m.named_parameters()},
            {n: b.clone() for n, b in m.named_buffers()})


def _assert_same(a, b):
    assert torch.equal(a[0], b[0])
    for n in a[1]:
        assert torch.equal(a[1][n], b[1][n]), n
    for n in a[2]:
        assert torch.equal(a[2][n], b[2][n]), n


def test_knn_and_graph_feature_ops(cuda):
    import dgx.library  # noqa: F401  (registers torch.ops.dgx)
    from dgx import ops
    x = _cloud(cuda, 2, 300)
    idx = torch.ops.dgx.knn(x, 16)
    assert idx.dtype == torch.int64 and torch.equal(idx, ops.knn(x, 16))
    with torch.autocast("cuda", dtype=torch.float16):   # autocast rule: distances stay fp32
        assert torch.equal(torch.ops.dgx.knn(x, 16), idx)
    for mode in (0, 1, 2):
        xa = x.detach().clone().requires_grad_(True)
        xb = x.detach().clone().requires_grad_(True)
        out, _ = torch.ops.dgx.graph_feature(xa, 16, mode)
        ref = ops.graph_feature(xb, 16, knn_only=mode == 2, disp_only=mode == 1)
        assert torch.equal(out, ref)
        g = torch.randn_like(out)
        out.backward(g)
        ref.backward(g)
        # the edge-tensor backward scatter-adds with atomics: equal up to summation order
        assert rel_err(xa.grad.cpu(), xb.grad.cpu()) < 1e-6


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_dgcnn_op_path_equals_function_path(cuda, monkeypatch, precision):
    """DGCNN through torch.ops.dgx == through the autograd Functions: train
    step (output, every gradient, every BN buffer) and eval forward."""
    from dgx import host, library, precision as prec
    monkeypatch.setattr(host, "ENABLED", False)   # the C++ train op is checked in test_host_ext_gpu
    base = _model()
    x = _cloud(cuda)
    gout = torch.randn((4, 128, 512), device=cuda)
    prec.set(precision)
    try:
        ma, mb = copy.deepcopy(base).to(cuda).train(), copy.deepcopy(base).to(cuda).train()
        a = _step(ma, x, gout)
        monkeypatch.setattr(library, "ENABLED", False)
        b = _step(mb, x, gout)
        _assert_same(a, b)
        ma.eval()
        mb.eval()
        with torch.no_grad():
            eb = mb(x)
        monkeypatch.setattr(library, "ENABLED", True)
        with torch.no_grad():
            ea = ma(x)
        assert torch.equal(ea, eb)
    finally:
        prec.set("fp32")


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_torch_compile_dgcnn_fullgraph(cuda, precision):
    """torch.compile(DGCNN, fullgraph=True): no graph break at the engine, and
    two compiled train steps equal two eager ones bit for bit (outputs,
    gradients, running statistics, batch counters)."""
    from dgx import precision as prec
    base = _model(seed=3)
    x = _cloud(cuda, seed=9)
    gout = torch.randn((4, 128, 512), device=cuda)
    prec.set(precision)
    try:
        me = copy.deepcopy(base).to(cuda).train()
        mc = copy.deepcopy(base).to(cuda).train()
        compiled = torch.compile(mc, backend="aot_eager", fullgraph=True)
        for _ in range(2):
            e = _step(me, x, gout)
            c = _step(mc, x, gout, call=compiled)
            _assert_same(e, c)
        assert int(mc.conv1[1].num_batches_tracked) == 2
    finally:
        prec.set("fp32")
        torch._dynamo.reset()


def test_torch_compile_dgcnn_follows_fp16_autocast(cuda):
    """Under fp16 autocast (main_partseg_dist.py:253) the compiled DGCNN takes
    the decision eager takes (precision.effective: split-bf16 fp32 GEMMs), as
    an explicit ``opts`` argument of its ops: the compiled train step equals
    the eager one bit for bit and differs from the plain fp32 mode's."""
    base = _model(256, 20, seed=4)
    x = _cloud(cuda, 4, 1024, seed=9)
    gout = torch.randn((4, 256, 1024), device=cuda)
    me, mc, mf = (copy.deepcopy(base).to(cuda).train() for _ in range(3))
    try:
        compiled = torch.compile(mc, backend="aot_eager", fullgraph=True)
        with torch.autocast("cuda", dtype=torch.float16):
            e = _step(me, x, gout)
            c = _step(mc, x, gout, call=compiled)
        _assert_same(e, c)
        assert not torch.equal(c[0], _step(mf, x, gout)[0])
    finally:
        torch._dynamo.reset()


def test_op_path_decision_taken_at_forward(cuda, monkeypatch):
    """The torch.ops.dgx path decides precision / options once, at forward
    entry, and its backward ops get that decision back: a forward inside
    precision "fp32_split" whose backward runs after the mode is "fp32" again
    equals the autograd-Function path run the same way, bit for bit."""
    from dgx import host, library, precision as prec
    monkeypatch.setattr(host, "ENABLED", False)   # m(x) below: the Function path
    base = _model(256, 20, seed=4)
    x = _cloud(cuda, 4, 1024, seed=9)
    gout = torch.randn((4, 256, 1024), device=cuda)

    def step(forward):
        m = copy.deepcopy(base).to(cuda).train()
        with prec.mode("fp32_split"):
            y = forward(m)
        assert prec.get() == "fp32"
        y.backward(gout)
        return (y.detach().clone(), {n: p.grad.clone() for n, p in m.named_parameters()},
                {n: b.clone() for n, b in m.named_buffers()})
    _assert_same(step(lambda m: library.dgcnn_forward(m, x)), step(lambda m: m(x)))


def test_torch_export_dgcnn_eval(cuda):
    """torch.export of the eval forward: one graph over the dgx ops, equal to eager."""
    import dgx.library  # noqa: F401
    m = _model(seed=4).to(cuda).eval()
    x = _cloud(cuda, seed=2)
    ep = torch.export.export(m, (x.contiguous(),))
    targets = {str(n.target) for n in ep.graph.nodes if n.op == "call_function"}
    assert any("dgx.edgeconv_chain" in t for t in targets) and any("dgx.pointconv" in t for t in targets), targets
    with torch.no_grad():
        assert rel_err(ep.module()(x.contiguous()).cpu(), m(x.contiguous()).cpu()) == 0.0


def test_bn_cumulative_average_op_path(cuda, monkeypatch):
    """BatchNorm with momentum=None (nn.BatchNorm's cumulative moving average):
    the op layer's finalize reads num_batches_tracked on the device (no host
    read, so the step stays capturable) and three train steps leave the same
    running statistics and counters as the autograd-Function path, which
    updates the module buffers in place like nn.BatchNorm."""
    from dgx import library
    base = _model(seed=6)
    for m in base.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.momentum = None
    x = _cloud(cuda, seed=11)
    gout = torch.randn((4, 128, 512), device=cuda)
    ma, mb = copy.deepcopy(base).to(cuda).train(), copy.deepcopy(base).to(cuda).train()
    for _ in range(3):
        monkeypatch.setattr(library, "ENABLED", True)
        a = _step(ma, x, gout)
        monkeypatch.setattr(library, "ENABLED", False)
        b = _step(mb, x, gout)
        _assert_same(a, b)
    assert int(ma.conv1[1].num_batches_tracked) == 3


def _net_step(m, x, lbl, gout, call=None):
    m.zero_grad(set_to_none=True)
    y = (call if call is not None else m)(x, lbl)
    y.backward(gout)
    return (y.detach().clone(), {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None},
            {n: b.clone() for n, b in m.named_buffers()})


@pytest.mark.parametrize("backend", ["eager", "aot_eager"])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_torch_compile_net_fullgraph(cuda, precision, backend):
    """torch.compile(Net, fullgraph=True) — the partseg model main_partseg_dist.py
    trains (reference models/model_partseg.py:142-194): the engine stages are
    dgx::knn / dgx::edgeconv_chain / dgx::pointconv / dgx::edge_mlp2 /
    dgx::hog_1x1 / dgx::attention ops, so the trace has no graph break and
    every one of them is a node of the captured graph. Dynamo's capture run
    as-is ("eager" backend) equals two eager train steps bit for bit (outputs,
    every buffer, every engine-stage gradient; the stock layers' gradients to
    1e-5, see assert_net_grads_same). Through AOTAutograd ("aot_eager") the
    stock layers are decomposed (nn.Transformer's linear / LayerNorm pieces run
    as other ATen kernels, whose fp32 rounding differs from the fused eager
    modules'; measured 1.3e-4 normwise at the output), so that run is held to
    the parity bars instead: 1e-3 (bf16 mode 2e-2) on the output and buffers,
    2e-2 on the fp32 run's gradients.
    Dropout 0 (the seeds would differ)."""
    from conftest import load_golden, rel_err
    from dgx import precision as prec
    from test_host_ext_gpu import assert_net_grads_same
    from test_partseg import _net
    g = load_golden("partseg_small.npz")
    base = _net(g)
    x = torch.from_numpy(g["x"]).to(cuda)
    lbl = torch.from_numpy(g["lbl"]).to(cuda)
    gout = torch.from_numpy(g["gout"]).to(cuda)
    targets = set()

    def capture(gm, example_inputs):
        targets.update(str(n.target) for n in gm.graph.nodes if n.op == "call_function")
        if backend == "eager":
            return gm.forward
        return torch._dynamo.backends.debugging.aot_eager(gm, example_inputs)
    prec.set(precision)
    try:
        me = copy.deepcopy(base).to(cuda).train()
        mc = copy.deepcopy(base).to(cuda).train()
        # a throwaway step: MIOpen picks the stock convs' algorithms on first call
        _net_step(copy.deepcopy(base).to(cuda).train(), x, lbl, gout)
        compiled = torch.compile(mc, backend=capture, fullgraph=True)
        for _ in range(2):
            e = _net_step(me, x, lbl, gout)
            c = _net_step(mc, x, lbl, gout, call=compiled)
            if backend == "eager":
                assert torch.equal(e[0], c[0])
                assert_net_grads_same(e[1], c[1])
                for n in e[2]:
                    assert torch.equal(e[2][n], c[2][n]), n
            else:
                tol, gtol = (1e-3, 2e-2) if precision == "fp32" else (2e-2, None)
                assert rel_err(e[0].cpu(), c[0].cpu()) < tol
                assert e[1].keys() == c[1].keys()
                for n in e[1]:
                    assert torch.isfinite(c[1][n]).all(), n
                    if precision == "bf16":
                        # bf16 mode: the engine rounds dPQ to bf16, and e.g. conv1's weight
                        # gradient is a small residual of cancelling per-point terms, so a
                        # 5e-3 change of the gradient arriving from the stock layers moves
                        # it by ~20 %: only the fp32 run compares gradients
                        continue
                    # a gradient that is rounding noise (|g| ~ 1e-5, e.g. the final
                    # attention's out_proj bias: a sum of cancelling rows) is held
                    # to an absolute floor instead of a relative bar
                    d = (e[1][n] - c[1][n]).abs().max().item()
                    assert d <= max(gtol * e[1][n].abs().max().item(), 1e-4), n
                for n in e[2]:
                    if e[2][n].is_floating_point():
                        assert rel_err(e[2][n].cpu(), c[2][n].cpu()) < tol, n
                    else:
                        assert torch.equal(e[2][n], c[2][n]), n
        for op in ("dgx.knn", "dgx.edgeconv_chain", "dgx.pointconv", "dgx.edge_mlp2", "dgx.hog_1x1",
                   "dgx.attention"):
            assert any(op in t for t in targets), (op, sorted(targets))
    finally:
        prec.set("fp32")
        torch._dynamo.reset()


def test_net_stage_ops_match_function_path(cuda):
    """dgx::edge_mlp2 (forward + its recomputing backward op), dgx::attention
    and dgx::hog_1x1 called directly equal the eager engine paths bit for bit."""
    from dgx import synth
    from dgx.attention import _Attention
    from dgx.edgemlp import edge_mlp2
    from dgx.hog import hog_1x1
    from dgx.library import edge_mlp2_call
    from models.dgcnn import knn
    torch.manual_seed(3)
    mk = lambda: (torch.nn.Sequential(torch.nn.Conv2d(6, 64, 1, bias=False), torch.nn.BatchNorm2d(64),  # noqa: E731
                                      torch.nn.LeakyReLU(0.2)),
                  torch.nn.Sequential(torch.nn.Conv2d(64, 128, 1, bias=False), torch.nn.BatchNorm2d(128),
                                      torch.nn.LeakyReLU(0.2)))
    c1, c2 = mk()
    d1, d2 = copy.deepcopy(c1).to(cuda), copy.deepcopy(c2).to(cuda)
    c1, c2 = c1.to(cuda), c2.to(cuda)
    pts = torch.from_numpy(synth.cube_clouds(2, 512, 8)).to(cuda).permute(0, 2, 1).contiguous()
    xa, xb = pts.clone().requires_grad_(True), pts.clone().requires_grad_(True)
    ya, yb = edge_mlp2(xa, 16, c1, c2), edge_mlp2_call(xb, 16, d1, d2)
    assert torch.equal(ya, yb)
    go = torch.randn_like(ya)
    ya.backward(go)
    yb.backward(go)
    assert torch.equal(xa.grad, xb.grad)
    for pa, pb in zip(list(c1.parameters()) + list(c2.parameters()), list(d1.parameters()) + list(d2.parameters())):
        assert torch.equal(pa.grad, pb.grad)
    for ba, bb in zip(list(c1.buffers()) + list(c2.buffers()), list(d1.buffers()) + list(d2.buffers())):
        assert torch.equal(ba, bb)
    q, k, v = (torch.randn(2, 256, 128, device=cuda, dtype=torch.float16, requires_grad=True) for _ in range(3))
    oa = _Attention.apply(q, k, v, 2, 0.0, 0.125)
    ob, _ = torch.ops.dgx.attention(q, k, v, 2, 0.0, 0.125, 0, None)
    assert torch.equal(oa, ob)
    ga = torch.autograd.grad(oa, (q, k, v), torch.ones_like(oa))
    gb = torch.autograd.grad(ob, (q, k, v), torch.ones_like(ob))
    assert all(torch.equal(a, b) for a, b in zip(ga, gb))
    idx = knn(pts, 20)
    assert torch.equal(torch.ops.dgx.hog_1x1(pts, idx), hog_1x1(pts, idx))
