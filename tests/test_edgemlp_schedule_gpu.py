"""PositionEmbedding's edge MLP (dgx.edgemlp) on the C++ schedule: the precision
decision is taken once at the forward's entry and carried into the backward
(the process-global precision mode is never rewritten), "fp32_split" stays
exact fp32 for this stage, and forward + backward capture into a HIP graph
with either running-statistics update (momentum, cumulative average)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

B, N, K = 2, 256, 20


def _convs(cuda, momentum=0.1):
    g = torch.Generator().manual_seed(7)

    def block(ci, co):
        blk = torch.nn.Sequential(torch.nn.Conv2d(ci, co, 1, bias=False), torch.nn.BatchNorm2d(co, momentum=momentum),
                                  torch.nn.LeakyReLU(0.2))
        with torch.no_grad():
            blk[0].weight.copy_(torch.randn(co, ci, 1, 1, generator=g) / ci ** 0.5)
            gam = 1.0 + 0.3 * torch.randn(co, generator=g)
            gam[::5] *= -1.0
            blk[1].weight.copy_(gam)
            blk[1].bias.copy_(0.2 * torch.randn(co, generator=g))
        return blk.to(cuda).train()
    return block(6, 64), block(64, 128)


def _inputs(cuda):
    from dgx import synth
    x = torch.from_numpy(synth.cube_clouds(B, N, 5)).to(cuda).permute(0, 2, 1)
    gout = torch.from_numpy(synth.uniform(3, (B, 128, N)) - 0.5).float().to(cuda)
    return x, gout


def _step(cuda, x, gout, autocast_fwd=None, autocast_bwd=None):
    """(output, gradients of x and the six parameters) of one forward + backward on fresh modules."""
    from dgx.edgemlp import edge_mlp2
    conv1, conv2 = _convs(cuda)
    x = x.clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=autocast_fwd, enabled=autocast_fwd is not None):
        y = edge_mlp2(x, K, conv1, conv2)
    with torch.autocast("cuda", dtype=autocast_bwd, enabled=autocast_bwd is not None):
        y.backward(gout)
    return [y.detach(), x.grad] + [p.grad for p in list(conv1.parameters()) + list(conv2.parameters())]


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(s, t) for s, t in zip(a, b))


def test_precision_decided_once_at_forward(cuda, monkeypatch):
    from dgx import precision as prec
    x, gout = _inputs(cuda)
    assert prec.get() == "fp32"
    prec.set("bf16")
    try:
        want = _step(cuda, x, gout)
    finally:
        prec.set("fp32")
    fp32 = _step(cuda, x, gout)
    assert not torch.equal(want[0], fp32[0])   # the two precisions are told apart at this shape

    def forbidden(*_a, **_k):
        raise AssertionError("the edge MLP rewrote the process-global precision mode")
    monkeypatch.setattr(prec, "set", forbidden)
    monkeypatch.setattr(prec, "mode", forbidden)
    both = _step(cuda, x, gout, autocast_fwd=torch.bfloat16, autocast_bwd=torch.bfloat16)
    fwd_only = _step(cuda, x, gout, autocast_fwd=torch.bfloat16)
    assert prec.get() == "fp32"
    assert _same(both, want)
    assert _same(fwd_only, want)   # the backward computes in the forward's precision


def test_fp32_split_is_exact_fp32_for_this_stage(cuda):
    from dgx import precision as prec
    x, gout = _inputs(cuda)
    fp32 = _step(cuda, x, gout)
    prec.set("fp32_split")
    try:
        split = _step(cuda, x, gout)
    finally:
        prec.set("fp32")
    assert _same(split, fp32)
    assert _same(_step(cuda, x, gout, autocast_fwd=torch.float16, autocast_bwd=torch.float16), fp32)


@pytest.mark.parametrize("momentum", [0.1, None])
def test_forward_backward_graph_capture(cuda, momentum):
    from dgx.edgemlp import edge_mlp2
    conv1, conv2 = _convs(cuda, momentum)
    x, gout = _inputs(cuda)
    x.requires_grad_(True)
    params = [x] + list(conv1.parameters()) + list(conv2.parameters())

    def step():
        for p in params:
            p.grad = None
        y = edge_mlp2(x, K, conv1, conv2)
        y.backward(gout)
        return y

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()   # eager warm-up
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = step()
    runs = []
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        runs.append([y.detach().clone()] + [p.grad.clone() for p in params])
    assert _same(runs[0], runs[1])
    assert all(torch.isfinite(t).all() for t in runs[0])
    # the batch counters advance on the device: the warm-up, then once per replay (the capture runs nothing)
    assert int(conv1[1].num_batches_tracked) == 3 and int(conv2[1].num_batches_tracked) == 3
