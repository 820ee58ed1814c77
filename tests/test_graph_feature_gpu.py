"""a2 parity: get_graph_feature (HIP gather) vs the reference's goldens."""
import numpy as np
import pytest
import torch

from conftest import rel_err
from oracle import reference as R

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ["xyz", "feat"])
def test_graph_feature_golden(golden, cuda, name):
    from models.dgcnn import get_graph_feature
    g = golden("graph_feature.npz")
    x = torch.from_numpy(g[name + "_x"]).to(cuda)
    np.testing.assert_array_equal(get_graph_feature(x, k=8).cpu().numpy(), g[name + "_cat"])
    np.testing.assert_array_equal(get_graph_feature(x, k=8, disp_only=True).cpu().numpy(), g[name + "_disp"])
    np.testing.assert_array_equal(get_graph_feature(x, k=8, knn_only=True).cpu().numpy(), g[name + "_knn"])


@pytest.mark.parametrize("mode", ["cat", "disp", "knn"])
def test_graph_feature_backward(cuda, mode):
    from models.dgcnn import get_graph_feature, knn
    torch.manual_seed(0)
    x = torch.randn(2, 5, 70)
    kw = {"knn_only": mode == "knn", "disp_only": mode == "disp"}
    xg = x.to(cuda).requires_grad_(True)
    out = get_graph_feature(xg, k=6, **kw)
    gout = torch.randn(out.shape)
    out.backward(gout.to(cuda))
    idx = knn(x.to(cuda), 6).cpu()
    xc = x.clone().requires_grad_(True)
    ref = R.graph_feature(xc, 6, idx=idx, **kw)
    ref.backward(gout)
    np.testing.assert_array_equal(out.detach().cpu().numpy(), ref.detach().numpy())
    assert rel_err(xg.grad.cpu(), xc.grad) < 1e-6


@pytest.mark.parametrize("mode", ["cat", "disp", "knn", "diff"])
def test_graph_feature_backward_deterministic(cuda, mode):
    """The backward pulls over the reverse kNN graph (dgx_graph_feature_bwd_csr_f32):
    bitwise repeatable, equal to the atomic scatter form up to summation order,
    at a hub-heavy graph (neighbours drawn mostly from 4 points)."""
    from dgx import _native as nat
    from dgx import ops
    torch.manual_seed(1)
    B, C, N, k = 3, 7, 300, 12
    x = torch.randn(B, C, N, device=cuda)
    idx = torch.where(torch.rand(B, N, k, device=cuda) < 0.6, torch.randint(0, 4, (B, N, k), device=cuda),
                      torch.randint(0, N, (B, N, k), device=cuda)).to(torch.int32)
    kw = {"knn_only": mode == "knn", "disp_only": mode == "disp", "mode": "diff" if mode == "diff" else "cat"}
    grads = []
    for _ in range(2):
        xg = x.clone().requires_grad_(True)
        out = ops.graph_feature(xg, k=k, idx=idx, **kw)
        out.backward(torch.ones_like(out) * torch.linspace(-1, 1, out.numel(), device=cuda).view(out.shape))
        grads.append(xg.grad)
    assert torch.equal(grads[0], grads[1])
    gm = {"cat": nat.GF_CAT, "disp": nat.GF_DISP, "knn": nat.GF_KNN_ONLY, "diff": nat.GF_DIFFCAT}[mode]
    out = ops.graph_feature(x, k=k, idx=idx, **kw)
    dout = (torch.ones_like(out) * torch.linspace(-1, 1, out.numel(), device=cuda).view(out.shape)).contiguous()
    dx = torch.zeros(B, C, N, device=cuda)
    nat.check(nat.lib().dgx_graph_feature_bwd_f32(nat.f32(dout), B, C, N, nat.i32(idx), k, gm, nat.f32(dx),
                                                  nat.stream_of(dx)), "atomic bwd")
    torch.cuda.synchronize()
    # both are fp32 sums in different orders over the hubs' ~540 in-edges each
    # (the atomic order varies per run; 1.04e-6 seen once): a few fp32 ulps
    assert rel_err(grads[0].cpu(), dx.cpu()) < 4e-6


def test_graph_feature_rejects_out_of_range_ids(cuda):
    """Caller-given neighbour ids outside [0, N) (or of the wrong shape) raise
    before any kernel reads them, as the reference's indexing raises; nothing
    is launched with them (the forward gather and the reverse-graph backward
    both assume 0 <= id < N)."""
    from dgx import ops
    B, C, N, k = 2, 5, 64, 8
    x = torch.randn(B, C, N, device=cuda)
    idx = torch.randint(0, N, (B, N, k), device=cuda)
    for bad in (N, -1):
        b = idx.clone()
        b[1, 7, 3] = bad
        with pytest.raises(IndexError, match=r"\[0, 64\)"):
            ops.graph_feature(x, k=k, idx=b)
    with pytest.raises(RuntimeError, match="does not match"):
        ops.graph_feature(x, k=k, idx=idx[:, :32])
    assert ops.graph_feature(x, k=k, idx=idx).shape == (B, 2 * C, N, k)


@pytest.mark.parametrize("mode", ["cat", "disp", "knn", "diff"])
def test_graph_feature_backward_atomic_route_exact(cuda, mode):
    """k = 65 > 64: the backward takes the float-atomic route
    (dgx_graph_feature_bwd_f32) through dgx_host::graph_feature_backward. With
    small-integer features and upstream gradients every fp32 sum is exact in
    any order, so the gradient equals the reference's autograd bit for bit."""
    from dgx import ops
    from models.dgcnn import knn
    B, C, N, k = 1, 3, 70, 65
    g = torch.Generator().manual_seed(11)
    x = torch.randint(-4, 5, (B, C, N), generator=g).float()
    idx = knn(x.to(cuda), k).cpu()

    def ref_feature(xc):
        if mode == "diff":   # (x_j - x_i, x_i): the reference's displacement and its centre half
            return torch.cat((R.graph_feature(xc, k, idx=idx, disp_only=True),
                              R.graph_feature(xc, k, idx=idx)[:, C:]), 1)
        return R.graph_feature(xc, k, idx=idx, knn_only=mode == "knn", disp_only=mode == "disp")
    xc = x.clone().requires_grad_(True)
    ref = ref_feature(xc)
    gout = torch.randint(-3, 4, ref.shape, generator=g).float()
    # every partial sum of the gradient is an integer below 2^24: exact in fp32, in any order
    assert float(gout.abs().sum()) < 2 ** 24 and float(x.abs().max()) * 2 < 2 ** 24
    ref.backward(gout)
    xg = x.to(cuda).requires_grad_(True)
    out = ops.graph_feature(xg, k=k, knn_only=mode == "knn", disp_only=mode == "disp", idx=idx.to(cuda),
                            mode="diff" if mode == "diff" else "cat")
    out.backward(gout.to(cuda))
    np.testing.assert_array_equal(out.detach().cpu().numpy(), ref.detach().numpy())
    np.testing.assert_array_equal(xg.grad.cpu().numpy(), xc.grad.numpy())
