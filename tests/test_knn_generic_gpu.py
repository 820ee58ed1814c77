"""kNN for the shapes outside the fused selection kernel (csrc/knn_generic.hip):
C > 128, k > 64, N > 12288 — reference models/dgcnn.py:6-12 accepts any of
them. Indices and selected values bit-exact against the oracle (its pd rounding
sequence is pinned by tests/golden up to C = 256; for C > 256 the reference's
sgemm no longer runs K in one chain, so the C = 512 case checks the engine
against the oracle's single-chain restatement only — parity with the
reference's distances is unpinned there) in canonical tie order, in
both rounding orders (the (B,C,N) tensor and the permuted view the scripts
feed), and identical to the fused kernel on shapes both paths take."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _cloud(B, C, N, seed, layout="bcn"):
    from dgx import synth
    pts = synth.uniform(seed, (B, N, C)).astype(np.float32) - 0.5
    t = torch.from_numpy(pts).permute(0, 2, 1)          # (B,C,N) view of a (B,N,C) buffer: VEC8X4 order
    return t if layout == "perm" else t.contiguous()    # contiguous (B,C,N): strided order


def _check(x, k):
    import oracle
    from dgx import ops
    xd = x.to("cuda")
    assert not ops.fast_shape(x.shape[1], k, x.shape[2])
    idx, vals = ops.knn_raw(xd, k, return_values=True)
    ref_idx, ref_vals = oracle.knn(x, k, return_values=True)
    np.testing.assert_array_equal(idx.cpu().numpy(), ref_idx)
    np.testing.assert_array_equal(vals.cpu().numpy(), ref_vals)


@pytest.mark.parametrize("layout", ["bcn", "perm"])
@pytest.mark.parametrize("B,C,N,k", [(2, 256, 600, 16), (2, 160, 333, 20), (1, 9, 500, 100), (2, 64, 300, 65),
                                     (1, 512, 1024, 20)])
def test_generic_knn_matches_oracle(cuda, B, C, N, k, layout):
    _check(_cloud(B, C, N, seed=C + k, layout=layout), k)


def test_generic_knn_large_cloud(cuda):
    """N above the fused kernel's 12288 points (its fix-up bitmap)."""
    _check(_cloud(1, 3, 13000, seed=4), 20)


def test_generic_knn_large_k(cuda):
    """k in the generic kernel's largest class (4096 < k <= 8192 = dgx_knn_generic_max_k()):
    the 8192-wide bitonic stage and its LDS buffer run on the device."""
    _check(_cloud(1, 3, 6000, seed=21), 5000)


def test_generic_knn_ties_canonical(cuda):
    """Duplicate points: equal distances at the k boundary, resolved by index
    (the canonical order the fused kernel and the oracle both use)."""
    from dgx import synth
    pts = synth.tie_clouds(2, 700, seed=3, frac=0.3)
    x = torch.from_numpy(pts).permute(0, 2, 1).contiguous()
    _check(x, 90)


def test_generic_equals_fused_kernel(cuda):
    """On a shape both paths take, the generic path returns the fused kernel's
    indices and values bit for bit (same Gram chain, same |x|^2, same order)."""
    from dgx import ops
    for layout in ("bcn", "perm"):
        x = _cloud(2, 64, 1024, seed=9, layout=layout).to("cuda")
        k = 20
        idx_f, val_f = ops.knn_raw(x, k, return_values=True)
        idx_g, val_g = ops.knn_raw(x, k, return_values=True, generic=True)
        assert torch.equal(idx_f, idx_g) and torch.equal(val_f, val_g), layout


def test_generic_graph_feature(cuda):
    """get_graph_feature (dgcnn.py:15-44) on 256-channel features: the edge
    tensor of the generic kNN, equal to the oracle's."""
    import oracle
    from models.dgcnn import get_graph_feature
    x = _cloud(2, 256, 400, seed=12)
    out = get_graph_feature(x.to("cuda"), k=24).cpu().numpy()
    ref = oracle.graph_feature(x.numpy(), oracle.knn(x, 24))
    np.testing.assert_array_equal(out, ref)
