"""The reference's ``loss`` module as a drop-in (reference loss.py:4-21) on host
tensors: importable and runnable without libdgx.so, equal to the reference's
recorded loss and gradient (tests/golden/loss_small.npz, written by
make_loss_goldens.py), equal to util.cal_loss, and the two target weights the
device kernels take equal to the reference's target in every dtype."""
import pytest
import torch

from conftest import load_golden

SHAPES = [(37, 50), (5, 2), (64, 13)]


def _case(g, M, C):
    tag = f"m{M}_c{C}"
    return tag, torch.from_numpy(g[f"{tag}_logits"]), torch.from_numpy(g[f"{tag}_labels"])


def test_loss_module_imports_and_runs_without_libdgx(monkeypatch):
    from dgx import _native as nat

    def no_lib():
        raise ImportError("libdgx.so unavailable (test)")
    monkeypatch.setattr(nat, "lib", no_lib)
    from loss import cross_entropy
    torch.manual_seed(0)
    pred = torch.randn(6, 50, requires_grad=True)
    seg = torch.randint(0, 50, (2, 3))
    loss = cross_entropy(pred, seg.view(-1, 1).squeeze())
    loss.backward()
    assert loss.shape == () and torch.isfinite(loss) and pred.grad.shape == (6, 50)


@pytest.mark.parametrize("M,C", SHAPES)
@pytest.mark.parametrize("smoothing", [True, False])
def test_host_loss_matches_reference_golden(M, C, smoothing):
    from loss import cross_entropy
    g = load_golden("loss_small.npz")
    tag, logits, labels = _case(g, M, C)
    kind = "smooth" if smoothing else "plain"
    x = logits.clone().requires_grad_(True)
    loss = cross_entropy(x, labels.view(-1, 1), smoothing=smoothing)
    loss.backward()
    assert loss.dtype == torch.float32
    assert torch.allclose(loss.detach(), torch.from_numpy(g[f"{tag}_{kind}_loss"]), atol=1e-6)
    assert torch.allclose(x.grad, torch.from_numpy(g[f"{tag}_{kind}_grad"]), atol=1e-6)


@pytest.mark.parametrize("smoothing", [True, False])
def test_host_loss_agrees_with_cal_loss(smoothing):
    from loss import cross_entropy
    from util import cal_loss
    g = load_golden("loss_small.npz")
    for M, C in SHAPES:
        _, logits, labels = _case(g, M, C)
        assert torch.allclose(cross_entropy(logits, labels, smoothing), cal_loss(logits, labels, smoothing),
                              atol=1e-6)


def test_host_loss_3d_convention_and_pred():
    """(B, C, N) logits with (B, N) labels equal their (B*N, C) rows; the
    arg-max is torch's."""
    from dgx.loss import smoothed_cross_entropy
    torch.manual_seed(1)
    x = torch.randn(3, 13, 7)
    y = torch.randint(0, 13, (3, 7))
    loss, pred = smoothed_cross_entropy(x, y, return_pred=True)
    rows = x.permute(0, 2, 1).reshape(-1, 13)
    assert torch.allclose(loss, smoothed_cross_entropy(rows, y.view(-1)), atol=1e-6)
    assert torch.equal(pred, x.max(dim=1)[1])
    with pytest.raises(ValueError):
        smoothed_cross_entropy(x, y.view(-1))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("C", [2, 13, 50])
def test_weights_equal_reference_target(dtype, C):
    """The target built from the two constants equals, elementwise, the
    reference's target (1 - eps on the labelled class, eps / (C - 1) elsewhere)
    evaluated as a whole tensor in ``dtype``, kept independent of dgx.cpu."""
    from dgx.cpu import ce_target
    from dgx.loss import ce_weights
    torch.manual_seed(C)
    M, eps = 29, 0.2
    pred = torch.randn(M, C).to(dtype)
    gold = torch.randint(0, C, (M,))
    hit = torch.nn.functional.one_hot(gold, C).to(dtype)
    want = hit * (1 - eps) + (1 - hit) * eps / (C - 1)
    w_true, w_other = ce_weights(dtype, C)
    got = torch.where(hit.bool(), torch.tensor(w_true, dtype=dtype), torch.tensor(w_other, dtype=dtype))
    assert got.dtype == want.dtype == dtype and torch.equal(got, want)
    assert torch.equal(ce_target(pred, gold), want)
    assert ce_weights(dtype, C, smoothing=False) == (1.0, 0.0)
    if dtype != torch.float32:   # the rounded weights no longer sum to 1 over a row
        assert w_true == float(torch.tensor(0.8, dtype=dtype))


def test_one_class_raises():
    from dgx.loss import ce_weights, smoothed_cross_entropy
    with pytest.raises(ValueError):
        ce_weights(torch.float32, 1)
    with pytest.raises(ValueError):
        smoothed_cross_entropy(torch.zeros(4, 1), torch.zeros(4, dtype=torch.int64))


def test_c_abi_validates_before_device_work():
    """Bad arguments return DGX_EINVAL / DGX_EUNSUPPORTED before anything is
    launched (the buffers here are host memory and are never touched)."""
    import ctypes
    from dgx import _native
    L = _native.lib()
    assert [L.dgx_smoothed_ce_workspace_bytes(m) for m in (0, 1, 128, 129)] == [0, 8, 8, 16]
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.cast(buf, ctypes.c_void_p)

    def fwd(logits=p, dtype=0, B=1, C=50, N=4, sb=200, sc=1, sn=50, ws_bytes=8):
        return L.dgx_smoothed_ce_fwd(logits, dtype, B, C, N, sb, sc, sn, p, 1, 0.8, 0.004, p, p, None, p, ws_bytes,
                                     None)

    def bwd(g=p, **kw):
        a = dict(dtype=0, B=1, C=50, N=4, sb=200, sc=1, sn=50)
        a.update(kw)
        return L.dgx_smoothed_ce_bwd(p, a["dtype"], a["B"], a["C"], a["N"], a["sb"], a["sc"], a["sn"], p, 1, 0.8,
                                     0.004, p, g, p, None)
    assert fwd(logits=None) == -1 and fwd(C=1) == -1 and fwd(dtype=3) == -1 and fwd(N=0) == -1
    assert fwd(ws_bytes=0) == -1
    assert fwd(B=2, C=50, N=4, sb=400, sc=8, sn=2) == -2   # neither layout
    assert bwd(g=None) == -1 and bwd(C=1) == -1 and bwd(sc=2) == -2
