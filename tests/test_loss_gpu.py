"""The loss head on the device (dgx.loss.smoothed_cross_entropy, csrc/loss.hip)
against an fp64 oracle written here: the formulas of the kernel's header
evaluated in fp64 from the same inputs, already rounded to their dtype, with
the same two target weights.

Bars (derived, not measured):
  * fp32 loss: |loss - loss64| <= 8 * 2^-23 * |loss64|. Each row's loss is a few
    roundings of O(1) quantities and a fixed-order sum over M <= 4099 positive
    terms adds at most log2(M) more; the kernels sum in fp64 and round once, so
    they sit at half a unit.
  * fp32 gradient: conftest.rel_err(grad, grad64) <= 1e-6.
  * fp16 / bf16 gradient (under autocast, g = 65536 on the device: the
    GradScaler case): every element at most one unit in the last place of the
    dtype from the oracle's value rounded to the dtype, compared as 16-bit
    patterns, and none flushed to zero where the oracle's is not.
  * the two layouts and the copy path: bit for bit (both forward kernels sum
    the same rows in the same order).
"""
import functools

import numpy as np
import pytest
import torch

from conftest import load_golden, rel_err

pytestmark = pytest.mark.gpu

# class-contiguous (M, C); (200, 129) makes a workgroup of the rows kernel stage a second LDS tile
# (its 128 rows against 63 rows of 516 bytes per tile in fp32, 127 of 258 bytes in fp16 / bf16)
ROWS = [(1, 2), (37, 50), (1000, 13), (4099, 50), (33, 129), (5, 1000), (200, 129)]
PLANES = [(3, 50, 70), (2, 13, 1025)]                                     # point-contiguous (B, C, N)
LOSS_BAR = 8 * 2.0 ** -23
GRAD_BAR = 1e-6
GOLDEN = [(37, 50), (5, 2), (64, 13)]


def oracle(x, y, w_true, w_other, g=1.0):
    """(loss, gradient) in fp64 for (M, C) logits x (any dtype, host) and labels y."""
    x = x.double()
    M, C = x.shape
    mx = x.max(dim=1, keepdim=True)[0]
    lse = mx + torch.log(torch.exp(x - mx).sum(dim=1, keepdim=True))
    w = torch.full_like(x, w_other)
    w[torch.arange(M), y.long()] = w_true
    loss = (-(w * (x - lse)).sum(dim=1)).mean()
    W = w_true + (C - 1) * w_other
    return float(loss), (g / M) * (W * torch.exp(x - lse) - w)


@functools.lru_cache(maxsize=None)
def rows_case(M, C, dtype=torch.float32):
    """Seeded host logits (rounded to dtype) and labels covering class 0 and C - 1."""
    g = torch.Generator().manual_seed(7 * M + C)
    x = (torch.randn(M, C, generator=g) * 2.0).to(dtype)
    y = torch.randint(0, C, (M,), generator=g)
    y[0], y[-1] = 0, C - 1
    return x, y


def label_sets(M, C, y):
    """The case's labels; a single row takes class 0 and class C - 1 in turn."""
    return [y] if M > 1 else [torch.tensor([0]), torch.tensor([C - 1])]


def run(x, y, g=None, autocast=False, **kw):
    """Engine loss and gradient of device logits x (a fresh leaf of the same strides)."""
    from dgx.loss import smoothed_cross_entropy
    x = x.detach().requires_grad_(True)
    with torch.autocast("cuda", dtype=x.dtype if autocast else torch.float16, enabled=autocast):
        out = smoothed_cross_entropy(x, y, **kw)
    loss = out[0] if isinstance(out, tuple) else out
    (loss if g is None else loss * g).backward()
    return out, x.grad


def ordered16(t):
    """16-bit patterns of a half tensor as integers ordered like the values."""
    i = t.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(i < 0, -(i & 0x7FFF), i)


def check_half_grad(got, want64):
    want = want64.to(got.dtype)
    got = got.cpu()
    diff = (ordered16(got) - ordered16(want)).abs()
    print("max 16-bit distance", int(diff.max()), "elements above 1:", int((diff > 1).sum()))
    assert int(diff.max()) <= 1
    assert not ((got == 0) & (want != 0)).any()


def check_loss(loss, want, bar=LOSS_BAR):
    err = abs(float(loss.detach()) - want) / abs(want)
    print(f"loss {float(loss.detach()):.9g} oracle {want:.9g} rel err {err:.3g} bar {bar:.3g}")
    assert np.isfinite(float(loss.detach())) and err <= bar


@pytest.mark.parametrize("M,C", GOLDEN)
@pytest.mark.parametrize("smoothing", [True, False])
def test_golden(cuda, M, C, smoothing):
    g = load_golden("loss_small.npz")
    tag, kind = f"m{M}_c{C}", "smooth" if smoothing else "plain"
    x = torch.from_numpy(g[f"{tag}_logits"]).to(cuda)
    y = torch.from_numpy(g[f"{tag}_labels"]).to(cuda)
    loss, grad = run(x, y, smoothing=smoothing)
    assert loss.dtype == torch.float32 and loss.shape == ()
    check_loss(loss, float(g[f"{tag}_{kind}_loss"]))
    assert rel_err(grad.cpu().numpy(), g[f"{tag}_{kind}_grad"]) <= GRAD_BAR


@pytest.mark.parametrize("M,C", ROWS)
def test_rows_fp32(cuda, M, C):
    from dgx.loss import ce_weights
    x, y = rows_case(M, C)
    for y in label_sets(M, C, y):
        want, want_grad = oracle(x, y, *ce_weights(torch.float32, C))
        (loss, pred), grad = run(x.to(cuda), y.to(cuda), return_pred=True)
        check_loss(loss, want)
        err = rel_err(grad.cpu().numpy(), want_grad.numpy())
        print("grad rel err", err)
        assert err <= GRAD_BAR and grad.dtype == torch.float32 and grad.is_contiguous()
        assert pred.dtype == torch.int64 and torch.equal(pred.cpu(), x.max(dim=1)[1])


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("M,C", ROWS)
def test_rows_half_autocast_scaled(cuda, M, C, dtype):
    from dgx.loss import ce_weights
    x, y = rows_case(M, C, dtype)
    scale = torch.full((), 65536.0, device=cuda)
    for y in label_sets(M, C, y):
        want, want_grad = oracle(x, y, *ce_weights(dtype, C), g=65536.0)
        loss, grad = run(x.to(cuda), y.to(cuda), g=scale, autocast=True)
        assert loss.dtype == torch.float32 and grad.dtype == dtype
        check_loss(loss, want)
        check_half_grad(grad, want_grad)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("B,C,N", PLANES)
def test_planes_match_oracle_and_rows_bitwise(cuda, B, C, N, dtype):
    """(B, C, N) input: the oracle's bars, and bit for bit the result of its
    permute(0, 2, 1).contiguous().view(-1, C) copy through the rows kernel,
    of the uncopied permuted view of that copy, and of a strided input that is
    neither layout (the copy path)."""
    from dgx.loss import ce_weights
    gen = torch.Generator().manual_seed(B * C * N)
    x = (torch.randn(B, C, N, generator=gen) * 2.0).to(dtype)
    y = torch.randint(0, C, (B, N), generator=gen)
    y[0, 0], y[-1, -1] = 0, C - 1
    half = dtype != torch.float32
    g = 65536.0 if half else 1.0
    scale = torch.full((), g, device=cuda)
    xr = x.permute(0, 2, 1).contiguous().view(-1, C)
    want, want_grad = oracle(xr, y.view(-1), *ce_weights(dtype, C), g=g)
    xd, yd = x.to(cuda), y.to(cuda)
    (loss, pred), grad = run(xd, yd, g=scale, autocast=half, return_pred=True)
    check_loss(loss, want)
    assert grad.shape == x.shape and grad.is_contiguous() and grad.dtype == dtype
    rows_grad = grad.permute(0, 2, 1).reshape(-1, C)
    if half:
        check_half_grad(rows_grad, want_grad)
    else:
        assert rel_err(rows_grad.cpu().numpy(), want_grad.numpy()) <= GRAD_BAR
    assert torch.equal(pred.cpu(), x.max(dim=1)[1])

    xrd = xd.permute(0, 2, 1).contiguous()
    (loss_r, pred_r), grad_r = run(xrd.view(-1, C), yd.view(-1), g=scale, autocast=half, return_pred=True)
    assert torch.equal(loss_r, loss) and torch.equal(grad_r, rows_grad) and torch.equal(pred_r, pred.view(-1))
    view = xrd.permute(0, 2, 1)   # (B, C, N) strides (N*C, 1, C): the rows kernel, no copy
    loss_v, grad_v = run(view, yd, g=scale, autocast=half)
    assert torch.equal(loss_v, loss) and torch.equal(grad_v, grad) and grad_v.stride() == view.stride()
    wide = torch.zeros(B, C, 2 * N, dtype=dtype, device=cuda)
    wide[:, :, ::2] = xd
    strided = wide[:, :, ::2]
    assert not strided.is_contiguous()
    loss_s, grad_s = run(strided, yd, g=scale, autocast=half)
    assert torch.equal(loss_s, loss) and torch.equal(grad_s, grad)


def test_rows_copy_path(cuda):
    """A row-strided (M, C) slice is neither layout: same result through the copy."""
    x, y = rows_case(37, 50)
    xd, yd = x.to(cuda), y.to(cuda)
    wide = torch.zeros(37, 100, device=cuda)
    wide[:, :50] = xd
    loss, grad = run(xd, yd)
    loss_s, grad_s = run(wide[:, :50], yd)
    assert torch.equal(loss_s, loss) and torch.equal(grad_s, grad)


def test_unaligned_rows(cuda):
    """Rows that start 2 or 4 bytes past a 16-byte boundary (a view into a
    larger buffer): the flat tile load and the backward's 16-byte path must
    not touch bytes outside the rows."""
    from dgx.loss import ce_weights
    for dtype, g in ((torch.float32, 1.0), (torch.float16, 65536.0)):
        x, y = rows_case(37, 50, dtype)
        buf = torch.full((37 * 50 + 16,), float("nan"), dtype=dtype, device=cuda)
        xd = buf[1:1 + 37 * 50].view(37, 50)
        xd.copy_(x)
        assert xd.data_ptr() % 16 != 0
        want, want_grad = oracle(x, y, *ce_weights(dtype, 50), g=g)
        loss, grad = run(xd, y.to(cuda), g=torch.full((), g, device=cuda), autocast=dtype != torch.float32)
        check_loss(loss, want)
        if dtype == torch.float32:
            assert rel_err(grad.cpu().numpy(), want_grad.numpy()) <= GRAD_BAR
        else:
            check_half_grad(grad, want_grad)


def test_range(cuda):
    """Large logits need the max subtraction: fp32 near 1e4 and fp16 over the
    whole fp16 range give a finite loss within the bars; one inf logit does not."""
    from dgx.loss import ce_weights
    gen = torch.Generator().manual_seed(5)
    y = torch.randint(0, 50, (37,), generator=gen)
    y[0], y[-1] = 0, 49
    x = torch.randn(37, 50, generator=gen) * 30 + 1e4
    want, want_grad = oracle(x, y, *ce_weights(torch.float32, 50))
    loss, grad = run(x.to(cuda), y.to(cuda))
    check_loss(loss, want)
    assert rel_err(grad.cpu().numpy(), want_grad.numpy()) <= GRAD_BAR
    xh = ((torch.rand(37, 50, generator=gen) * 2 - 1) * 6e4).half()
    want, want_grad = oracle(xh, y, *ce_weights(torch.float16, 50), g=65536.0)
    loss, grad = run(xh.to(cuda), y.to(cuda), g=torch.full((), 65536.0, device=cuda), autocast=True)
    check_loss(loss, want)
    check_half_grad(grad, want_grad)
    x[3, 7] = float("inf")
    loss, _ = run(x.to(cuda), y.to(cuda))
    assert not torch.isfinite(loss)


def test_labels(cuda):
    """int32 labels equal int64 bit for bit. Labels are only compared with the
    class index in the kernels (ce_row / ce_grad in csrc/loss.hip: ``j == y``,
    never ``x[y]``), so a label outside [0, C) is safe to run: it gives a NaN
    loss and NaN in exactly its gradient rows, every other row as before."""
    x, y = rows_case(37, 50)
    xd, yd = x.to(cuda), y.to(cuda)
    loss, grad = run(xd, yd)
    loss32, grad32 = run(xd, yd.int())
    assert torch.equal(loss32, loss) and torch.equal(grad32, grad)
    bad = yd.clone()
    bad[5], bad[20] = -1, 50
    loss_b, grad_b = run(xd, bad)
    assert torch.isnan(loss_b)
    rows = torch.zeros(37, dtype=torch.bool, device=cuda)
    rows[5] = rows[20] = True
    assert torch.isnan(grad_b[rows]).all() and torch.equal(grad_b[~rows], grad[~rows])
    planes = xd.view(1, 37, 50).permute(0, 2, 1).contiguous()   # (1, 50, 37): the planes kernels
    loss_p, grad_p = run(planes, bad.view(1, 37))
    assert torch.isnan(loss_p)
    assert torch.isnan(grad_p[0, :, rows]).all() and torch.equal(grad_p[0, :, ~rows].t(), grad[~rows])


def test_argmax_ties(cuda):
    from dgx.loss import smoothed_cross_entropy
    x, y = rows_case(37, 50)
    x = x.clone()
    x[4, 9] = x[4, 31] = x[4].max() + 1.0
    x[0, 0] = x[0, 49] = x[0].max() + 1.0
    for xd in (x.to(cuda), x.t().contiguous().view(1, 50, 37).to(cuda)):
        yd = y.to(cuda).view(xd.shape[:1] + xd.shape[2:])
        _, pred = smoothed_cross_entropy(xd, yd, return_pred=True)
        pred = pred.view(-1).cpu()
        assert pred[4] == 9 and pred[0] == 0
        keep = torch.ones(37, dtype=torch.bool)
        keep[[0, 4]] = False
        assert torch.equal(pred[keep], x.max(dim=1)[1][keep])


def test_deterministic(cuda):
    x, y = rows_case(4099, 50)
    xd, yd = x.to(cuda), y.to(cuda)
    a, b = run(xd, yd), run(xd, yd)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_result_dtype(cuda):
    """The reference's result dtype: fp32 under autocast, the logits' dtype outside it."""
    from dgx.loss import ce_weights, smoothed_cross_entropy
    x, y = rows_case(37, 50, torch.float16)
    loss = smoothed_cross_entropy(x.to(cuda), y.to(cuda))
    assert loss.dtype == torch.float16
    want, _ = oracle(x, y, *ce_weights(torch.float16, 50))
    assert float(loss) == float(torch.tensor(want).half())
    with torch.autocast("cuda", dtype=torch.float16):
        assert smoothed_cross_entropy(x.to(cuda), y.to(cuda)).dtype == torch.float32
    with pytest.raises(ValueError):
        smoothed_cross_entropy(torch.zeros(4, 1, device=cuda), torch.zeros(4, dtype=torch.int64, device=cuda))


def test_graph_capture(cuda):
    """Forward + backward at (300, 50) fp16 captured in one graph on one
    stream; each of two replays with new logits, labels and g equals eager."""
    from dgx.loss import smoothed_cross_entropy

    def step(x, y, g):
        with torch.autocast("cuda", dtype=torch.float16):
            loss = smoothed_cross_entropy(x, y)
        return loss, torch.autograd.grad(loss * g, x)[0]

    gen = torch.Generator().manual_seed(11)
    sx = (torch.randn(300, 50, generator=gen) * 2).half().to(cuda).requires_grad_(True)
    sy = torch.randint(0, 50, (300,), generator=gen).to(cuda)
    sg = torch.full((), 65536.0, device=cuda)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(sx, sy, sg)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step(sx, sy, sg)
    for scale in (1024.0, 8.0):
        x = (torch.randn(300, 50, generator=gen) * 2).half().to(cuda)
        y = torch.randint(0, 50, (300,), generator=gen).to(cuda)
        with torch.no_grad():
            sx.copy_(x)
            sy.copy_(y)
            sg.fill_(scale)
        graph.replay()
        want = step(x.requires_grad_(True), y, torch.full((), scale, device=cuda))
        assert torch.equal(out[0], want[0]) and torch.equal(out[1], want[1])


def test_no_host_sync(cuda):
    x, y = rows_case(37, 50, torch.float16)
    xd, yd = x.to(cuda), y.to(cuda)
    planes = xd.view(1, 37, 50).permute(0, 2, 1).contiguous()
    scale = torch.full((), 65536.0, device=cuda)
    run(xd, yd, g=scale, autocast=True)   # library and kernels loaded before the mode is set
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        run(xd, yd, g=scale, autocast=True, return_pred=True)
        run(planes, yd.view(1, 37), g=scale, autocast=True, return_pred=True)
    finally:
        torch.cuda.set_sync_debug_mode(prev)


def test_drop_in_call(cuda):
    """loss.cross_entropy as the part-segmentation script calls it."""
    from dgx.loss import ce_weights
    from loss import cross_entropy
    gen = torch.Generator().manual_seed(3)
    seg_pred_host = torch.randn(2, 19, 50, generator=gen)
    seg_host = torch.randint(0, 50, (2, 19), generator=gen)
    seg_pred = seg_pred_host.to(cuda).requires_grad_(True)
    seg = seg_host.to(cuda)
    loss = cross_entropy(seg_pred.view(-1, 50), seg.view(-1, 1).squeeze())
    loss.backward()
    want, want_grad = oracle(seg_pred_host.view(-1, 50), seg_host.view(-1), *ce_weights(torch.float32, 50))
    check_loss(loss, want)
    assert rel_err(seg_pred.grad.view(-1, 50).cpu().numpy(), want_grad.numpy()) <= GRAD_BAR
