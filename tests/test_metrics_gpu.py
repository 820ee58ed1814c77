"""dgx.metrics on the device (csrc/metrics.hip): the reference's recorded
epoch-end numbers, the loss head's arg-max, the host path (dgx.cpu) at every
edge of the kernel's geometry, containment of bad data, capacity, HIP-graph
replay and accumulation. All state is integer (and one fp32 sum added in the
same order), so every comparison is an equality."""
import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    return load_golden("seg_metrics.npz")


def _parts(C):
    """A part table over C classes: category 0 owns the whole range (max_parts
    = C: the part-slot loop strides over the waves), the others own runs of 1,
    2, 3, 1, ... classes."""
    start, count, at, n = [0], [C], 0, 1
    while at < C:
        n = min(n, C - at)
        start.append(at)
        count.append(n)
        at += n
        n = n % 3 + 1
    return start, count


def _layout(x, rows):
    """(B, C, N) logits point-contiguous, or class-contiguous with the same shape."""
    return x.permute(0, 2, 1).contiguous().permute(0, 2, 1) if rows else x.contiguous()


def _pair(C, dev, capacity=0, parts=None, **kw):
    from dgx import metrics
    start, count = parts if parts is not None else (None, None)
    return (metrics.SegMetrics(C, capacity, start, count, device=dev, **kw),
            metrics.SegMetrics(C, capacity, start, count, **kw))


@pytest.mark.parametrize("ids", [torch.int64, torch.int32])
@pytest.mark.parametrize("name", ["all", "one"])
def test_fixture_on_the_device(cuda, gold, name, ids):
    from dgx import metrics
    start = gold["part_start"] if name == "all" else np.zeros_like(gold["part_start"])
    pred, seg, label = (torch.from_numpy(gold[f"{name}_{k}"].astype(np.int64)).to(cuda).to(ids)
                        for k in ("pred", "seg", "label"))
    B = seg.shape[0]
    m = metrics.SegMetrics(50, capacity=B, part_start=start, part_count=gold["part_count"], device=cuda)
    cuts = [0, 1, 3, 4, 5, 6, 8, B] if B < 12 else [0, 1, 3, 10, 11, 20, 33, B]
    for feed in ([0, B], cuts):
        m.reset()
        for a, b in zip(feed[:-1], feed[1:]):
            m.update(pred[a:b], seg[a:b], label[a:b].view(-1, 1))
        r = m.compute()
        assert np.array_equal(r["shape_ious"], gold[f"{name}_shape_ious"])
        assert r["acc"] == float(gold[f"{name}_acc"]) and r["avg_acc"] == float(gold[f"{name}_avg_acc"])
        assert r["count"] == B
    choice = None if name == "all" else "chair"
    assert metrics.calculate_shape_IoU(pred, seg, label, choice) == gold[f"{name}_shape_ious"].tolist()


@pytest.mark.parametrize("rows", [False, True], ids=["planes", "rows"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("data", ["random", "ties", "nonfinite"])
def test_argmax_is_the_loss_heads(cuda, data, dtype, rows):
    """update(logits) and update(pred of dgx.loss on the same logits) leave the
    same state: the kernel's arg-max is the loss head's (csrc/ce_row.h)."""
    from dgx import loss as L
    B, C, P = 3, 50, 257
    g = torch.Generator().manual_seed(17)
    if data == "ties":
        x = torch.randint(0, 4, (B, C, P), generator=g).float()          # 4 levels: every row has equal maxima
    else:
        x = torch.randn(B, C, P, generator=g) * 3
    if data == "nonfinite":
        inf = float("inf")
        x[0, 0, 0:40] = float("nan")            # NaN in class 0: the row keeps class 0
        x[0, 7, 20:80] = float("nan")           # NaN elsewhere: passed over
        x[1, :, 5] = -inf                       # all -inf: class 0
        x[1, 11, 60:90] = inf
        x[1, 30, 70:100] = inf                  # two +inf: the first
        x[2, :, 100:130] = float("nan")         # all NaN
        x[2, 49, 200:] = -inf
    x = _layout(x.to(dtype).to(cuda), rows)
    seg = torch.randint(0, C, (B, P), generator=g).to(cuda)
    label = torch.tensor([0, 5, 16], device=cuda)
    parts = _parts(C)
    _, pred = L.smoothed_cross_entropy(x, seg, return_pred=True)
    m1, _ = _pair(C, cuda, B, parts)
    m2, _ = _pair(C, cuda, B, parts)
    m1.update(x, seg, label)
    m2.update(pred, seg, label)
    assert torch.equal(m1._buf, m2._buf)
    assert int(m1.confusion.sum()) == B * P and int(m1.state[1]) == 0
    if data == "random" and dtype == torch.float32:   # no equal maxima: torch's own arg-max
        assert torch.equal(pred, x.max(dim=1)[1])
        m2.reset()
        m2.update(x.max(dim=1)[1], seg, label)
        assert torch.equal(m1._buf, m2._buf)


# (B, C, N, source, cat): each against the host path on the same data.
#   source: logits dtype + layout ("rows" class-contiguous, staged in LDS; "planes" point-contiguous), or ids.
#   N: 1, 63 / 64 / 65 (below, at, above a wave), 257 (four waves and a ragged tail of 1), 1025 (a second
#      chunk of 1024 points, the workgroup's size, with a tail of 1)
#   C: 2 minimum, 13 semseg, 50 partseg (100-byte fp16 rows: unaligned), 64 (the 16 KiB table's limit),
#      65 (first size on the 64 KiB table), 128 (its limit; fp32 rows fill a 32 KiB tile 64 at a time)
#   B: 1, 3, 33 workgroups (or, without cat, the shapes the flat chunks straddle)
EDGES = [
    (1, 2, 1, "fp32-planes", True),       # the smallest call
    (3, 13, 63, "fp16-planes", True),     # below a wave
    (3, 13, 64, "bf16-rows", True),       # exactly a wave, rows of 26 bytes
    (3, 50, 65, "fp16-rows", True),       # a wave and one lane; 100-byte rows
    (33, 50, 257, "fp16-planes", True),   # the flagship layout: ragged tail, 33 workgroups
    (3, 50, 1025, "fp16-planes", True),   # the flagship layout: a second chunk
    (1, 13, 1025, "bf16-rows", True),     # rows: a full tile of 1024 rows, then a second chunk
    (3, 50, 1025, "int64", False),        # no cat: four chunks on one workgroup
    (1, 50, 257, "fp32-rows", True),      # 200-byte rows: 163 per tile, two tiles in a chunk
    (3, 64, 65, "bf16-planes", True),     # the small table's last size
    (3, 65, 65, "fp16-rows", True),       # the large table's first size
    (3, 128, 257, "fp32-rows", True),     # LDS limit: 64 KiB table, 64 rows per tile, five tiles
    (1, 128, 64, "bf16-planes", True),    # LDS limit, one wave
    (33, 128, 63, "fp16-rows", True),     # LDS limit, 33 workgroups
    (33, 2, 1, "int64", True),            # one point per shape
    (3, 13, 257, "int32", True),
    (1, 65, 63, "int64", True),
    (33, 128, 65, "int32", True),
    (3, 50, 257, "fp16-planes", False),   # no cat: 771 flat rows, one chunk across the shapes
    (33, 13, 257, "bf16-rows", False),    # no cat: 9 chunks on 3 workgroups, rows layout across shapes
    (3, 64, 64, "int64", False),
    (1, 2, 1, "fp16-rows", False),        # one point, one 4-byte row
    (33, 65, 63, "fp32-planes", False),
    (3, 128, 257, "int32", False),
]


def _source(kind, B, C, P, g, dev):
    if kind.startswith("int"):
        ids = torch.randint(0, C, (B, P), generator=g)
        return ids.to(torch.int64 if kind == "int64" else torch.int32).to(dev), ids
    dtype, layout = kind.split("-")
    x = (torch.randn(B, C, P, generator=g) * 2).to({"fp32": torch.float32, "fp16": torch.float16,
                                                    "bf16": torch.bfloat16}[dtype])
    return _layout(x.to(dev), layout == "rows"), x


@pytest.mark.parametrize("B,C,P,kind,cat", EDGES)
def test_edges_equal_the_host_path(cuda, B, C, P, kind, cat):
    g = torch.Generator().manual_seed(1000 * C + P)
    parts = _parts(C)
    dm, hm = _pair(C, cuda, 2 * B if cat else 0, parts if cat else None)
    for step in range(2):   # the second call continues at the cursor
        dx, hx = _source(kind, B, C, P, g, cuda)
        seg = torch.randint(0, C, (B, P), generator=g)
        seg = torch.where(torch.rand(B, P, generator=g) < 0.5, seg, hx if hx.dim() == 2 else hx.float().argmax(1))
        label = torch.randint(0, len(parts[0]), (B,), generator=g) if cat else None
        if cat:
            label[0] = 0   # the category with all C part slots
        loss = torch.rand((), generator=g)
        dm.update(dx, seg.to(cuda), None if label is None else label.to(cuda), loss.to(cuda))
        hm.update(hx, seg, label, loss)
    assert torch.equal(dm._buf.cpu(), hm._buf)
    assert int(dm.state[4]) == 0 and int(dm.state[3]) == 2 * B and int(dm.confusion.sum()) == 2 * B * P
    r = dm.compute()
    assert r["shape_ious"].shape == ((2 * B,) if cat else (0,))


@pytest.mark.parametrize("M,C,dtype", [(1, 50, torch.float16), (4099, 13, torch.float32), (4099, 50, torch.bfloat16)])
def test_classification_geometry(cuda, M, C, dtype):
    """(M, C) logits with (M,) labels, no categories: the grid-strided path
    (4099 rows: 5 chunks on 2 workgroups, 3 and 2)."""
    g = torch.Generator().manual_seed(M + C)
    x = torch.randn(M, C, generator=g).to(dtype)
    y = torch.randint(0, C, (M,), generator=g)
    dm, hm = _pair(C, cuda)
    dm.update(x.to(cuda), y.to(cuda))
    hm.update(x, y)
    assert torch.equal(dm._buf.cpu(), hm._buf)
    if dtype == torch.float32:   # no equal maxima: the column sums count torch's own arg-max
        assert torch.equal(dm.confusion.sum(dim=0).cpu(), torch.bincount(x.argmax(1), minlength=C))
    # strides of neither layout: one copy, same result
    wide = torch.randn(M, 2 * C, generator=g).to(dtype)
    dm.reset(), hm.reset()
    dm.update(wide.to(cuda)[:, ::2], y.to(cuda))
    hm.update(wide[:, ::2], y)
    assert torch.equal(dm._buf.cpu(), hm._buf)


def test_too_many_classes_raise_before_any_launch(cuda):
    from dgx import _native, metrics
    with pytest.raises(ValueError, match="128"):
        metrics.SegMetrics(129, device=cuda)
    # the C ABI itself: argument checks come first (null streams and buffers are never reached)
    L = _native.lib()
    one = torch.zeros(8, dtype=torch.int64, device=cuda)
    p = _native.ptr(one)
    args = [p, 3, 1, 129, 8, 0, 0, 0, p, 1, None, 0, None, None, 0, p, None, None, 0, 1, p, None, None, None]
    assert L.dgx_seg_metrics_update(*args) == -2
    args[3] = 1
    assert L.dgx_seg_metrics_update(*args) == -1
    torch.cuda.synchronize()
    assert int(one.sum()) == 0


def test_bad_data_is_contained(cuda):
    """Labels, predictions and categories outside their range are counted in
    ``invalid`` and never used as an address: the sentinel words around every
    state region stay as they were."""
    B, C, P = 4, 50, 129
    g = torch.Generator().manual_seed(3)
    parts = _parts(C)
    seg = torch.randint(0, C, (B, P), generator=g)
    pred = torch.randint(0, C, (B, P), generator=g)
    label = torch.tensor([0, 3, 5, 7])
    bad_seg, bad_pred, bad_label = seg.clone(), pred.clone(), label.clone()
    bad_seg[0, 0], bad_seg[1, 64], bad_seg[3, 128] = -1, C, 2 ** 40
    bad_pred[0, 1], bad_pred[2, 65], bad_pred[3, 127] = -1, C, 2 ** 40
    bad_pred[0, 0] = -7                     # the same point as a bad seg: one invalid point
    bad_label[1], bad_label[2] = len(parts[0]), -1
    planted = 6 + 2
    dm, hm = _pair(C, cuda, B, parts, _guard=64)
    assert dm._guards_intact()
    dm.update(bad_pred.to(cuda), bad_seg.to(cuda), bad_label.to(cuda))
    hm.update(bad_pred, bad_seg, bad_label)
    torch.cuda.synchronize()
    assert dm._guards_intact()
    assert int(dm.state[1]) == planted and int(dm.state[2]) == 0
    assert int(dm.confusion.sum()) == B * P - 6
    assert torch.equal(dm._buf.cpu(), hm._buf)
    assert dm.nparts.tolist() == [C, 0, 0, parts[1][7]]
    with pytest.raises(ValueError, match=f"invalid={planted}"):
        dm.compute()
    # logits with bad labels (fp16 planes and rows), int32 ids
    x = torch.randn(B, C, P, generator=g).half()
    bad_seg[3, 128] = 2 ** 31 - 1
    for rows in (False, True):
        dm.reset(), hm.reset()
        dm.update(_layout(x.to(cuda), rows), bad_seg.int().to(cuda), bad_label.int().to(cuda))
        hm.update(x, bad_seg, bad_label)
        assert dm._guards_intact() and int(dm.state[1]) == 3 + 2
        assert torch.equal(dm._buf.cpu(), hm._buf)
    dm.reset()
    dm.update(pred.to(cuda), seg.to(cuda), label.to(cuda))
    assert dm._guards_intact() and dm.compute()["count"] == B


def test_capacity(cuda):
    B, C, P = 3, 50, 129
    g = torch.Generator().manual_seed(4)
    parts = _parts(C)
    dm, hm = _pair(C, cuda, 5, parts, _guard=64)
    for _ in range(2):
        pred, seg = torch.randint(0, C, (B, P), generator=g), torch.randint(0, C, (B, P), generator=g)
        label = torch.randint(0, len(parts[0]), (B,), generator=g)
        dm.update(pred.to(cuda), seg.to(cuda), label.to(cuda))
        hm.update(pred, seg, label)
    assert int(dm.state[2]) == 1 and int(dm.state[0]) == 6 and dm._guards_intact()
    assert int(dm.confusion.sum()) == 6 * P
    assert torch.equal(dm._buf.cpu(), hm._buf)
    with pytest.raises(ValueError, match="overflow=1"):
        dm.compute()


def test_graph_replay_equals_eager(cuda):
    """One captured update, replayed three times on new inputs, leaves the
    state of three eager updates: nothing in update() synchronises or
    allocates, and the cursor, count and loss sum advance on the device."""
    B, C, P = 4, 50, 257
    g = torch.Generator().manual_seed(9)
    parts = _parts(C)
    dm, em = _pair(C, cuda, 3 * B, parts)[0], _pair(C, cuda, 3 * B, parts)[0]
    sx = torch.zeros(B, C, P, dtype=torch.float16, device=cuda)
    sy = torch.zeros(B, P, dtype=torch.int64, device=cuda)
    sl = torch.zeros(B, dtype=torch.int64, device=cuda)
    sloss = torch.zeros((), device=cuda)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        dm.update(sx, sy, sl, sloss)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        dm.update(sx, sy, sl, sloss)
    dm.reset()
    want = torch.zeros((), dtype=torch.float32)
    for _ in range(3):
        x = torch.randn(B, C, P, generator=g).half()
        y = torch.randint(0, C, (B, P), generator=g)
        lab = torch.randint(0, len(parts[0]), (B,), generator=g)
        loss = torch.rand((), generator=g) * 3
        sx.copy_(x), sy.copy_(y), sl.copy_(lab), sloss.copy_(loss)
        graph.replay()
        em.update(x.to(cuda), y.to(cuda), lab.to(cuda), loss.to(cuda))
        want = want + loss
    torch.cuda.synchronize()
    assert torch.equal(dm._buf, em._buf)
    r = dm.compute()
    assert r["count"] == 3 * B and r["loss_sum"] == float(want) and r["shape_ious"].shape == (3 * B,)


def test_update_neither_synchronises_nor_allocates(cuda):
    B, C, P = 3, 50, 65
    g = torch.Generator().manual_seed(2)
    parts = _parts(C)
    m = _pair(C, cuda, 4 * B, parts)[0]
    x = torch.randn(B, C, P, generator=g).half().to(cuda)
    seg = torch.randint(0, C, (B, P), generator=g).to(cuda)
    label, loss = torch.tensor([0, 1, 2], device=cuda), torch.ones((), device=cuda)
    ids, rows = x.max(dim=1)[1], _layout(x, True)
    m.update(x, seg, label, loss)   # library and kernels loaded before the mode is set
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    before = torch.cuda.memory_stats(cuda)["allocation.all.allocated"]
    try:
        m.update(x, seg, label, loss)
        m.update(ids, seg, label)
        m.update(rows, seg.view(-1))
        m.reset()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert torch.cuda.memory_stats(cuda)["allocation.all.allocated"] == before


def test_accumulation(cuda):
    """50 updates of one batch equal one update of the batch 50 times over;
    every int64 table entry is 50 times the single one."""
    B, C, P = 2, 50, 129
    g = torch.Generator().manual_seed(21)
    x = _layout((torch.randn(B, C, P, generator=g)).half().to(cuda), False)
    seg = torch.randint(0, C, (B, P), generator=g).to(cuda)
    parts = _parts(C)
    label = torch.tensor([0, 9], device=cuda)
    one, many = _pair(C, cuda, B, parts)[0], _pair(C, cuda, 50 * B, parts)[0]
    big = _pair(C, cuda, 50 * B, parts)[0]
    one.update(x, seg, label)
    for _ in range(50):
        many.update(x, seg, label)
    big.update(x.repeat(50, 1, 1), seg.repeat(50, 1), label.repeat(50))
    assert torch.equal(many._buf, big._buf)
    assert torch.equal(many.confusion, 50 * one.confusion) and int(many.state[3]) == 50 * B
    assert torch.equal(many.iu[:B], one.iu) and torch.equal(many.iu[-B:], one.iu)
