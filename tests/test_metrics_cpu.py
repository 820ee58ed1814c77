"""dgx.metrics on host tensors (the dgx.cpu path) against what the reference's
own epoch end computed (tests/golden/seg_metrics.npz, recorded by
make_metrics_goldens.py from main_partseg_dist.calculate_shape_IoU and
sklearn's accuracy_score / balanced_accuracy_score). compute() divides the
same integers in the same arithmetic, so every comparison is an equality."""
import numpy as np
import pytest
import torch

from conftest import load_golden


@pytest.fixture(scope="module")
def gold():
    return load_golden("seg_metrics.npz")


def _set(gold, name):
    return tuple(torch.from_numpy(gold[f"{name}_{k}"].astype(np.int64)) for k in ("pred", "seg", "label"))


def _metrics(gold, name, capacity=None, **kw):
    from dgx import metrics
    start = gold["part_start"] if name == "all" else np.zeros_like(gold["part_start"])   # class_choice: labels from 0
    B = gold[f"{name}_seg"].shape[0]
    return metrics.SegMetrics(50, capacity=B if capacity is None else capacity, part_start=start,
                              part_count=gold["part_count"], **kw)


def _check(gold, name, r):
    assert r["shape_ious"].dtype == np.float64
    assert np.array_equal(r["shape_ious"], gold[f"{name}_shape_ious"])
    assert r["acc"] == float(gold[f"{name}_acc"])
    assert r["avg_acc"] == float(gold[f"{name}_avg_acc"])
    assert r["count"] == gold[f"{name}_seg"].shape[0]


def sem_iou_numpy(pred_np, seg_np, n, visual=False):
    """The six lines of the reference's calculate_sem_IoU (main_semseg.py:47-61) for n classes."""
    I_all, U_all = np.zeros(n), np.zeros(n)
    for idx in range(seg_np.shape[0]):
        for sem in range(n):
            I_all[sem] += np.sum(np.logical_and(pred_np[idx] == sem, seg_np[idx] == sem))
            U_all[sem] += np.sum(np.logical_or(pred_np[idx] == sem, seg_np[idx] == sem))
    if visual:
        for sem in range(n):
            if U_all[sem] == 0:
                I_all[sem] = U_all[sem] = 1
    with np.errstate(invalid="ignore"):
        return I_all / U_all


@pytest.mark.parametrize("name", ["all", "one"])
def test_fixture_properties(gold, name):
    """The fixture holds the branches it was built for."""
    ious = gold[f"{name}_shape_ious"]
    pred, seg = gold[f"{name}_pred"], gold[f"{name}_seg"]
    assert ious.shape == (seg.shape[0],) and seg.shape[1] == 129
    if name == "all":
        assert set(gold["all_label"].tolist()) == set(range(16))
        assert ious[0] == 1.0 and (pred[0] == seg[0]).all()                     # a perfect shape
        assert not np.isin([33, 35], np.concatenate([pred[16], seg[16]])).any()   # U == 0 parts
        assert (pred == 49).any() and not (seg == 49).any()                     # a class in pred only
        assert 0.7 < float(gold["all_acc"]) < 0.9
    else:
        assert (gold["one_label"] == 4).all() and seg.max() == 3


@pytest.mark.parametrize("name", ["all", "one"])
def test_host_path_equals_reference(gold, name):
    pred, seg, label = _set(gold, name)
    m = _metrics(gold, name)
    m.update(pred, seg, label)
    _check(gold, name, m.compute())
    # 7 uneven updates, labels as (B, 1) as the loaders give them, int32 ids
    m.reset()
    B = seg.shape[0]
    cuts = [0, 1, 3, 4, 5, 6, 8, B] if B < 12 else [0, 1, 3, 10, 11, 20, 33, B]
    for a, b in zip(cuts[:-1], cuts[1:]):
        m.update(pred[a:b].int(), seg[a:b].int(), label[a:b].view(-1, 1))
    _check(gold, name, m.compute())


def test_logits_take_the_loss_heads_argmax(gold):
    """Logits in both layouts give the state of their arg-max; ties go to the
    smallest class, a NaN is never a maximum (csrc/ce_row.h)."""
    from dgx import cpu, metrics
    pred, seg, label = _set(gold, "all")
    B, P = seg.shape
    g = torch.Generator().manual_seed(5)
    logits = torch.randint(0, 4, (B, 50, P), generator=g).float()      # 4 levels: many ties
    logits[0, 0, :7] = float("nan")
    logits[1, 3, :7] = float("nan")
    logits[2, :, 0] = float("-inf")
    want = cpu.seg_argmax(logits)
    first_max = (logits[3] == logits[3].max(dim=0)[0]).float().argmax(dim=0)
    assert torch.equal(want[3], first_max)
    assert (want[0, :7] == 0).all() and (want[2, 0] == 0) and not (want[1, :7] == 3).any()
    states = []
    for x in (logits, logits.permute(0, 2, 1).contiguous().permute(0, 2, 1), want):
        m = _metrics(gold, "all")
        m.update(x, seg, label)
        states.append(m._buf.clone())
    assert torch.equal(states[0], states[2]) and torch.equal(states[1], states[2])
    # (M, C) rows: the classification geometry, no categories
    m2, m3 = metrics.SegMetrics(50), metrics.SegMetrics(50)
    m2.update(logits.permute(0, 2, 1).reshape(-1, 50), seg.reshape(-1))
    m3.update(want.reshape(-1), seg.reshape(-1))
    assert torch.equal(m2.confusion, m3.confusion) and int(m2.confusion.sum()) == B * P
    assert m2.compute()["count"] == 1 and m2.compute()["shape_ious"].shape == (0,)


def test_sem_iou(gold):
    from dgx import metrics
    g = torch.Generator().manual_seed(11)
    seg = torch.randint(0, 12, (5, 300), generator=g)                  # class 12 in neither: U == 0
    pred = torch.where(torch.rand(5, 300, generator=g) < 0.3, torch.randint(0, 12, (5, 300), generator=g), seg)
    m = metrics.SegMetrics(13)
    for b in range(5):                                                  # per room, as the semseg loop feeds it
        m.update(pred[b:b + 1], seg[b:b + 1])
    for visual in (False, True):
        want = sem_iou_numpy(pred.numpy(), seg.numpy(), 13, visual)
        got = m.compute(visual=visual)["sem_iou"]
        assert got.dtype == np.float64 and np.array_equal(got, want, equal_nan=True)
        assert (got[12] == 1.0) if visual else np.isnan(got[12])
        conv = metrics.calculate_sem_IoU(pred.numpy(), seg.numpy(), visual=visual)
        assert isinstance(conv, np.ndarray) and np.array_equal(conv, want, equal_nan=True)


def test_convenience_shape_iou(gold):
    """The reference's signature and return type: a list of np.float64."""
    from dgx import metrics
    for name, choice in (("all", None), ("one", "chair")):
        got = metrics.calculate_shape_IoU(gold[f"{name}_pred"], gold[f"{name}_seg"],
                                          gold[f"{name}_label"].reshape(-1, 1), choice)
        assert isinstance(got, list) and all(isinstance(v, np.float64) for v in got)
        assert got == gold[f"{name}_shape_ious"].tolist()
        assert np.mean(got) == np.mean(gold[f"{name}_shape_ious"].tolist())


def test_invalid_and_overflow_raise_and_reset_clears(gold):
    pred, seg, label = _set(gold, "all")
    m = _metrics(gold, "all")
    bad_seg = seg.clone()
    bad_seg[0, 0], bad_seg[1, 1], bad_seg[2, 2] = -1, 50, 2 ** 40
    bad_label = label.clone()
    bad_label[3] = 16
    m.update(pred, bad_seg, bad_label)
    assert int(m.state[1]) == 4 and int(m.confusion.sum()) == seg.numel() - 3
    with pytest.raises(ValueError, match="invalid=4"):
        m.compute()
    m.reset()
    m.update(pred, seg, label)
    _check(gold, "all", m.compute())
    small = _metrics(gold, "all", capacity=5)
    small.update(pred[:3], seg[:3], label[:3])
    small.update(pred[3:6], seg[3:6], label[3:6])
    assert int(small.state[2]) == 1 and int(small.confusion.sum()) == 6 * seg.shape[1]
    with pytest.raises(ValueError, match="overflow=1"):
        small.compute()
    small.reset()
    small.update(pred[:5], seg[:5], label[:5])
    assert np.array_equal(small.compute()["shape_ious"], gold["all_shape_ious"][:5])


def test_limits():
    from dgx import _native, metrics
    assert _native.lib().dgx_seg_metrics_max_classes() == metrics.MAX_CLASSES == 128
    with pytest.raises(ValueError, match="128"):
        metrics.SegMetrics(129)
    metrics.SegMetrics(128)
    with pytest.raises(ValueError):
        metrics.SegMetrics(50, part_start=[0, 48], part_count=[2, 3])   # 48 + 3 > 50
    with pytest.raises(ValueError, match="part_start"):
        metrics.SegMetrics(50).update(torch.zeros(2, 4, dtype=torch.int64), torch.zeros(2, 4, dtype=torch.int64),
                                      label=torch.zeros(2, dtype=torch.int64))


def test_loss_sum_is_the_fp32_running_sum():
    from dgx import metrics
    m = metrics.SegMetrics(4)
    ids = torch.zeros(3, 5, dtype=torch.int64)
    losses = torch.tensor([0.1, 1e-8, 3.3, 7e3], dtype=torch.float32)
    want = torch.zeros((), dtype=torch.float32)
    for v in losses:
        m.update(ids, ids, loss=v)
        want = want + v
    r = m.compute()
    assert r["loss_sum"] == float(want) and r["count"] == 12 and r["acc"] == 1.0
