"""Segmentation and classification metrics accumulated on the device.

The reference's loops end every step on the host (main_partseg_dist.py:259-274:
``seg_pred.max(dim=2)[1]`` on a transposed copy, two blocking ``.cpu().numpy()``
copies, lists that grow by B * N labels, ``loss.item()``) and compute the
epoch's numbers there in Python loops. ``SegMetrics.update`` is one launch of
dgx_seg_metrics_update (csrc/metrics.hip) that adds the batch to integer state
on the device — the (C, C) confusion table, each shape's part intersections and
unions, the loss sum — without a copy, an allocation or a synchronisation, so
it can be captured in a HIP graph with the step. ``compute()`` is the one copy
to the host per epoch; it divides there, in the reference's own arithmetic, so
its numbers equal the reference's bit for bit.

Host tensors take dgx.cpu (same state, torch ops).
"""
import numpy as np
import torch

from . import _native as N
from . import cpu
from .loss import _geometry   # (B, C, N, sb, sc, sn) of logits in one of the two layouts, or None

MAX_CLASSES = 128      # dgx_seg_metrics_max_classes(): a 128 x 128 uint32 table is the kernel's 64 KiB of LDS
STATE_WORDS = 8        # DGX_SEG_STATE_WORDS: cursor, invalid, overflow, count, ticket
_CURSOR, _INVALID, _OVERFLOW, _COUNT = 0, 1, 2, 3
_DTYPES = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2, torch.int64: 3, torch.int32: 4}
_GUARD_WORD = 0x5A5A5A5A5A5A5A5A

# ShapeNetPart (reference main_partseg_dist.py:39-40): parts of each of the 16 categories
SHAPENET_PART_COUNT = (4, 2, 2, 4, 4, 3, 3, 2, 4, 2, 6, 2, 3, 3, 3, 3)
SHAPENET_PART_START = (0, 4, 6, 8, 12, 16, 19, 22, 24, 28, 30, 36, 38, 41, 44, 47)


class SegMetrics:
    """Accumulator of the reference's segmentation / classification metrics.

    ``num_classes``: C, 2 to 128. ``part_start`` / ``part_count`` (the
    reference's ``index_start`` / ``seg_num``; all-zero starts for a
    ``class_choice`` run) and ``capacity`` (shapes per epoch) are needed only
    for per-shape IoUs, i.e. when ``update`` gets ``label``. All state lives
    in one device buffer made here; ``update`` allocates nothing.
    """

    def __init__(self, num_classes, capacity=0, part_start=None, part_count=None, device=None, _guard=0):
        C = int(num_classes)
        if C > MAX_CLASSES:
            raise ValueError(f"dgx: SegMetrics counts at most {MAX_CLASSES} classes (the kernel's LDS table), "
                             f"got {C}")
        if C < 2:
            raise ValueError(f"dgx: SegMetrics needs at least 2 classes, got {C}")
        if (part_start is None) != (part_count is None):
            raise ValueError("dgx: part_start and part_count come together")
        self.num_classes = C
        self.capacity = int(capacity)
        self.device = torch.device("cpu" if device is None else device)
        if part_count is not None:
            start = torch.as_tensor(part_start, dtype=torch.int32).reshape(-1)
            count = torch.as_tensor(part_count, dtype=torch.int32).reshape(-1)
            if start.numel() != count.numel() or count.numel() == 0:
                raise ValueError("dgx: part_start and part_count need one entry per category")
            if int(start.min()) < 0 or int(count.min()) < 0 or int((start + count).max()) > C:
                raise ValueError(f"dgx: a part range lies outside the {C} classes")
            self.max_parts = max(int(count.max()), 1)
            self.part_start, self.part_count = start.to(self.device), count.to(self.device)
        else:
            if self.capacity:
                raise ValueError("dgx: a capacity needs part_start and part_count")
            self.max_parts, self.part_start, self.part_count = 1, None, None
        if self.capacity < 0:
            raise ValueError("dgx: negative capacity")
        # one int64 buffer: confusion | state | loss_sum (fp32 in one word) | iu (int32) | nparts (int32),
        # each region whole words; _guard words of a sentinel around every region (for tests)
        self._guard = int(_guard)
        self._words = (C * C, STATE_WORDS, 1, self.capacity * self.max_parts, (self.capacity + 1) // 2)
        self._buf = torch.full((sum(self._words) + self._guard * (len(self._words) + 1),),
                               _GUARD_WORD if self._guard else 0, dtype=torch.int64, device=self.device)
        self._regions, self._guards = self._carve(self._buf)
        self.confusion, self.state, self.loss_sum, self.iu, self.nparts = self._views(self._regions)
        self.reset()

    def _carve(self, buf):
        regions, guards, at, g = [], [], 0, self._guard
        for w in self._words:
            guards.append(buf[at:at + g])
            regions.append(buf[at + g:at + g + w])
            at += g + w
        guards.append(buf[at:at + g])
        return regions, guards

    def _views(self, r):
        C = self.num_classes
        return (r[0].view(C, C), r[1], r[2].view(torch.float32)[:1],
                r[3].view(torch.int32).view(self.capacity, self.max_parts, 2), r[4].view(torch.int32)[:self.capacity])

    def reset(self):
        """Zero the state (device memsets, no synchronisation)."""
        if self._guard:
            for r in self._regions:
                r.zero_()
        else:
            self._buf.zero_()

    def _guards_intact(self):
        return all(bool((g == _GUARD_WORD).all()) for g in self._guards)

    def update(self, scores_or_pred, seg, label=None, loss=None):
        """Add one batch. ``scores_or_pred``: logits (B, C, N) (class- or
        point-contiguous, e.g. the partseg Net's output as it is or its
        ``permute(0, 2, 1)``) or (M, C), fp32 / fp16 / bf16, whose arg-max is
        taken with the loss head's rule; or class ids (B, N) / (M,), int64 or
        int32. ``seg``: true classes of the same points. ``label``: each
        shape's category, (B,) or (B, 1), for per-shape IoUs. ``loss``: a
        scalar tensor added to ``loss_sum`` in fp32. Returns nothing."""
        x = scores_or_pred
        C = self.num_classes
        if x.is_floating_point():
            if x.dim() == 2:
                x = x.t().unsqueeze(0)   # (M, C) as B = 1, N = M, class-contiguous
            if x.dim() != 3 or x.shape[1] != C:
                raise ValueError(f"dgx: logits {tuple(scores_or_pred.shape)} want (B, {C}, N) or (M, {C})")
            B, P = x.shape[0], x.shape[2]
        else:
            if x.dim() == 1:
                x = x.unsqueeze(0)
            if x.dim() != 2:
                raise ValueError(f"dgx: class ids {tuple(scores_or_pred.shape)} want (B, N) or (M,)")
            B, P = x.shape
        if seg.numel() != B * P or B * P == 0:
            raise ValueError(f"dgx: {tuple(seg.shape)} labels for {B} x {P} points")
        seg = seg.reshape(B, P)
        if label is not None:
            if self.part_count is None:
                raise ValueError("dgx: per-shape IoUs need part_start and part_count")
            if label.numel() != B:
                raise ValueError(f"dgx: {label.numel()} categories for {B} shapes")
            label = label.reshape(B)
        if loss is not None and loss.numel() != 1:
            raise ValueError("dgx: loss is a scalar")
        tensors = [t for t in (x, seg, label, loss) if t is not None]
        host = self.device.type == "cpu" and all(cpu.is_cpu(t) for t in tensors)
        if host or torch.compiler.is_compiling():   # traced as torch's own expression, as dgx.loss is
            cpu.seg_metrics_update(x, seg, label, self.part_start, self.part_count, self.confusion, self.iu,
                                   self.nparts, self.state, loss, self.loss_sum)
            return
        N.require_device(*tensors, self._buf)
        if x.is_floating_point():
            if x.dtype not in _DTYPES:
                raise RuntimeError(f"dgx: SegMetrics takes fp32, fp16 or bf16 logits, got {x.dtype}")
            geo = _geometry(x)
            if geo is None:   # any other strides: one copy
                x = x.contiguous()
                geo = _geometry(x)
        else:
            x, geo = self._ids(x), (B, C, P, 0, 0, 0)
        seg, label = self._ids(seg), self._ids(label)
        if loss is not None and loss.dtype != torch.float32:
            loss = loss.detach().float()
        N.check(N.lib().dgx_seg_metrics_update(
            N.ptr(x, *_DTYPES), _DTYPES[x.dtype], *geo, N.ptr(seg, N.I64, N.I32), int(seg.dtype == torch.int64),
            N.ptr(label, N.I64, N.I32), int(label is not None and label.dtype == torch.int64),
            N.i32(self.part_start), N.i32(self.part_count), 0 if self.part_count is None else self.part_count.numel(),
            N.ptr(self.confusion, N.I64), N.i32(self.iu), N.i32(self.nparts), self.capacity, self.max_parts,
            N.ptr(self.state, N.I64), N.f32(loss), N.f32(self.loss_sum), N.stream_of(x)), "seg_metrics_update")

    @staticmethod
    def _ids(t):
        if t is None:
            return None
        if t.dtype not in (torch.int64, torch.int32):
            t = t.long()
        return t.contiguous()

    def compute(self, visual=False):
        """Copy the state to the host (the one synchronisation) and finish
        there in the reference's arithmetic. Returns a dict:

        acc         trace / total (sklearn accuracy_score)
        avg_acc     mean of diag / rowsum over classes that occur in ``seg``
                    (sklearn balanced_accuracy_score)
        shape_ious  float64 array, one per recorded shape in update order:
                    np.mean over the shape's parts of 1 if U == 0 else I / float(U)
                    (calculate_shape_IoU)
        sem_iou     per class diag / (rowsum + colsum - diag) (calculate_sem_IoU
                    over everything seen); ``visual``: 0 / 0 counts as 1 / 1
        loss_sum    the fp32 sum of the losses passed, as a float
        count       samples seen
        confusion   the (C, C) int64 table, [true][pred]

        Raises ValueError if invalid labels or categories were met or shapes
        did not fit the capacity."""
        confusion, state, loss_sum, iu, nparts = (t.numpy() for t in self._views(self._carve(self._buf.cpu())[0]))
        loss_sum = float(loss_sum[0])
        if state[_INVALID] or state[_OVERFLOW]:
            raise ValueError(f"dgx: SegMetrics met invalid={int(state[_INVALID])} labels or categories outside "
                             f"their range and overflow={int(state[_OVERFLOW])} shapes beyond capacity "
                             f"{self.capacity}")
        diag, rows, cols = np.diag(confusion), confusion.sum(axis=1), confusion.sum(axis=0)
        total = int(rows.sum())
        seen = rows > 0
        with np.errstate(divide="ignore", invalid="ignore"):
            acc = float(np.float64(int(diag.sum())) / np.float64(total))
            avg_acc = float(np.mean(diag[seen] / rows[seen])) if seen.any() else float("nan")
            inter, union = diag.astype(np.float64), (rows + cols - diag).astype(np.float64)
            if visual:
                empty = union == 0
                inter[empty], union[empty] = 1, 1
            sem_iou = inter / union
        shapes = min(int(state[_CURSOR]), self.capacity)
        shape_ious = np.empty(shapes, np.float64)
        for s in range(shapes):
            part_ious = [1 if u == 0 else i / float(u) for i, u in iu[s, :nparts[s]].astype(np.int64)]
            shape_ious[s] = np.mean(part_ious) if part_ious else np.nan
        return {"acc": acc, "avg_acc": avg_acc, "shape_ious": shape_ious, "sem_iou": sem_iou, "loss_sum": loss_sum,
                "count": int(state[_COUNT]), "confusion": confusion.copy()}


def _tensor(a, device=None):
    t = a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a))
    return t if device is None else t.to(device)


def calculate_shape_IoU(pred, seg, label, class_choice, visual=False):
    """The reference's calculate_shape_IoU (main_partseg_dist.py:63-84) on
    device or host tensors (or arrays): the list of each shape's mean part IoU
    over ShapeNetPart's part table. ``pred`` / ``seg``: (B, N) class ids;
    ``label``: the shapes' categories; with ``class_choice`` the parts are
    ``range(seg_num[label[0]])`` for every shape. One update, one compute.
    ``visual`` only changes how the reference squeezes ``label``; any shape
    of ``label`` is taken here."""
    pred = _tensor(pred)
    dev = pred.device
    seg, label = _tensor(seg, dev), _tensor(label, dev).reshape(-1)
    if class_choice:
        label = label[:1].expand(pred.shape[0])
        start = (0,) * len(SHAPENET_PART_START)
    else:
        start = SHAPENET_PART_START
    m = SegMetrics(SHAPENET_PART_START[-1] + SHAPENET_PART_COUNT[-1], capacity=pred.shape[0], part_start=start,
                   part_count=SHAPENET_PART_COUNT, device=dev)
    m.update(pred, seg, label)
    return list(m.compute()["shape_ious"])


def calculate_sem_IoU(pred, seg, visual=False, num_classes=13):
    """The reference's calculate_sem_IoU (main_semseg.py:47-61): per-class
    I / U over all the rooms of ``pred`` / ``seg`` (B, N), a float64 array of
    ``num_classes`` (S3DIS: 13); ``visual``: 0 / 0 counts as 1."""
    pred = _tensor(pred)
    m = SegMetrics(num_classes, device=pred.device)
    m.update(pred, _tensor(seg, pred.device))
    return m.compute(visual=visual)["sem_iou"]
