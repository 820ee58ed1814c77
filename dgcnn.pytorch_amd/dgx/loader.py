"""Device-resident datasets and batches assembled in one launch.

The reference builds every batch on the host (main_partseg_dist.py:151-156,
``num_workers=0``): per item up to three small torch ops in a random order
(data.py:353-364), the default collate, a Python loop for the one-hot label
(:241-244), three H2D copies, then ``permute(0, 2, 1)`` and ``.contiguous()``.
A ShapeNetPart split is about 340 MB and an S3DIS area a few GB: either fits in
HBM many times over. ``DeviceLoader`` keeps the dataset there and builds each
batch with one launch of dgx_batch_assemble (csrc/loader.hip): sample
selection, point shuffle, the reference's augmentations, the (B, C, N) layout,
``seg - seg_start_index`` and the one-hot label — without a copy from the host
or a synchronisation, so ``next_into`` can be captured in a HIP graph with the
model, the loss, the optimizer and the metrics.

The random draws are Philox4x32-10 words keyed by the seed and counted by
(item, epoch, stream, block) — include/dgx.h states the layout — so a cloud's
augmentation depends on (seed, epoch, item) alone: not on the batch size, the
world size, its place in the batch or eager launch versus graph replay.

Host tensors take dgx.cpu (the same words, a stable argsort, the same fp32
operation sequence).
"""
import ctypes

import torch
from torch.utils.data.distributed import DistributedSampler

from . import _native as N
from . import cpu

MAX_SHUFFLE_POINTS = 4096   # dgx_batch_max_points(): the shuffle sorts 8 bytes per point in 32 KiB of LDS
STATE_WORDS = 8             # DGX_BATCH_STATE_WORDS: cursor, epoch, invalid, overrun, batches, ticket
_CURSOR, _EPOCH, _INVALID, _OVERRUN, _BATCHES = 0, 1, 2, 3, 4
_GUARD_WORD = 0x5A5A5A5A5A5A5A5A


class _Outputs:
    """The outputs of one launch, carved from one int64 buffer (one allocation
    per batch), each region whole words; ``guard`` words of a sentinel around
    every region (for tests)."""

    def __init__(self, B, C, n, ncat, seg, label, debug, noise, guard, device):
        sizes = (("data", B * C * n, torch.float32, (B, C, n)),
                 ("seg", B * n * 2 if seg else 0, torch.int64, (B, n)),
                 ("label", B * 2 if label else 0, torch.int64, (B,)),
                 ("onehot", B * ncat, torch.float32, (B, ncat)),
                 ("perm", B * n if debug else 0, torch.int32, (B, n)),
                 ("params", B * 16 if debug else 0, torch.float32, (B, 16)),
                 ("noise", B * n * 3 if debug and noise else 0, torch.float32, (B, n, 3)))
        words = [(cells + 1) // 2 for _, cells, _, _ in sizes]
        self.buf = torch.full((sum(words) + guard * (len(words) + 1),), _GUARD_WORD if guard else 0,
                              dtype=torch.int64, device=device)
        self.guards, at = [], 0
        for (name, cells, dtype, shape), w in zip(sizes, words):
            self.guards.append(self.buf[at:at + guard])
            region = self.buf[at + guard:at + guard + w]
            numel = cells // 2 if dtype == torch.int64 else cells
            setattr(self, name, region.view(dtype)[:numel].view(shape) if cells else None)
            at += guard + w
        self.guards.append(self.buf[at:at + guard])

    def intact(self):
        return all(bool((g == _GUARD_WORD).all()) for g in self.guards)


class DeviceLoader:
    """Batches of a dataset held on ``device``.

    ``points`` (n, P, C) fp32; ``seg`` (n, P) and ``label`` (n,) or (n, 1)
    integers, optional. Iterating yields ``(data (B, C, N), label, seg)`` —
    ``(data, onehot (B, num_categories), seg, label)`` when ``num_categories``
    is set — with ``data`` fp32 contiguous, ``label`` / ``seg`` int64 (absent
    ones None) and ``seg`` already minus ``seg_start_index``. ``num_points``
    takes each cloud's first N points (before the shuffle, the reference's
    ``[:num_points]``). ``shuffle`` / ``seed`` / ``num_replicas`` / ``rank`` /
    ``drop_last`` are torch's ``DistributedSampler``'s, which ``set_epoch``
    itself runs: this rank's item order is the reference's by construction.
    The last batch of an epoch may be partial (the reference's DataLoader
    keeps it). ``shuffle_points`` (default: ``shuffle``) permutes each cloud's
    points; ``augment``: "none", "translate" (ModelNet40 train) or "random3"
    (ShapeNetPart_Augmented train); both need C == 3. The stored dataset is
    never changed.
    """

    def __init__(self, points, seg=None, label=None, batch_size=1, num_points=None, shuffle=True,
                 shuffle_points=None, augment="none", seg_start_index=0, num_categories=None, drop_last=False,
                 seed=0, num_replicas=1, rank=0, device=None, _guard=0, _debug=False, _force=None):
        points = torch.as_tensor(points)
        if points.dim() != 3 or points.shape[0] == 0:
            raise ValueError(f"dgx: points {tuple(points.shape)} want (n_items, P, C)")
        self.device = torch.device(points.device if device is None else device)
        n, P, C = points.shape
        self.n_items, self.P, self.C = n, P, C
        self.num_points = P if num_points is None else int(num_points)
        if not 1 <= self.num_points <= P:
            raise ValueError(f"dgx: num_points {self.num_points} outside [1, {P}]")
        self.batch_size = int(batch_size)
        if self.batch_size < 1:
            raise ValueError("dgx: batch_size < 1")
        self.shuffle = bool(shuffle)
        self.shuffle_points = self.shuffle if shuffle_points is None else bool(shuffle_points)
        order, switches = _force if _force is not None else (None, None)
        self.flags = cpu.batch_flags(self.shuffle_points, augment, order, switches)
        self.augment = augment
        if augment != "none" and C != 3:
            raise ValueError(f"dgx: augmentation needs 3 channels, got {C}")
        if self.shuffle_points and self.num_points > MAX_SHUFFLE_POINTS:
            raise ValueError(f"dgx: the point shuffle takes at most {MAX_SHUFFLE_POINTS} points per cloud (the "
                             f"kernel's LDS), got {self.num_points}")
        if seg is not None and tuple(seg.shape) != (n, P):
            raise ValueError(f"dgx: seg {tuple(seg.shape)} for points {tuple(points.shape)}")
        if label is not None and label.numel() != n:
            raise ValueError(f"dgx: {label.numel()} labels for {n} items")
        self.num_categories = 0 if num_categories is None else int(num_categories)
        if self.num_categories and label is None:
            raise ValueError("dgx: a one-hot label needs label")
        self.seg_start_index = int(seg_start_index)
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.points = points.to(self.device, torch.float32).contiguous()
        self.seg = None if seg is None else torch.as_tensor(seg).to(self.device, torch.int32).contiguous()
        self.label = None if label is None else torch.as_tensor(label).reshape(n).to(self.device,
                                                                                       torch.int32).contiguous()
        # the sampler of the reference's prepare_dl; both numbers given: no process group is asked for
        self.sampler = DistributedSampler(range(n), num_replicas=int(num_replicas), rank=int(rank),
                                          shuffle=self.shuffle, seed=int(seed), drop_last=bool(drop_last))
        self.n_epoch = self.sampler.num_samples
        self.order = torch.zeros(max(self.n_epoch, 1), dtype=torch.int32, device=self.device)
        self._state = torch.zeros(STATE_WORDS, dtype=torch.int64, device=self.device)
        self._guard, self._debug = int(_guard), bool(_debug)
        self._fixed = None
        self.epoch = 0
        self._pos = None     # the host's mirror of the cursor; None: set_epoch has not run

    def __len__(self):
        return -(-self.n_epoch // self.batch_size)

    def set_epoch(self, epoch):
        """This rank's item ids of ``epoch`` (``DistributedSampler``'s), the
        epoch number and a zero cursor into the fixed device buffers: two
        copies from the host, no synchronisation."""
        self.epoch = int(epoch)
        self.sampler.set_epoch(self.epoch)
        self._write_order(torch.tensor(list(self.sampler), dtype=torch.int32))

    def _write_order(self, ids):
        self.order[:self.n_epoch].copy_(ids)
        self._state[:2].copy_(torch.tensor([0, self.epoch], dtype=torch.int64))
        self._pos = 0

    def __iter__(self):
        if self._pos != 0:
            self.set_epoch(self.epoch)
        while self._pos < self.n_epoch:
            b = min(self.batch_size, self.n_epoch - self._pos)
            yield self._tuple(self._launch(self._outputs(b), b))

    def next_into(self):
        """The next batch into fixed output tensors (made at the first call;
        the same objects every time): one launch of ``batch_size`` workgroups,
        no allocation, the cursor on the device — capturable in a HIP graph,
        and a replay follows a ``set_epoch`` made between replays. Slots past
        the epoch's end are not written and counted in ``overrun``."""
        if self._pos is None:
            self.set_epoch(self.epoch)
        if self._fixed is None:
            self._fixed = self._outputs(self.batch_size)
        return self._tuple(self._launch(self._fixed, self.batch_size))

    def state(self, check=True):
        """The device's state words as a dict (one copy to the host, the only
        synchronisation of the loader). Raises ValueError if item ids or labels
        outside their range were met or launches ran past the epoch's end."""
        s = self._state.cpu().tolist()
        out = {"cursor": s[_CURSOR], "epoch": s[_EPOCH], "invalid": s[_INVALID], "overrun": s[_OVERRUN],
               "batches": s[_BATCHES]}
        if check and (out["invalid"] or out["overrun"]):
            raise ValueError(f"dgx: DeviceLoader met invalid={out['invalid']} item ids or labels outside their range "
                             f"and overrun={out['overrun']} clouds asked for past the epoch's {self.n_epoch}")
        return out

    def _outputs(self, b):
        return _Outputs(b, self.C, self.num_points, self.num_categories, self.seg is not None,
                        self.label is not None, self._debug, self.augment != "none", self._guard, self.device)

    def _tuple(self, o):
        if self.num_categories:
            return o.data, o.onehot, o.seg, o.label
        return o.data, o.label, o.seg

    def _launch(self, o, b):
        args = (self.n_items, self.P, self.C)
        if self.device.type == "cpu":
            cpu.batch_assemble(self.points, self.seg, self.label, self.order[:self.n_epoch], self._state, b,
                               self.num_points, self.seg_start_index, self.num_categories, self.seed, self.flags,
                               o.data, o.seg, o.label, o.onehot, o.perm, o.params, o.noise)
        else:
            N.require_device(self.points, o.buf)
            N.check(N.lib().dgx_batch_assemble(
                N.f32(self.points), N.i32(self.seg), N.i32(self.label), *args, N.i32(self.order), self.n_epoch,
                N.ptr(self._state, N.I64), b, self.num_points, self.seg_start_index, self.num_categories,
                ctypes.c_uint64(self.seed), self.flags, N.f32(o.data), N.ptr(o.seg, N.I64), N.ptr(o.label, N.I64),
                N.f32(o.onehot), N.i32(o.perm), N.f32(o.params), N.f32(o.noise), N.stream_of(self.points)),
                "batch_assemble")
        self._pos = min(self._pos + b, self.n_epoch)
        self.last = o
        return o
