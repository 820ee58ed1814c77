"""What the per-step metrics bookkeeping costs at the part-segmentation geometry
(BASELINE cfg4: 32 clouds x 2048 points x 50 classes, fp16 logits in the Net's
own (B, C, N) layout), behind a stream that is kept busy, so that a drain of
the stream shows up as the device idling while the host enqueues again:

  work_only       --work GEMMs (4096^3, fp16) per step and nothing else: the stand-in for a step
  reference_tail  the GEMMs, then the reference's own lines (main_partseg_dist.py:255-274, :259):
                  permute(0, 2, 1).contiguous(), max(dim=2)[1], seg.cpu().numpy(),
                  pred.detach().cpu().numpy(), appends to two lists, loss.item()
  seg_metrics     the GEMMs, then SegMetrics.update(logits, seg, label, loss): one launch, no copy

Each figure is wall-clock us per step over a window of --steps steps that ends
in a device synchronise, the median (with the smallest and largest) of --reps
windows after --warmup steps; the three forms are timed alternately, window by
window. ``tail_us`` is a form's median minus work_only's. The device time of the
update alone is taken by HIP events around a window of replays of a graph of 16
captured updates (one after the other; a graph of one launch is bound by the
host's replay call), per update, with the bytes it must read (logits, labels)
and the GB/s they imply, on two kinds of data: ``partseg`` (labels inside each shape's part range, the
arg-max right for 80 % of the points and any of the 50 classes for the rest:
what a trained Net gives, and what the wall-clock forms use) and ``random``
(labels and logits independent, so that each shape meets all 2500 (true, pred)
pairs: the most entries a workgroup can have to add to the global table).
Last, compute() is timed (host clock, it synchronises) on an epoch of 2874
shapes, ShapeNetPart's test split.

  python tools/metrics_bench.py [--steps 100] [--warmup 10] [--reps 7] [--work 8] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "dgcnn.pytorch_amd")]
import torch  # noqa: E402

B, C, N = 32, 50, 2048
EPOCH_SHAPES = 2874
CHAIN = 16   # updates captured in one graph: a replay of one launch is bound by the host's replay call


def summary(xs):
    return {"median": round(statistics.median(xs), 2), "min": round(min(xs), 2), "max": round(max(xs), 2)}


def wall_window(fn, steps):
    """Wall-clock us per step of ``steps`` calls and the synchronise that ends them."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / steps


def event_window(fn, steps):
    """Device us per step by HIP events around ``steps`` calls."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--work", type=int, default=8, help="4096^3 fp16 GEMMs enqueued per step")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from dgx import metrics
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    label = torch.randint(0, 16, (B, 1), generator=gen)
    start = torch.tensor(metrics.SHAPENET_PART_START)[label]
    count = torch.tensor(metrics.SHAPENET_PART_COUNT)[label]
    seg = start + (torch.rand(B, N, generator=gen) * count).long()
    peak = torch.where(torch.rand(B, N, generator=gen) < 0.8, seg, torch.randint(0, C, (B, N), generator=gen))
    logits = torch.randn(B, C, N, generator=gen).scatter_add_(1, peak.unsqueeze(1), torch.full((B, 1, N), 8.0))
    logits, seg, label = logits.half().to(dev), seg.to(dev), label.to(dev)
    random_logits = (torch.randn(B, C, N, generator=gen) * 2).half().to(dev)
    random_seg = torch.randint(0, C, (B, N), generator=gen).to(dev)
    loss = torch.rand((), generator=gen).to(dev)
    ga = torch.randn(4096, 4096, generator=gen).half().to(dev)
    gb = torch.randn(4096, 4096, generator=gen).half().to(dev)
    gc = torch.empty_like(ga)
    m = metrics.SegMetrics(C, capacity=1 << 20, part_start=metrics.SHAPENET_PART_START,
                           part_count=metrics.SHAPENET_PART_COUNT, device=dev)
    lists = [[], []]
    total = [0.0]

    def work():
        for _ in range(a.work):
            torch.mm(ga, gb, out=gc)

    def reference_tail():
        work()
        seg_pred = logits.permute(0, 2, 1).contiguous()
        total[0] += loss.item()
        pred = seg_pred.max(dim=2)[1]
        seg_np = seg.cpu().numpy()
        pred_np = pred.detach().cpu().numpy()
        lists[0].append(seg_np.reshape(-1))
        lists[1].append(pred_np.reshape(-1))

    def seg_metrics():
        work()
        m.update(logits, seg, label, loss)

    forms = {"work_only": work, "reference_tail": reference_tail, "seg_metrics": seg_metrics}
    for fn in forms.values():
        for _ in range(a.warmup):
            fn()
    wall = {k: [] for k in forms}
    for _ in range(a.reps):
        for k, fn in forms.items():
            wall[k].append(wall_window(fn, a.steps))
            lists[0].clear(), lists[1].clear()
    wall = {k: summary(v) for k, v in wall.items()}
    overflowed = int(m.state[2])   # the capacity covers every timed shape
    m.reset()

    # the update alone on the device: replays of CHAIN captured launches
    replay = {}
    for kind, x, y in (("partseg", logits, seg), ("random", random_logits, random_seg)):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            m.update(x, y, label, loss)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(CHAIN):
                m.update(x, y, label, loss)
        for _ in range(a.warmup):
            graph.replay()
        replay[kind] = summary([event_window(graph.replay, a.steps) / CHAIN for _ in range(a.reps)])
        replay[kind]["table_entries_per_shape"] = round(
            sum(float((torch.bincount(y[b] * C + x[b].float().argmax(0), minlength=C * C) > 0).sum())
                for b in range(B)) / B, 1)
        m.reset()
    nbytes = logits.numel() * 2 + seg.numel() * 8 + label.numel() * 8

    # the epoch end: 2874 shapes, then compute()
    epoch = metrics.SegMetrics(C, capacity=EPOCH_SHAPES, part_start=metrics.SHAPENET_PART_START,
                               part_count=metrics.SHAPENET_PART_COUNT, device=dev)
    pred = logits.max(dim=1)[1]
    compute_us = []
    for _ in range(a.reps):
        epoch.reset()
        for at in range(0, EPOCH_SHAPES, B):
            n = min(B, EPOCH_SHAPES - at)
            epoch.update(pred[:n], seg[:n], label[:n])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = epoch.compute()
        compute_us.append((time.perf_counter() - t0) * 1e6)
    assert r["shape_ious"].shape == (EPOCH_SHAPES,) and r["count"] == EPOCH_SHAPES

    base = wall["work_only"]["median"]
    res = {"bench": "metrics_bench", "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "shape": {"B": B, "C": C, "N": N}, "steps": a.steps, "warmup": a.warmup, "reps": a.reps,
           "work_gemms": a.work, "wall_us_per_step": wall,
           "tail_us": {k: round(wall[k]["median"] - base, 2) for k in ("reference_tail", "seg_metrics")},
           "update_graph_replay_us": replay, "update_bytes": nbytes,
           "update_gbs": {k: round(nbytes / v["median"] * 1e-3, 1) for k, v in replay.items()},
           "compute_us_2874_shapes": summary(compute_us), "overflowed": overflowed}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
