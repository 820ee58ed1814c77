"""What building a training batch costs at the part-segmentation geometry
(run.sh's batch: 24 clouds x 2048 points, ShapeNetPart_Augmented train), the
host path of the reference's loop against dgx.loader:

  host_path      data.ShapeNetPart_Augmented + DataLoader(num_workers=0, shuffle, drop_last) + the one-hot
                 loop (main_partseg_dist.py:241-244) + three H2D copies + permute(0, 2, 1).contiguous(), as the
                 reference's loop does it (:236-250): wall-clock ms per batch over a window of --steps batches
                 that ends in a device synchronise
  loader_eager   DeviceLoader.next_into(): device us per batch by HIP events around --steps launches
  loader_graph   the same launch captured, CHAIN launches per graph: device us per batch by HIP events around
                 --steps / CHAIN replays (a graph of one launch measures the host's replay call)
  shuffled_*     both again with the point shuffle on top (not this dataset's policy: the cost of the LDS sort)

each the median (with the smallest and largest) of --reps windows after a warm-up window. The dataset is the
first --items clouds of the split; without the reference's file (DGX_SYNTHETIC_DATA=1) the synthetic clouds are
generated once and held in a TensorDataset, as the reference's file holds them, so that the host path indexes
tensors and does not generate. ``batch_bytes`` is what the kernel must move for one batch: the clouds and part
labels it reads (fp32, int32) and the clouds, int64 part labels, labels and one-hot rows it writes.

  python tools/loader_bench.py [--steps 100] [--reps 7] [--items 2400] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "dgcnn.pytorch_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

B, N, NCAT = 24, 2048, 16
CHAIN = 20


def summary(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--items", type=int, default=2400)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.steps % CHAIN or a.items < a.steps * B:
        ap.error(f"--steps is a multiple of {CHAIN} and --items at least steps x {B}")
    if not torch.cuda.is_available():
        sys.exit("loader_bench: no ROCm device")
    import data
    from dgx.loader import DeviceLoader
    dev = torch.device("cuda:0")
    if not os.path.exists(os.path.join(data.DATA_DIR, "shapenetpart_train_dataset.pt")):
        os.environ["DGX_SYNTHETIC_DATA"] = "1"
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ds = data.ShapeNetPart_Augmented("trainval")
    synthetic = ds.SYNTHETIC
    points, label, seg = ds.raw(slice(0, a.items))
    points, label, seg = torch.from_numpy(points), torch.from_numpy(label).view(-1, 1), torch.from_numpy(seg)
    ds.data = torch.utils.data.TensorDataset(points, label, seg)     # the reference's file: tensors, indexed per item

    # the reference's loop
    loader = torch.utils.data.DataLoader(ds, batch_size=B, shuffle=True, drop_last=True, num_workers=0)

    def host_window():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        batches = 0
        for pc, lab, sg in loader:
            onehot = np.zeros((len(lab), NCAT))              # float64, filled row by row, then cast: the loop's cost
            for row, cat in enumerate(lab):
                onehot[row, cat] = 1
            onehot = torch.from_numpy(onehot.astype(np.float32))
            pc, onehot, sg = pc.to(dev), onehot.to(dev), sg.to(dev)
            pc = pc.permute(0, 2, 1).contiguous()
            batches += 1
            if batches == a.steps:
                break
        torch.cuda.synchronize()
        assert batches == a.steps and pc.shape == (B, 3, N)
        return (time.perf_counter() - t0) * 1e3 / batches

    host_window()
    host_ms = summary([host_window() for _ in range(a.reps)])

    def event_window(fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.steps

    def device_loader(shuffle_points):
        """Eager and replayed us per batch of the device loader on the same items."""
        dl = DeviceLoader(points, seg.to(torch.int32), label.to(torch.int32), batch_size=B, shuffle=True,
                          shuffle_points=shuffle_points, augment="random3", num_categories=NCAT, drop_last=True,
                          device=dev)

        def eager_window(epoch):
            dl.set_epoch(epoch)
            return event_window(dl.next_into, a.steps)

        eager_window(0)
        eager = summary([eager_window(1 + r) for r in range(a.reps)])
        dl.set_epoch(0)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            dl.next_into()
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(CHAIN):
                dl.next_into()

        def graph_window(epoch):
            dl.set_epoch(epoch)
            return event_window(graph.replay, a.steps // CHAIN)

        graph_window(0)
        replay = summary([graph_window(1 + r) for r in range(a.reps)])
        state = dl.state()       # raises on invalid ids or launches past the epoch's end
        assert state["cursor"] == a.steps * B
        return eager, replay

    eager_us, graph_us = device_loader(False)               # ShapeNetPart_Augmented's own policy
    shuffled_eager_us, shuffled_graph_us = device_loader(True)   # with the point shuffle (the sort in LDS) on top

    nbytes = B * N * (3 * 4 + 4) + B * N * (3 * 4 + 8) + B * (4 + 8 + NCAT * 4)
    res = {"bench": "loader_bench", "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "shape": {"B": B, "N": N, "C": 3, "items": a.items}, "synthetic": synthetic, "steps": a.steps,
           "reps": a.reps, "chain": CHAIN, "host_path_ms_per_batch": host_ms, "loader_eager_us_per_batch": eager_us,
           "loader_graph_us_per_batch": graph_us, "shuffled_eager_us_per_batch": shuffled_eager_us,
           "shuffled_graph_us_per_batch": shuffled_graph_us, "batch_bytes": nbytes,
           "loader_graph_gbs": round(nbytes / graph_us["median"] * 1e-3, 1)}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
