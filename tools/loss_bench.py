"""Loss-head time at the part-segmentation geometry (BASELINE cfg4: 32 clouds x
2048 points x 50 classes), forward + backward, from the network's (B, C, N)
output to the gradient of that output, in fp32 and in fp16 under autocast with
a GradScaler-scaled backward:

  torch_script    the reference script's own steps with torch ops: the transpose copy
                  (permute(0, 2, 1).contiguous()), its label-smoothed cross entropy launch for
                  launch (zero fill, scatter, the soft target's elementwise ops, log_softmax,
                  product, row sum, mean) and the arg-max pass (max(dim=2)[1])
  engine_script   the same script with loss.cross_entropy bound to the engine: transpose copy,
                  dgx.loss on the class-contiguous copy, arg-max pass
  engine_rows     dgx.loss alone on class-contiguous (M, C) logits (no copy, no arg-max)
  engine_planes   dgx.loss on the (B, C, N) output itself with return_pred=True (no copy, the
                  arg-max from the same pass)
  engine_*_fwd    the two engine forms, forward only (no_grad)

Each form is timed eagerly (bound by the host's enqueue for kernels this
small) and as one captured step replayed as a HIP graph (the device side).
Each figure is the median over --reps windows of --steps steps after --warmup
steps, with the smallest and largest window, by HIP events around the window;
the forms are timed alternately, window by window. The bytes each engine launch
must move (logits, labels, lse, gradient) are computed from the shapes, and the
GB/s they imply over the graph-replay times is reported with them. One JSON
line, also written to --out.

  python tools/loss_bench.py [--steps 200] [--warmup 20] [--reps 7] [--out profiles/loss_bench_mi355x.json]

With --trace nothing is timed: torch_script, engine_rows and engine_planes run
30 eager steps each in both dtypes, the workload for a kernel trace taken in a
run of its own (profiles/loss_kernel_stats_mi355x.csv holds its per-kernel
statistics):

  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o loss -- python tools/loss_bench.py --trace
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "dgcnn.pytorch_amd")]
import torch  # noqa: E402

B, C, N = 32, 50, 2048
HBM_GBS = 6300.0   # achievable HBM rate of an MI355X, GB/s


def torch_smoothed_ce(logits, labels, smooth=0.2):
    """Label-smoothed cross entropy of (M, C) logits with torch ops, launch for launch what the
    reference's loss runs (a zero fill, a scatter, five elementwise ops for the soft target in the
    logits' dtype, log_softmax, a product, a row sum, a mean, a negation), with the same roundings."""
    n_class = logits.shape[1]
    hit = torch.zeros_like(logits)
    hit.scatter_(1, labels.unsqueeze(1), 1.0)
    target = (1.0 - smooth) * hit + smooth * (1.0 - hit) / (n_class - 1)
    logp = torch.log_softmax(logits, dim=1)
    return (target * logp).sum(dim=1).mean().neg()


def window(fn, steps):
    """Device us per step by HIP events around ``steps`` calls."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / steps


def summary(xs):
    return {"median": round(statistics.median(xs), 2), "min": round(min(xs), 2), "max": round(max(xs), 2)}


def graphed(fn):
    """``fn`` captured in a HIP graph after eager runs on a side stream; returns its replay."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        keep = fn()

    def replay(graph=graph, keep=keep):   # the outputs live in the graph's pool
        graph.replay()
    return replay


def compare(forms, a):
    for fn in forms.values():
        for _ in range(a.warmup):
            fn()
    ev = {k: [] for k in forms}
    for _ in range(a.reps):
        for k, fn in forms.items():
            ev[k].append(window(fn, a.steps))
    return {k: summary(v) for k, v in ev.items()}


def forms_for(dtype, dev):
    """{name: step function} for one dtype; each returns what it computed."""
    from dgx.loss import smoothed_cross_entropy
    from loss import cross_entropy
    half = dtype != torch.float32
    gen = torch.Generator().manual_seed(0)
    out = (torch.randn(B, C, N, generator=gen) * 2).to(dtype).to(dev).requires_grad_(True)   # the network's output
    rows = out.detach().permute(0, 2, 1).contiguous().view(-1, C).requires_grad_(True)
    seg = torch.randint(0, C, (B, N), generator=gen).to(dev)
    scaler = torch.amp.GradScaler("cuda", enabled=half)
    scaler.scale(torch.zeros((), device=dev))   # the scale tensor exists before any capture

    def amp():
        return torch.autocast("cuda", dtype=torch.float16, enabled=half)

    def script(loss_fn):
        def step():
            with amp():
                seg_pred = out.permute(0, 2, 1).contiguous()
                loss = loss_fn(seg_pred.view(-1, C), seg.view(-1, 1).squeeze())
            pred = seg_pred.max(dim=2)[1]
            return torch.autograd.grad(scaler.scale(loss), out)[0], pred
        return step

    def engine_rows():
        with amp():
            loss = smoothed_cross_entropy(rows, seg.view(-1))
        return torch.autograd.grad(scaler.scale(loss), rows)[0]

    def engine_planes():
        with amp():
            loss, pred = smoothed_cross_entropy(out, seg, return_pred=True)
        return torch.autograd.grad(scaler.scale(loss), out)[0], pred

    def engine_rows_fwd():
        with torch.no_grad(), amp():
            return smoothed_cross_entropy(rows, seg.view(-1))

    def engine_planes_fwd():
        with torch.no_grad(), amp():
            return smoothed_cross_entropy(out, seg, return_pred=True)

    return {"torch_script": script(torch_smoothed_ce), "engine_script": script(cross_entropy),
            "engine_rows": engine_rows, "engine_planes": engine_planes, "engine_rows_fwd": engine_rows_fwd,
            "engine_planes_fwd": engine_planes_fwd}


def launch_bytes(es):
    """Bytes each engine launch must move at (B, C, N): logits of ``es`` bytes, int64 labels, fp64 lse."""
    M = B * N
    fwd = M * C * es + M * 8 + M * 8
    return {"fwd": fwd, "fwd_with_pred": fwd + M * 8, "bwd": 2 * M * C * es + M * 8 + M * 8}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", action="store_true", help="run the forms untimed, for a kernel trace")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    if a.trace:
        for dtype in (torch.float32, torch.float16):
            forms = forms_for(dtype, dev)
            for name in ("torch_script", "engine_rows", "engine_planes"):
                for _ in range(30):
                    forms[name]()
            torch.cuda.synchronize()
        return
    res = {"bench": "loss_bench", "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "shape": {"B": B, "C": C, "N": N}, "steps": a.steps, "warmup": a.warmup, "reps": a.reps,
           "unit": "us per step (HIP events)", "hbm_gbs": HBM_GBS, "runs": {}}
    for name, dtype in (("fp32", torch.float32), ("fp16_autocast_gradscaler", torch.float16)):
        forms = forms_for(dtype, dev)
        eager = compare(forms, a)
        graph = compare({k: graphed(fn) for k, fn in forms.items()}, a)
        nbytes = launch_bytes(4 if dtype == torch.float32 else 2)
        rates = {}
        for form, with_pred in (("engine_rows", False), ("engine_planes", True)):
            fwd_us = graph[form + "_fwd"]["median"]
            both_us = graph[form]["median"]
            fb = nbytes["fwd_with_pred" if with_pred else "fwd"]
            rates[form] = {
                "fwd_gbs": round(fb / fwd_us * 1e-3, 1),
                "fwd_bwd_gbs": round((fb + nbytes["bwd"]) / both_us * 1e-3, 1),
                "fwd_bwd_fraction_of_hbm": round((fb + nbytes["bwd"]) / both_us * 1e-3 / HBM_GBS, 4),
            }
        res["runs"][name] = {
            "eager_us": eager, "graph_us": graph, "launch_bytes": nbytes, "graph_rates": rates,
            "speedup_vs_torch_script": {
                mode: {k: round(t["torch_script"]["median"] / t[k]["median"], 2)
                       for k in ("engine_script", "engine_planes")}
                for mode, t in (("eager", eager), ("graph", graph))},
        }
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
