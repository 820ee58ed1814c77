"""Optimizer-step and GradScaler-step time on the parameter lists of
DGCNN(emb 1024) and of the partseg Net (cfg4 arguments: k 40, emb 512, 4 heads),
gradients filled once:

  (a) one optimizer step: torch.optim.Adam(foreach=True), torch.optim.Adam(fused=True), dgx.optim.Adam,
      and one captured step replayed as a HIP graph: torch.optim.Adam(fused=True, capturable=True), dgx.optim.Adam
  (b) scaler.step(opt); scaler.update():
        torch.amp.GradScaler + torch.optim.AdamW(fused=True)
        torch.amp.GradScaler + an SGD without the GradScaler protocol (dgx_sgd_step_f32 after
            torch's unscale and found_inf.item(): dgx.optim.SGD before it had the protocol)
        dgx.optim.GradScaler + dgx.optim.AdamW

Each figure is the median over --reps windows of --steps steps after --warmup
steps, with the smallest and largest window: HIP events around the window
(device time per step) and, for (b), also the host clock around the window
ended by a synchronise — a host synchronisation inside the step shows only
there. The forms are timed alternately, window by window. One JSON line.

  python tools/optim_bench.py [--steps 200] [--warmup 20] [--reps 7]
"""
import argparse
import json
import os
import statistics
import sys
import time
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "dgcnn.pytorch_amd")]
import torch  # noqa: E402


def param_list(model, dev, seed):
    """Fresh leaf copies of a model's parameters on the device, with seeded gradients."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    out = []
    for p in model.parameters():
        q = p.detach().clone().to(dev).requires_grad_(True)
        q.grad = (torch.randn(p.shape, generator=g) * 1e-2).to(dev)
        out.append(q)
    return out


def window(fn, steps):
    """(device us per step by HIP events, host us per step by the clock around a synchronised loop)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    return e0.elapsed_time(e1) * 1e3 / steps, (t1 - t0) * 1e6 / steps


def summary(xs):
    return {"median": round(statistics.median(xs), 2), "min": round(min(xs), 2), "max": round(max(xs), 2)}


def graphed(opt):
    """One optimizer step captured in a HIP graph (after eager steps, so the state exists); returns its replay."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            opt.step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()

    def replay(keep=opt):   # the graph holds raw addresses: the optimizer (parameters, gradients, state) must outlive it
        graph.replay()
    return replay


def compare(forms, a):
    """forms: {name: step function}; alternating windows."""
    for fn in forms.values():
        for _ in range(a.warmup):
            fn()
    ev, wall = {k: [] for k in forms}, {k: [] for k in forms}
    for _ in range(a.reps):
        for k, fn in forms.items():
            d, h = window(fn, a.steps)
            ev[k].append(d)
            wall[k].append(h)
    return {k: {"event_us": summary(ev[k]), "wall_us": summary(wall[k])} for k in forms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    from dgx import optim as dopt
    from models.dgcnn import DGCNN
    from models.model_partseg import Net
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    models = {
        "DGCNN(emb=1024)": DGCNN(types.SimpleNamespace(emb_dim=1024, k=20)),
        "partseg Net (cfg4)": Net(types.SimpleNamespace(k=40, emb_dim=512, n_heads=4, n_blocks=1, ff_dims=512,
                                                        dropout=0.5, nclasses=50)),
    }

    class PlainSGD(dopt.SGD):   # dgx.optim.SGD as it was without the GradScaler protocol
        _step_supports_amp_scaling = False

    out = {"bench": "optim_bench", "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "steps": a.steps, "warmup": a.warmup, "reps": a.reps, "unit": "us per step", "lists": {}}
    for name, model in models.items():
        plist = list(model.parameters())
        res = {"tensors": len(plist), "elements": sum(p.numel() for p in plist)}
        kw = dict(lr=1e-3, weight_decay=1e-4)
        opts = {"torch_adam_foreach": torch.optim.Adam(param_list(model, dev, 1), foreach=True, **kw),
                "torch_adam_fused": torch.optim.Adam(param_list(model, dev, 1), fused=True, **kw),
                "dgx_adam": dopt.Adam(param_list(model, dev, 1), **kw)}
        forms = {k: o.step for k, o in opts.items()}
        # the eager forms are bound by the host's enqueue; one captured step replayed shows the device side
        forms["torch_adam_fused_capturable_graph"] = graphed(
            torch.optim.Adam(param_list(model, dev, 1), fused=True, capturable=True, **kw))
        forms["dgx_adam_graph"] = graphed(dopt.Adam(param_list(model, dev, 1), **kw))
        res["optimizer_step"] = compare(forms, a)

        def scaled(scaler_cls, opt):
            # the gradients are filled once and every step unscales them in place, so keep the scale at 1:
            # the work per step is the same, the values stay finite for any number of steps
            sc = scaler_cls("cuda", init_scale=1.0, growth_interval=1 << 30)
            sc.scale(torch.zeros((), device=dev))

            def fn():
                sc.step(opt)
                sc.update()
            return fn
        forms = {
            "torch_scaler+torch_adamw_fused": scaled(torch.amp.GradScaler,
                                                     torch.optim.AdamW(param_list(model, dev, 1), fused=True, **kw)),
            "torch_scaler+dgx_sgd_no_protocol": scaled(torch.amp.GradScaler,
                                                       PlainSGD(param_list(model, dev, 1), lr=1e-3, momentum=0.9,
                                                                weight_decay=1e-4)),
            "dgx_scaler+dgx_adamw": scaled(dopt.GradScaler, dopt.AdamW(param_list(model, dev, 1), **kw)),
        }
        res["scaler_step"] = compare(forms, a)
        out["lists"][name] = res
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
