"""kNN vector attention (dgx.vattn, csrc/vattn.hip) against the composed
stock-op form (dgx.cpu.vector_attention on the device: what the reference's
VectorAttention.forward launches after its projections), at run.sh's
``pointransformer`` geometry (B 24, N 2048, k 32, d_qkv 64) and at B 4:

  fwd_fused_fp32 / fwd_fused_bf16   the fused forward kernel in each operand mode (no_grad)
  fwd_composed                      the composed device forward (no_grad)
  step_fused_fp32 / step_fused_bf16 forward + the chunked-recompute backward to D, V and the 8 parameters
  step_composed                     the composed forward + torch autograd

Every figure is the median over --reps windows (with the smallest and largest)
of HIP-event time around a window of steps sized to about --window seconds
after a warm-up; the forms are timed alternately, window by window, so a drift
of the machine lands on all of them. The per-call floors of the fused kernel
are computed from the shapes: MFMA = 2 (Hp Dm + Dm H + H Dm) flops per edge over
the matrix peak of the mode (2.5 PF bf16, 157 TF fp32), gather = the D_j and V_j
rows, positions and id of every edge (528 B) over the HBM rate, i.e. as if no
gathered row were served from L2. The outputs of the forms are compared on the
timed inputs before anything is timed. One JSON line, also written to --out.

  python tools/vattn_bench.py [--reps 5] [--window 0.3] [--out profiles/vattn_bench_mi355x.json]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "dgcnn.pytorch_amd")]
import torch  # noqa: E402

DM, H, HP = 64, 256, 64
PEAK = {"bf16": 2.5e15, "fp32": 157.3e12}
HBM_BS = 6.3e12


def make(B, N, k, dev):
    torch.manual_seed(0)
    pos_mlp = torch.nn.Sequential(torch.nn.Linear(3, HP), torch.nn.ReLU(), torch.nn.Linear(HP, DM)).to(dev)
    attn_mlp = torch.nn.Sequential(torch.nn.Linear(DM, H), torch.nn.ReLU(), torch.nn.Linear(H, DM)).to(dev)
    from dgx import ops, synth
    pts = torch.from_numpy(synth.cube_clouds(B, N, 1)).to(dev).permute(0, 2, 1).contiguous()   # (B, 3, N)
    idx = ops.knn_raw(pts, k, out_dtype=torch.int32)
    D = torch.randn(B * N, DM, device=dev)
    V = torch.randn(B * N, DM, device=dev)
    return D, V, pts.view(B * N, 3), idx, pos_mlp, attn_mlp


def forms(B, N, k, dev):
    from dgx import cpu, precision as prec, vattn
    D, V, pos, idx, pos_mlp, attn_mlp = make(B, N, k, dev)
    params = cpu.vattn_params(pos_mlp, attn_mlp)
    g = torch.randn(B * N, DM, device=dev)
    Dl, Vl = D.clone().requires_grad_(True), V.clone().requires_grad_(True)

    def fused(mode, train):
        def run():
            with prec.mode(mode):
                if not train:
                    with torch.no_grad():
                        return vattn.vector_attention(D, V, pos, idx, pos_mlp, attn_mlp, 0, ids_checked=True)
                out = vattn.vector_attention(Dl, Vl, pos, idx, pos_mlp, attn_mlp, 0, ids_checked=True)
                return torch.autograd.grad(out, [Dl, Vl] + params, g)
        return run

    def composed(train):
        def run():
            if not train:
                with torch.no_grad():
                    return cpu.vector_attention(D, V, pos, idx, pos_mlp, attn_mlp, 0)
            out = cpu.vector_attention(Dl, Vl, pos, idx, pos_mlp, attn_mlp, 0)
            return torch.autograd.grad(out, [Dl, Vl] + params, g)
        return run

    return {"fwd_fused_fp32": fused("fp32", False), "fwd_fused_bf16": fused("bf16", False),
            "fwd_composed": composed(False), "step_fused_fp32": fused("fp32", True),
            "step_fused_bf16": fused("bf16", True), "step_composed": composed(True)}


def window_ms(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def bench(B, N, k, dev, reps, window):
    f = forms(B, N, k, dev)
    ref = f["fwd_composed"]()
    check = {"fwd_fused_fp32_vs_composed": rel(f["fwd_fused_fp32"](), ref),
             "fwd_fused_bf16_vs_composed": rel(f["fwd_fused_bf16"](), ref)}
    gref = f["step_composed"]()
    gfus = f["step_fused_fp32"]()
    check["step_grads_vs_composed"] = max(rel(a, b) for a, b in zip(gfus, gref))
    del ref, gref, gfus
    steps = {}
    for name, fn in f.items():   # warm-up, and the steps of a window
        fn()
        torch.cuda.synchronize()
        steps[name] = max(2, min(200, int(window * 1e3 / max(window_ms(fn, 2), 1e-3))))
    times = {name: [] for name in f}
    for _ in range(reps):
        for name, fn in f.items():
            times[name].append(window_ms(fn, steps[name]))
    E = B * N * k
    out = {"B": B, "N": N, "k": k, "edges": E, "check": check, "steps_per_window": steps,
           "ms": {n: {"median": statistics.median(t), "min": min(t), "max": max(t)} for n, t in times.items()}}
    flops = 2.0 * (HP * DM + DM * H + H * DM) * E
    out["floor_ms"] = {"mfma_bf16": flops / PEAK["bf16"] * 1e3, "mfma_fp32": flops / PEAK["fp32"] * 1e3,
                       "gather": 528.0 * E / HBM_BS * 1e3}
    med = {n: v["median"] for n, v in out["ms"].items()}
    out["speedup"] = {"fwd_fp32": med["fwd_composed"] / med["fwd_fused_fp32"],
                      "fwd_bf16": med["fwd_composed"] / med["fwd_fused_bf16"],
                      "step_fp32": med["step_composed"] / med["step_fused_fp32"],
                      "step_bf16": med["step_composed"] / med["step_fused_bf16"]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="24x2048x32,4x2048x32")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("vattn_bench: needs a ROCm device (no CPU timing)")
    dev = torch.device("cuda:0")
    res = {"bench": "vattn", "device": torch.cuda.get_device_name(0), "reps": a.reps, "shapes": []}
    for s in a.shapes.split(","):
        B, N, k = (int(v) for v in s.split("x"))
        res["shapes"].append(bench(B, N, k, dev, a.reps, a.window))
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
