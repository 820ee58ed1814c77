"""Bit comparison of PositionEmbedding's edge MLP across two trees:
`python tools/emlp_bitcmp.py OUT.pt` runs the stage (dgx.edgemlp.edge_mlp2 and
the dgx::edge_mlp2 op) over a matrix of small cases — every forward / backward
branch, precision decision, BatchNorm configuration and gradient layout — with
the build of the tree this file lies in, and saves each case's output, gradients
and both BNs' buffers; `--compare A.pt B.pt` lists every tensor that differs and
exits non-zero if any does."""
import os
import sys

import torch
from torch import nn

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "dgcnn.pytorch_amd"))


def _convs(cin, c1, c2, momentum, track):
    def block(ci, co):
        bn = nn.BatchNorm2d(co, momentum=momentum, track_running_stats=track)
        with torch.no_grad():
            bn.weight.normal_(0.0, 1.0)   # both signs: the max over k follows sign(gamma)
            bn.bias.normal_(0.0, 0.1)
            if track:
                bn.running_mean.normal_(0.0, 0.1)
                bn.running_var.uniform_(0.5, 1.5)
                bn.num_batches_tracked.fill_(3)
        return nn.Sequential(nn.Conv2d(ci, co, 1, bias=False), bn, nn.LeakyReLU(0.2))
    return block(2 * cin, c1).cuda(), block(c1, c2).cuda()


# name, mode, (B, N, k), then what differs from: input C = 3, widths 64 -> 128, both BNs training,
# x.requires_grad, a (B, C2, N)-contiguous gradient
CASES = [
    ("bf16_fused", "bf16", (2, 256, 20), {}),
    ("bf16_c2_64", "bf16", (3, 256, 10), {"c2": 64}),
    ("bf16_partial_tile", "bf16", (3, 128, 7), {}),
    ("bf16_b1_odd_n", "bf16", (1, 300, 33), {}),
    # k > 64 is beyond the gather / max-over-k / scatter kernels: the stage refuses it, and the refusal is compared
    ("bf16_k72", "bf16", (1, 160, 72), {}),
    # unfused forward with the bf16 conv2 GEMM's statistics epilogue, LDS GEMM backward
    ("bf16_c1_128", "bf16", (2, 128, 12), {"c1": 128}),
    ("bf16_c1_128_bn2_eval", "bf16", (2, 128, 12), {"c1": 128, "eval": (False, True)}),
    ("bf16_c1_32", "bf16", (2, 128, 12), {"c1": 32}),
    ("bf16_cin32", "bf16", (2, 256, 20), {"cin": 32}),
    ("bf16_compact", "bf16", (2, 2048, 33), {"c1": 128, "tall": True}),
    ("fp32", "fp32", (2, 256, 20), {}),
    ("fp32_partial_tile", "fp32", (3, 128, 7), {}),
    ("fp32_cin32", "fp32", (2, 256, 20), {"cin": 32}),
    ("fp32_split", "fp32_split", (2, 256, 20), {}),
    ("autocast_fp16", "fp32", (2, 256, 20), {"autocast": torch.float16}),
    ("autocast_bf16", "fp32", (2, 256, 20), {"autocast": torch.bfloat16}),
    ("bn_eval_bf16", "bf16", (2, 256, 20), {"eval": (True, True)}),
    ("bn_eval_fp32", "fp32", (2, 256, 20), {"eval": (True, True)}),
    ("bn1_eval_bn2_train", "bf16", (2, 256, 20), {"eval": (True, False)}),
    ("bn_cumulative_bf16", "bf16", (2, 256, 20), {"momentum": None}),
    ("bn_cumulative_fp32", "fp32", (2, 256, 20), {"momentum": None}),
    ("bn_untracked", "bf16", (2, 256, 20), {"track": False}),
    ("grad_channel_major", "fp32", (2, 256, 20), {"grad": "cm"}),
    ("grad_point_major_bf16", "bf16", (2, 256, 20), {"grad": "pm"}),
    ("grad_point_major_fp32", "fp32", (2, 256, 20), {"grad": "pm"}),
    ("knn_src", "bf16", (2, 256, 20), {"cin": 9, "knn_src": True}),
    ("x_no_grad", "bf16", (2, 256, 20), {"xgrad": False}),
    ("x_view", "bf16", (2, 256, 20), {"xview": True}),
    ("unfused_bwd", "bf16", (2, 256, 20), {"fused_bwd": False}),
    ("op_bf16", "bf16", (2, 256, 20), {"op": True}),
    ("op_fp32_cumulative", "fp32", (2, 256, 20), {"op": True, "momentum": None}),
]


def _op_call(x, k, conv1, conv2, bf16):
    """torch.ops.dgx.edge_mlp2 called directly; the updated statistics come back as outputs."""
    import dgx.library  # noqa: F401  (registers the ops)
    (cv1, bn1, a1), (cv2, bn2, a2) = conv1, conv2
    bufs = [[bn.running_mean, bn.running_var, bn.num_batches_tracked] for bn in (bn1, bn2)]
    res = torch.ops.dgx.edge_mlp2(
        x, k, cv1.weight, bn1.weight, bn1.bias, *bufs[0], cv2.weight, bn2.weight, bn2.bias, *bufs[1],
        [bn1.training, bn2.training], [bn1.track_running_stats, bn2.track_running_stats],
        [-1.0 if bn.momentum is None else float(bn.momentum) for bn in (bn1, bn2)], [bn1.eps, bn2.eps],
        [a1.negative_slope, a2.negative_slope], bf16, None)
    return res[0], dict(zip(("bn1.running_mean", "bn1.running_var", "bn1.num_batches_tracked", "bn2.running_mean",
                             "bn2.running_var", "bn2.num_batches_tracked"), res[1:]))


def _run_case(name, mode, shape, o, res):
    from dgx import _native as nat, edgemlp as EM, precision as prec
    B, N, k = shape
    cin, c1, c2 = o.get("cin", 3), o.get("c1", 64), o.get("c2", 128)
    if o.get("tall"):   # the per-tile BN partials are tall enough for the pre-reduce before the finalize
        assert nat.lib().dgx_gemm_stats_rows(B * N * k) > 1024 and c1 != 64, "case must reach the partial pre-reduce"
    torch.manual_seed(B * N + k + cin + c1 + c2)   # cases of one shape (fp32 / fp32_split) see the same data
    conv1, conv2 = _convs(cin, c1, c2, o.get("momentum", 0.1), o.get("track", True))
    ev = o.get("eval", (False, False))
    conv1[1].train(not ev[0])
    conv2[1].train(not ev[1])
    if o.get("xview"):   # a channel slice of a wider, point-major buffer
        x = torch.randn(B, N, cin + 5, device="cuda")[:, :, 2:2 + cin].permute(0, 2, 1)
    else:
        x = torch.randn(B, cin, N, device="cuda")
    x.requires_grad_(o.get("xgrad", True))
    knn_src = x.detach()[:, 6:9] if o.get("knn_src") else None
    g = (torch.randn(B, N, c2, device="cuda").permute(0, 2, 1) if o.get("grad") == "pm"
         else torch.randn(B, c2, N, device="cuda"))
    prec.set(mode)
    old = EM.FUSED_BWD
    EM.FUSED_BWD = o.get("fused_bwd", True)
    stats = None
    y = None
    try:
        if o.get("op"):
            y, stats = _op_call(x, k, conv1, conv2, mode == "bf16")
        elif o.get("autocast") is not None:
            with torch.autocast("cuda", dtype=o["autocast"]):
                y = EM.edge_mlp2(x, k, conv1, conv2, knn_src=knn_src)
        else:
            y = EM.edge_mlp2(x, k, conv1, conv2, knn_src=knn_src)
        y.backward(g)
    except RuntimeError as e:   # a shape the stage refuses: both trees must refuse it
        print(f"{name}: RuntimeError: {e}")
        res[f"{name}.raised"] = torch.tensor([0 if y is None else 1])   # in the forward / in the backward
        return
    finally:
        EM.FUSED_BWD = old
        prec.set("fp32")
    torch.cuda.synchronize()
    res[f"{name}.y"] = y.detach().cpu()
    if x.grad is not None:
        res[f"{name}.grad.x"] = x.grad.cpu()
    for tag, seq in (("conv1", conv1), ("conv2", conv2)):
        for n, p in seq.named_parameters():
            res[f"{name}.grad.{tag}.{n}"] = p.grad.cpu()
        if stats is None:
            for n, b in seq.named_buffers():
                res[f"{name}.buf.{tag}.{n}"] = b.cpu()
    for n, t in (stats or {}).items():
        res[f"{name}.buf.{n}"] = t.cpu()


def run(path):
    res = {}
    for name, mode, shape, o in CASES:
        _run_case(name, mode, shape, o, res)
    assert [n for n in res if n.endswith(".raised")] == ["bf16_k72.raised"]
    # "fp32_split" keeps meaning exact fp32 for this stage
    for n in [n for n in res if n.startswith("fp32.")]:
        assert torch.equal(res[n], res["fp32_split." + n[5:]]), n
    torch.save(res, path)
    print(f"{len(CASES)} cases, {len(res)} tensors -> {path}")


def compare(a, b):
    A, B = torch.load(a, weights_only=True), torch.load(b, weights_only=True)
    bad = [n for n in sorted(set(A) | set(B)) if n not in A or n not in B or not torch.equal(A[n], B[n])]
    print(f"{len(CASES)} cases, {len(A)} tensors, {len(bad)} differ" + (": " + ", ".join(bad) if bad else ""))
    return 1 if bad else 0


if __name__ == "__main__":
    if sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    run(sys.argv[1])
