"""PositionEmbedding's per-edge MLP: reference models/layers.py:45-52.

Reference:
    e  = get_graph_feature(x, k)                      (B, 2C, N, k)   layers.py:45
    h1 = conv1(e)   Conv2d(2C,64) + BN2d + LeakyReLU   per edge        layers.py:17-18, 48
    t  = conv2(h1)  Conv2d(64,128) + BN2d + LeakyReLU  per edge        layers.py:19-20, 49
    t  = t.max(dim=-1)[0]                             (B, 128, N)     layers.py:52

Engine: one autograd node over the C++ schedule (libdgx_torch.so,
dgx_host::edge_mlp2_forward / edge_mlp2_backward through dgx.schedule — the
same code dgx::edge_mlp2 runs; the launch schedule and its kernels are
described there). This module keeps the entry checks, the kNN call (so the
kNN-sharing scope and ``knn_src`` stay in Python), the precision decision —
read once at entry and carried into the backward — and the debug capture.
"""
import torch

from . import _native as nat
from . import cpu
from . import precision as prec
from . import schedule as S
from .edgeconv import debug_capture
from .ops import knn_raw, reduction_order

# bf16 mode, C1 = 64 / C2 = 128 (PositionEmbedding): one backward kernel for
# conv2 + LReLU/BN1 (dgx_edge_mlp_fused_bwd_bf16: z2, dZ2, dH1 and dW2 in
# registers / LDS, h1 rebuilt from PQ), so the forward does not store h1.
# False keeps the unfused GEMM path (dZ2 / dH1 / dW2 GEMMs over a stored h1).
FUSED_BWD = True


def _fused_bwd_ok(bf16, C1, C2, k):
    return FUSED_BWD and bf16 and C1 == 64 and C2 == 128 and k <= 64


def _capture(saved, bf16):
    """Debug capture (tests): the stage's routing inputs under "emlp" — the kNN
    graph, conv1's decomposed PQ and BN1 affine (h1's LeakyReLU signs follow
    from them), conv2's selected pre-BN value / slot and BN2 affine. ``fused``:
    h1 was built as fma(a1, P_j, fma(a1, Q_i, b1)) and fed to the MFMA in bf16
    (emlp_fwd_kernel); otherwise as fma(a1, P_j + Q_i, b1) (mlp_h1_kernel)."""
    dbg = debug_capture()
    if dbg is not None:
        s = S.EmlpSaved(*saved)
        dbg["emlp"] = {"idx": s.idx.clone(), "PQ": s.PQ.clone(), "a1": s.scale1.clone(), "b1": s.shift1.clone(),
                       "ysel": s.ysel.clone(), "arg": s.arg.clone(), "a2": s.scale2.clone(), "b2": s.shift2.clone(),
                       "bf16": bf16, "fused": s.Z2.numel() == 0}


def knn_graph(x, knn_src, k):
    """int32 (B, N, k) neighbours of the stage, found on x or on ``knn_src`` (layers.py:45 -> dgcnn.py:21)."""
    kx = x if knn_src is None else knn_src.float()
    return knn_raw(kx, k, order=reduction_order(kx), out_dtype=torch.int32)


class _EdgeMLP2(torch.autograd.Function):
    @staticmethod
    @prec.no_autocast
    def forward(ctx, x, k, bn, need_grad, knn_src, d, *params):
        x = x.float()
        out, saved = S.edge_mlp2_forward(x, knn_graph(x, knn_src, k), k, params, bn, d.bf16, need_grad, FUSED_BWD)
        _capture(saved, d.bf16)
        ctx.meta = (k, tuple(x.shape), bn.evals, bn.groups, bn.slopes, d)
        if need_grad:
            # the BN state and conv2's bf16 copies are made here and stay on the node as they are
            n = S.EMLP_FIELDS.index("scale1")
            ctx.state = saved[n:]
            ctx.save_for_backward(*saved[:n], params[0], params[3])
        return out

    @staticmethod
    @prec.no_autocast
    def backward(ctx, dout):
        k, shape, evals, groups, slopes, d = ctx.meta
        *saved, w1, w2 = ctx.saved_tensors
        dx, *grads = S.edge_mlp2_backward(dout, saved + list(ctx.state), w1, w2, shape, k, evals, groups, slopes, d,
                                          ctx.needs_input_grad[0])
        return (dx if dx.numel() else None, None, None, None, None, None, *grads)


def edge_mlp2(x, k, conv1, conv2, training=None, knn_src=None):
    """max_k conv2(conv1(get_graph_feature(x, k))) for conv1/conv2 =
    nn.Sequential(Conv2d(1x1, bias=False), BatchNorm2d, LeakyReLU) as
    PositionEmbedding builds them (reference models/layers.py:17-20, 45-52).
    Returns (B, C2, N) contiguous, as the reference's max over k.
    ``training`` is accepted for call compatibility only (dgx.bn: each BN
    module's own flags decide batch vs running statistics). ``knn_src``:
    optional (B, C', N) tensor the neighbours are searched on instead of x
    (upstream's dim9 semseg graph: kNN on the normalised xyz channels).
    GEMM precision: bf16 operands in the bf16 mode or under bf16 autocast
    (``precision.effective()`` at entry), exact fp32 otherwise ("fp32_split"
    included). A host tensor takes the CPU path (dgx.cpu)."""
    if cpu.is_cpu(x):
        return cpu.edge_mlp2(x, k, conv1, conv2, training, knn_src)
    nat.require_device(x)
    if torch.compiler.is_compiling():   # traced as one dgx::edge_mlp2 op (dgx.library)
        from . import library
        return library.edge_mlp2_call(x, k, conv1, conv2, knn_src)
    if x.dtype != torch.float32:
        x = x.float()
    (cv1, bn1, act1), (cv2, bn2, act2) = (conv1[0], conv1[1], conv1[2]), (conv2[0], conv2[1], conv2[2])
    if bn1.weight is None or bn2.weight is None:
        raise NotImplementedError("dgx edge MLP expects affine BatchNorm (as the reference builds it)")
    c1w, c2w = cv1.weight.shape[0], cv2.weight.shape[0]
    if c1w < 8 or c1w % 8 or 256 % (c1w // 4) or c2w % 8:
        raise NotImplementedError("dgx edge MLP: conv1 width a multiple of 8 dividing 1024, conv2 width a "
                                  "multiple of 8 (PositionEmbedding: 64, 128)")
    if cv1.weight.shape[1] != 2 * x.shape[1]:
        raise RuntimeError(f"dgx edge MLP: conv1 expects {cv1.weight.shape[1]} edge channels, input has C={x.shape[1]}")
    params = (cv1.weight, bn1.weight, bn1.bias, cv2.weight, bn2.weight, bn2.bias)
    need_grad = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params))
    if knn_src is not None:
        nat.require_device(knn_src)
        knn_src = knn_src.detach()
        if knn_src.shape[0] != x.shape[0] or knn_src.shape[2] != x.shape[2]:
            raise RuntimeError("dgx edge MLP: knn_src must be (B, C', N) with the input's B and N")
    bn = S.bn_lists((bn1, bn2), (act1.negative_slope, act2.negative_slope))
    return _EdgeMLP2.apply(x, k, bn, need_grad, knn_src, S.decide(), *params)
