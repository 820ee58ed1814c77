"""The loss head: label-smoothed cross entropy (reference loss.py:4-21) as two
C-ABI calls (dgx_smoothed_ce_fwd / dgx_smoothed_ce_bwd, csrc/loss.hip) in place
of torch's zeros_like, scatter, two scaled copies, log_softmax, product, row
sum, mean and their backward. The incoming gradient (a GradScaler's scale) is
read on the device; nothing here synchronises with the host, so forward and
backward can be captured in a HIP graph.

Logits are taken as they are in two layouts: class-contiguous (M, C) — also
the (B, C, N) view of a (B, N, C) tensor — and point-contiguous (B, C, N), the
partseg Net's own output, which spares the scripts' transpose copy. Any other
strides are made contiguous first. Host tensors take dgx.cpu.
"""
import torch
from torch.autograd.function import once_differentiable

from . import _native as N
from . import cpu
from .cpu import ce_weights  # noqa: F401  (the public name of the weights helper)

_DTYPES = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}   # DGX_CE_F32 / _F16 / _BF16


def _geometry(x):
    """(B, C, N, sb, sc, sn) of logits in one of the kernels' layouts, or None."""
    if x.dim() == 2:
        M, C = x.shape
        return (1, C, M, M * C, 1, C) if x.is_contiguous() else None
    B, C, P = x.shape
    sb, sc, sn = x.stride()
    if x.is_contiguous() or (sc == 1 and (P == 1 or sn == C) and (B == 1 or sb == P * C)):
        return B, C, P, sb, sc, sn
    return None


class _SmoothedCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, w_true, w_other, return_pred):
        geo = _geometry(logits)
        if geo is None:
            logits = logits.contiguous()
            geo = _geometry(logits)
        B, C, P = geo[:3]
        M = B * P
        target = target.contiguous()
        lib = N.lib()
        dev = logits.device
        lse = torch.empty(M, device=dev, dtype=torch.float64)
        loss = torch.empty((), device=dev, dtype=torch.float32)
        pred = torch.empty(target.shape, device=dev, dtype=torch.int64) if return_pred else None
        ws_bytes = lib.dgx_smoothed_ce_workspace_bytes(M)
        ws = torch.empty(ws_bytes // 8, device=dev, dtype=torch.float64)
        N.check(lib.dgx_smoothed_ce_fwd(N.ptr(logits, *_DTYPES), _DTYPES[logits.dtype], *geo,
                                        N.ptr(target, N.I64, N.I32), int(target.dtype == torch.int64), w_true,
                                        w_other, N.ptr(lse, N.F64), N.f32(loss), N.ptr(pred, N.I64),
                                        N.ptr(ws, N.F64), ws_bytes, N.stream_of(logits)), "smoothed_ce_fwd")
        ctx.save_for_backward(logits, target, lse)
        ctx.geo, ctx.weights = geo, (w_true, w_other)
        if return_pred:
            ctx.mark_non_differentiable(pred)
            return loss, pred
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, g, *_):
        logits, target, lse = ctx.saved_tensors
        if g.dtype != torch.float32:
            g = g.float()
        g = g.contiguous()
        dlogits = torch.empty_strided(logits.shape, logits.stride(), device=logits.device, dtype=logits.dtype)
        N.check(N.lib().dgx_smoothed_ce_bwd(N.ptr(logits, *_DTYPES), _DTYPES[logits.dtype], *ctx.geo,
                                            N.ptr(target, N.I64, N.I32), int(target.dtype == torch.int64),
                                            *ctx.weights, N.ptr(lse, N.F64), N.f32(g), N.ptr(dlogits, *_DTYPES),
                                            N.stream_of(logits)), "smoothed_ce_bwd")
        return dlogits, None, None, None, None


def smoothed_cross_entropy(logits, target, smoothing=True, eps=0.2, return_pred=False):
    """Mean over rows of the cross entropy of ``logits`` against the
    reference's smoothed target: 1 - eps on the labelled class, eps / (C - 1)
    on every other, both rounded as the reference rounds them in the logits'
    dtype (``ce_weights``); ``smoothing=False``: plain cross entropy.

    logits (M, C) with target (M,), or (B, C, N) with (B, N) — F.cross_entropy's
    convention; fp32, fp16 or bf16; labels int64 or int32. The result has the
    reference's dtype: fp32 for fp32 logits and for half logits under autocast,
    else the logits' dtype (computed in fp64, rounded once to fp32 and from
    there). A label outside [0, C) gives a NaN loss and NaN in that row of the
    gradient instead of the reference's device assert. With ``return_pred``
    also returns each row's arg-max class (int64, target's shape; the smallest
    index among equal maxima) from the same pass.
    """
    if logits.dim() not in (2, 3) or target.shape != logits.shape[:1] + logits.shape[2:]:
        raise ValueError(f"dgx: logits {tuple(logits.shape)} want (M, C) with (M,) labels or (B, C, N) with (B, N), "
                         f"got labels {tuple(target.shape)}")
    if cpu.is_cpu(logits) and cpu.is_cpu(target):
        return cpu.smoothed_cross_entropy(logits, target, smoothing, eps, return_pred)
    N.require_device(logits, target)
    w_true, w_other = ce_weights(logits.dtype, logits.shape[1], smoothing, eps)   # ValueError for C < 2
    if torch.compiler.is_compiling():   # traced as torch's own expression; a custom op is not registered for it
        return cpu.smoothed_cross_entropy(logits, target, smoothing, eps, return_pred)
    if logits.dtype not in _DTYPES:
        raise RuntimeError(f"dgx: the loss head takes fp32, fp16 or bf16 logits, got {logits.dtype}")
    if logits.numel() == 0:
        raise ValueError("dgx: the loss head needs at least one row")
    out = _SmoothedCE.apply(logits, target, w_true, w_other, return_pred)
    loss, pred = out if return_pred else (out, None)
    if logits.dtype != torch.float32 and not torch.is_autocast_enabled(logits.device.type):
        loss = loss.to(logits.dtype)
    return (loss, pred) if return_pred else loss
