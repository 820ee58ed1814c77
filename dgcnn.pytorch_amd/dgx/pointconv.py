"""Pointwise Conv(1x1) + BatchNorm + LeakyReLU on point-major features.

Replaces conv5 of reference models/dgcnn.py:74-78, 100-102: the reference
concatenates x1..x4 into (B,512,N,1) and runs Conv2d -> BatchNorm2d ->
LeakyReLU -> view(B,emb,N). Here the input is the EdgeConv chain's point-major
concat buffer (B*N, 512) as is; Z = X W^T is one engine GEMM (bf16 MFMA with
the BN statistics in its epilogue, or the fp32 MFMA GEMM in parity mode), BN
statistics / affine / LeakyReLU and the transpose to the reference's (B,emb,N)
layout are libdgx passes (pointconv.hip), issued by the C++ schedule
(csrc/dgx_torch.cpp). BN follows nn.BatchNorm rules per
module (dgx.bn: batch or running statistics by the BN's own flags, biased
batch var for normalisation, unbiased for running_var, momentum or cumulative
average).
"""
import torch

from . import _native as nat
from . import cpu
from . import precision as prec
from . import schedule as S


class _PointConvBNLReLU(torch.autograd.Function):
    """One autograd node over the C++ schedule (libdgx_torch.so:
    dgx_host::pointconv_forward / pointconv_backward, shared with the eager
    DGCNN op and the torch.library ops)."""

    @staticmethod
    @prec.no_autocast
    def forward(ctx, X, X16, B, N, bn, nt, tn, d, weight, gamma, beta):
        if X16 is None:
            X16 = torch.empty(0, dtype=torch.bfloat16, device=X.device)
        out, saved = S.pointconv_forward(X, X16, B, N, weight, gamma, beta, bn, d, nt, tn)
        ctx.meta = (B, N, bn.slopes[0], bn.evals[0], bn.groups[0], d)
        ctx.save_for_backward(weight, *saved)
        return out

    @staticmethod
    @prec.no_autocast
    def backward(ctx, dout):
        B, N, slope, ev, g, d = ctx.meta
        weight, *saved = ctx.saved_tensors
        dX, dW, dg, db = S.pointconv_backward(dout, saved, weight, B, N, slope, ev, g, d)
        return dX, None, None, None, None, None, None, None, dW, dg, db


def pointconv_bn_lrelu(X, B, N, seq, training=None, X16=None, wprep=None):
    """X (B*N, K) point-major -> (B, Co, N) = LeakyReLU(BN(Conv1x1(X))) with the
    modules of ``seq`` = nn.Sequential(Conv2d(K,Co,1,bias=False) or Conv1d,
    BatchNorm2d/1d, LeakyReLU) (reference dgcnn.py:74-78). ``X16``: optional bf16 twin of X
    (the GEMM operand in bf16; the LDS-DMA GEMMs take it when K and Co are
    multiples of 64, any other width runs the register-staged bf16 GEMMs on
    X). ``wprep``: optional bf16 (W, W^T) of the conv
    weight already made for this step (gemm.prep_weights). GEMM precision:
    ``precision.effective()`` at entry (bf16 mode or fp16/bf16 autocast ->
    bf16 MFMA). ``training`` is accepted for call compatibility only (dgx.bn:
    each BN module's own flags decide). A host tensor takes the CPU path (dgx.cpu)."""
    if cpu.is_cpu(X):
        return cpu.pointconv_bn_lrelu(X, B, N, seq, training)
    nat.require_device(X)
    conv, bn, act = seq[0], seq[1], seq[2]
    S.require_plain_conv_bn(conv, bn)
    nt, tn = wprep if wprep is not None else (None, None)
    return _PointConvBNLReLU.apply(X, X16, B, N, S.bn_lists([bn], [act.negative_slope]), nt, tn, S.decide(),
                                   conv.weight, bn.weight, bn.bias)
