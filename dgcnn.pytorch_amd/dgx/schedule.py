"""The one Python binding of the C++ schedule (libdgx_torch.so,
csrc/dgx_torch.cpp): every ``torch.ops.dgx_host`` call of the EdgeConv chain,
conv5, PositionEmbedding's edge MLP and the one-op DGCNN goes through here, for
the eager op (dgx.host), the autograd Functions (dgx.edgeconv, dgx.pointconv,
dgx.edgemlp) and the torch.library ops (dgx.library) alike, and so do the kNN
dispatch, the reverse graphs and the graph feature that dgx.ops binds; dgx.gemm
binds the schedule's GEMM and weight-prep helpers through ``host_ops``. What
they share lives here once: the precision / options decision taken at forward
entry, the BatchNorm argument lists, the kNN-sharing lookup, and the names of
the saved-state lists the schedule hands back for backward
(``dgx_host::layout()`` returns the C++ side's tables; a test holds the two
equal).
"""
from collections import namedtuple

import torch

from . import bn as bn_
from . import gemm as G
from . import ops
from . import precision as prec

# a chain's saved list: the point-major cloud, then per block these fields
CHAIN_FIELDS = ("idx", "PQ", "ysel", "arg", "sumP", "scale", "shift", "mean", "invstd")
# conv5's saved list
PC_FIELDS = ("Xop", "Z", "scale", "shift", "mean", "invstd", "nt", "tn", "xhi", "xlo")
# the edge MLP's saved list (absent tensors are empty): conv1's operand and kNN
# graph, PQ, sum_k P_j, h1 / z2 where the forward stored them, conv2's selected
# value and slot, the two BN layers' per-channel state, conv2's bf16 weight copies
EMLP_FIELDS = ("X", "idx", "PQ", "sumP", "H1", "Z2", "ysel", "arg", "scale1", "shift1", "mean1", "invstd1",
               "scale2", "shift2", "mean2", "invstd2", "nt", "tn")
# bit i of the opts word is the A/B switch of this name (module attributes of
# dgx.edgeconv, documented there); bits 8-15 carry gemm.SLAB_CAP_MB
OPT_BITS = ("SCATTER_PACKED", "FOLD_BN_BWD", "FUSE_KNN_IMAGE", "FUSE_EDGE_DZ", "SPLIT32", "SPLIT32_EDGE")

ChainBlock = namedtuple("ChainBlock", CHAIN_FIELDS)
PcSaved = namedtuple("PcSaved", PC_FIELDS)
EmlpSaved = namedtuple("EmlpSaved", EMLP_FIELDS)
Decision = namedtuple("Decision", "bf16 opts")
BnLists = namedtuple("BnLists", "t f i groups slopes evals")


def chain_blocks(saved):
    """The blocks of a chain ``saved`` list, one ChainBlock each (all fields
    empty tensors for a block that ran without selection state)."""
    n = len(CHAIN_FIELDS)
    return [ChainBlock(*saved[j:j + n]) for j in range(1, len(saved), n)]


def opts(split=False):
    """The schedule's ``opts`` word (csrc/dgx_torch.cpp ``decode``) from the
    A/B switches as dgx.edgeconv holds them now and gemm.SLAB_CAP_MB.
    ``split``: whether the fp32 GEMMs run as split bf16, as ``decide`` found."""
    from . import edgeconv as E   # the switches live there (tools override them by module:NAME)
    word = max(0, min(255, int(G.SLAB_CAP_MB))) << 8
    for i, name in enumerate(OPT_BITS):
        word |= int(bool(getattr(E, name) or (split and name == "SPLIT32"))) << i
    return word


def decide():
    """(bf16, opts) of an op entered now: ``precision.effective()`` (which sees
    autocast) read once. Every entry takes this at forward and carries it into
    its backward."""
    eff = prec.effective()
    return Decision(eff == "bf16", opts(eff == "fp32_split"))


def shared_idx0(x, k):
    """Block 1's kNN ids from the kNN-sharing scope's cache (Net.forward), or
    None outside a scope (the schedule then runs that kNN itself)."""
    if getattr(ops._tls, "cache", None) is None:
        return None
    return ops.knn_raw(x.detach(), k, order=ops.reduction_order(x), out_dtype=torch.int32)


def plain_conv_bn(conv, bn):
    """Conv(bias=False) + affine BatchNorm, as the reference builds them (dgcnn.py:54-78)."""
    return conv.bias is None and bn.weight is not None


def require_plain_conv_bn(conv, bn):
    if not plain_conv_bn(conv, bn):
        raise NotImplementedError("dgx expects Conv(bias=False) + affine BatchNorm "
                                  "(as the reference builds them, dgcnn.py:54-78)")


def bn_lists(bns, slopes, targets=True):
    """The per-layer BatchNorm arguments of the schedule, concatenated over
    layers (dgx.bn.op_args): tensors (with the update targets of a functional
    caller, or just the three module buffers), (momentum, eps, slope) floats,
    (training, track) ints, process-group names; plus the slopes and whether
    each layer normalises with its running statistics."""
    r = BnLists([], [], [], [], [float(s) for s in slopes], [])
    for bn, slope in zip(bns, r.slopes):
        t, f, i, g = bn_.op_args(bn)
        r.t.extend(t if targets else t[:3])
        r.f.extend(f + [slope])
        r.i.extend(i)
        r.groups.append(g)
        # bn.mode's rule on what op_args read: running statistics normalise unless training or none are kept
        r.evals.append(int(not (i[0] or (t[0] is None and t[1] is None))))
    return r


def _host():
    from . import host
    host.load()
    return torch.ops.dgx_host


# dgx.gemm's handle: its functions are the dgx_host::gemm_* / weight_prep* ops one to one, with nothing to share here
host_ops = _host


def knn(x, k, order, out_dtype, return_values, generic, prepared):
    """-> [ids (B, N, k)] or [ids, values] of a (B, C, N) fp32 view; ``prepared``: (xx, image) or None."""
    return _host().knn(x, k, order, out_dtype, return_values, generic, *(prepared or (None, None)))


def knn_image_buffers(B, C, N, dev):
    """-> (xx, image) scratch of one fused-kernel kNN call, for a producer kernel to fill."""
    return _host().knn_image_buffers(B, C, N, torch.device(dev))


def knn_timing(on):
    """True: record this thread's kNN selection launches; False: stop, -> [ms, flops, B, C, N, k] per launch."""
    return _host().knn_timing(on)


def reverse_graphs(idxs):
    """-> [(rowptr, edges)] per contiguous int32 (B, N, k) graph: the CSR lists of its in-edges."""
    r = _host().reverse_graphs(idxs)
    return list(zip(r[:len(idxs)], r[len(idxs):]))


def graph_feature(x, idx, mode):
    """-> the edge tensor of an fp32 (B, C, N) cloud over its int32 kNN graph, in the layout of ``mode`` (nat.GF_*)."""
    return _host().graph_feature(x, idx, mode)


def graph_feature_backward(dout, idx, C, mode):
    """-> dx (B, C, N)"""
    return _host().graph_feature_backward(dout, idx, C, mode)


def vattn_forward(D, V, pos, idx, gather_stride, weights, d):
    """-> agg (B*N, Dm) of the fused kNN vector attention; ``weights``: pos_mlp's and attn_mlp's (w1, b1, w2, b2),
    ``d``: decide() — bf16 runs the bf16 kernel, fp32 and fp32_split the fp32 one (never narrower than asked)."""
    return _host().vattn_forward(D, V, pos, idx, int(gather_stride), list(weights), bool(d.bf16))


def chain_forward(x, k, weights, gammas, betas, bn, d, need_grad, prep, idx0):
    """-> (xcat, xcat16, saved, prep); ``bn``: bn_lists of the blocks, ``d``: decide()."""
    return _host().chain_forward(x, k, weights, gammas, betas, bn.t, bn.f, bn.i, bn.groups, bn.slopes, d.bf16,
                                 bool(need_grad), prep, idx0, d.opts)


def chain_backward(dxcat, xcat, xcat16, saved, weights, prep, shape, k, evals, groups, slopes, d, x_needs_grad):
    """-> (dx or empty, dW, dgamma, dbeta per block)"""
    return _host().chain_backward(dxcat, xcat, xcat16, saved, weights, prep, list(shape), k, evals, groups, slopes,
                                  d.bf16, x_needs_grad, d.opts)


def pointconv_forward(X, X16, B, N, weight, gamma, beta, bn, d, nt, tn):
    """-> (out (B, Co, N), saved as PC_FIELDS); ``bn``: bn_lists of the one layer."""
    return _host().pointconv_forward(X.float(), X16, B, N, weight, gamma, beta, bn.t, bn.f, bn.i, bn.groups[0], d.bf16,
                                     nt, tn, d.opts)


def pointconv_backward(dout, saved, weight, B, N, slope, ev, group, d):
    """-> (dX, dW, dgamma, dbeta)"""
    return _host().pointconv_backward(dout, list(saved), weight, B, N, slope, bool(ev), group, d.bf16, d.opts)


def dgcnn(x, k, params, bn, d, idx0):
    """DGCNN.forward as one op; ``bn``: bn_lists(..., targets=False) of blocks + conv5."""
    return _host().dgcnn(x, params, bn.t, bn.f, bn.i, bn.groups, idx0, k, d.bf16, d.opts)


def edge_mlp2_forward(x, idx, k, params, bn, bf16, need_grad, fused_bwd):
    """-> (out (B, C2, N), saved as EMLP_FIELDS); ``params``: (w1, g1, b1, w2, g2, b2),
    ``bn``: bn_lists of the two layers, ``idx``: int32 (B, N, k) kNN graph."""
    return _host().edge_mlp2_forward(x, idx, k, *params, bn.t, bn.f, bn.i, bn.groups, bool(bf16), bool(need_grad),
                                     bool(fused_bwd))


def edge_mlp2_backward(dout, saved, w1, w2, shape, k, evals, groups, slopes, d, x_needs_grad):
    """-> (dx or empty, dW1, dgamma1, dbeta1, dW2, dgamma2, dbeta2)"""
    return _host().edge_mlp2_backward(dout, list(saved), w1, w2, list(shape), k, evals, groups, slopes, d.bf16,
                                      bool(x_needs_grad), d.opts)


def bn_batch_stats(partials, rows, count, gamma, beta, bn):
    """-> [scale, shift, mean, invstd]; ``bn``: bn_lists of the one layer."""
    return _host().bn_batch_stats(partials, rows, float(count), gamma, beta, bn.t, bn.f, bn.i, bn.groups[0])


def bn_backward_consts(partials, rows, count, scale, mean, invstd, ev, group):
    """-> [dgamma, dbeta, c0, c1]"""
    return _host().bn_backward_consts(partials, rows, float(count), scale, mean, invstd, bool(ev), group)
