"""BatchNorm decisions of the engine's fused layers, as the C++ schedule
(csrc/dgx_torch.cpp: BnSpec, batch_stats, running_stats, backward_consts)
takes them; this module reads an nn.BatchNorm into that schedule's argument
lists (``op_args``) and binds its two finalize steps for callers that drive
single kernels.

The reference's EdgeConv blocks, conv5 and PositionEmbedding convs are
``nn.BatchNorm2d`` modules (models/dgcnn.py:54-78, models/layers.py:14-20).
The engine folds their arithmetic into its kernels but takes every decision
the way ``nn.BatchNorm``'s own forward takes it, per BN module:

* batch statistics when ``bn.training`` or the module tracks no running
  statistics; running statistics otherwise (e.g. ``model.train()`` with the BN
  layers frozen in ``eval()``);
* running statistics updated only when ``bn.training`` and
  ``bn.track_running_stats``, with momentum or the cumulative average;
* SyncBatchNorm (main_partseg_dist.py:189) synchronises only in training mode.

Backward: train mode gives BN's full input gradient, dy = a*dz + c0 + c1*y
per element (c0, c1 from the fp64 finalize); eval mode is the fixed affine,
dy = a*dz (c0 = c1 = 0), with dgamma/dbeta over the running-statistics yhat.
"""
from collections import namedtuple

from . import dist as dist_

# per-channel fp32 tensors (Co,) + the SyncBatchNorm process-group name (or None)
# + whether the running statistics normalised this forward
Stats = namedtuple("Stats", "scale shift mean invstd group eval")


def mode(bn):
    """(use batch statistics, update running statistics) — nn.BatchNorm's rule."""
    use_batch = bn.training or (bn.running_mean is None and bn.running_var is None)
    update = bool(bn.training and bn.track_running_stats and bn.running_mean is not None)
    return use_batch, update


def op_args(bn):
    """One BN layer's arguments for the C++ schedule (libdgx_torch.so,
    dgx_host::chain_* / pointconv_* / dgcnn): ([running_mean, running_var,
    num_batches_tracked, and the three update targets of a functional caller
    (``bn.stats_out``) or None for in place], [momentum (-1 = None), eps],
    [training, track_running_stats], SyncBatchNorm process-group name or "").
    The C++ side takes every decision (batch or running statistics, the
    running-statistics update, SyncBatchNorm's all-reduce) from these, as
    nn.BatchNorm does."""
    out = getattr(bn, "stats_out", None)
    rm_o, rv_o, nb_o = out if out is not None else (None, None, None)
    sync, group = dist_.sync_group(bn)
    return ([bn.running_mean, bn.running_var, bn.num_batches_tracked, rm_o, rv_o, nb_o],
            [-1.0 if bn.momentum is None else float(bn.momentum), float(bn.eps)],
            [int(bool(bn.training)), int(bool(bn.track_running_stats))],
            group.group_name if sync else "")


def batch_stats(partials, rows, count, bn, gamma, beta, stream=None):
    """Finalize batch statistics from per-block (sum y, sum y^2) partials
    (rows, 2, Co) over ``count`` elements on the current stream; updates the
    running statistics as nn.BatchNorm would (into ``bn.stats_out`` when the
    caller gives one). ``stream`` is accepted for call compatibility only."""
    from . import schedule as S
    lists = S.bn_lists([bn], [0.0])
    return Stats(*S.bn_batch_stats(partials, rows, count, gamma, beta, lists), lists.groups[0] or None, False)


def backward_consts(partials, rows, count, st, stream=None):
    """(dgamma, dbeta, c0, c1) from per-block (sum g, sum g*yhat) partials, where
    g is the gradient w.r.t. the BN output at every element: BN's train-mode
    input gradient a*g + c0 + c1*y, or the eval-mode affine (c0 = c1 = 0)."""
    from . import schedule as S
    return tuple(S.bn_backward_consts(partials, rows, count, st.scale, st.mean, st.invstd, st.eval, st.group or ""))
