"""Eager dispatch of DGCNN.forward through the C++ op layer (libdgx_torch.so,
csrc/dgx_torch.cpp): ``torch.ops.dgx_host.dgcnn`` runs the EdgeConv chain +
conv5 forward (reference models/dgcnn.py:80-103) and, from a C++ autograd
node, the whole backward — the ~60 launches of a step are issued from C++
instead of one Python dispatch each.

It is the same schedule the engine's autograd Functions (dgx.edgeconv,
dgx.pointconv) and torch.library ops (dgx.library) call — all through the one
binding, dgx.schedule, which also carries the kNN dispatch (dgx_host::knn: the
chain's own kNN function, bound by dgx.ops.knn_raw) and the graph-feature ops —
one C++ implementation for every configuration the reference's scripts run:
precision bf16, fp32 or fp32_split (bf16 autocast -> bf16 GEMMs, fp16
autocast -> split-bf16 fp32 GEMMs, dgx.precision.effective), BatchNorm in
training or eval mode, momentum or cumulative running statistics, plain
BatchNorm2d or SyncBatchNorm (main_partseg_dist.py:189: the statistics
all-reduce is issued from C++ over the module's process
group), any (B, C, N, k). The Function path is taken only while tests capture
routing decisions (dgx.edgeconv.set_debug_capture), while torch.compile traces
(dgx.library ops), or with ``DGX_HOST_EXT=0`` (A/B runs).
"""
import os
import threading

import torch

from . import edgeconv as E
from . import schedule as S

ENABLED = os.environ.get("DGX_HOST_EXT", "1") == "1"
_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DGX_TORCH_LIB", os.path.join(_HERE, "libdgx_torch.so"))
_lock = threading.Lock()
_loaded = False


def load():
    """Register torch.ops.dgx_host (once). The engine's device schedule lives
    there: a missing libdgx_torch.so is an error, never a fallback."""
    global _loaded
    if not _loaded:
        with _lock:
            if not _loaded:
                if not os.path.exists(LIB_PATH):
                    raise ImportError(f"dgx: C++ op library not built ({LIB_PATH}); run `make -C "
                                      "dgcnn.pytorch_amd/csrc` or __graft_entry__.build()")
                from . import _native
                _native.lib()   # libdgx.so first: libdgx_torch.so links against it
                torch.ops.load_library(LIB_PATH)
                _loaded = True


def applies(model, x):
    """Whether DGCNN ``model``'s forward on ``x`` takes the one-op C++ path."""
    if not ENABLED or torch.compiler.is_compiling() or E.debug_capture() is not None:
        return False
    if x.device.type != "cuda" or x.dim() != 3 or not x.is_floating_point():
        return False
    for seq in model.edge_blocks() + [model.conv5]:
        conv, bn = seq[0], seq[1]
        if not S.plain_conv_bn(conv, bn) or conv.weight.dtype != torch.float32:
            return False
    return True


def dgcnn_forward(model, x):
    """DGCNN.forward through the one-op schedule (dgx_host::dgcnn)."""
    if x.dtype != torch.float32:
        x = x.float()
    params, bns, slopes = [], [], []
    weights = model.edge_weights() + [model.conv5[0].weight]   # re-parameterised in edge_mode "diff"
    for w, seq in zip(weights, model.edge_blocks() + [model.conv5]):
        bn, act = seq[1], seq[2]   # (one lookup each: nn.Sequential indexing is slow on this path)
        params += [w, bn.weight, bn.bias]
        bns.append(bn)
        slopes.append(act.negative_slope)
    # the running statistics are updated in place: the module buffers only
    bn = S.bn_lists(bns, slopes, targets=False)
    return S.dgcnn(x, model.k, params, bn, S.decide(), S.shared_idx0(x, model.k))
