"""Device ops behind the reference's graph functions (models/dgcnn.py:6-44).

``knn`` and ``graph_feature`` keep the reference's argument meaning, return
shapes and dtypes. Their launch schedule is the C++ one (libdgx_torch.so:
dgx_host::knn, graph_feature, graph_feature_backward, reverse_graphs, called
through dgx.schedule), on the tensor's own device and current stream; what
lives here is what is Python's: the drop-in signatures, the reference's
rounding-order rule (part of the kNN-sharing scope's key), that scope, and
the autograd plumbing. Host tensors take dgx.cpu and load neither library.
"""
import contextlib
import threading

import torch

from . import _native as nat
from . import cpu

_tls = threading.local()

def reduction_order(x):
    """Rounding order of the reference's ``sum(x**2, dim=1)`` (dgcnn.py:8) for a
    (B,C,N) tensor with these strides: torch reduces a channel-innermost layout
    with its vectorised inner reduction, an N-innermost one with the strided
    cascade (see oracle/knn_oracle.c, pinned by tests/golden)."""
    _, C, N = x.shape
    _, sC, sN = x.stride()
    if C > 1 and N > 1 and sC < sN:
        return nat.ORDER_VEC8X4
    return nat.ORDER_STRIDED


def _as_f32(x):
    # autocast may hand fp16/bf16 features; distances are always fp32
    return x if x.dtype == torch.float32 else x.float()


def knn_image_buffers(B, C, N, dev):
    """(xx, image) scratch of one kNN call, for a producer kernel to fill and hand to knn_raw(prepared=...)."""
    from . import schedule as S
    return S.knn_image_buffers(B, C, N, dev)


def fast_shape(C, k, N):
    """Whether the fused selection kernel is built for the shape (the rest take
    the generic one): the kernels' own answer, a host query (no device needed)."""
    return bool(nat.lib().dgx_knn_fast_shape(C, k, N))


def knn_raw(x, k, order=None, out_dtype=torch.int64, strides=None, shape=None, return_values=False, prepared=None,
            generic=False):
    """kNN on a (B,C,N) fp32 view, by the C++ schedule's dispatch
    (dgx_host::knn: the fused kernel where it is built for the shape, else the
    generic one). ``strides``/``shape`` let callers describe a strided slice of
    a larger buffer (the engine's point-major concat buffer). ``prepared``:
    (xx, image) already holding |x|^2 in ``order`` and the operand image of
    exactly this view (knn_image_buffers + a producer kernel): the prepare pass
    is skipped. ``generic``: the generic kernel on a shape the fused one takes
    too. Inside a knn_cache scope a repeated call launches nothing."""
    from . import schedule as S
    nat.require_device(x)
    if order is None:
        order = reduction_order(x)
    if strides is not None or shape is not None:
        x = torch.as_strided(x, shape if shape is not None else x.shape, strides if strides is not None else x.stride())
    cache = getattr(_tls, "cache", None)
    key = None
    if cache is not None and not return_values:
        key = (x.device, x.data_ptr(), tuple(x.shape), x.stride(), x._version, k, order)
        hit = cache.get(key)
        if hit is not None:
            hit = hit[0]
            return hit if hit.dtype == out_dtype else hit.to(out_dtype)
    r = S.knn(x.detach() if x.requires_grad else x, k, order, out_dtype, return_values, generic, prepared)
    if key is not None:
        # the entry holds x too: its storage (whose address is part of the key)
        # cannot be freed and reused by another tensor while the scope lives
        cache[key] = (r[0], x)
    return tuple(r) if return_values else r[0]


@contextlib.contextmanager
def knn_cache():
    """Scope in which kNN calls on the same view of the same storage (pointer,
    shape, strides, version counter) with the same k and rounding order share
    one computation. ``Net.forward`` reaches the kNN of its input cloud three
    times (reference model_partseg.py:177 -> dgcnn.py:84, :179 -> :26 and
    :183 -> layers.py:45); the result is a deterministic function
    of those keys, so the shared result is the one each call would compute.
    Each entry keeps its input tensor alive for the whole scope, so a storage
    address cannot be reused by another tensor inside it. Thread-local (DataParallel
    replicas run in threads)."""
    prev = getattr(_tls, "cache", None)
    _tls.cache = {} if prev is None else prev
    try:
        yield
    finally:
        _tls.cache = prev


class _Elapsed:
    """A measured launch (the C++ dispatch's HIP events), shaped like a
    (start_event, end_event) pair: start.elapsed_time(end) -> ms."""

    def __init__(self, ms):
        self.ms = ms

    def elapsed_time(self, _end):
        return self.ms


def set_knn_timing(lst):
    """Optional per-thread instrumentation (tools, bench.py's roofline leg):
    while a list is set, the C++ dispatch (dgx_host::knn, the schedule's own
    kNN calls included) puts HIP events around every fused-kernel selection
    launch of this thread on its launch stream; switching the timing off again
    (set_knn_timing(None)) appends (start_event, end_event, gram_flops,
    (B, C, N, k)) per launch to that list, in launch order."""
    from . import schedule as S
    prev = getattr(_tls, "timing", None)
    if lst is not None:
        S.knn_timing(True)
    elif prev is not None:
        v = S.knn_timing(False)
        for j in range(0, len(v), 6):
            prev.append((_Elapsed(v[j]), None, v[j + 1], (int(v[j + 2]), int(v[j + 3]), int(v[j + 4]), int(v[j + 5]))))
    _tls.timing = lst


def knn(x, k):
    """Drop-in for reference ``knn(x, k)`` (models/dgcnn.py:6-12): int64 (B,N,k)
    local indices, nearest first; ties in canonical (index ascending) order."""
    if torch.compiler.is_compiling():   # traced as one dgx::knn op (dgx.library)
        from . import library  # noqa: F401
        return torch.ops.dgx.knn(x, k)
    if cpu.is_cpu(x):   # host tensors: the CPU path (dgx.cpu), same canonical result
        return cpu.knn(x, k)
    x = _as_f32(x.detach())
    return knn_raw(x, k)


class _GraphFeature(torch.autograd.Function):
    """Autograd over dgx_host::graph_feature / graph_feature_backward."""

    @staticmethod
    def forward(ctx, x, idx32, mode):
        from . import schedule as S
        ctx.save_for_backward(idx32)
        ctx.mode = mode
        ctx.C = x.shape[1]
        return S.graph_feature(x.float(), idx32, mode)

    @staticmethod
    def backward(ctx, dout):
        from . import schedule as S
        (idx32,) = ctx.saved_tensors
        return S.graph_feature_backward(dout, idx32, ctx.C, ctx.mode), None, None


def graph_feature(x, k=20, knn_only=False, disp_only=False, idx=None, mode="cat"):
    """Drop-in for reference ``get_graph_feature`` (models/dgcnn.py:15-44).

    Default: (B,2C,N,k) fp32 contiguous, channels [0,C) = x_j, [C,2C) = x_i
    (dgcnn.py:42). knn_only: (B,N,k,C) neighbour rows (dgcnn.py:37-38).
    disp_only: (B,C,N,k) x_j - x_i (dgcnn.py:39-40). ``mode="diff"`` (engine
    extension): channels [0,C) = x_j - x_i, the paper's / test.ipynb:131 form.
    Differentiable w.r.t. x."""
    if mode not in ("cat", "diff"):
        raise ValueError(f"get_graph_feature: mode must be 'cat' or 'diff', got {mode!r}")
    diff = mode == "diff"
    mode = nat.GF_KNN_ONLY if knn_only else (nat.GF_DISP if disp_only else (nat.GF_DIFFCAT if diff else nat.GF_CAT))
    if torch.compiler.is_compiling() and idx is None:   # traced as one dgx::graph_feature op
        from . import library  # noqa: F401
        return torch.ops.dgx.graph_feature(x, k, mode)[0]
    if cpu.is_cpu(x):
        return cpu.graph_feature(x, k, knn_only, disp_only, idx, mode="diff" if diff else "cat")
    nat.require_device(x)
    x = _as_f32(x)
    if idx is None:
        idx = knn_raw(x.detach(), k, out_dtype=torch.int32)
    else:
        # caller-given ids (an engine extension): every kernel of the forward and
        # the reverse-graph backward assumes 0 <= id < N, so check once (one host
        # sync, only on this path); the reference's indexing raises likewise
        B, _, N = x.shape
        if idx.dim() != 3 or idx.shape[0] != B or idx.shape[1] != N:
            raise RuntimeError(f"get_graph_feature: idx of shape {tuple(idx.shape)} does not match x "
                               f"{tuple(x.shape)} (expected (B, N, k))")
        if idx.numel():
            lo, hi = torch.aminmax(idx.detach())
            if int(lo) < 0 or int(hi) >= N:
                raise IndexError(f"get_graph_feature: neighbour ids must lie in [0, {N}), got [{int(lo)}, {int(hi)}]")
        if idx.dtype != torch.int32:
            idx = idx.to(torch.int32)
    return _GraphFeature.apply(x, idx.contiguous(), mode)
