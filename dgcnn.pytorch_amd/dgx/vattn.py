"""kNN vector attention (reference models/attention.py:107-150,
VectorAttention.forward between its projections and ``to_out``) on the engine.

``vector_attention(D, V, pos, idx, pos_mlp, attn_mlp, gather_stride=0)`` takes
the gather tables D = w_q(query) - w_k(key) and V = w_v(value) ((rows, Dm):
q[idx] - k[idx] == (q - k)[idx] bitwise, so the reference has no centre term),
the (B*N, 3) positions and the (B, N, k) local kNN ids, and returns agg
(B*N, Dm). ``gather_stride`` is the row offset between clouds in the tables: 0
reproduces the reference (its ids carry no batch offset: every cloud gathers
cloud 0's rows), N gathers each cloud's own.

Forward: one fused kernel (csrc/vattn.hip, through dgx.schedule) where
``fused_shape`` holds — Dm 64, H 256, Hp 64, k <= 64 — in the precision
``schedule.decide()`` finds at entry (bf16 -> bf16 MFMA operands, fp32 and
fp32_split -> exact fp32 products); no per-edge tensor is written.

Backward: recompute, keeping nothing per edge between forward and backward.
The points are walked in chunks of about ``BWD_CHUNK_MB`` of recompute state;
per chunk the composed op sequence (dgx.cpu.vattn_edges, fp32 in both modes)
runs under ``enable_grad`` with the gathered rows D[idx], V[idx] as leaves, the
weight and bias gradients are accumulated, and the gathered rows' gradients go
to two (E, Dm) buffers that the engine's deterministic reverse-graph pull
(dgx_host::graph_feature_backward, gathered-neighbours mode) reduces to dD and
dV — summed over clouds when gather_stride is 0. No float atomics.

Everything else takes the composed path (dgx.cpu.vector_attention) with torch
autograd: host tensors, shapes outside the fused one, and any call whose
``pos`` requires grad (the fused path has no gradient to the positions).
"""
import torch

from . import _native as nat
from . import cpu

BWD_CHUNK_MB = 256   # recompute state per backward chunk (module attribute, read at call time)


@torch._dynamo.assume_constant_result   # a host query of static sizes: a constant of a traced graph
def fused_shape(Dm, H, Hp, k):
    """Whether the fused forward kernel is built for the shape: the kernel's own answer (a host query)."""
    return bool(nat.lib().dgx_vattn_fused_shape(int(Dm), int(H), int(Hp), int(k)))


def fwd_points():
    """Points per workgroup of the fused forward (tests place cases at this tile edge)."""
    return int(nat.lib().dgx_vattn_fwd_points())


def _chunk_points(k, Dm, H, Hp):
    # fp32 per edge in the recompute and its autograd graph: ~8 Dm-wide, 3 H-wide and 2 Hp-wide tensors
    per_point = 4 * k * (8 * Dm + 3 * H + 2 * Hp)
    return max(1, (int(BWD_CHUNK_MB) << 20) // per_point)


def backward(g, D, V, pos, idx, gather_stride, params):
    """-> (dD, dV, [8 parameter gradients]) of the fused forward, by chunked
    recompute (module docstring). ``idx``: contiguous int32 (B, N, k)."""
    from . import schedule as S
    B, N, k = idx.shape
    M, Dm = B * N, D.shape[1]
    if gather_stride not in (0, N):
        raise NotImplementedError("dgx vattn backward: gather_stride is 0 (the reference) or N (per-cloud)")
    g = g.contiguous().float()
    rows_all = cpu.vattn_rows(idx, gather_stride)
    gD = torch.empty((M * k, Dm), dtype=torch.float32, device=D.device)
    gV = torch.empty_like(gD)
    leaves = [p.detach().float().requires_grad_() for p in params]
    acc = [torch.zeros_like(p) for p in leaves]
    Dd, Vd, posd = D.detach(), V.detach(), pos.detach()
    step = _chunk_points(k, Dm, params[4].shape[0], params[0].shape[0])
    with torch.enable_grad(), torch.autocast("cuda", enabled=False):
        for p0 in range(0, M, step):
            p1 = min(M, p0 + step)
            rows = rows_all[p0:p1].reshape(-1)
            Dj = Dd[rows].view(p1 - p0, k, Dm).requires_grad_()
            Vj = Vd[rows].view(p1 - p0, k, Dm).requires_grad_()
            delta = posd[rows].view(p1 - p0, k, 3) - posd[p0:p1].view(p1 - p0, 1, 3)
            out = cpu.vattn_edges(Dj, Vj, delta, leaves)
            gr = torch.autograd.grad(out, [Dj, Vj] + leaves, g[p0:p1])
            gD[p0 * k:p1 * k] = gr[0].reshape(-1, Dm)
            gV[p0 * k:p1 * k] = gr[1].reshape(-1, Dm)
            for a, x in zip(acc, gr[2:]):
                a += x
            del out, gr, Dj, Vj, delta
    outs = []
    for ge, table in ((gD, D), (gV, V)):
        # (B, Dm, N): every row's sum over its in-edges, in the reverse graph's order
        pulled = S.graph_feature_backward(ge.view(B, N, k, Dm), idx, Dm, nat.GF_KNN_ONLY)
        dt = torch.zeros(table.shape, dtype=torch.float32, device=table.device)
        if gather_stride == 0:
            dt[:N] = pulled.sum(dim=0).t()          # every cloud gathered cloud 0's rows
        else:
            dt[:M] = pulled.permute(0, 2, 1).reshape(M, Dm)
        outs.append(dt)
    return outs[0], outs[1], acc


class _VAttn(torch.autograd.Function):
    """Autograd over dgx_host::vattn_forward and the chunked recompute."""

    @staticmethod
    def forward(ctx, D, V, pos, idx, gather_stride, *params):
        from . import schedule as S
        weights = [p.detach().float().contiguous() for p in params]
        agg = S.vattn_forward(D, V, pos, idx, gather_stride, weights, S.decide())
        ctx.save_for_backward(D, V, pos, idx, *params)
        ctx.gather_stride = gather_stride
        return agg

    @staticmethod
    def backward(ctx, g):
        D, V, pos, idx, *params = ctx.saved_tensors
        dD, dV, dparams = backward(g, D, V, pos, idx, ctx.gather_stride, params)
        return (dD, dV, None, None, None, *(dp.to(p.dtype) for dp, p in zip(dparams, params)))


def check_ids(idx, B, N):
    """Caller-supplied ids: every kernel of the forward and the reverse-graph
    backward assumes 0 <= id < N (one host sync, skipped while a stream captures)."""
    if idx.dim() != 3 or idx.shape[0] != B or idx.shape[1] != N:
        raise RuntimeError(f"vector_attention: idx of shape {tuple(idx.shape)} does not match (B, N, k) = ({B}, {N}, k)")
    if idx.numel() and not torch.cuda.is_current_stream_capturing():
        lo, hi = torch.aminmax(idx.detach())
        if int(lo) < 0 or int(hi) >= N:
            raise IndexError(f"vector_attention: neighbour ids must lie in [0, {N}), got [{int(lo)}, {int(hi)}]")


def vector_attention(D, V, pos, idx, pos_mlp, attn_mlp, gather_stride=0, ids_checked=False):
    """agg (B*N, Dm) of the kNN vector attention (module docstring). ``pos_mlp``,
    ``attn_mlp``: the Linear-ReLU-Linear Sequentials (or their (w1, b1, w2, b2));
    ``ids_checked``: the ids come from the engine's kNN (no range check)."""
    params = cpu.vattn_params(pos_mlp, attn_mlp)
    if cpu.is_cpu(D):
        return cpu.vector_attention(D, V, pos, idx, params[:4], params[4:], gather_stride)
    nat.require_device(D, V, pos, idx)
    B, N, k = idx.shape
    Dm, H, Hp = D.shape[1], params[4].shape[0], params[0].shape[0]
    if pos.shape != (B * N, 3) or D.shape != V.shape or D.dim() != 2:
        raise RuntimeError(f"vector_attention: D/V (rows, Dm) and pos (B*N, 3) expected, got {tuple(D.shape)}, "
                           f"{tuple(V.shape)}, {tuple(pos.shape)}")
    if gather_stride not in (0, N) or (B - 1) * gather_stride + N > D.shape[0]:
        raise RuntimeError(f"vector_attention: gather_stride {gather_stride} is 0 or N = {N}, inside the tables")
    compiling = torch.compiler.is_compiling()
    if not ids_checked and not compiling:
        check_ids(idx, B, N)
    if pos.requires_grad or not fused_shape(Dm, H, Hp, k):
        with torch.autocast("cuda", enabled=False):
            return cpu.vector_attention(D.float(), V.float(), pos.float(), idx, [p.float() for p in params[:4]],
                                        [p.float() for p in params[4:]], gather_stride)
    idx32 = idx.detach().to(torch.int32).contiguous()
    D, V, pos = (t.float().contiguous() for t in (D, V, pos))
    if compiling:   # traced as one dgx::vattn op (dgx.library)
        from . import library  # noqa: F401
        from . import precision as prec
        return torch.ops.dgx.vattn(D, V, pos, idx32, gather_stride, *params, prec.effective() == "bf16")
    return _VAttn.apply(D, V, pos.detach(), idx32, gather_stride, *params)
