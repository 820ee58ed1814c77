"""fp64 restatement of the kNN vector attention (reference
models/attention.py:107-157), the oracle of the GPU tests; pinned to the
reference's own results by tests/test_vattn_cpu.py.

    idx   = knn(canonical, k)                    (B, N, k) LOCAL ids
    flat  = canonical.view(B*N, 3)               a reinterpretation, no transpose
    D     = (w_q(query) - w_k(key)).view(B*N, Dm);  V = w_v(value).view(B*N, Dm)
    delta = flat[b*gs + idx] - flat[b*N + i]     gs = 0: rows of cloud 0 for every b
    r     = pos_mlp(delta);  s = attn_mlp(D[b*gs + idx] + r)
    a     = softmax(s over Dm);  t = a / max(|a|_2 over the k neighbours, 1e-12)
    agg   = sum_j t (V[b*gs + idx] + r);  out = to_out(agg)

``bf16=True`` rounds the operands of the three GEMMs the fused kernel runs on
the MFMA (pos_mlp layer 2, attn_mlp layers 1 and 2: activations and weights) to
bf16, everything else staying fp64: the yardstick of the kernel's bf16 mode.
Differentiable (torch fp64 autograd) in D, V and the parameters.
"""
import torch
import torch.nn.functional as F


class _RoundBf16(torch.autograd.Function):
    """Round to bf16 (straight-through gradient: the engine's backward is fp32 in both modes)."""

    @staticmethod
    def forward(ctx, x):
        return x.float().bfloat16().double()

    @staticmethod
    def backward(ctx, g):
        return g


def _rnd(x, bf16):
    return _RoundBf16.apply(x) if bf16 else x


def vattn(D, V, pos, idx, params, gather_stride=0, bf16=False):
    """agg (B*N, Dm) fp64. D, V (rows, Dm), pos (B*N, 3), idx (B, N, k) local
    ids, params = pos_mlp's then attn_mlp's (w1, b1, w2, b2)."""
    D, V, pos = D.double(), V.double(), pos.double()
    pw1, pb1, pw2, pb2, aw1, ab1, aw2, ab2 = (p.double() for p in params)
    B, N, k = idx.shape
    rows = (idx.long() + torch.arange(B, device=idx.device).view(B, 1, 1) * gather_stride).view(-1)
    delta = pos[rows].view(B * N, k, 3) - pos.view(B * N, 1, 3)
    e = F.relu(F.linear(delta, pw1, pb1))
    r = F.linear(_rnd(e, bf16), _rnd(pw2, bf16), pb2)
    u = D[rows].view(B * N, k, -1) + r
    h = F.relu(F.linear(_rnd(u, bf16), _rnd(aw1, bf16), ab1))
    s = F.linear(_rnd(h, bf16), _rnd(aw2, bf16), ab2)
    a = s.softmax(dim=-1)
    t = a / a.norm(dim=-2, keepdim=True).clamp_min(1e-12)
    return (t * (V[rows].view(B * N, k, -1) + r)).sum(dim=1)


MLP_KEYS = ("pos_mlp.0.weight", "pos_mlp.0.bias", "pos_mlp.2.weight", "pos_mlp.2.bias",
            "attn_mlp.0.weight", "attn_mlp.0.bias", "attn_mlp.2.weight", "attn_mlp.2.bias")


def module(state, query, key, value, canonical, idx, batch_local=False, bf16=False):
    """VectorAttention.forward in fp64 from a state_dict-like mapping of
    tensors (B, N, emb) -> (B, N, emb); ``idx``: the (B, N, k) kNN ids."""
    w = {n: t.double() for n, t in state.items()}
    B, N = query.shape[0], query.shape[1]
    D = (F.linear(query.double(), w["w_q.weight"]) - F.linear(key.double(), w["w_k.weight"])).reshape(B * N, -1)
    V = F.linear(value.double(), w["w_v.weight"]).reshape(B * N, -1)
    if batch_local:
        pos, gs = canonical.double().transpose(1, 2).reshape(B * N, 3), N
    else:
        pos, gs = canonical.double().contiguous().view(B * N, 3), 0
    agg = vattn(D, V, pos, idx, [w[n] for n in MLP_KEYS], gs, bf16)
    return F.linear(agg.view(B, N, -1), w["to_out.weight"], w["to_out.bias"])
