"""Drop-in for reference ``models/attention.py``: ``MultiHeadedAttention``,
``VectorAttention`` and ``MultiHeadVectorAttention`` with the reference's
constructor signatures, attribute names and state_dict keys.

``VectorAttention`` (attention.py:74-157, the point-transformer attention that
``--d_qkv`` configures) keeps its four projections as stock ``nn.Linear`` and
runs everything between them — the kNN of the positions, the positional MLP,
the attention MLP over the kNN edges, softmax, normalisation and aggregation —
on the engine: ``knn`` + ``dgx.vattn.vector_attention`` (one fused HIP kernel
where its shape holds). The reference gathers its neighbour rows with local
ids from the (B*N, C) views (attention.py:115-134), so every cloud reads cloud
0's rows, and reinterprets the (B, 3, N) positions as (B*N, 3) without a
transpose; both are reproduced. ``batch_local=True`` (an engine extension,
opt-in) gathers each cloud's own rows and its transposed positions instead.

``MultiHeadVectorAttention`` (attention.py:160-255) is the composed op
sequence with the engine kNN: its head split, local-id gathers, softmax over
the neighbours and normalisation over the points are kept as the reference
has them. ``MultiHeadedAttention`` (attention.py:31-71) is stock ops.
"""
import copy
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from dgx.vattn import vector_attention
from models.dgcnn import knn


def clones(module, N):
    """N deep copies of ``module`` in a ModuleList."""
    return nn.ModuleList([copy.deepcopy(module) for _ in range(N)])


def attention(query, key, value, mask=None, dropout=None):
    """softmax(q k^T / sqrt(d)) v and the attention weights (attention.py:17-28)."""
    scores = torch.matmul(query, key.transpose(-2, -1).contiguous()) / math.sqrt(query.size(-1))
    if mask is not None:
        scores = scores.masked_fill(mask == 0, -1e9)
    p_attn = scores.softmax(dim=-1)
    if dropout is not None:
        p_attn = dropout(p_attn)
    return torch.matmul(p_attn, value), p_attn


class MultiHeadedAttention(nn.Module):
    def __init__(self, h, d_model, dropout=0.1):
        super().__init__()
        assert d_model % h == 0
        self.d_k = d_model // h
        self.h = h
        self.linears = clones(nn.Linear(d_model, d_model), 4)
        self.attn = None
        self.dropout = nn.Dropout(p=dropout)

    def forward(self, query, key, value, mask=None):
        if mask is not None:
            mask = mask.unsqueeze(1)   # one mask for all heads
        n = query.size(0)
        query, key, value = [lin(x).view(n, -1, self.h, self.d_k).transpose(1, 2).contiguous()
                             for lin, x in zip(self.linears, (query, key, value))]
        x, self.attn = attention(query, key, value, mask=mask, dropout=self.dropout)
        x = x.transpose(1, 2).contiguous().view(n, -1, self.h * self.d_k)
        return self.linears[-1](x)


def _mlp(c_in, hidden, c_out):
    return nn.Sequential(nn.Linear(c_in, hidden), nn.ReLU(), nn.Linear(hidden, c_out))


class VectorAttention(nn.Module):
    def __init__(self, args, pos_mlp_hidden_dim=64, attn_mlp_hidden_mult=4, batch_local=False):
        super().__init__()
        inner_dim = args.d_qkv
        self.num_neighbors = args.k
        self.size = args.emb_dim
        self.batch_local = batch_local
        self.w_q = nn.Linear(args.emb_dim, inner_dim, bias=False)
        self.w_k = nn.Linear(args.emb_dim, inner_dim, bias=False)
        self.w_v = nn.Linear(args.emb_dim, inner_dim, bias=False)
        self.to_out = nn.Linear(inner_dim, args.emb_dim)
        self.pos_mlp = _mlp(3, pos_mlp_hidden_dim, inner_dim)
        self.attn_mlp = _mlp(inner_dim, inner_dim * attn_mlp_hidden_mult, inner_dim)

    def forward(self, query, key, value, canonical, mask=None):
        """query / key / value (B, N, emb), canonical (B, 3, N) -> (B, N, emb)."""
        B, N = query.shape[0], query.shape[1]
        # q[idx] - k[idx] == (q - k)[idx] bitwise: one gather table   attention.py:125-130
        D = (self.w_q(query) - self.w_k(key)).reshape(B * N, -1)
        V = self.w_v(value).reshape(B * N, -1)
        idx = knn(canonical, k=self.num_neighbors)                  # attention.py:115
        if self.batch_local:
            pos, stride = canonical.transpose(1, 2).reshape(B * N, 3), N
        else:
            pos, stride = canonical.contiguous().view(B * N, 3), 0  # attention.py:116-119
        agg = vector_attention(D, V, pos, idx, self.pos_mlp, self.attn_mlp, stride, ids_checked=True)
        return self.to_out(agg.view(B, N, -1))                      # attention.py:157


class MultiHeadVectorAttention(nn.Module):
    def __init__(self, args, dim_head=64, pos_mlp_hidden_dim=64, attn_mlp_hidden_mult=4):
        super().__init__()
        self.heads = args.n_heads
        inner_dim = dim_head * self.heads
        self.num_neighbors = args.k
        self.size = args.emb_dim
        self.w_q = nn.Linear(args.emb_dim, inner_dim, bias=False)
        self.w_k = nn.Linear(args.emb_dim, inner_dim, bias=False)
        self.w_v = nn.Linear(args.emb_dim, inner_dim, bias=False)
        self.to_out = nn.Linear(inner_dim, args.emb_dim)
        self.pos_mlp = _mlp(3, pos_mlp_hidden_dim, inner_dim)
        hidden = inner_dim * attn_mlp_hidden_mult
        self.attn_mlp = nn.Sequential(nn.Conv2d(inner_dim, hidden, 1, groups=self.heads), nn.ReLU(),
                                      nn.Conv2d(hidden, inner_dim, 1, groups=self.heads))

    def forward(self, query, key, value, canonical, mask=None):
        B, N, h, k = query.shape[0], query.shape[1], self.heads, self.num_neighbors
        # 'b n (h d) -> b h n d'                                     attention.py:204-205
        q, kk, v = (t.view(B, N, h, -1).permute(0, 2, 1, 3) for t in (self.w_q(query), self.w_k(key), self.w_v(value)))
        idx = knn(canonical, k=k).view(-1)
        flat = canonical.contiguous().view(B * N, -1)
        rel = self.pos_mlp(flat[idx, :].view(B, N, k, 3) - canonical.contiguous().view(B, N, 1, 3))
        rel = rel.view(B, N, k, h, -1).permute(0, 3, 1, 2, 4)        # 'b i j (h d) -> b h i j d'
        # the (b h n d) memory read as (b n, h d) rows, gathered with local ids   attention.py:221-229
        q, kk, v = (t.contiguous().view(B * N, -1)[idx, :].view(B, h, N, k, -1) for t in (q, kk, v))
        v = v + rel
        x = (q - kk + rel).permute(0, 1, 4, 2, 3).reshape(B, -1, N, k)   # 'b h i j d -> b (h d) i j'
        attn = F.normalize(self.attn_mlp(x).softmax(dim=-1), dim=-2)      # over the neighbours, then the points
        v = v.permute(0, 2, 3, 1, 4).reshape(B, N, k, -1)                 # 'b h i j d -> b i j (h d)'
        agg = torch.einsum('b d i j, b i j d -> b i d', attn, v).contiguous()
        return self.to_out(agg)
