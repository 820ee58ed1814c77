"""CPU dispatch of the engine's building blocks ("CPU tensors ->
CPU restatement path").

The reference runs its hot path on CPU tensors too (models/dgcnn.py:19-20
picks the device from the input; BASELINE cfg1 is main_cls.py at B=4 on the
host). Every engine entry point — ``knn``, ``graph_feature``, the EdgeConv
block chain, the point conv, the PositionEmbedding edge stage, the HOG
histogram and the attention — sends a CPU tensor here and a ROCm tensor to
libdgx.so; a ROCm tensor never reaches this module (no fallback: a missing
HIP library still raises on the device path).

The arithmetic is torch's CPU kernels, so results follow the reference:
  * ``knn``: the reference's own op sequence (dgcnn.py:7-11: matmul, sum of
    squares, the two broadcast subtractions), bit for bit the same values; the
    top-k is a stable descending sort, i.e. ties in canonical (index
    ascending) order, as on the device (the reference's topk orders ties
    arbitrarily).
  * EdgeConv blocks: the decomposition the device uses — the 1x1 conv on
    cat(x_j, x_i) is P_j + Q_i with P = X W1^T, Q = X W2^T (dgcnn.py:41-43, 55)
    — then the block's own BatchNorm / LeakyReLU modules and the max over k,
    with torch autograd. k times fewer GEMM flops than the edge tensor; equal
    to the reference within fp32 rounding (the 1e-3 parity bar).
  * the other stages call the reference modules on the same tensors.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F


def is_cpu(t):
    return isinstance(t, torch.Tensor) and t.device.type == "cpu"


def knn(x, k):
    """int64 (B, N, k) local ids (reference dgcnn.py:6-12), canonical tie order."""
    x = x.detach()
    if x.dtype != torch.float32:
        x = x.float()   # distances in fp32 whatever the input
    B, C, N = x.shape
    if not (1 <= k <= N):
        raise RuntimeError(f"knn: selected index k out of range (k={k}, N={N})")
    inner = -2 * torch.matmul(x.transpose(2, 1).contiguous(), x)
    xx = torch.sum(x ** 2, dim=1, keepdim=True)
    pd = -xx - inner - xx.transpose(2, 1).contiguous()
    return pd.sort(dim=-1, descending=True, stable=True)[1][..., :k].contiguous()


def graph_feature(x, k=20, knn_only=False, disp_only=False, idx=None, mode="cat"):
    """Edge features of reference dgcnn.py:15-44 (differentiable in x);
    mode "diff": (x_j - x_i, x_i) of test.ipynb:131."""
    if x.dtype != torch.float32:
        x = x.float()
    B, C, N = x.shape
    if idx is None:
        idx = knn(x, k)
    k = idx.shape[-1]
    flat = (idx.long() + torch.arange(B).view(-1, 1, 1) * N).view(-1)
    rows = x.transpose(2, 1).contiguous()
    nbr = rows.view(B * N, -1)[flat, :].view(B, N, k, C)
    if knn_only:
        return nbr
    ctr = rows.view(B, N, 1, C).repeat(1, 1, k, 1)
    if disp_only:
        return (nbr - ctr).permute(0, 3, 1, 2).contiguous()
    first = nbr - ctr if mode == "diff" else nbr
    return torch.cat((first, ctr), dim=3).permute(0, 3, 1, 2).contiguous()


def _edge_values(x, idx, weight):
    """y[b, o, i, j] = (W [x_j; x_i])_o for the kNN edges (i, idx[i, j]) of
    every cloud, as P_j + Q_i (B, Co, N, k)."""
    B, C, N = x.shape
    k = idx.shape[-1]
    Co = weight.shape[0]
    w = weight.reshape(Co, 2 * C)
    rows = x.transpose(2, 1)                                        # (B, N, C)
    P = torch.matmul(rows, w[:, :C].t())                            # (B, N, Co)
    Q = torch.matmul(rows, w[:, C:].t())
    flat = (idx.long() + torch.arange(B).view(-1, 1, 1) * N).view(-1)
    Pj = P.reshape(B * N, Co)[flat].view(B, N, k, Co)
    return (Pj + Q.unsqueeze(2)).permute(0, 3, 1, 2)               # (B, Co, N, k)


def edgeconv_block(x, k, seq, weight=None):
    """max_k LeakyReLU(BN(Conv2d_1x1(get_graph_feature(x, k)))), reference
    dgcnn.py:84-98, with the block's own modules; x (B, C, N) -> (B, Co, N).
    ``weight``: the conv weight to use instead of the module's (edge_mode "diff")."""
    conv, bn, act = seq[0], seq[1], seq[2]
    y = _edge_values(x, knn(x, k), conv.weight if weight is None else weight)
    if conv.bias is not None:
        y = y + conv.bias.view(1, -1, 1, 1)
    return act(bn(y)).max(dim=-1, keepdim=False)[0]


def edgeconv_stack_pair(x, k, convs, training=None, preps=None, weights=None):
    """The engine's chain contract (dgx.edgeconv.edgeconv_stack_pair): the
    blocks' outputs concatenated point-major (B*N, sum Co), and an empty bf16
    twin. Block l > 1 searches its neighbours on the previous block's
    contiguous (B, C, N) output, as the reference does (dgcnn.py:86-96)."""
    if x.dtype != torch.float32:
        x = x.float()
    B, _, N = x.shape
    h, outs = x, []
    for li, seq in enumerate(convs):
        h = edgeconv_block(h, k, seq, None if weights is None else weights[li])
        outs.append(h)
    cat = torch.cat(outs, dim=1)                                    # (B, sum Co, N)  dgcnn.py:100
    return cat.permute(0, 2, 1).reshape(B * N, -1), torch.empty(0, dtype=torch.bfloat16)


def pointconv_bn_lrelu(X, B, N, seq, training=None, X16=None, wprep=None):
    """X (B*N, K) point-major -> (B, Co, N) = seq(X) with the modules of seq
    (reference dgcnn.py:100-102: conv5 on the unsqueezed concat)."""
    K = X.shape[1]
    z = X.view(B, N, K).permute(0, 2, 1)
    if isinstance(seq[0], torch.nn.Conv2d):
        return seq(z.unsqueeze(-1)).view(B, -1, N)
    return seq(z)


def edge_mlp2(x, k, conv1, conv2, training=None, knn_src=None):
    """max_k conv2(conv1(get_graph_feature(x, k))) (reference layers.py:45-52):
    conv1 decomposed over the kNN graph, conv2 on the (B, C1, N, k) edges."""
    if x.dtype != torch.float32:
        x = x.float()
    idx = knn(knn_src if knn_src is not None else x, k)
    c1, bn1, a1 = conv1[0], conv1[1], conv1[2]
    y1 = _edge_values(x, idx, c1.weight)
    h1 = a1(bn1(y1))
    return conv2(h1).max(dim=-1, keepdim=False)[0].contiguous()


def vattn_params(pos_mlp, attn_mlp):
    """(w1, b1, w2, b2) of pos_mlp then of attn_mlp: Linear-ReLU-Linear Sequentials
    (reference attention.py:93-105), or already a sequence of those four tensors."""
    out = []
    for m in (pos_mlp, attn_mlp):
        out += [m[0].weight, m[0].bias, m[2].weight, m[2].bias] if isinstance(m, torch.nn.Module) else list(m)
    return out


def vattn_edges(Dj, Vj, delta, params):
    """The per-edge body of VectorAttention.forward (reference attention.py:121-150)
    on gathered rows Dj = (q - k)[idx], Vj = v[idx] (P, k, Dm) and delta (P, k, 3),
    in the reference's op order -> agg (P, Dm). Any dtype and device."""
    pw1, pb1, pw2, pb2, aw1, ab1, aw2, ab2 = params
    r = F.linear(F.relu(F.linear(delta, pw1, pb1)), pw2, pb2)          # attention.py:121
    sim = F.linear(F.relu(F.linear(Dj + r, aw1, ab1)), aw2, ab2)       # :141
    attn = F.normalize(sim.softmax(dim=-1), dim=-2)                     # :145-146
    return torch.einsum('ijd,ijd->id', attn, Vj + r).contiguous()      # :137, :150


def vattn_rows(idx, gather_stride):
    """(B*N, k) int64 rows of the gather tables: b * gather_stride + id."""
    B, N, k = idx.shape
    off = torch.arange(B, device=idx.device).view(B, 1, 1) * int(gather_stride)
    return (idx.long() + off).view(B * N, k)


def vector_attention(D, V, pos, idx, pos_mlp, attn_mlp, gather_stride=0):
    """The composed kNN vector attention (reference attention.py:115-150): D =
    w_q(query) - w_k(key) and V = w_v(value) as (rows, Dm) tables, pos (B*N, 3),
    idx (B, N, k) local ids; the gathered row of cloud b is b * gather_stride + id
    (0: the reference's gather of cloud 0's rows) -> agg (B*N, Dm). Generic in
    dtype and device, differentiable by torch autograd in everything but idx."""
    B, N, k = idx.shape
    rows = vattn_rows(idx, gather_stride).view(-1)
    Dj = D[rows].view(B * N, k, -1)
    Vj = V[rows].view(B * N, k, -1)
    delta = pos[rows].view(B * N, k, 3) - pos.view(B * N, 1, 3)
    return vattn_edges(Dj, Vj, delta, vattn_params(pos_mlp, attn_mlp))


def hog_1x1(x, idx):
    """compute_hog_1x1 after its kNN call (reference model_partseg.py:28-92) on
    the host, as the reference runs it: LAPACK SVD (numpy) of every point's
    centred neighbourhood, the first right singular vector's angles voted into
    9 bins of 20 degrees per angle, L2-normalised. The neighbourhood gather uses
    LOCAL ids over x.view(B*N, -1), as the reference does."""
    B, _, P = x.shape
    k = idx.shape[-1]
    nn_idx = idx.reshape(-1)
    x_nn = x.contiguous().view(B * P, -1)[nn_idx, :].view(B, P, k, 3)
    centered = x_nn - x_nn.mean(dim=2, keepdim=True)
    _, s, v = np.linalg.svd(centered.detach().numpy(), full_matrices=False)
    v = torch.from_numpy(v)
    s = torch.from_numpy(np.sqrt(s))
    grad = v[:, :, 0].reshape(B * P, -1)[nn_idx, :].view(B, P, k, 3)
    mag = s[:, :, 0].unsqueeze(-1).reshape(B * P, -1)[nn_idx, :].view(B, P, k, 1)
    zenith = torch.acos(grad[..., 2]).unsqueeze(-1) * 180 / np.pi
    azimuth = torch.atan(grad[..., 1] / grad[..., 0]).unsqueeze(-1) * 180 / np.pi
    cells = torch.cat((zenith.int(), azimuth.int(), mag), dim=-1)
    cells[cells < 0] += 180
    hist = torch.zeros((B, P, 9, 2))
    bins = torch.floor(cells[..., :2] / 20.0 - 0.5) % 9
    first = cells[..., 2].unsqueeze(-1) * ((20.0 * ((bins + 1) % 9 + 0.5) - cells[..., :2]) % 180) / 20.0
    second = cells[..., 2].unsqueeze(-1) * ((cells[..., :2] - 20.0 * (bins + 0.5)) % 180) / 20.0
    for c in range(9):
        hist[:, :, c] += (first * (bins == c)).sum(dim=2)
        hist[:, :, (c + 1) % 9] += (second * (bins == c)).sum(dim=2)
    return F.normalize(hist, p=2.0, dim=2).view(B, P, -1)


def ce_weights(dtype, n_class, smoothing=True, eps=0.2):
    """(w_true, w_other): the two values the reference's smoothed target takes
    (loss.py:13-14), as Python floats. The reference builds its target in the
    logits' dtype, so its expression is evaluated here on one-element tensors of
    that dtype at one-hot values 1 and 0; in fp16 the weights are fp16(0.8) and
    fp16(fp16(0.2) / (C - 1)) and no longer sum to 1 over a row. Without
    smoothing the target is the one-hot itself."""
    if n_class < 2:
        raise ValueError(f"dgx: a cross entropy over {n_class} class(es) has no smoothed target "
                         "(the reference divides by n_class - 1)")
    if not smoothing:
        return 1.0, 0.0
    hit = torch.tensor([1.0, 0.0], dtype=dtype)   # labelled class, any other class
    w = hit * (1 - eps) + (1 - hit) * eps / (n_class - 1)
    return float(w[0]), float(w[1])


def ce_target(logits, target, smoothing=True, eps=0.2):
    """The reference's soft target (loss.py:13-14) for (M, C) or (B, C, N)
    logits, built from its two values."""
    w_true, w_other = ce_weights(logits.dtype, logits.shape[1], smoothing, eps)
    return torch.full_like(logits, w_other).scatter_(1, target.long().unsqueeze(1), w_true)


def smoothed_cross_entropy(logits, target, smoothing=True, eps=0.2, return_pred=False):
    """Label-smoothed cross entropy with torch's own kernels (reference
    loss.py:4-21): soft target times log_softmax, summed over classes, mean
    over rows; F.cross_entropy without smoothing. (M, C) logits with (M,)
    labels or (B, C, N) with (B, N)."""
    if logits.shape[1] < 2:
        raise ValueError(f"dgx: a cross entropy needs at least 2 classes, got logits {tuple(logits.shape)}")
    if smoothing:
        loss = -(ce_target(logits, target, True, eps) * F.log_softmax(logits, dim=1)).sum(dim=1).mean()
    else:
        loss = F.cross_entropy(logits, target.long(), reduction="mean")
    return (loss, logits.detach().max(dim=1)[1]) if return_pred else loss


def seg_argmax(scores):
    """Arg-max over dim 1 with the loss head's rule (csrc/ce_row.h): the
    smallest index among equal maxima; a NaN never compares greater, so a row
    whose logit 0 is NaN keeps class 0 and a NaN elsewhere is passed over
    (torch's own max treats a NaN as the maximum)."""
    x = scores.detach().float()
    nan = torch.isnan(x)
    arg = torch.where(nan, torch.full_like(x, float("-inf")), x).argmax(dim=1)
    return torch.where(nan.select(1, 0), torch.zeros_like(arg), arg)


def seg_metrics_update(scores, seg, cat, part_start, part_count, confusion, iu, nparts, state, loss, loss_sum):
    """dgx_seg_metrics_update (include/dgx.h) with torch ops, on the state
    tensors of dgx.metrics.SegMetrics in place: ``scores`` (B, C, N) logits or
    (B, N) class ids, ``seg`` (B, N), ``cat`` (B,) or None. Each shape's
    (true, pred) pairs are counted as a bincount of ``true * C + pred`` (a
    scatter-add into a (B, C * C) table); invalid labels, categories and
    shapes beyond the capacity are counted as the kernel counts them."""
    C = confusion.shape[0]
    pred = seg_argmax(scores) if scores.is_floating_point() else scores.long()
    B = seg.shape[0]
    true, pred = seg.long().reshape(B, -1), pred.reshape(B, -1)
    ok = (true >= 0) & (true < C) & (pred >= 0) & (pred < C)
    flat = torch.where(ok, true * C + pred, torch.zeros_like(true))
    per = torch.zeros(B, C * C, dtype=torch.int64, device=seg.device).scatter_add_(1, flat, ok.long())
    confusion += per.sum(dim=0).view(C, C)
    invalid = (~ok).sum()
    if cat is not None:
        cat = cat.long().reshape(B)
        capacity, max_parts = iu.shape[0], iu.shape[1]
        cat_ok = (cat >= 0) & (cat < part_start.numel())
        c = torch.where(cat_ok, cat, torch.zeros_like(cat))
        start, count = part_start.long()[c], part_count.long()[c]
        cat_ok = cat_ok & (start >= 0) & (count >= 0) & (count <= max_parts) & (start <= C - count)
        count = torch.where(cat_ok, count, torch.zeros_like(count))
        invalid = invalid + (~cat_ok).sum()
        table = per.view(B, C, C)
        inter = table.diagonal(dim1=1, dim2=2)
        union = table.sum(dim=2) + table.sum(dim=1) - inter           # rowsum + colsum - I
        q = torch.arange(max_parts, device=seg.device)
        live = q[None, :] < count[:, None]
        part = torch.where(live, start[:, None] + q[None, :], torch.zeros_like(live, dtype=torch.int64))
        rec = torch.stack([inter.gather(1, part), union.gather(1, part)], dim=2) * live[:, :, None]
        slot = state[0] + torch.arange(B, device=seg.device)
        fits = (slot >= 0) & (slot < capacity)
        iu[slot[fits]] = rec[fits].to(iu.dtype)
        nparts[slot[fits]] = count[fits].to(nparts.dtype)
        state[2] += (~fits).sum()
        state[0] += B
    state[1] += invalid
    state[3] += B
    if loss is not None:
        loss_sum.copy_(loss_sum + loss.detach().to(torch.float32).reshape(loss_sum.shape))


def attention(q, k, v, heads, dropout_p=0.0, scale=None):
    """dropout(softmax(scale q k^T)) v per head on the host (torch's
    scaled_dot_product_attention, the kernel nn.MultiheadAttention uses)."""
    B, Nq, E = q.shape
    D = E // heads
    if scale is None:
        scale = 1.0 / math.sqrt(D)
    qh, kh, vh = (t.reshape(B, -1, heads, D).transpose(1, 2) for t in (q, k, v))
    o = F.scaled_dot_product_attention(qh, kh, vh, dropout_p=dropout_p, scale=scale)
    return o.transpose(1, 2).reshape(B, Nq, E)



# ---- dgx_batch_assemble (include/dgx.h) on the host: the same Philox4x32-10 words, the same stable argsort, the
# same fp32 operation sequence (numpy rounds every multiply and add on its own). The libm-dependent draws (theta,
# cos, sin, noise) are evaluated in fp64 and rounded once, so they may differ from the device's in the last bits.
BATCH_SHUFFLE, BATCH_TRANSLATE, BATCH_RANDOM3, BATCH_FORCE = 1, 1 << 1, 2 << 1, 8
BATCH_ORDERS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))   # 0 translate, 1 jitter, 2 rotate
_B_CURSOR, _B_EPOCH, _B_INVALID, _B_OVERRUN, _B_BATCHES = 0, 1, 2, 3, 4
_U32 = np.uint64(0xFFFFFFFF)
_f32 = np.float32


def batch_flags(shuffle_points, augment, order=None, switches=None):
    """The flags word of dgx_batch_assemble. ``order`` (0..5) and ``switches``
    (bit a: augmentation a on) force the random3 draw (tests only)."""
    aug = {"none": 0, "translate": BATCH_TRANSLATE, "random3": BATCH_RANDOM3}
    if augment not in aug:
        raise ValueError(f"dgx: augment is one of {sorted(aug)}, got {augment!r}")
    flags = (BATCH_SHUFFLE if shuffle_points else 0) | aug[augment]
    if order is not None or switches is not None:
        if augment != "random3" or not 0 <= int(order or 0) <= 5 or not 0 <= int(switches or 0) <= 7:
            raise ValueError("dgx: a forced draw needs augment='random3', order 0..5 and switches 0..7")
        flags |= BATCH_FORCE | int(order or 0) << 4 | int(switches or 0) << 7
    return flags


def philox4x32(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al., SC'11) on broadcastable integer arrays:
    the four output words as uint32 arrays."""
    c0, c1, c2, c3 = (np.asarray(v).astype(np.uint64) & _U32 for v in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = np.uint64(int(k0) & 0xFFFFFFFF), np.uint64(int(k1) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _U32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _U32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & _U32, (k1 + np.uint64(0xBB67AE85)) & _U32
    return tuple(v.astype(np.uint32) for v in (c0, c1, c2, c3))


def _unit(w):      # U(w): [0, 1), exact in fp32
    return (np.asarray(w, np.uint32) >> np.uint32(8)).astype(_f32) * _f32(2.0 ** -24)


def _normal64(wr, wa, sin=False):
    """Box-Muller in fp64 from the words' exact fp32 uniforms: R(wr) cos / sin(2 pi U(wa))."""
    u1 = ((np.asarray(wr, np.uint32) >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24
    ang = 2.0 * np.pi * _unit(wa).astype(np.float64)
    return np.sqrt(-2.0 * np.log(u1)) * (np.sin(ang) if sin else np.cos(ang))


def batch_words(item, epoch, seed, stream, block):
    return philox4x32(np.uint32(int(item) & 0xFFFFFFFF), np.uint32(int(epoch) & 0xFFFFFFFF), stream, block,
                      int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)


def batch_draws64(item, epoch, seed, n_points):
    """The libm-dependent draws of one cloud in fp64 from the same integer
    words: (theta, noise (n_points, 3) before rounding to fp32)."""
    w = batch_words(item, epoch, seed, 0, 0)
    theta = 2.0 * np.pi * float(_normal64(w[2], w[3]))
    g = batch_words(item, epoch, seed, 2, np.arange(n_points, dtype=np.uint32))
    z = np.stack([_normal64(g[0], g[1]), _normal64(g[0], g[1], sin=True), _normal64(g[2], g[3])], axis=1)
    return theta, np.clip(0.01 * z, -0.02, 0.02)


def batch_params(item, epoch, seed, flags):
    """One cloud's stream-0 draws: the (16,) fp32 row that dgx_batch_assemble
    exports as ``params``."""
    q = np.zeros(16, _f32)
    aug = (flags >> 1) & 3
    q[4:7] = 1.0
    q[11] = 1.0
    if aug:
        w0 = batch_words(item, epoch, seed, 0, 0)
        order, sw = (int(w0[0]) % 6, int(w0[1]) & 7) if aug == 2 else (0, 1)
        if flags & BATCH_FORCE:
            order, sw = min((flags >> 4) & 7, 5), (flags >> 7) & 7
        w1, w2 = batch_words(item, epoch, seed, 0, 1), batch_words(item, epoch, seed, 0, 2)
        q[0] = order
        q[1:4] = [(sw >> a) & 1 for a in range(3)]
        q[4:7] = _f32(2.0) / _f32(3.0) + _unit(np.stack(w1[:3])) * (_f32(5.0) / _f32(6.0))
        q[7:10] = _f32(-0.2) + _unit(np.stack(w2[:3])) * _f32(0.4)
        q[10] = _f32(2.0 * np.pi) * _f32(_normal64(w0[2], w0[3]))
        q[11], q[12] = np.cos(np.float64(q[10])), np.sin(np.float64(q[10]))
    q[13:15] = np.array([int(item) & 0xFFFFFFFF, int(epoch) & 0xFFFFFFFF], np.uint32).view(_f32)
    return q


def batch_perm(item, epoch, seed, n_points):
    """The shuffle of one cloud's first ``n_points`` points: a stable argsort
    of the stream-1 keys (the order of the distinct words (key << 32) | j)."""
    j = np.arange(n_points, dtype=np.uint32)
    words = np.stack(batch_words(item, epoch, seed, 1, j >> np.uint32(2)))   # (4, n): word r of block j / 4
    return np.argsort(words[j & np.uint32(3), j], kind="stable").astype(np.int32)


def batch_apply(pc, params, noise):
    """The augmentations of one cloud ``pc`` (N, 3) fp32 in the order and with
    the switches of its ``params`` row, each operation rounded to fp32 on its
    own: translate is data.translate_pointcloud's ``pc * scale + shift``."""
    pc = np.array(pc, _f32)
    scale, shift, c, s = params[4:7], params[7:10], params[11], params[12]
    for op in BATCH_ORDERS[int(params[0])]:
        if not params[1 + op]:
            continue
        if op == 0:
            pc = pc * scale + shift
        elif op == 1:
            pc = pc + noise
        else:
            x, z = pc[:, 0].copy(), pc[:, 2].copy()
            pc[:, 0] = x * c + z * s
            pc[:, 2] = -(x * s) + z * c
    return pc


def batch_assemble(points, seg, label, order, state, B, N, seg_start, ncat, seed, flags, out, seg_out=None,
                   label_out=None, onehot=None, perm=None, params=None, noise=None):
    """dgx_batch_assemble on host tensors, outputs and ``state`` in place."""
    pts = points.numpy()
    n_items, n_epoch = pts.shape[0], order.numel()
    cursor, epoch = int(state[_B_CURSOR]), int(state[_B_EPOCH])
    aug = (flags >> 1) & 3
    for b in range(B):
        slot = cursor + b
        if cursor < 0 or slot >= n_epoch:
            state[_B_OVERRUN] += 1
            continue
        item = int(order[slot])
        ok = 0 <= item < n_items
        lab = int(label[item]) if ok and label is not None else 0
        if ok and ncat > 0 and not 0 <= lab < ncat:
            ok = False
        if not ok:
            state[_B_INVALID] += 1
            for t in (out, seg_out, label_out, onehot, perm, params, noise):
                if t is not None:
                    t[b].zero_()
            continue
        src = batch_perm(item, epoch, seed, N) if flags & BATCH_SHUFFLE else np.arange(N, dtype=np.int32)
        pc = pts[item, src.astype(np.int64)]
        q = batch_params(item, epoch, seed, flags)
        if aug:
            nz = None
            if noise is not None or q[2]:
                nz = batch_draws64(item, epoch, seed, N)[1].astype(_f32)
            pc = batch_apply(pc, q, nz)
            if noise is not None:
                noise[b] = torch.from_numpy(nz)
        out[b] = torch.from_numpy(np.ascontiguousarray(pc.T))
        if seg_out is not None:
            seg_out[b] = torch.from_numpy(seg.numpy()[item, src.astype(np.int64)].astype(np.int64) - int(seg_start))
        if label_out is not None:
            label_out[b] = lab
        if onehot is not None:
            onehot[b].zero_()
            onehot[b, lab] = 1.0
        if perm is not None:
            perm[b] = torch.from_numpy(src)
        if params is not None:
            params[b] = torch.from_numpy(q)
    if 0 <= cursor < n_epoch:
        state[_B_CURSOR] = min(cursor + B, n_epoch)
    state[_B_BATCHES] += 1
