"""Python binding of the engine's GEMM layer (csrc/dgx_torch.cpp, "GEMMs" and
"bf16 weight prep"): each function here is one ``dgx_host`` op over the very
C++ helper the schedule calls, so operand classification, epilogue choice,
split-K and slab counts and output allocation are the product's own. Tests and
tools drive the GEMM kernels through it; the product itself uses the weight
prep (dgx.library) and ``SLAB_CAP_MB`` (dgx.schedule.opts).

Every GEMM is ``C[i][j] = sum_k opA(i,k) opB(j,k)`` with fp32 or bf16 operands
read in place (column slices of the concat buffer included). Three single
launches with no schedule arithmetic (mm_smallk, mm_smallk_split,
lds_xwt_edge_dz) go to the C ABI directly, as the schedule does inline.
"""
import torch

from . import _native as nat
from . import schedule as S


def mm_xwt(x, w, out=None, stats=False):
    """out (M,N) = x (M,K) @ w (N,K)^T; with ``stats`` also returns the column
    partials (rows, 2, N) of the train-mode BatchNorm statistics."""
    out, part = S.host_ops().gemm_xwt(x, w, out, stats, False, None, False)
    return (out, part) if stats else out


def mm32(a, b, out=None, accumulate=False, addend=None):
    """out (M,N) = a (M,K) @ b (K,N) on the engine's fp32 MFMA GEMM
    (dgx_gemm_f32, exact fp32 products): the parity mode's GEMMs. Transposed
    views are read in place; a long reduction (K >= 2048 over few outputs,
    the weight gradients over B*N rows) is split over workgroups into slabs
    summed in a fixed order (deterministic). ``accumulate``: out += a @ b;
    ``addend``: out = addend + a @ b."""
    return S.host_ops().gemm32(a, b, out, accumulate, addend)


SMALLK_MAX = 16


def mm_smallk(x, w):
    """Exact fp32 (M,N) = x (M,K) @ w (N,K)^T for K <= 16 (dgx_gemm_smallk_f32):
    the layer-1 GEMM on raw coordinates, exact in every precision mode."""
    M, K = x.shape
    N = w.shape[0]
    if x.stride(1) != 1:
        x = x.contiguous()
    w = w.contiguous()
    out = torch.empty((M, N), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        nat.check(nat.lib().dgx_gemm_smallk_f32(nat.f32(x), x.stride(0) if M > 1 else K, nat.f32(w), M, N, K,
                                                nat.f32(out), N, nat.stream_of(x)), "gemm small-k")
    return out


def mm_smallk_split(x, wref, co):
    """mm_smallk(x, [W1; W2]) for a conv weight wref (Co, 2K[,1,1]) = [W1 | W2]
    in the reference layout (dgx_gemm_smallk_split_f32): the EdgeConv PQ of the
    3-channel block, no reshuffled weight copy."""
    M, K = x.shape
    if x.stride(1) != 1:
        x = x.contiguous()
    w = wref.reshape(co, 2 * K)
    if not w.is_contiguous():
        w = w.contiguous()
    out = torch.empty((M, 2 * co), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        nat.check(nat.lib().dgx_gemm_smallk_split_f32(nat.f32(x), x.stride(0) if M > 1 else K, nat.f32(w), M, co, K,
                                                      nat.f32(out), 2 * co, nat.stream_of(x)), "gemm small-k")
    return out


def mm_xw(x, w, out=None, accumulate=False):
    """out (M,N) (+)= x (M,K) @ w (K,N)."""
    return S.host_ops().gemm_xw(x, w, out, accumulate)


def mm_atb(a, b, out, split_rows=None):
    """out = a^T @ b for a (R, M), b (R, N) (reduction over the R rows, split-K
    over workgroups, deterministic slab sum). ``split_rows`` = Co un-stacks a
    [W1;W2] result into out = [W1 | W2] (out is (M - Co, 2N))."""
    S.host_ops().gemm_atb(a, b, out, split_rows or 0, False, 0)
    return out


# ---- bf16-operand path (LDS-DMA staging, dgx_gemm_lds_bf16) ------------------

def _bf16_2d(t):
    if t.dtype != torch.bfloat16 or t.dim() != 2 or t.stride(1) != 1:
        raise RuntimeError("dgx gemm (bf16 path): operands must be row-major bf16 2-D views")
    return t.stride(0) if t.shape[0] > 1 else max(8, t.shape[1])


def lds_xwt(x16, w16, out=None, stats=False, accumulate=False, addend=None, out_bf16=False):
    """out (M,N) = x16 (M,K) @ w16 (N,K)^T (bf16 operands, K % 64 == 0).
    A split weight w16 (N, 2K) = [W_hi | W_lo] (prep_weights(..., split=True))
    gives x16 (W_hi + W_lo)^T: the weight with 16 significant bits.
    ``stats``: also returns the BatchNorm column partials (rows, 2, N);
    with ``out_bf16`` the product is stored bf16 (stats from the fp32 sums).
    ``accumulate``: out += ... (the output as its own addend, as the schedule
    does); with ``addend``: out = addend + ... ."""
    if accumulate and addend is None:
        addend = out
    out, part = S.host_ops().gemm_xwt(x16, w16, out, stats, out_bf16, addend, True)
    return (out, part) if stats else out


def lds_xwt_edge_dz(x16, w16, addend, ysel, arg, st, slope):
    """dY = addend + x16 @ w16^T with the previous EdgeConv block's LeakyReLU'
    applied in the epilogue (dgx_gemm_edge_dz_bf16): returns (packed dz|slot
    words (M, N) fp32, column partials (rows, 2, N), rows) — what
    dgx_edge_bwd_dz_packed_f32 would make from the stored dY."""
    M, K = x16.shape
    N = w16.shape[0]
    L = nat.lib()
    rows = L.dgx_gemm_edge_dz_rows(M, N)
    dz = torch.empty((M, N), dtype=torch.float32, device=x16.device)
    part = torch.empty((rows, 2, N), dtype=torch.float32, device=x16.device)
    if addend.dtype != torch.float32 or addend.stride(1) != 1:
        raise RuntimeError("dgx gemm: addend must be a row-major fp32 view")
    with torch.cuda.device(x16.device):
        nat.check(L.dgx_gemm_edge_dz_bf16(
            nat.ptr(x16), _bf16_2d(x16), nat.ptr(w16), _bf16_2d(w16), M, N, K, nat.f32(addend), addend.stride(0),
            nat.f32(ysel), nat.u8(arg), nat.f32(st.scale), nat.f32(st.shift), nat.f32(st.mean), nat.f32(st.invstd),
            float(slope), nat.f32(dz), nat.f32(part), rows, nat.stream_of(x16)), "gemm edge dz")
    return dz, part, rows


# cap (MiB) on the split-K slab of the small bf16 weight-gradient GEMMs (output
# < 1 MiB: the EdgeConv blocks' dW). Default 8: block 4's dW takes 32 splits
# instead of 128 (33.5 -> 8.4 MB of slab); measured at cfg2 1.3442 -> 1.3384
# ms/step (2 / 4 MB: 1.401 / 1.359, too few workgroups). DGX_SLAB_CAP_MB=0
# restores dgx_gemm_splits's own rule.
SLAB_CAP_MB = int(__import__("os").environ.get("DGX_SLAB_CAP_MB", "8"))


def lds_atb(a16, b16, out, split_rows=None):
    """out = a16^T @ b16 for a16 (R, M), b16 (R, N) bf16 (reduction over R rows,
    split-K slabs under SLAB_CAP_MB summed deterministically); ``split_rows``
    as in mm_atb."""
    S.host_ops().gemm_atb(a16, b16, out, split_rows or 0, True, SLAB_CAP_MB)
    return out


def prep_weight(w, rows, cols, stacked):
    """bf16 operand copies of a conv weight by the single-weight kernel
    (dgx_weight_prep_bf16): (nt (R, cols), tn (cols, R)) with R = 2*rows for a
    stacked EdgeConv weight (rows = Co, cols = C)."""
    return S.host_ops().weight_prep_one(w, rows, cols, stacked)


def prep_layout(shapes):
    """Layout of prep_weights' shared bf16 buffer for (rows, cols, stacked,
    split) jobs: (total elements, [(nt offset, nt shape, tn offset, tn shape)])
    with every view 16-byte aligned. Plain Python because dynamo and
    torch.export trace through it (dgx.library); the layout itself is the C++
    schedule's ``prep_views``, which dgx_host::weight_prep_layout reports — a
    test holds the two equal."""
    total, out = 0, []
    for (r, c, st, sp) in shapes:
        R = 2 * r if st else r
        n_tn, n_nt = R * c, (2 if sp else 1) * R * c
        p_tn, p_nt = -(-n_tn // 8) * 8, -(-n_nt // 8) * 8
        out.append((total, (R, 2 * c if sp else c), total + p_nt, (c, R)))
        total += p_nt + p_tn
    return total, out


def prep_views(buf, shapes):
    """[(nt, tn)] views of a prep_weights buffer (prep_layout's layout)."""
    _, lay = prep_layout(shapes)
    return [(buf[o1:o1 + s1[0] * s1[1]].view(s1), buf[o2:o2 + s2[0] * s2[1]].view(s2)) for (o1, s1, o2, s2) in lay]


def prep_weights(jobs, buf=None):
    """prep_weight for several (w, rows, cols, stacked[, split]) jobs in one
    launch (dgx_host::weight_prep); the bf16 copies share one allocation
    (``buf``, prep_layout's size, or a fresh one). Returns [(nt, tn), ...].
    ``split``: nt is (R, 2*cols) = [W_hi | W_lo] for lds_xwt's split-weight
    form; tn (the backward's operand) is W_hi^T either way."""
    if not jobs:
        return []
    ws, rows, cols, stacked, split = (list(f) for f in zip(*(tuple(j) + (False,) * (5 - len(j)) for j in jobs)))
    buf = S.host_ops().weight_prep(ws, rows, cols, stacked, split, buf)
    return prep_views(buf, list(zip(rows, cols, stacked, split)))


def edge_dz_ok(dpq16, cin):
    """Whether dgx_gemm_edge_dz_bf16 takes this block's input-gradient GEMM
    (dX columns = cin, K = dPQ width): the kernel's own limits (cin a multiple
    of 8 and <= 128, K a multiple of its 64-deep K step, 16-byte rows);
    otherwise the caller keeps the dY + dz-pass path."""
    return S.host_ops().gemm_edge_dz_ok(dpq16, cin)
