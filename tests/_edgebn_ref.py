"""fp64 restatements of the per-channel BatchNorm arithmetic between the gather
and the scatter of an EdgeConv block (csrc/edgeconv.hip: bn_finalize, eval
affine, BN + LeakyReLU apply, dz and its partials, backward finalize; the
schedule's batch_stats / backward_consts / compact of csrc/dgx_torch.cpp;
include/dgx.h section a3, dgx/bn.py; reference models/dgcnn.py:54-98), and the
given data the oracle tests hand to the C ABI. Everything a kernel receives is
given data: each restatement evaluates the documented formula from the same
fp32 / fp64 inputs, in plain torch fp64 (any device) or exact rational
arithmetic where a cancellation would otherwise cost the reference digits.

  finalize    mean = S1 / count, var = max(S2 / count - mean^2, 0),
              invstd = 1 / sqrt(var + eps), a = gamma invstd, b = beta - mean a,
              rm' = (1 - m) rm + m mean, rv' = (1 - m) rv + m var count / (count - 1)
              (var itself when count <= 1), m = momentum, or 1 / (nbt + 1) when
              momentum < 0 (0 without a counter), nbt' = nbt + 1.
              S1, S2: the column sums of the (nrows, 2, Co) partial rows, summed
              exactly (math.fsum); mean and var in rational arithmetic.
  eval_affine fp32 by contract: invstd = 1 / sqrtf(rv + (float)eps)
  apply       z = fl32(a y + b) (ONE rounding of the exact value: an fma),
              out = z > 0 ? z : fl32(z slope), twin = bf16 RNE of out
  dz          d = fl32(dY (a y + b > 0 ? 1 : slope)): the sign of the exact
              a y + b, the slope branch at exactly 0; packed word =
              (bits(d) & ~63) | arg
  dz partials per row block: (sum d, sum d (y - mean) invstd) of the unpacked d
  bwd_consts  dbeta = S1 (+ prev), dgamma = S2 (+ prev), g_i = S_i / count,
              c0 = a (-g1 + g2 mean invstd), c1 = -a g2 invstd

EXACT ROUNDING. a y is exact in fp64 (24 x 24 bits); the sum a y + b is formed
with the error-free TwoSum (s + e = a y + b exactly, |e| <= ulp64(s) / 2) and
rounded to fp32 once: fl32(s) unless s is exactly the midpoint of two fp32
neighbours and e != 0, where e breaks the tie (a non-midpoint fp64 s and s + e
lie on the same side of every fp32 midpoint, all of which are fp64 numbers).
s == 0 iff a y + b == 0, else sign(s) is the exact sign. So apply and dz are
reproducible bit for bit on any finite data; only sums carry bounds.

BOUNDS (u = 2^-24; none comes from a run).
  finalize, bwd_consts: each output is an fp64 value rounded once to fp32: half
    an fp32 ulp of the result (in the binade of |ref| + its propagated bound),
    plus the first-order propagation of the kernel's fp64 summation error
    e_i = nrows 2^-53 sum|p_i| :  dmean = e1 / count,
    dvar = e2 / count + 2 |mean| dmean,  dinvstd = invstd^3 dvar / 2,
    da = |gamma| dinvstd,  db = |a| dmean + |mean| da,  drm = m dmean,
    drv = m dvar count / (count - 1);  ddbeta = e1, ddgamma = e2,
    dc0 = |a| (e1 + e2 |mean invstd|) / count,  dc1 = |a invstd| e2 / count.
    Through the schedule's `compact` (more than 1024 partial rows are first
    summed in fp32 as S slabs of 128 rows) e_i grows by (S + 3) u sum|p_i|.
  eval_affine: fp32 throughout. rv + eps rounds (u); the square root halves that
    and rounds (allow 1 ulp = 2u); the reciprocal rounds (allow 2u): invstd to
    5u |invstd| (4.5 rounded up). a = gamma invstd rounds once more: 6u |a|.
    b = beta - rm a, contracted to an fma or not: |rm| times a's error plus a
    rounding of the product and one of the difference: 7u |rm a| + u |b|.
  dz partials: d exact; (y - mean), (.) invstd and the fma into the sum round
    (3u of the term), the n-row block is summed by four waves and four adds:
    (n + 4) u sum|term|, n the number of rows of the block. Blocks past M hold 0.

LATTICE CASES (bit-exact). Small integers times powers of two, so every product
and sum the kernels form is exact whatever the order:
  finalize   count in {1, 2, 4}; mean a multiple of 1/4, |mean| <= 2; eps = 1/4
             and var in {3/4, 15/4, 63/4}: var + eps in {1, 4, 16}, invstd in
             {1, 1/2, 1/4}, and the unbiased var count / (count - 1) is 2 var or
             4 var / 3 = 1, 5, 21; gamma in +-{1/2, 1, 2, 3}, beta a multiple of
             1/4; momentum 1/4, or nbt in {0, 1, 3} (factor 1, 1/2, 1/4); the
             partial rows are multiples of 1/16 (fp32 and fp64 alike) whose
             column sums hit count mean and count (var + mean^2); one channel
             has S2 / count - mean^2 = -1/2 (the clamp: invstd = 1 / sqrt(eps) = 2)
  apply, dz  y a multiple of 1/4, |y| <= 2; a in +-{1/2, 1, 2}; b = -a y0 for a
             lattice y0 (exact zeros of z in every channel); slope 1/4; dY a
             multiple of 1/16, |dY| <= 4; mean a multiple of 1/4, invstd in
             {1/2, 1, 2}: d a multiple of 1/64, yhat of 1/8 with |yhat| <= 8,
             d yhat of 1/512 with |d yhat| <= 32; a block of n <= 64 rows sums
             to < 2^20 quanta (assert_dz_exact checks sum|term| / q < 2^24)
  bwd_consts count a power of two, partial rows multiples of 1/16 with |p| <= 4,
             a in +-{1/2, 1, 2}, mean a multiple of 1/4, invstd in {1/2, 1, 2}:
             every output has at most 24 significant bits (checked: the fp64
             reference must survive a round trip through fp32)
"""
import math
from fractions import Fraction

import torch

from _edgemlp_ref import (SENT, SLOPE_LATTICE, SLOPE_RANDOM, U, Case, _choice, bf16_round, f32_value,  # noqa: F401
                          guard_intact, guarded, lrelu_grad, rowsum, within, worst)

U53 = 2.0 ** -53
LIM = float(2 ** 24)
F64 = torch.float64


def half_ulp32(x, slack=0.0):
    """half an fp32 ulp in the binade of |x| + slack (0 at 0)"""
    m = x.abs() + slack
    _, e = torch.frexp(m)                                   # m = f 2^e, f in [0.5, 1)
    h = torch.ldexp(torch.ones_like(m), e - 25)             # 2^(floor(log2 m) - 24)
    return torch.where(m > 0, h, torch.zeros_like(m))


def exact_sums(partials):
    """(S, A), each (2, Co) fp64 on the CPU: the correctly rounded column sums of
    the (nrows, 2, Co) partial rows and of their magnitudes"""
    p = partials.detach().double().cpu()
    cols = p.reshape(p.shape[0], -1).t().tolist()
    S = torch.tensor([math.fsum(c) for c in cols], dtype=F64)
    A = torch.tensor([math.fsum(abs(v) for v in c) for c in cols], dtype=F64)
    return S.view(2, -1), A.view(2, -1)


def with_count(sums, count):
    """the device-count form's buffer: the fp64 sums, then the element count"""
    return torch.cat([sums.double().reshape(-1), torch.tensor([float(count)], dtype=F64)])


def _split_count(partials, count, co):
    if count < 0:
        flat = partials.detach().double().cpu().reshape(-1)
        return flat[:-1].view(-1, 2, co), float(flat[-1])
    return partials, float(count)


def _sum_error(nrows, slabs, A):
    return (nrows * U53 + ((slabs + 3) * U if slabs else 0.0)) * A


def compact_slabs(rows):
    """the number of 128-row slabs the schedule's `compact` pre-reduces in fp32 (0: none)"""
    return rows // 128 if rows > 1024 else 0


def _fr(t):
    return [Fraction(v) for v in t.tolist()]


def _d(t):
    return None if t is None else t.detach().double().cpu()


def finalize(partials, count, gamma, beta, rm, rv, momentum, eps, nbt, co=None, slabs=0):
    """-> Case with scale, shift, mean, invstd, rm, rv (fp64 (Co,), None where the
    input is absent), nbt (int or None) and the bound of each as <name>_b.
    count < 0: `partials` is with_count(sums, count) and `co` its channel count."""
    partials, count = _split_count(partials, count, co)
    nrows = partials.shape[0]
    S, A = exact_sums(partials)
    cnt = Fraction(count)
    mean_q = [s / cnt for s in _fr(S[0])]
    var_q = [max(s2 / cnt - m * m, Fraction(0)) for s2, m in zip(_fr(S[1]), mean_q)]
    unb_q = [v * cnt / (cnt - 1) if cnt > 1 else v for v in var_q]
    mean, var, unb = (torch.tensor([float(v) for v in q], dtype=F64) for q in (mean_q, var_q, unb_q))
    e = _sum_error(nrows, slabs, A)
    dmean = e[0] / abs(count)
    dvar = e[1] / abs(count) + 2 * mean.abs() * dmean
    invstd = 1.0 / torch.sqrt(var + eps)
    dinv = 0.5 * invstd ** 3 * dvar
    g = _d(gamma) if gamma is not None else torch.ones_like(mean)
    b = _d(beta) if beta is not None else torch.zeros_like(mean)
    a = g * invstd
    da = g.abs() * dinv
    r = Case()

    def put(name, val, prop):
        setattr(r, name, val)
        setattr(r, name + "_b", half_ulp32(val, prop) + prop)

    put("scale", a, da)
    put("shift", b - mean * a, a.abs() * dmean + mean.abs() * da)
    put("mean", mean, dmean)
    put("invstd", invstd, dinv)
    if momentum < 0:
        m = 1.0 / (nbt + 1) if nbt is not None else 0.0
    else:
        m = momentum
    r.rm = r.rv = r.rm_b = r.rv_b = None
    if rm is not None:
        put("rm", (1.0 - m) * _d(rm) + m * mean, m * dmean)
    if rv is not None:
        put("rv", (1.0 - m) * _d(rv) + m * unb, m * dvar * (count / (count - 1) if count > 1 else 1.0))
    r.nbt = None if nbt is None else nbt + 1
    r.var, r.momentum = var, m
    return r


def eval_affine(gamma, beta, rm, rv, eps):
    """-> Case scale, shift, invstd (+ _b) of the fp32 eval-mode affine
    1 / sqrtf(rv + (float)eps). Bounds (module docstring, "eval_affine"): three
    fp32 operations lead to invstd (add u, root u/2 of that + 2u, reciprocal 2u:
    5u), one more product to a (6u), product and difference to b."""
    rm, rv = rm.detach().double(), rv.detach().double()
    invstd = 1.0 / torch.sqrt(rv + f32_value(eps))
    g = gamma.detach().double() if gamma is not None else torch.ones_like(rm)
    b = beta.detach().double() if beta is not None else torch.zeros_like(rm)
    r = Case()
    r.invstd, r.invstd_b = invstd, 5 * U * invstd
    r.scale = g * invstd
    r.scale_b = 6 * U * r.scale.abs()
    r.shift = b - rm * r.scale
    r.shift_b = 7 * U * (rm * r.scale).abs() + U * r.shift.abs()
    return r


def _two_sum(p, q):
    s = p + q
    bb = s - p
    return s, (p - (s - bb)) + (q - bb)


def fl32(s, e):
    """the exact s + e (|e| <= ulp64(s) / 2) rounded once to fp32, as fp64"""
    f = s.float()
    r = s - f.double()
    inf = torch.full_like(f, float("inf"))
    g = torch.nextafter(f, torch.where(r > 0, inf, -inf))
    tie = (r != 0) & (r == g.double() - s) & (e != 0)
    return torch.where(tie & ((e > 0) == (r > 0)), g, f).double()


def affine(ysel, scale, shift):
    """(s, e) with s + e = a y + b exactly; (M, Co) fp64"""
    return _two_sum(scale.double() * ysel.double(), shift.double().expand_as(ysel))


def apply(ysel, scale, shift, slope):
    """-> (out, bf16 twin, z == 0 mask); out holds fp32 values as fp64"""
    s, e = affine(ysel, scale, shift)
    z = fl32(s, e)
    out = torch.where(z > 0, z, (z * slope).float().double())
    return out, bf16_round(out), s == 0


def dz(dY, ysel, scale, shift, slope, f32=True):
    """-> (d, z > 0 mask, z == 0 mask); d holds fp32 values as fp64 (f32=False:
    the unrounded product, for fp64 data)"""
    s, _ = affine(ysel, scale, shift)
    g = dY.double()
    gs = g * slope
    return torch.where(s > 0, g, gs.float().double() if f32 else gs), s > 0, s == 0


def packed(d, arg):
    """the packed dz words as int32: (bits(d) & ~63) | arg"""
    return (d.float().contiguous().view(torch.int32) & ~63) | arg.to(torch.int32)


def row_blocks(M, nrows):
    """block of every row for dgx_edge_bwd_dz[_packed]_f32: [b rows, min((b + 1) rows, M))"""
    rows = -(-M // nrows)
    return torch.arange(M) // rows


def cm_blocks(B, N):
    """(block of every point, nrows) for the channel-major form: b ceil(N / 64) + n // 64"""
    tiles = -(-N // 64)
    n = torch.arange(N)
    return (torch.arange(B).view(B, 1) * tiles + (n // 64).view(1, N)).reshape(-1), B * tiles


def dz_partials(d, ysel, mean, invstd, blocks, nrows):
    """-> (partials (nrows, 2, Co) fp64, bound, sum|term|)"""
    y = ysel.double()
    t2 = d * ((y - mean.double()) * invstd.double())
    blocks = blocks.to(d.device)
    part = torch.stack([rowsum(d, blocks, nrows), rowsum(t2, blocks, nrows)], 1)
    mag = torch.stack([rowsum(d.abs(), blocks, nrows), rowsum(t2.abs(), blocks, nrows)], 1)
    n = torch.bincount(blocks, minlength=nrows).double().view(nrows, 1, 1)
    return part, (n + 4) * U * mag, mag


def assert_dz_exact(mag):
    """the lattice condition of the dz partial sums: quanta 1/64 and 1/512"""
    assert float(mag[:, 0].max()) * 64 < LIM and float(mag[:, 1].max()) * 512 < LIM


def bwd_consts(partials, count, scale, mean, invstd, accumulate, prev=None, co=None, slabs=0, eval=False):
    """-> Case dgamma, dbeta, c0, c1 (+ _b). prev = (dgamma, dbeta) before the
    call, added when `accumulate`. count < 0: the device-count form, as finalize.
    eval: the fixed affine of running statistics, c0 = c1 = 0 exactly (dgx/bn.py)."""
    partials, count = _split_count(partials, count, co)
    nrows = partials.shape[0]
    S, A = exact_sums(partials)
    e = _sum_error(nrows, slabs, A)
    a, mu, ist = _d(scale), _d(mean), _d(invstd)
    cnt = Fraction(count)
    fa, fm, fi = _fr(a), _fr(mu), _fr(ist)
    g1, g2 = [s / cnt for s in _fr(S[0])], [s / cnt for s in _fr(S[1])]
    c0 = torch.tensor([float(x * (-p + q * m * i)) for x, p, q, m, i in zip(fa, g1, g2, fm, fi)], dtype=F64)
    c1 = torch.tensor([float(-x * q * i) for x, q, i in zip(fa, g2, fi)], dtype=F64)
    db, dg = S[0].clone(), S[1].clone()
    if accumulate:
        dg, db = dg + _d(prev[0]), db + _d(prev[1])
    r = Case()
    for name, val, prop in (("dbeta", db, e[0]), ("dgamma", dg, e[1]),
                            ("c0", c0, a.abs() * (e[0] + e[1] * (mu * ist).abs()) / abs(count)),
                            ("c1", c1, (a * ist).abs() * e[1] / abs(count))):
        if eval and name in ("c0", "c1"):
            val, prop = torch.zeros_like(val), torch.zeros_like(prop)
        setattr(r, name, val)
        setattr(r, name + "_b", half_ulp32(val, prop) + prop)
    return r


def fits_f32(*tensors):
    """every value survives a round trip through fp32 (the lattice outputs' condition)"""
    return all(bool((t.float().double() == t).all()) for t in tensors if t is not None)


# ---- given data -------------------------------------------------------------------

EPS_LATTICE = 0.25
EPS_RANDOM = 1e-5
VARS = (0.75, 3.75, 15.75)
RS = (0.0, 4.0, 64.0)


def clamp_channel(Co):
    return Co - 1


def make_finalize_case(kind, Co, nrows, count, seed, f64=False):
    """Partial rows (nrows, 2, Co) (fp32, or fp64 for the f64 entries), gamma,
    beta, running statistics; c.count, c.eps. Lattice: module docstring. Random:
    the rows are the block sums of normal samples with |mean| / std = RS[c % 3]
    (count = 4 nrows samples), rounded to the partials' type; the clamp channel
    (the last) has its sum y doubled at r = 4, so S2 / count - mean^2 < 0."""
    g = torch.Generator().manual_seed(seed)
    c = Case()
    c.kind, c.Co, c.nrows = kind, Co, nrows
    cc = clamp_channel(Co)
    if kind == "lattice":
        c.count, c.eps = float(count), EPS_LATTICE
        mean = torch.randint(-8, 9, (Co,), generator=g).double() / 4
        var = torch.tensor([VARS[o % 3] for o in range(Co)], dtype=F64)
        e2 = var + mean ** 2
        mean[cc], e2[cc] = 1.0, 0.5
        p = torch.randint(-32, 33, (nrows, 2, Co), generator=g).double() / 16
        p[0] = 0
        p[0] = torch.stack([c.count * mean, c.count * e2]) - p.sum(0)
        c.gamma = _choice(g, [-3.0, -2.0, -1.0, -0.5, 0.5, 1.0, 2.0, 3.0], (Co,))
        c.beta = torch.randint(-8, 9, (Co,), generator=g).float() / 4
        c.rm = torch.randint(-8, 9, (Co,), generator=g).float() / 4
        c.rv = torch.randint(1, 17, (Co,), generator=g).float() / 4
        c.momentum = 0.25
    else:
        c.count, c.eps = 4.0 * nrows, EPS_RANDOM
        r = torch.tensor([RS[o % 3] for o in range(Co)], dtype=F64)
        r[cc] = 4.0
        y = torch.randn(nrows, 4, Co, generator=g, dtype=F64) + r * (1 - 2 * (torch.arange(Co) % 2))
        p = torch.stack([y.sum(1), (y * y).sum(1)], 1)
        p[:, 0, cc] *= 2
        c.gamma, c.beta = torch.randn(Co, generator=g), 0.3 * torch.randn(Co, generator=g)
        c.rm, c.rv = torch.randn(Co, generator=g), torch.rand(Co, generator=g) + 0.5
        c.momentum = 0.1
    c.partials = p if f64 else p.float()
    if kind == "lattice":
        assert torch.equal(c.partials.double(), p)
    return c


def make_bwdfin_case(kind, Co, nrows, seed, f64=False):
    g = torch.Generator().manual_seed(seed)
    c = Case()
    c.kind, c.Co, c.nrows = kind, Co, nrows
    if kind == "lattice":
        c.count = 64.0
        p = torch.randint(-64, 65, (nrows, 2, Co), generator=g).double() / 16
        c.scale = _choice(g, [-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], (Co,))
        c.mean = torch.randint(-8, 9, (Co,), generator=g).float() / 4
        c.invstd = _choice(g, [0.5, 1.0, 2.0], (Co,))
        c.prev = (torch.randint(-64, 65, (Co,), generator=g).float() / 16,
                  torch.randint(-64, 65, (Co,), generator=g).float() / 16)
    else:
        c.count = 20.0 * nrows
        p = torch.randn(nrows, 2, Co, generator=g, dtype=F64)
        c.scale, c.mean = torch.randn(Co, generator=g), torch.randn(Co, generator=g)
        c.invstd = torch.rand(Co, generator=g) + 0.5
        c.prev = (torch.randn(Co, generator=g), torch.randn(Co, generator=g))
    c.partials = p if f64 else p.float()
    return c


def make_edge_case(kind, M, Co, seed, k=64):
    """ysel, dY (M, Co), arg (M, Co) u8 spanning 0..k-1, per-channel scale, shift,
    mean, invstd; c.slope. Lattice: b = -a y0, so z has exact zeros in every
    channel (row 0 is planted on y0: at least one zero per channel)."""
    g = torch.Generator().manual_seed(seed)
    c = Case()
    c.kind, c.M, c.Co = kind, M, Co
    if kind == "lattice":
        c.slope = SLOPE_LATTICE
        c.ysel = torch.randint(-8, 9, (M, Co), generator=g).float() / 4
        c.scale = _choice(g, [-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], (Co,))
        y0 = torch.randint(-4, 5, (Co,), generator=g).float() / 4
        c.ysel[:1] = y0
        c.shift = -c.scale * y0
        c.dY = torch.randint(-64, 65, (M, Co), generator=g).float() / 16
        c.mean = torch.randint(-8, 9, (Co,), generator=g).float() / 4
        c.invstd = _choice(g, [0.5, 1.0, 2.0], (Co,))
    else:
        c.slope = f32_value(SLOPE_RANDOM)
        c.ysel, c.dY = torch.randn(M, Co, generator=g), torch.randn(M, Co, generator=g)
        c.scale, c.shift = torch.randn(Co, generator=g), 0.3 * torch.randn(Co, generator=g)
        c.mean, c.invstd = 0.1 * torch.randn(Co, generator=g), torch.rand(Co, generator=g) + 0.5
    c.arg = ((torch.arange(M).view(M, 1) * 7 + torch.arange(Co).view(1, Co) * 3) % k).to(torch.uint8)
    return c


# ---- the grids of tests/test_edgebn_kernels_gpu.py -----------------------------------
FIN_COS = (1, 3, 4, 5, 64, 130)
FIN_ROWS = (1, 63, 64, 65, 1024)
FIN_GRID = [(co, nr) for co in FIN_COS for nr in FIN_ROWS]
COMPACT_ROWS = (1024, 1025, 1151, 1152)      # no pre-reduce; left = 1, 127, 0
# apply: (M, Co, ldo, bf16 twin, out / ysel / twin offsets in elements, 4-wide kernel expected)
APPLY_GRID = [
    (7, 1, 1, 0, 0, 0, 0, False), (7, 3, 5, 1, 0, 0, 0, False), (5, 65, 65, 1, 0, 0, 0, False),
    (9, 65, 70, 0, 0, 0, 0, False),
    (7, 4, 4, 1, 0, 0, 0, True), (5, 64, 64, 0, 0, 0, 0, True), (5, 68, 72, 1, 0, 0, 0, True),
    (3, 64, 128, 1, 0, 0, 0, True),
    (5, 64, 65, 1, 0, 0, 0, False), (5, 68, 69, 0, 0, 0, 0, False),   # ldo odd
    (5, 64, 64, 0, 1, 0, 0, False), (5, 4, 8, 1, 1, 0, 0, False),     # out offset by one float
    (5, 64, 64, 1, 0, 1, 0, False), (5, 68, 72, 0, 0, 1, 0, False),   # ysel offset by one float
    (5, 64, 64, 1, 0, 0, 1, False), (5, 4, 8, 1, 0, 0, 1, False),     # bf16 twin offset by one element
]
APPLY_STRIDE_GRID = [(32771, 65, 65, 1), (131075, 68, 72, 1)]        # just past 8192 x 256 threads
DZ_COS = (1, 63, 64, 65, 130)
DZ_ROWS = ((1, 1), (5, 8), (64, 1), (65, 2), (130, 3), (1000, 16), (1091, 33))
DZ_GRID = [(M, nr, co, (0, 3, 64)[(i + j) % 3]) for i, (M, nr) in enumerate(DZ_ROWS) for j, co in enumerate(DZ_COS)]
CM_BS = (1, 3)
CM_NS = (1, 63, 64, 65, 130)
CM_GRID = [(CM_BS[(i + j) % 2], n, co) for i, n in enumerate(CM_NS) for j, co in enumerate(DZ_COS)]
