"""fp64 restatements of PositionEmbedding's per-edge MLP kernels (csrc/edgemlp.hip
and the two edge-MLP epilogues of csrc/gemm.hip; include/dgx.h section a6;
reference models/layers.py:45-52) and the given data the oracle tests hand to
the C ABI. Everything a kernel receives is given data, so each restatement is
the kernel's documented formula evaluated in float64 from the same fp32 / bf16
inputs (plain torch, any device). Edge rows e = i*k + s, i = global point,
j = cloud base + idx[e]:

  y    = P_j + Q_i,  z1 = a1 y + b1,  h1 = z1 > 0 ? z1 : slope z1     (E, C1)
  z2   = h1_bf16 W2^T                                                (E, C2)
  arg  = first slot s maximising dir2 z2 over the point's k edges,
  ysel = z2 there;  BN2 partial row (cloud b, 8-point tile t) = b*tiles + t:
         (sum z2, sum z2^2) over the row's edges
  dZ2  = c1 z2 + c0 + [arg == s] a2 dz                               (E, C2)
  dH1  = dZ2_bf16 W2,  g = dH1 (z1 > 0 ? 1 : slope)                  (E, C1)
  BN1-backward partial row = (sum g, sum g yhat), yhat = (y - mean1) invstd1,
         summed over the unrounded g (64-point tiles for the fused backward,
         128-edge-row tiles for the GEMM epilogue, grid-stride blocks for the
         fp32 kernel); dW2 slab row = sum_e dZ2_bf16[e]^T h1_bf16[e]
  dQ_i = a sum_s g + c0 k + c1 (k Q_i + sumP_i)
  dP_p = sum over p's in-edges (src, s) of a g + c0 + c1 (P_p + Q_src)

LATTICE CASES (bit-exact). make_case(kind="lattice") puts every input on a
small dyadic grid:
  P, Q in {0, +-1/4, +-1/2};  a1 = +-1;  b1 in {0, +-1/4};  slope = 1/4
    -> z1 a multiple of 1/4 with |z1| <= 5/4 (exact zeros are frequent: there
       `>` and `>=` differ), h1 a multiple of 1/16 with <= 5 significant bits
  W2 rows with four non-zeros from {+-1, +-2} (+-2 one time in four), all rows
  and all columns distinct -> z2 a multiple of 1/16, |z2| <= 10
  c1 in {0, 0, +-1};  c0 a multiple of 1/16 with |c0| <= 1/4, dz one with
  |dz| <= 1;  a2 in {+-1, +-2}
    -> dZ2 a multiple of 1/16 with |dZ2| <= 12.25 < 16: 8 significant bits, bf16
  dH1 a multiple of 1/16, g of 1/64;  mean1 a multiple of 1/4, invstd1 in
  {1, 2} -> yhat a multiple of 1/4, g yhat of 1/256;  dZ2 h1 of 1/256.
(The magnitudes are kept this small because the fused backward sums g yhat over
a block of up to 64 points x 64 edges: with c1 of +-1/2 or invstd1 of 1/2 the
quantum halves and that sum passes 2^24 quanta.)
Every product the kernels form is then exact in fp32, and every sum is a sum of
integer multiples of one quantum q. While sum|term| / q < 2^24, each partial sum
in ANY order (serial, shuffle tree, MFMA accumulator, two-wave exchange) is an
integer below 2^24 times q, hence representable: no fp32 addition rounds and the
kernel output must equal the fp64 value bit for bit; gE must be that value
rounded once (RNE) to bf16. assert_exact() checks these conditions in fp64 for
the case at hand (bf16 representability of h1 and dZ2, the quantum of every
term, sum|term| / q < 2^24 for the z2, z2^2, dH1, g, g yhat and dW2 sums over
the largest block row), so a case that breaks one fails on the CPU. Lattice
data ties constantly; make_case also plants the self-edge in slot 0 of every
third point and duplicate neighbours (slot k-1 repeats slot 0; slot 16 repeats
slot 1, i.e. the same z2 in two 16-row tiles).

RANDOM CASES (rounding behaviour). Normal data, gammas of both signs.
Tolerances come from the arithmetic (u = 2^-24), never from a run:
  MFMA dot of K terms            K u sum|a||b|
  a sum of n addends             n u sum|term| on top of each term's own bound
  a bf16 store                   the fp32 bound + 2^-8 |ref|
  h1 of the fused kernels        e_h = 4 u (|a1 P| + |a1 Q| + |b1|) in fp32 (two
                                 fma roundings and the slope product), stored
                                 as bf16: 2^-8 |ref| (1 + 2^-12) + e_h, and,
                                 tighter, RNE(h1 - e_h) <= H1 <= RNE(h1 + e_h).
                                 (bf16 keeps 8 significant bits, p = 8: the unit
                                 roundoff, half an ulp, is up to 2^-8 |x|, the
                                 "bf16 store" rung above; 2^-9 |x| would be the
                                 roundoff of a 9-bit format.)
  the bf16 h1 as MFMA operand    where h1 +- e_h round to different bf16 values
                                 the kernel may hold either: that difference
                                 (slack_h, zero almost everywhere) times |W2|
                                 is added to the z2 bound:
  bz = K u (|h1_bf16| + slack_h) |W2|^T + slack_h |W2|^T
  arg                            the returned slot's reference value lies within
                                 bz[got] + bz[ref] of the extremum; where the
                                 reference extremum leads every other slot by
                                 more than the two bounds, arg equals it
  dZ2 (never seen, fused)        e_d = |c1| bz + 3 u (|c1 z2| + |c0| + |a2 dz|);
                                 the reference keeps dZ2 unrounded, so the
                                 kernel's bf16 value is within e_d + 2^-8 |dZ2|
  dH1                            (e_d + 2^-8 |dZ2|) |W2| + C2 u |dZ2| |W2|
  g                              the dH1 bound + u |g|; where |z1| <= e_h the
                                 fp32 sign of z1 may differ: + (1 - slope)|dH1|
  partial rows, slab rows        the sums of the per-term bounds + n u sum|term|
  scatter                        (deg + k + 8) u sum|term|
  op level (edge_mlp2, all seven gradients): the same rungs composed along the
  backward. dz = dout LReLU'(a2 ysel + b2): u |dz|, + (1 - slope)|dout| where
  |z| <= 2u(|a2 ysel| + |b2|); BN sums as above; BN-backward constants c1 =
  -a dgamma invstd / E, c0 = -a dbeta / E - c1 mean: the sums' bounds through
  those factors + 4u sum|term|; these input bounds enter dZ2 (Ref.backward) and
  the scatter (scatter_ref); totals over partial rows in any order: + E u
  sum|term|; the dX / dW1 GEMMs may round both operands to bf16 when staged:
  (delta + 2^-8|a|)(1 + 2^-8)|b| + 2^-8|a||b| per product + K u sum|a||b|.
The lattice cases carry exactness; the random cases prove range and rounding.
"""
import torch

from _gemm_ref import Buf

U = 2.0 ** -24
SENT = 12288.0          # exactly representable in bf16 and fp32
LIM = float(2 ** 24)
SLOPE_LATTICE = 0.25
SLOPE_RANDOM = 0.2
C1 = 64


def f32_value(x):
    return float(torch.tensor(x, dtype=torch.float32))


def bf16_round(x):
    """fp64 -> the bf16 value (RNE) as fp64. Exact for lattice data (fp32 holds
    it); for random data the fp32 step is what the kernels round from."""
    return x.float().bfloat16().double()


def lrelu_grad(pos, slope):
    """1 where pos, else slope, in fp64 (torch.where of two Python floats is fp32)"""
    one = torch.ones((), dtype=torch.float64, device=pos.device)
    return torch.where(pos, one, one * slope)


def edge_ij(idx, B, N, k):
    """global (i, j) of every edge row e = i*k + s"""
    M = B * N
    i = torch.arange(M, device=idx.device).repeat_interleave(k)
    j = (i // N) * N + idx.reshape(-1)[:M * k].long()
    return i, j


def tile_rows(B, N, ppb):
    """partial-statistics / slab row of every point: prow = b*tiles + n // ppb"""
    tiles = (N + ppb - 1) // ppb
    n = torch.arange(N)
    row = (torch.arange(B).view(B, 1) * tiles + (n // ppb).view(1, N)).reshape(-1)
    return row, B * tiles


def rowsum(x, rows, nrows):
    """sum of x's rows per partial row"""
    out = torch.zeros(nrows, x.shape[1], dtype=torch.float64, device=x.device)
    return out.index_add_(0, rows.to(x.device), x)


def graph_reverse(idx, B, N, k):
    """(rowptr (M+1), edges (E)) int32 from idx (B*N*k local ids): the in-edge
    list of every global point, ids (global i << 6) | s in ascending order."""
    M = B * N
    idx = idx.reshape(-1)[:M * k].cpu()
    i, j = edge_ij(idx, B, N, k)
    s = torch.arange(k).repeat(M)
    ids = (i << 6) | s
    order = torch.argsort(j * (1 << 40) + ids)
    rowptr = torch.zeros(M + 1, dtype=torch.int64)
    rowptr[1:] = torch.bincount(j, minlength=M).cumsum(0)
    return rowptr.int(), ids[order].int()


class Case:
    pass


def _choice(g, values, shape):
    v = torch.tensor(values, dtype=torch.float32)
    return v[torch.randint(0, len(values), shape, generator=g)]


def _lattice_w2(g, C2):
    while True:
        W = torch.zeros(C2, C1)
        for r in range(C2):
            cols = torch.randperm(C1, generator=g)[:4]
            W[r, cols] = _choice(g, [-2.0, -1.0, -1.0, -1.0, 1.0, 1.0, 1.0, 2.0], (4,))
        if len({tuple(r.tolist()) for r in W}) == C2 and len({tuple(c.tolist()) for c in W.t()}) == C1:
            return W


def make_idx(g, B, N, k):
    """(B*N, k) local neighbour ids, all valid, with the planted self-edge and
    duplicates described in the module docstring"""
    idx = torch.randint(0, N, (B * N, k), generator=g)
    n = torch.arange(B * N) % N
    idx[::3, 0] = n[::3]
    idx[::2, k - 1] = idx[::2, 0]
    if k > 16:
        idx[1::2, 16] = idx[1::2, 1]
    return idx.int()


def make_case(kind, B, N, k, C2, seed, pad=0):
    """Given data (CPU tensors) of one geometry. Indexed inputs carry a guard
    row in the same allocation: PQ / dz rows of NaN (and NaN in PQ's pad
    columns), arg 255, idx the local id N (a valid row: the next cloud's first
    point or PQ's NaN guard row), so an over-read poisons the output."""
    g = torch.Generator().manual_seed(seed)
    c = Case()
    c.kind, c.B, c.N, c.k, c.C2, c.M, c.E = kind, B, N, k, C2, B * N, B * N * k
    c.ldpq = 2 * C1 + pad
    M = c.M
    lat = kind == "lattice"
    if lat:
        c.slope = SLOPE_LATTICE
        PQ = _choice(g, [-0.5, -0.25, 0.0, 0.25, 0.5], (M, 2 * C1))
        c.a1 = _choice(g, [-1.0, 1.0], (C1,))
        c.b1 = _choice(g, [0.0, 0.25, -0.25], (C1,))
        c.mean1 = _choice(g, [-0.5, -0.25, 0.0, 0.25, 0.5], (C1,))
        c.invstd1 = _choice(g, [1.0, 2.0], (C1,))
        c.W2 = _lattice_w2(g, C2)
        c.dz = torch.randint(-16, 17, (M, C2), generator=g).float() / 16
        c.c0 = torch.randint(-4, 5, (C2,), generator=g).float() / 16
        c.c1 = _choice(g, [0.0, 0.0, 1.0, -1.0], (C2,))
        c.a2 = _choice(g, [-2.0, -1.0, 1.0, 2.0], (C2,))
    else:
        c.slope = f32_value(SLOPE_RANDOM)
        PQ = torch.randn(M, 2 * C1, generator=g)
        c.a1 = torch.randn(C1, generator=g)
        c.b1 = 0.3 * torch.randn(C1, generator=g)
        c.mean1 = 0.1 * torch.randn(C1, generator=g)
        c.invstd1 = torch.rand(C1, generator=g) + 0.5
        c.W2 = (0.125 * torch.randn(C2, C1, generator=g)).bfloat16().float()
        c.dz = torch.randn(M, C2, generator=g)
        c.c0 = 0.1 * torch.randn(C2, generator=g)
        c.c1 = 0.1 * torch.randn(C2, generator=g)
        c.a2 = torch.randn(C2, generator=g)
    c.a1[0], c.a1[C1 - 1] = c.a1[0].abs(), -c.a1[C1 - 1].abs()
    c.dir2 = _choice(g, [-1.0, 1.0], (C2,))
    c.dir2[0], c.dir2[C2 - 1] = 1.0, -1.0
    c.PQg = torch.full((M + 1, c.ldpq), float("nan"))
    c.PQg[:M, :2 * C1] = PQ
    idx = make_idx(g, B, N, k)
    c.idxg = torch.cat([idx, torch.full((1, k), N, dtype=torch.int32)])
    # the backward's slots are given data: random, with slot 0, slot k-1 and four
    # different slots inside one aligned group of four channels (byte unpacking)
    arg = torch.randint(0, k, (M, C2), generator=g)
    arg[:, 0], arg[:, 1] = 0, k - 1
    arg[:, 4:8] = (torch.arange(4).view(1, 4) + torch.arange(M).view(M, 1)) % k
    c.argg = torch.cat([arg, torch.full((1, C2), 255)]).to(torch.uint8)
    c.dzg = torch.cat([c.dz, torch.full((1, C2), float("nan"))])
    c.consts = torch.cat([c.c0, c.c1, c.a2])
    return c


class Ref:
    """The restatement of the whole chain for one case (fp64, on `dev`).
    arg: the slots the backward is given (default: the case's planted ones)."""

    def __init__(self, c, dev="cpu", arg=None, dz=None, c0=None, c1=None, rounding=True):
        d = lambda t: t.to(dev).double()
        rnd = bf16_round if rounding else (lambda t: t)   # rounding=False: the chain in exact arithmetic
        self.rnd, self.dev = rnd, dev
        B, N, k, C2, M, E = c.B, c.N, c.k, c.C2, c.M, c.E
        self.c = c
        PQ = d(c.PQg[:M])
        idx = c.idxg[:M].to(dev)
        self.i, self.j = edge_ij(idx, B, N, k)
        P, Q = PQ[:, :C1], PQ[:, C1:2 * C1]
        a1, b1, sl = d(c.a1), d(c.b1), c.slope
        Pj, Qi = P[self.j], Q[self.i]
        self.y = Pj + Qi
        self.z1 = a1 * self.y + b1
        self.pos = self.z1 > 0
        self.h1 = torch.where(self.pos, self.z1, sl * self.z1)
        self.e_h = 4 * U * ((a1 * Pj).abs() + (a1 * Qi).abs() + b1.abs())
        self.h1b = rnd(self.h1)
        self.h1b_lo, self.h1b_hi = rnd(self.h1 - self.e_h), rnd(self.h1 + self.e_h)
        self.slack_h = torch.maximum((self.h1b_hi - self.h1b).abs(), (self.h1b - self.h1b_lo).abs())
        self.h1_bound = 2.0 ** -8 * self.h1.abs() * (1 + 2.0 ** -12) + self.e_h
        W2 = d(c.W2)
        self.W2, aW = W2, W2.abs()
        self.z2 = self.h1b @ W2.t()
        self.bz = C1 * U * ((self.h1b.abs() + self.slack_h) @ aW.t()) + self.slack_h @ aW.t()
        # forward
        dir2 = d(c.dir2)
        v = (self.z2 * dir2).view(M, k, C2)
        best = v.max(dim=1, keepdim=True)[0]
        slots = torch.arange(k, device=dev).view(1, k, 1).expand(M, k, C2)
        self.arg = torch.where(v == best, slots, k).min(dim=1)[0]
        self.v, self.best = v, best.squeeze(1)
        self.ysel = torch.gather(self.z2.view(M, k, C2), 1, self.arg.unsqueeze(1)).squeeze(1)
        rows8, self.nrows8 = tile_rows(B, N, 8)
        self.erows8 = rows8.to(dev).repeat_interleave(k)
        self.part2 = torch.stack([rowsum(self.z2, self.erows8, self.nrows8),
                                  rowsum(self.z2 ** 2, self.erows8, self.nrows8)], 1)
        n8 = min(N, 8) * k + 8
        self.part2_abs = torch.stack([rowsum(self.z2.abs(), self.erows8, self.nrows8),
                                      rowsum(self.z2 ** 2, self.erows8, self.nrows8)], 1)
        self.part2_bound = torch.stack(
            [rowsum(self.bz, self.erows8, self.nrows8),
             rowsum(2 * self.z2.abs() * self.bz + self.bz ** 2, self.erows8, self.nrows8)], 1) \
            + n8 * U * self.part2_abs
        self.mean1, self.invstd1 = d(c.mean1), d(c.invstd1)
        if hasattr(c, "dz"):
            self.backward(c.argg[:M] if arg is None else arg, c.dz if dz is None else dz,
                          c.c0 if c0 is None else c0, c.c1 if c1 is None else c1, c.a2)

    def backward(self, arg, dz, c0, c1, a2, dz_b=None, c0_b=None, c1_b=None):
        """the backward chain for the given slots, dz and BN2-backward constants;
        dz_b / c0_b / c1_b: how far the kernel's own dz, c0, c1 may be from them
        (the op-level test, where they are results of earlier kernels)"""
        c, dev, rnd = self.c, self.dev, self.rnd
        B, N, k, C2, M, E = c.B, c.N, c.k, c.C2, c.M, c.E
        d = lambda t: t.to(dev).double()
        slots = torch.arange(k, device=dev).view(1, k, 1)
        arg, dz = arg.to(dev).long(), d(dz)
        k0, k1, a2 = d(c0), d(c1), d(a2)
        self.consts = torch.cat([k0, k1, a2]).float()
        hit = (arg.unsqueeze(1) == slots).reshape(E, C2)
        t = (a2 * dz).repeat_interleave(k, dim=0) * hit
        self.dZ2 = k1 * self.z2 + k0 + t
        self.dZ2b = rnd(self.dZ2)
        self.e_d3 = 3 * U * ((k1 * self.z2).abs() + k0.abs() + t.abs())
        self.e_d = k1.abs() * self.bz + self.e_d3
        if dz_b is not None:
            self.e_d = self.e_d + d(c1_b) * self.z2.abs() + d(c0_b) + (a2.abs() * d(dz_b)).repeat_interleave(k, dim=0) * hit
        rows64, self.nrows64 = tile_rows(B, N, 64)
        self.erows64 = rows64.to(dev).repeat_interleave(k)
        # lattice: dZ2 == dZ2b; random: the unrounded dZ2 with the 2^-8 |dZ2| term
        dd = self.dZ2b if c.kind == "lattice" else self.dZ2
        dd_b = self.e_d + 2.0 ** -8 * self.dZ2.abs()
        self.bwd = self.h1bwd(dd, self.erows64, self.nrows64, dd_b)
        # dW2 slab rows
        self.slab = torch.zeros(self.nrows64, C2, C1, dtype=torch.float64, device=dev)
        self.slab_abs = torch.zeros_like(self.slab)
        self.slab_bound = torch.zeros_like(self.slab)
        for r in range(self.nrows64):
            m = self.erows64 == r
            self.slab[r] = dd[m].t() @ self.h1b[m]
            self.slab_abs[r] = dd[m].abs().t() @ self.h1b[m].abs()
            self.slab_bound[r] = dd_b[m].t() @ (self.h1b[m].abs() + self.slack_h[m]) + dd[m].abs().t() @ self.slack_h[m] \
                + (int(m.sum()) + 16) * U * self.slab_abs[r]
        self.dW2 = self.slab.sum(0)

    def dz2_gemm(self):
        """dgx_gemm_dz2_bf16 from the given bf16 h1: (dZ2 unrounded, its bound)"""
        bz = C1 * U * (self.h1b.abs() @ self.W2.abs().t())
        k1 = self.consts[self.c.C2:2 * self.c.C2].double()
        return self.dZ2, k1.abs() * bz + self.e_d3 + 2.0 ** -8 * self.dZ2.abs()

    def h1bwd(self, dZ2, erows, nrows, dZ2_bound=None):
        """g, its bf16 rounding and the BN1-backward partial rows from a given dZ2
        (E, C2); dZ2_bound: how far the kernel's own dZ2 may be from it."""
        c, sl = self.c, self.c.slope
        aW = self.W2.abs()
        r = Case()
        r.dH = dZ2 @ self.W2
        bdh = c.C2 * U * (dZ2.abs() @ aW)
        if dZ2_bound is not None:
            bdh = bdh + dZ2_bound @ aW
        f = lrelu_grad(self.pos, sl)
        r.g = r.dH * f
        amb = (self.z1.abs() <= self.e_h).double()
        r.g_bound = bdh + U * r.g.abs() + amb * (r.dH.abs() + bdh) * (1 - sl)
        r.gb = self.rnd(r.g)
        r.gb_bound = r.g_bound + 2.0 ** -8 * r.g.abs()
        yhat = (self.y - self.mean1) * self.invstd1
        e_yhat = 3 * U * (self.y.abs() + self.mean1.abs()) * self.invstd1
        t2 = r.g * yhat
        r.part = torch.stack([rowsum(r.g, erows, nrows), rowsum(t2, erows, nrows)], 1)
        r.part_abs = torch.stack([rowsum(r.g.abs(), erows, nrows), rowsum(t2.abs(), erows, nrows)], 1)
        n = int(torch.bincount(erows).max()) + 16
        r.part_bound = torch.stack([rowsum(r.g_bound, erows, nrows),
                                    rowsum(r.g_bound * yhat.abs() + r.g.abs() * e_yhat + U * t2.abs(), erows, nrows)],
                                   1) + n * U * r.part_abs
        return r


def assert_exact(c, r):
    """The lattice case's exactness conditions (module docstring), in fp64."""
    assert c.kind == "lattice"

    def quantum(x, q, what):
        assert bool((x / q == (x / q).round()).all()), f"{what}: not a multiple of {q}"

    def small(abs_sum, q, what):
        assert float(abs_sum.max()) / q < LIM, f"{what}: sum|term| / q = {float(abs_sum.max()) / q:.3g} >= 2^24"

    assert torch.equal(r.h1b, r.h1), "h1 not bf16-representable"
    assert torch.equal(r.dZ2b, r.dZ2), "dZ2 not bf16-representable"
    assert bool((r.z1 == 0).any()), "no exact zero of z1 in the case"
    quantum(r.z2, 1 / 16, "z2")
    small(r.h1b.abs() @ r.W2.abs().t(), 1 / 16, "z2 dot")
    small(r.part2_abs[:, 0], 1 / 16, "sum z2")
    small(r.part2_abs[:, 1], 1 / 256, "sum z2^2")
    quantum(r.dZ2, 1 / 16, "dZ2")
    small(r.dZ2.abs() @ r.W2.abs(), 1 / 16, "dH1 dot")
    quantum(r.bwd.g, 1 / 64, "g")
    small(r.bwd.part_abs[:, 0], 1 / 64, "sum g")
    quantum((r.y - r.mean1) * r.invstd1, 1 / 4, "yhat")
    small(r.bwd.part_abs[:, 1], 1 / 256, "sum g yhat")
    small(r.slab_abs, 1 / 256, "dW2 slab")
    small(r.slab_abs.sum(0), 1 / 256, "dW2")
    # the 128-edge-row tiles of the unfused GEMM epilogue
    er = torch.arange(c.E, device=r.z2.device) // 128
    u = r.h1bwd(r.dZ2b, er, int(er.max()) + 1)
    small(u.part_abs[:, 0], 1 / 64, "sum g (128-row tiles)")
    small(u.part_abs[:, 1], 1 / 256, "sum g yhat (128-row tiles)")


# ---- the scatter --------------------------------------------------------------

def make_scatter_case(kind, B, N, k, C, seed, graph="random", pad=0):
    """Given data of dgx_edge_mlp_scatter_f32: g (E, C) on the bf16 grid, PQ,
    sumP, BN1-backward constants, and a hand-made graph:
      random  make_idx
      hub     every point's slot 0 -> point 0 of its cloud
      last    every point's slot 0 -> the last point of its cloud
      degrees in-degrees 0, 1, 3, 4, 5, 63, 64, 65 planted on points 1..8 (N >= 66)
    """
    g = torch.Generator().manual_seed(seed)
    c = Case()
    c.kind, c.B, c.N, c.k, c.C, c.M, c.E, c.ldpq = kind, B, N, k, C, B * N, B * N * k, 2 * C + pad
    M, E = c.M, c.E
    idx = make_idx(g, B, N, k).long()
    if graph == "hub":
        idx[:, 0] = 0
    elif graph == "last":
        idx[:, 0] = N - 1
    elif graph == "degrees":
        want = [0, 1, 3, 4, 5, 63, 64, 65]
        assert N >= 66 + 9 and k >= len(want)            # one slot per planted target
        idx = torch.randint(9, N, (M, k), generator=g)       # targets 0..8 free
        for t, deg in enumerate(want):
            # `deg` distinct sources (points 9 .. 9+deg-1 of each cloud) aim slot t % k at point t + 1
            src = torch.arange(9, 9 + deg)
            for b in range(B):
                idx[b * N + src, t % k] = t + 1
        c.want_deg = want
    c.idx = idx.int()
    if kind == "lattice":
        c.g = torch.randint(-32, 33, (E, C), generator=g).float() / 8
        PQ = _choice(g, [-0.5, -0.25, 0.0, 0.25, 0.5], (M, 2 * C))
        c.a = _choice(g, [-1.0, 1.0], (C,))
        c.c0 = torch.randint(-16, 17, (C,), generator=g).float() / 16
        c.c1 = _choice(g, [0.0, 0.5, -0.5], (C,))
    else:
        c.g = torch.randn(E, C, generator=g).bfloat16().float()
        PQ = torch.randn(M, 2 * C, generator=g)
        c.a = torch.randn(C, generator=g)
        c.c0 = 0.1 * torch.randn(C, generator=g)
        c.c1 = 0.1 * torch.randn(C, generator=g)
    c.PQg = torch.full((M + 1, c.ldpq), float("nan"))
    c.PQg[:M, :2 * C] = PQ
    c.gg = torch.cat([c.g, torch.full((1, C), float("nan"))])
    i, j = edge_ij(c.idx, B, N, k)
    c.sumP = PQ[:, :C][j].double().view(M, k, C).sum(1).float()   # exact on the lattice; given data otherwise
    c.rowptr, c.edges = graph_reverse(c.idx, B, N, k)
    return c


def scatter_ref(c, dev="cpu"):
    """(dPQ (M, 2C) fp64, bound) of dgx_edge_mlp_scatter_f32's formula"""
    d = lambda t: t.to(dev).double()
    M, k, C = c.M, c.k, c.C
    PQ = d(c.PQg[:M])
    P, Q, g = PQ[:, :C], PQ[:, C:2 * C], d(c.g)
    a, k0, k1, sumP = d(c.a), d(c.c0), d(c.c1), d(c.sumP)
    rowptr, edges = c.rowptr.to(dev).long(), c.edges.to(dev).long()
    deg = rowptr[1:] - rowptr[:-1]
    tgt = torch.arange(M, device=dev).repeat_interleave(deg)
    src, slot = edges >> 6, edges & 63
    erow = src * k + slot
    zero = torch.zeros(M, C, dtype=torch.float64, device=dev)
    ig = zero.clone().index_add_(0, tgt, g[erow])
    iq = zero.clone().index_add_(0, tgt, Q[src])
    iga = zero.clone().index_add_(0, tgt, g[erow].abs())
    iqa = zero.clone().index_add_(0, tgt, Q[src].abs())
    degf = deg.double().view(M, 1)
    dP = a * ig + k0 * degf + k1 * (degf * P + iq)
    dPa = a.abs() * iga + k0.abs() * degf + k1.abs() * (degf * P.abs() + iqa)
    sg, sga = g.view(M, k, C).sum(1), g.abs().view(M, k, C).sum(1)
    dQ = a * sg + k0 * k + k1 * (k * Q + sumP)
    dQa = a.abs() * sga + k0.abs() * k + k1.abs() * (k * Q.abs() + sumP.abs())
    bound = torch.cat([(degf + k + 8) * U * dPa, (k + 8) * U * dQa.expand(M, C)], 1)
    if hasattr(c, "g_b"):   # g, c0, c1 are themselves only known to these bounds (op-level test)
        g_b, k0_b, k1_b = d(c.g_b), d(c.c0_b), d(c.c1_b)
        ig_b = zero.clone().index_add_(0, tgt, g_b[erow])
        bound = bound + torch.cat([a.abs() * ig_b + k0_b * degf + k1_b * (degf * P.abs() + iqa),
                                   a.abs() * g_b.view(M, k, C).sum(1) + k0_b * k + k1_b * (k * Q.abs() + sumP.abs())], 1)
    return torch.cat([dP, dQ], 1), bound, torch.cat([dPa, dQa], 1)


def assert_scatter_exact(c, dev="cpu"):
    _, _, mag = scatter_ref(c, dev)
    assert float(mag.max()) * 64 < LIM, "scatter: sum|term| / (1/64) >= 2^24"


# ---- dgx_edge_mlp_h1_bwd_f32 (any C1) -----------------------------------------

def make_h1bwd_case(kind, B, N, k, C, seed):
    g = torch.Generator().manual_seed(seed)
    c = Case()
    c.kind, c.B, c.N, c.k, c.C, c.M, c.E, c.ldpq = kind, B, N, k, C, B * N, B * N * k, 2 * C
    M, E = c.M, c.E
    if kind == "lattice":
        c.slope = SLOPE_LATTICE
        PQ = _choice(g, [-0.5, -0.25, 0.0, 0.25, 0.5], (M, 2 * C))
        c.a1, c.b1 = _choice(g, [-1.0, 1.0], (C,)), _choice(g, [0.0, 0.25, -0.25], (C,))
        c.mean1, c.invstd1 = _choice(g, [-0.5, -0.25, 0.0, 0.25, 0.5], (C,)), _choice(g, [0.5, 1.0, 2.0], (C,))
        c.dH = torch.randint(-64, 65, (E, C), generator=g).float() / 16
    else:
        c.slope = f32_value(SLOPE_RANDOM)
        PQ = torch.randn(M, 2 * C, generator=g)
        c.a1, c.b1 = torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)
        c.mean1, c.invstd1 = 0.1 * torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
        c.dH = torch.randn(E, C, generator=g)
    c.PQg = torch.full((M + 1, 2 * C), float("nan"))
    c.PQg[:M] = PQ
    c.idxg = torch.cat([torch.randint(0, N, (M, k), generator=g).int(), torch.full((1, k), N, dtype=torch.int32)])
    return c


def h1bwd_f32_ref(c, nrows, dev="cpu"):
    """g = dH LReLU'(z1) and the partial rows of mlp_h1_bwd_kernel: block r sums
    the edges e with (e // epb) % nrows == r, epb = 256 / (C / 4). Lattice: g is a
    multiple of 1/64, g yhat of 1/512 (yhat of 1/8), a few hundred terms a row."""
    d = lambda t: t.to(dev).double()
    M, C = c.M, c.C
    PQ = d(c.PQg[:M])
    i, j = edge_ij(c.idxg[:M].to(dev), c.B, c.N, c.k)
    y = PQ[:, :C][j] + PQ[:, C:][i]
    a1, b1 = d(c.a1), d(c.b1)
    z1 = a1 * y + b1
    e_z = 4 * U * ((a1 * y).abs() + b1.abs())
    r = Case()
    dH = d(c.dH)
    r.g = dH * lrelu_grad(z1 > 0, c.slope)
    r.g_bound = U * r.g.abs() + (z1.abs() <= e_z).double() * dH.abs() * (1 - c.slope)
    yhat = (y - d(c.mean1)) * d(c.invstd1)
    t2 = r.g * yhat
    epb = 256 // (C // 4)
    rows = (torch.arange(c.E, device=dev) // epb) % nrows
    r.part = torch.stack([rowsum(r.g, rows, nrows), rowsum(t2, rows, nrows)], 1)
    r.part_abs = torch.stack([rowsum(r.g.abs(), rows, nrows), rowsum(t2.abs(), rows, nrows)], 1)
    n = int(torch.bincount(rows).max()) + 16
    e_t2 = r.g_bound * yhat.abs() + r.g.abs() * 3 * U * (y.abs() + d(c.mean1).abs()) * d(c.invstd1) + U * t2.abs()
    r.part_bound = torch.stack([rowsum(r.g_bound, rows, nrows), rowsum(e_t2, rows, nrows)], 1) + n * U * r.part_abs
    if c.kind == "lattice":
        assert float(r.part_abs.max()) * 512 < LIM, "h1_bwd partial: sum|term| / (1/512) >= 2^24"
    return r


# ---- the geometry grids of tests/test_edgemlp_kernels_gpu.py ---------------------
# The full cross product of the axes is thousands of launches. Each grid walks
# all axes at once: case t of 24 takes value t mod len(axis) of the B, N and k
# axes (6, 5 and 9 values) and the two-valued axes (C2, H1 given, ldpq pad) follow
# three square waves of t chosen (by search) so that every value of every axis
# meets at least two values of every other axis; test_edgemlp_ref_cpu.py checks
# exactly that property. The backward grid is the same walk with C2 = 128.
KS = (1, 15, 16, 17, 32, 33, 48, 49, 64)
BS = (1, 2, 3, 5, 8, 9)
FWD_NS = (1, 7, 8, 9, 17)
BWD_NS = (1, 63, 64, 65, 130)
AXES = ("B", "N", "k", "C2", "h1", "pad")


def geometry_grid(Ns, T=24):
    """[(B, N, k, C2, H1 given, ldpq pad)]"""
    return [(BS[t % 6], Ns[t % 5], KS[t % 9], (64, 128)[(t + t // 18) % 2], bool((t // 3 + t // 5) % 2),
             4 * ((t // 3 + t // 18) % 2)) for t in range(T)]


FWD_GRID = geometry_grid(FWD_NS)
BWD_GRID = [(B, N, k, pad) for B, N, k, _, _, pad in geometry_grid(BWD_NS)]   # C2 = 128, no H1
# the unfused GEMM epilogues: (B, N, k, C2); E = B N k covers k, 127, 128, 129 = 3*43,
# 2*128 + 16 and cloud boundaries inside a 128-row tile (B = 3)
GEMM_GRID = [(1, 1, 7, 64), (1, 1, 64, 128), (1, 127, 1, 128), (1, 128, 1, 64), (1, 2, 64, 128), (1, 129, 1, 64),
             (3, 43, 1, 128), (1, 272, 1, 128), (3, 43, 7, 64), (1, 4, 40, 64), (3, 5, 40, 128), (3, 3, 64, 64)]
# dgx_edge_mlp_h1_bwd_f32: (B, N, k, C1); the last engages the 2048-row cap
H1BWD_GRID = [(1, 1, 1, 8), (2, 5, 3, 8), (1, 1, 1, 64), (3, 7, 5, 64), (1, 1, 1, 128), (2, 9, 4, 128),
              (5, 3277, 16, 64)]
# dgx_edge_mlp_scatter_f32: (g bf16, C1, B, N, k, graph, ldpq pad, g offset in elements)
SCATTER_GRID = [
    (1, 64, 1, 130, 1, "hub", 0, 0), (1, 64, 1, 130, 5, "hub", 0, 0), (1, 64, 3, 130, 64, "hub", 0, 0),
    (1, 64, 3, 130, 9, "degrees", 0, 0), (1, 64, 9, 17, 5, "last", 0, 0), (1, 64, 1, 1, 1, "random", 0, 0),
    (1, 64, 3, 15, 3, "random", 0, 0), (1, 64, 1, 16, 64, "last", 0, 0), (1, 64, 9, 16, 2, "random", 0, 0),
    (1, 64, 3, 17, 17, "hub", 0, 0),
    (1, 128, 1, 130, 5, "hub", 0, 0), (1, 128, 3, 75, 9, "degrees", 0, 0), (1, 128, 9, 17, 1, "last", 0, 0),
    (1, 64, 1, 130, 5, "hub", 2, 0), (1, 64, 3, 75, 9, "degrees", 0, 4), (1, 64, 9, 16, 64, "last", 2, 4),
    (0, 8, 1, 130, 5, "hub", 0, 0), (0, 8, 3, 75, 9, "degrees", 0, 0), (0, 32, 9, 17, 1, "last", 0, 0),
    (0, 32, 1, 130, 64, "hub", 0, 0), (0, 64, 3, 75, 9, "degrees", 0, 0), (0, 64, 1, 1, 1, "random", 0, 0),
    (0, 64, 9, 15, 5, "last", 0, 0),
]


# ---- helpers of the GPU tests -------------------------------------------------

def guarded(rows, cols, dev, dtype=torch.float32, fill=SENT):
    """(buffer of rows + 1 canary row, all `fill`; view of the rows): the
    dense one-guard-row form of the GEMM tests' Buf (tests/_gemm_ref.py)"""
    b = Buf(rows, cols, dev, dtype, fill, guard_rows=1)
    return b.full, b.view


def guard_intact(full, fill=SENT):
    return bool((full[-1].float() == fill).all())


def within(got, ref, bound):
    return bool(((got.double() - ref).abs() <= bound).all())


def worst(got, ref, bound):
    r = (got.double() - ref).abs() / bound.clamp_min(1e-300)
    return float(r.nan_to_num(nan=float("inf")).max())
