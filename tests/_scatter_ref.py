"""Host oracle of the EdgeConv backward scatter (edge_bwd_scatter_kernel in
csrc/edgeconv.hip; dgx_edge_bwd_scatter_f32 / _packed_f32 / _fin_f32). numpy
and torch on the CPU only.

  dP_j = a sum_{in-edges (i,s) of j, s = arg_i} dz_i + deg_j c0 + c1 (deg_j P_j + sum_in Q_i)
  dQ_i = a dz_i + k c0 + c1 (k Q_i + sumP_i)

* reverse_graph: the CSR of in-edges over global points, edge id =
  (source point << 6) | slot, ascending within a row — what the GPU tests feed
  the kernel, so they do not depend on the engine's reverse-graph kernel.
* ref64: every term in fp64, any Co, any ldpq, duplicate neighbour ids within a
  row (only the edge whose slot equals arg carries dz).
* lattice: integer-valued P, Q, dz, sumP and a, c0, c1 from {0, +-1, +-2,
  +-0.5}. Every partial sum of dP and dQ, in any order and any grouping, is a
  multiple of 1/2 below 2^23 (twice it an integer below 2^24) — the builder
  asserts that from the in-degrees — so fp32 arithmetic is exact whatever the
  order and the kernel must equal ref64 bit for bit. dz is an integer below
  2^17, so its 6 low mantissa bits are free for the packed slot.
* ordered_sums: the kernel's own fp32 order of the two sums, for random data.
* the case tables of tests/test_scatter_oracle_gpu.py, with the launch form
  each entry is meant to hit; tests/test_scatter_ref_cpu.py checks them against
  dgx_edge_bwd_scatter_geometry.

Launch forms (slices, cs, tpp) x 4 output modes, 36 over 27 instantiations
(a mode-2 and a mode-3 launch share the SPLIT instantiation):
  unpacked cs 8, 4, 2, 1 at tpp 1; packed cs 4, 2, 1 at tpp 1; packed cs 8 at
  tpp 2 and 4.
Compiled but unreachable, and so untested: packed CS = 8 with TPP = 1 (the
lane rule gives packed 8-channel slices at least two lanes) in its three
output forms, and TPP = 8 (SCATTER_SMALL_TPP is 4) in its three."""
import numpy as np
import torch

EC_THREADS = 512          # csrc/edgeconv.hip
BW_EB = 16                # in-edge ids per batch; 8 per lane at TPP = 2, 4 at TPP = 4
BW_BUCKETS = 64           # degree buckets: in-degrees >= 63 share one
GUARD = 64                # NaN elements on both sides of every output
LIM = float(2 ** 23)
NAN = float("nan")

# (a, c0, c1) of channel c: TRIPLES[c % 9]; every value of {0, +-1, +-2, +-0.5} in every position
TRIPLES = [(1, -1, 0.5), (-2, 0.5, 1), (0.5, 2, -1), (-1, 1, -2), (2, -0.5, 2), (-0.5, -2, -0.5), (1, 0, 1),
           (0, 1, -1), (-1, -1, 0)]
# bf16 ties above 256 (spacing 2: odd integers; 257 -> 256, 259 -> 260, 385 -> 384, 387 -> 388 to even), both
# lattice neighbours of a tie, the representable values around them, and ties / non-ties above 512
TIE_VALUES = [257., 259., 385., 387., 256.5, 257.5, 258.5, 259.5, 256., 258., 260., 384., 386., 388., -257., -259.,
              -385., -387., 511., 513., 514., 515., 517., 518., -514., 1026., 1030.]


class Case:
    """B, N, k, Co, ldpq, M; idx (M, k) int64 local ids; PQ (M, ldpq) fp32 (NaN in
    columns >= 2Co); dz (M, Co) fp32; arg (M, Co) u8; sumP (M, Co) fp32; a, c0, c1
    (Co) fp32; rowptr (M+1), edges (M k) int32."""

    def dz_values(self, packed):
        """dz as the kernel reads it: packed words lose their 6 low mantissa bits"""
        if not packed:
            return self.dz
        return (self.dz.view(torch.int32) & ~63).view(torch.float32)

    def dz_words(self):
        """dgx_edge_bwd_dz_packed_f32's words: dz | slot"""
        return ((self.dz.view(torch.int32) & ~63) | self.arg.to(torch.int32)).view(torch.float32)


def global_idx(idx, B, N, k):
    """(M, k) int64 global neighbour ids of local ids idx (B*N*k)"""
    idx = torch.as_tensor(idx).reshape(B, N, k).long()
    return (idx + (torch.arange(B) * N).view(B, 1, 1)).reshape(B * N, k)


def reverse_graph(idx, B, N, k):
    """(rowptr (M+1), edges (M k)) int32: the in-edges of every global point,
    ids (global source << 6) | slot ascending within a row"""
    M = B * N
    j = global_idx(idx, B, N, k).reshape(-1).numpy()
    ids = (np.repeat(np.arange(M, dtype=np.int64), k) << 6) | np.tile(np.arange(k, dtype=np.int64), M)
    order = np.lexsort((ids, j))
    rowptr = np.zeros(M + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(np.bincount(j, minlength=M))
    assert M * 64 < 2 ** 31
    return torch.from_numpy(rowptr.astype(np.int32)), torch.from_numpy(ids[order].astype(np.int32))


def reverse_graph_brute(idx, B, N, k):
    """the same by enumeration (tiny graphs)"""
    M = B * N
    g = global_idx(idx, B, N, k).tolist()
    rows = [[] for _ in range(M)]
    for i in range(M):
        for s in range(k):
            rows[g[i][s]].append((i << 6) | s)
    rowptr, edges = [0], []
    for r in rows:
        edges += sorted(r)
        rowptr.append(len(edges))
    return torch.tensor(rowptr, dtype=torch.int32), torch.tensor(edges, dtype=torch.int32)


# ---- graphs ---------------------------------------------------------------------------------------------------------
LADDER = (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65)


def make_idx(kind, B, N, k, seed=0):
    """(B, N, k) int64 local neighbour ids.
    random: uniform; hubs: three in four edges enter one of 4 hub points;
    ladder: points 1.. of in-degree LADDER (point 1 has none), every other edge on
    hub 0, dealt to the slots in a seeded random order (N k >= 337 + 66);
    all0: every edge enters point 0; dups: rows of at most two distinct ids."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * N + k)
    if kind == "random":
        return torch.randint(0, N, (B, N, k), generator=g)
    if kind == "hubs":
        hub = torch.randint(0, min(4, N), (B, N, k), generator=g)
        return torch.where(torch.rand(B, N, k, generator=g) < 0.75, hub, torch.randint(0, N, (B, N, k), generator=g))
    if kind == "all0":
        return torch.zeros(B, N, k, dtype=torch.int64)
    if kind == "dups":
        two = torch.randint(0, N, (B, N, 2), generator=g)
        pick = torch.randint(0, 2, (B, N, k), generator=g)
        return torch.gather(two, 2, pick)
    assert kind == "ladder" and N * k >= sum(LADDER) + 66 and N > len(LADDER)
    out = []
    for _ in range(B):
        t = torch.zeros(N * k, dtype=torch.int64)
        pos = 0
        for p, d in enumerate(LADDER):
            t[pos:pos + d] = p + 1
            pos += d
        out.append(t[torch.randperm(N * k, generator=g)].view(N, k))
    return torch.stack(out)


def in_degrees(c):
    return (c.rowptr[1:] - c.rowptr[:-1]).long()


# ---- cases ----------------------------------------------------------------------------------------------------------
def _finish(c, idx, B, N, k, Co, ldpq):
    c.B, c.N, c.k, c.Co, c.M = B, N, k, Co, B * N
    c.ldpq = 2 * Co if ldpq is None else ldpq
    assert c.ldpq >= 2 * Co
    c.idx = torch.as_tensor(idx).reshape(B * N, k).long()
    c.gidx = global_idx(c.idx, B, N, k)
    c.rowptr, c.edges = reverse_graph(c.idx, B, N, k)
    return c


def _pad_pq(P, Q, ldpq):
    M, Co = P.shape
    PQ = torch.full((M, ldpq), NAN, dtype=torch.float32)
    PQ[:, :Co], PQ[:, Co:2 * Co] = P, Q
    return PQ


def lattice_bound(c):
    """The largest sum of |terms| of any dP_j or dQ_i (fp64), from the in-degrees:
    every partial sum the kernel can form, in any order, is below it."""
    P, Q = c.PQ[:, :c.Co].double().abs(), c.PQ[:, c.Co:2 * c.Co].double().abs()
    a, c0, c1 = c.a.double().abs(), c.c0.double().abs(), c.c1.double().abs()
    deg = in_degrees(c).double().unsqueeze(1)
    sdz, sq = torch.zeros(c.M, c.Co, dtype=torch.float64), torch.zeros(c.M, c.Co, dtype=torch.float64)
    for s in range(c.k):
        sdz.index_add_(0, c.gidx[:, s], c.dz.double().abs())
        sq.index_add_(0, c.gidx[:, s], Q)
    dP = a * sdz + deg * c0 + c1 * (deg * P + sq)
    dQ = a * c.dz.double().abs() + c.k * c0 + c1 * (c.k * Q + c.sumP.double().abs())
    # the unscaled sums are partial sums too
    return float(max(dP.max(), dQ.max(), sdz.max(), (deg * P + sq).max(), (c.k * Q + c.sumP.double().abs()).max()))


def make_lattice(B, N, k, Co, idx, ldpq=None, seed=0, arg=None):
    """A lattice case on the graph idx (B, N, k). The first rows' dz are solved so
    that dQ takes TIE_VALUES where an integer dz does it."""
    c = _finish(Case(), idx, B, N, k, Co, ldpq)
    c.kind = "lattice"
    M = c.M
    g = torch.Generator().manual_seed(seed + 31 * N + Co)
    ri = lambda *s: torch.randint(-3, 4, s, generator=g).float()
    P, Q, c.sumP, c.dz = ri(M, Co), ri(M, Co), ri(M, Co), ri(M, Co)
    c.arg = torch.randint(0, k, (M, Co), generator=g, dtype=torch.uint8) if arg is None else arg
    t = torch.tensor([TRIPLES[o % len(TRIPLES)] for o in range(Co)], dtype=torch.float32)
    c.a, c.c0, c.c1 = t[:, 0].contiguous(), t[:, 1].contiguous(), t[:, 2].contiguous()
    nt = min(M, len(TIE_VALUES))
    Q[:nt] = 2 * torch.randint(-1, 2, (nt, Co), generator=g).float()        # even: k c0 + c1 (k Q + sumP) whole
    c.sumP[:nt] = 2 * torch.randint(-1, 2, (nt, Co), generator=g).float()   # unless k c0 is a half
    rest = k * c.c0.double() + c.c1.double() * (k * Q[:nt].double() + c.sumP[:nt].double())
    want = torch.tensor(TIE_VALUES[:nt], dtype=torch.float64).unsqueeze(1)
    dzt = (want - rest) / torch.where(c.a == 0, torch.ones_like(c.a), c.a).double()
    ok = (c.a != 0).unsqueeze(0) & (dzt == dzt.round()) & (dzt.abs() < 2 ** 12)
    c.dz[:nt] = torch.where(ok, dzt.float(), c.dz[:nt])
    c.PQ = _pad_pq(P, Q, c.ldpq)
    # exactness: integers (dz below 2^17: 6 free mantissa bits), halves only from a, c0, c1
    for x in (P, Q, c.sumP, c.dz):
        assert bool((x == x.round()).all())
    assert float(c.dz.abs().max()) < 2 ** 17 and bool(((c.dz.view(torch.int32) & 63) == 0).all())
    c.maxdeg = int(in_degrees(c).max())
    c.bound = lattice_bound(c)
    assert c.bound < LIM, (c.bound, c.maxdeg)
    return c


def make_random(B, N, k, Co, idx, ldpq=None, seed=0):
    """Gaussian P, Q, dz, constants; sumP = the fp32 rounding of the true sum_k P_j."""
    c = _finish(Case(), idx, B, N, k, Co, ldpq)
    c.kind = "random"
    g = torch.Generator().manual_seed(seed + 17 * N + Co)
    P, Q = torch.randn(c.M, Co, generator=g), torch.randn(c.M, Co, generator=g)
    c.dz = torch.randn(c.M, Co, generator=g)
    c.arg = torch.randint(0, k, (c.M, Co), generator=g, dtype=torch.uint8)
    c.sumP = P.double()[c.gidx].sum(1).float()
    c.a, c.c0, c.c1 = (torch.randn(Co, generator=g) for _ in range(3))
    c.PQ = _pad_pq(P, Q, c.ldpq)
    return c


# ---- references -----------------------------------------------------------------------------------------------------
def ref64(c, packed=False, a=None, c0=None, c1=None):
    """(M, 2Co) fp64: [dP | dQ], every term in fp64"""
    Co, k, M = c.Co, c.k, c.M
    P, Q = c.PQ[:, :Co].double(), c.PQ[:, Co:2 * Co].double()
    dz = c.dz_values(packed).double()
    a = (c.a if a is None else a).double()
    c0 = (c.c0 if c0 is None else c0).double()
    c1 = (c.c1 if c1 is None else c1).double()
    jsel = torch.gather(c.gidx, 1, c.arg.long())      # the target of the edge at slot arg: that edge alone carries dz
    sd = torch.zeros(M, Co, dtype=torch.float64).scatter_add_(0, jsel, dz)
    deg = in_degrees(c).double().unsqueeze(1)
    sq = torch.zeros(M, Co, dtype=torch.float64)
    for s in range(k):
        sq.index_add_(0, c.gidx[:, s], Q)
    dP = a * sd + c0 * deg + c1 * (deg * P + sq)
    dQ = a * dz + k * c0 + c1 * (k * Q + c.sumP.double())
    return torch.cat([dP, dQ], 1)


def ref_brute(c, packed=False):
    """ref64 by a loop over the CSR rows (tiny graphs)"""
    Co, k, M = c.Co, c.k, c.M
    P, Q = c.PQ[:, :Co].double(), c.PQ[:, Co:2 * Co].double()
    dz = c.dz_values(packed).double()
    out = torch.zeros(M, 2 * Co, dtype=torch.float64)
    for j in range(M):
        for e in c.edges[c.rowptr[j]:c.rowptr[j + 1]].tolist():
            i, s = e >> 6, e & 63
            assert int(c.gidx[i, s]) == j
            for o in range(Co):
                if int(c.arg[i, o]) == s:
                    out[j, o] += float(c.a[o]) * dz[i, o]
                out[j, o] += float(c.c0[o]) + float(c.c1[o]) * (P[j, o] + Q[i, o])
    for i in range(M):
        for o in range(Co):
            out[i, Co + o] = float(c.a[o]) * dz[i, o] + k * float(c.c0[o]) + float(c.c1[o]) * (k * Q[i, o] + c.sumP[i, o])
    return out


def _ordered(vals, rowptr, tpp):
    """fp32 sums of the (E, Co) per-edge values over each CSR row in the kernel's
    order: lane s of tpp takes edges beg + s + tpp v, v ascending, from 0; the
    lanes combine as (s0 + s1) or (s0 + s1) + (s2 + s3)."""
    rp = rowptr.long().numpy()
    vals = vals.numpy().astype(np.float32)
    M, deg = len(rp) - 1, np.diff(rp)
    lanes = []
    for s in range(tpp):
        acc = np.zeros((M, vals.shape[1]), dtype=np.float32)
        cnt = np.maximum(0, (deg - s + tpp - 1) // tpp)
        for v in range(int(cnt.max()) if M else 0):
            rows = np.nonzero(cnt > v)[0]
            acc[rows] = acc[rows] + vals[rp[rows] + s + tpp * v]
        lanes.append(acc)
    while len(lanes) > 1:
        lanes = [lanes[i] + lanes[i + 1] for i in range(0, len(lanes), 2)]
    assert lanes[0].dtype == np.float32
    return torch.from_numpy(lanes[0])


def ordered_sums(c, packed, tpp):
    """(sd, sq) (M, Co) fp32: sum of the selected dz and of Q over the in-edges, in the kernel's order"""
    src, slot = (c.edges.long() >> 6), (c.edges.long() & 63)
    dz = c.dz_values(packed)
    sel = torch.where(c.arg.long()[src] == slot.unsqueeze(1), dz[src], torch.zeros((), dtype=torch.float32))
    return _ordered(sel, c.rowptr, tpp), _ordered(c.PQ[:, c.Co:2 * c.Co][src], c.rowptr, tpp)


def ordered_brute(c, packed, tpp):
    """ordered_sums by a scalar loop (tiny graphs)"""
    dz = c.dz_values(packed).numpy()
    Q = c.PQ[:, c.Co:2 * c.Co].numpy()
    sd, sq = np.zeros((c.M, c.Co), np.float32), np.zeros((c.M, c.Co), np.float32)
    for j in range(c.M):
        beg, end = int(c.rowptr[j]), int(c.rowptr[j + 1])
        for o in range(c.Co):
            ld, lq = [], []
            for s in range(tpp):
                d, q = np.float32(0), np.float32(0)
                for u in range(beg + s, end, tpp):
                    e = int(c.edges[u])
                    i, sl = e >> 6, e & 63
                    q = np.float32(q + Q[i, o])
                    if int(c.arg[i, o]) == sl:
                        d = np.float32(d + dz[i, o])
                ld.append(d)
                lq.append(q)
            if tpp == 2:
                sd[j, o], sq[j, o] = np.float32(ld[0] + ld[1]), np.float32(lq[0] + lq[1])
            elif tpp == 4:
                sd[j, o] = np.float32(np.float32(ld[0] + ld[1]) + np.float32(ld[2] + ld[3]))
                sq[j, o] = np.float32(np.float32(lq[0] + lq[1]) + np.float32(lq[2] + lq[3]))
            else:
                sd[j, o], sq[j, o] = ld[0], lq[0]
    return torch.from_numpy(sd), torch.from_numpy(sq)


def expected_planes(ref, mode):
    """What mode ``mode`` must hold for the exact fp32 result ref (M, 2Co): fp32;
    torch's round-to-nearest-even bf16; or the planes hi = bf16(v), lo = bf16(v -
    hi) and (mode 3) hi again — None for mode 2's untouched third plane."""
    v = ref.float()
    if mode == 0:
        return [v]
    hi = v.to(torch.bfloat16)
    if mode == 1:
        return [hi]
    lo = (v - hi.float()).to(torch.bfloat16)
    return [hi, lo, hi if mode == 3 else None]


def exact_f32(x):
    """the fp64 tensor as fp32, asserting nothing is lost"""
    y = x.float()
    assert torch.equal(y.double(), x)
    return y


# ---- the finalize (scatter_consts) ----------------------------------------------------------------------------------
def make_finalize(Co, nrows, seed=0):
    """Lattice partial rows (nrows, 2, Co) and power-of-two count, mean, invstd:
    dbeta = sum of rows' first plane, dgamma = of the second, c0 = a (-dbeta +
    dgamma mean invstd) / count, c1 = -a dgamma invstd / count — all exact in fp64
    and in fp32 (asserted)."""
    g = torch.Generator().manual_seed(seed + 3 * nrows + Co)
    part = torch.randint(-3, 4, (nrows, 2, Co), generator=g).float()
    mean = torch.tensor([(1., 2., -4., 0.5)[o % 4] for o in range(Co)])
    invstd = torch.tensor([(0.5, 1., 0.25)[o % 3] for o in range(Co)])
    return part, 64.0, mean, invstd


def finalize_ref(part, count, a, mean, invstd, ev):
    r = part.double().sum(0)
    dbeta, dgamma = r[0], r[1]
    g1, g2 = dbeta / count, dgamma / count
    if ev:
        c0 = c1 = torch.zeros_like(g1)
    else:
        c0 = a.double() * (-g1 + g2 * mean.double() * invstd.double())
        c1 = -a.double() * g2 * invstd.double()
    return tuple(exact_f32(x) for x in (dgamma, dbeta, c0, c1))


# ---- the case tables ------------------------------------------------------------------------------------------------
def form_of(B, N, Co, packed):
    """(cs, parts, tpp) by the launcher's rules restated — the CPU test holds this
    against dgx_edge_bwd_scatter_geometry for every table entry"""
    per_pc = 8 if packed else 9
    cs = 8
    while cs > 1 and per_pc * N * cs > 72 * 1024:
        cs //= 2
    slices = -(-Co // cs)

    def lds(parts):
        per = -(-N // parts)
        return 8 * N * cs + (0 if packed else (N * cs + 15) // 16 * 16) + (per + 7) // 8 * 8 * 2 + 64 * 4 + 16 * 2 * 8 * 8 + 64

    parts = 1
    while B * slices * parts < 512 and parts * 64 < N:
        parts *= 2
    while lds(parts) > 160 * 1024 and parts * 64 < N:
        parts *= 2
    per = -(-N // parts)
    tpp = 1
    if packed and cs == 8:
        tpp = 4 if per * 4 <= EC_THREADS else 2
    return cs, parts, tpp


# (B, N, k, Co) of a form; the default shape is B = 1, k = 4, Co = 8
def _shape(N, B=1, k=4, Co=8):
    return (B, N, k, Co)


# a. every launch form: name -> (shape, packed, (cs, tpp)); each runs the four output modes
FORMS = {
    "u8": (_shape(200), False, (8, 1)),
    "u4": (_shape(1100), False, (4, 1)),
    "u2": (_shape(2100), False, (2, 1)),
    "u1": (_shape(4200), False, (1, 1)),
    "p4": (_shape(1200), True, (4, 1)),
    "p2": (_shape(2400), True, (2, 1)),
    "p1": (_shape(4700), True, (1, 1)),
    "p8x4": (_shape(200), True, (8, 4)),
    "p8x2": (_shape(516, B=16, Co=64), True, (8, 2)),      # 4 parts of 129 points
}
REACHABLE = ([(False, cs, 1) for cs in (8, 4, 2, 1)] + [(True, cs, 1) for cs in (4, 2, 1)] +
             [(True, 8, 2), (True, 8, 4)])
MODES = (0, 1, 2, 3)

# b. both sides of every boundary: (shape, packed, (cs, tpp)); big = the 160 KiB mode past one-channel 72 KiB slices
BOUNDARIES = [
    (_shape(1024), False, (8, 1)), (_shape(1025), False, (4, 1)),
    (_shape(2048), False, (4, 1)), (_shape(2049), False, (2, 1)),
    (_shape(4096), False, (2, 1)), (_shape(4097), False, (1, 1)),
    (_shape(8192), False, (1, 1)), (_shape(8193), False, (1, 1)),
    (_shape(1152), True, (8, 4)), (_shape(1153), True, (4, 1)),
    (_shape(2304), True, (4, 1)), (_shape(2305), True, (2, 1)),
    (_shape(4608), True, (2, 1)), (_shape(4609), True, (1, 1)),
    (_shape(9216), True, (1, 1)), (_shape(9217), True, (1, 1)),
    (_shape(512, B=16, Co=64), True, (8, 4)), (_shape(516, B=16, Co=64), True, (8, 2)),   # per_pts 128 | 129
]
SMALL_N = [(_shape(1, k=1), pk) for pk in (False, True)] + [(_shape(N), pk) for N in (2, 63, 64, 65)
                                                            for pk in (False, True)]
# B with an odd number of (part x slice) tiles — 5 slices, the last of 4 channels, one part: the XCD map's
# repeated (B = 2, 3: 4 and 2 XCDs per cloud, the last short or empty) and padded (5, 9) forms
XCD_BS = (2, 3, 5, 8, 9)
XCD_SHAPE = dict(N=60, k=4, Co=36)

# c. several passes at one point part: (shape, packed, (cs, tpp), passes, points in the last pass)
PASSES = [
    (_shape(700, B=64, Co=64), False, (8, 1), 2, 188),     # 512 + a partly filled reversed pass
    (_shape(1024, B=64, Co=64), False, (8, 1), 2, 512),
    (_shape(1100, B=32, Co=64), False, (4, 1), 3, 76),     # unpacked 8-channel slices end at N = 1024
    (_shape(300, B=64, Co=64), True, (8, 2), 2, 44),
    (_shape(512, B=64, Co=64), True, (8, 2), 2, 256),
    (_shape(700, B=64, Co=64), True, (8, 2), 3, 188),
]

# d. channels and strides
CS8_COS = (1, 3, 6, 12, 20)
LDPQ_EXTRA = (0, 4, 1)
PARTIAL_SLICES = [(_shape(1100, Co=6), False, (4, 1)), (_shape(1200, Co=6), True, (4, 1)),
                  (_shape(2100, Co=3), False, (2, 1)), (_shape(2400, Co=3), True, (2, 1))]

# e / f. lanes per point 1, 2, 4 (and packed words at one lane)
LANE_FORMS = {1: (_shape(200), False, (8, 1)), 4: (_shape(200), True, (8, 4)),
              2: (_shape(516, B=16, Co=64), True, (8, 2)), "p1": (_shape(1200), True, (4, 1))}
KS = (1, 16, 17, 64)

# g. the finalize at every CS: nrows around G = 512 / CS and its 4 G unroll
FIN_FORMS = [("u8", 8), ("u4", 4), ("u2", 2), ("u1", 1), ("p8x4", 8), ("p4", 4), ("p2", 2), ("p1", 1)]


def fin_nrows(cs):
    G = EC_THREADS // cs
    return (1, G - 1, G, G + 1, 4 * G, 4 * G + 1)


def all_table_entries():
    """every (shape, packed, (cs, tpp)) the GPU file launches with a stated form"""
    out = [v for v in FORMS.values()] + list(BOUNDARIES) + [e[:3] for e in PASSES] + list(PARTIAL_SLICES)
    out += list(LANE_FORMS.values())
    out += [(_shape(200, Co=Co), pk, (8, 4 if pk else 1)) for Co in CS8_COS for pk in (False, True)]
    return out
