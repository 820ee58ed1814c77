"""Oracle, case builders, guarded buffers and shape grids of the GEMM tests
(csrc/gemm.hip, csrc/gemm32.hip): tests/test_gemm_oracle_gpu.py runs them on
the GPU, tests/test_gemm_ref_cpu.py checks this file without one.

The oracle of every GEMM is ``a.double() @ b.double().t()`` for the logical
operands a (M, K), b (N, K): C[i][j] = sum_k a[i][k] b[j][k].

Lattice cases (exact, compared with torch.equal)
------------------------------------------------
Operands are integers in [-LIM_STATS, LIM_STATS] (cases with statistics) or
[-LIM, LIM] (others), store-only cases add dyadic fractions n/8 (|n| <= 32).
Every value has at most 6 significant bits, so it is exact in bf16 (8) and the
bf16 rounding of the kernels' staging changes nothing. Products are multiples
of 1/s with s = 64 (two fractions) or 1 (integers). If

    max_ij  s * sum_k |a_ik| |b_jk|  (+ s * |addend_ij|)  <  2^24

then every partial sum of any subset of the products of one output, taken in
any order, is a multiple of 1/s below 2^24 / s in magnitude: representable in
fp32. Each fp32 addition or fma of the chain is then exact whatever the MFMA's
internal order, tree shape or rounding, the split-K slabs and their sum
included, and the result equals the fp64 product bit for bit. For statistics
the same holds for the column sums if, per 128-row partial,

    sum_i z_ij^2 < 2^24     (z integer, so |z| <= z^2 covers sum z too).

``exact_or_raise`` asserts both on the fp64 reference of EVERY lattice case; it
is never assumed.

Random cases (bounded per element, no element excluded)
-------------------------------------------------------
Operands are normal; fp32 operands of the bf16 kernels are rounded with
torch's ``.to(bfloat16)`` first (the kernels' documented RNE staging), so the
products a_ik b_jk are exact in fp32 (8 x 8 significant bits) and only the
K - 1 additions of the accumulation round. By the standard forward error
bound of a recursive sum in ANY order (Higham, Accuracy and Stability of
Numerical Algorithms, (3.5) / (4.4)): |fl(sum) - sum| <= gamma_{K-1} sum|x|,
gamma_n = n u / (1 - n u). We use the looser gamma_K and

    |got - ref|_ij <= gamma_K(u) * (|a| @ |b|^T)_ij

  u = 2^-23 on the bf16 MFMA paths: one bit looser than round-to-nearest
      (u = 2^-24) because the rounding of the MFMA's internal accumulation is
      not documented (a truncating adder has u = 2^-23);
  u = 2^-24 for gemm32 and smallk: the fp32 MFMA is a k-ordered fmaf chain
      (kernel guide), i.e. K correctly rounded operations.
Split-K adds the S - 1 additions of the slab sum over S slabs, each bounded by
u times the running magnitude <= sum|x|: the bound gains gamma_S(2^-24)
(``gamma(K, u) + gamma(S, U32)``). An ACCUM epilogue adds one rounding of
(addend + product): u32 * (|addend| + |a||b|^T). Column statistics sum R <= 128
stored values: gamma_R(2^-24) * sum_i |z_ij| (resp. z^2, each square itself
rounded once: gamma_{R+1}) on top of the error of the z themselves. None of
these numbers comes from a run.

Guarded buffers
---------------
``Buf`` allocates every operand, output, partial and slab inside a larger
allocation pre-filled with a sentinel: canonical NaN round all operands (an
over-read poisons the result), a NaN with the payload GUARD where the kernel
overwrites (a stray store of a value computed from an over-read operand NaN is
the canonical NaN and so still differs from it), the bf16-exact SENT where the
epilogue accumulates. Guard rows follow the last row, guard columns are the
``ld`` padding on both sides of the view, an optional front offset misaligns
the base. ``Buf.hit()`` names the first guard element whose bits changed.
Every address a kernel is given lies inside the allocation: nothing here can
fault even if a guard were violated.
"""
import itertools

import torch

STORE, ACCUM, STATS, SLAB, STATS16, EDZ = 0, 1, 2, 3, 4, 7
OK, EINVAL, EUNSUPPORTED = 0, -1, -2
U32 = 2.0 ** -24          # unit roundoff of fp32 round-to-nearest
U_MFMA16 = 2.0 ** -23     # assumed for the bf16 MFMA's accumulation (see above)
TWO24 = float(2 ** 24)
SENT = 12288.0            # exact in bf16 and fp32
NAN = float("nan")
GUARD = "NaN with payload"          # output sentinel: 0x7fc00123 (fp32), 0x7fd3 (bf16)
_GUARD_BITS = {4: 0x7FC00123, 2: 0x7FD3}
LIM, LIM_STATS = 4, 2


def gamma(n, u):
    return n * u / (1.0 - n * u)


# ---- operands -------------------------------------------------------------------

def lattice(g, rows, cols, lim=LIM, frac=False, dev="cpu"):
    """(rows, cols) fp32 of integers in [-lim, lim]; ``frac``: about one in
    eight elements is n/8 with |n| <= 32 instead."""
    v = torch.randint(-lim, lim + 1, (rows, cols), generator=g, device=dev).float()
    if frac:
        f = torch.randint(-32, 33, (rows, cols), generator=g, device=dev).float() / 8.0
        pick = torch.randint(0, 8, (rows, cols), generator=g, device=dev) == 0
        v = torch.where(pick, f, v)
    return v


def one_hot_rows(g, rows, cols, dev="cpu"):
    """One 1 per row (at column k(i)): with it as A, C[i][j] = B[j][k(i)] names
    the source element a wrong output read. Returns (matrix, k)."""
    k = torch.randint(0, cols, (rows,), generator=g, device=dev)
    a = torch.zeros(rows, cols, device=dev)
    a[torch.arange(rows, device=dev), k] = 1.0
    return a, k


def oracle(a, b):
    return a.double() @ b.double().t()


def exact_or_raise(a, b, s, addend=None, stats_rows=0, what=""):
    """fp64 reference of a lattice case after asserting the docstring's
    exactness conditions on it. Returns the reference (with the addend)."""
    ref = oracle(a, b)
    mag = a.double().abs() @ b.double().abs().t()
    if addend is not None:
        ref = ref + addend.double()
        mag = mag + addend.double().abs()
    top = float(mag.max()) * s if mag.numel() else 0.0
    assert top < TWO24, f"{what}: lattice case not exact: s * sum|a||b| = {top}"
    assert bool((ref * s == (ref * s).round()).all()), f"{what}: products are not multiples of 1/{s}"
    if stats_rows:
        assert s == 1
        q = float((_blocks(ref, stats_rows) ** 2).sum(1).max())
        assert q < TWO24, f"{what}: statistics not exact: sum z^2 = {q}"
    return ref


def _blocks(ref, rows):
    """(ceil(M / rows), rows, N) view of ref padded with zero rows."""
    M, N = ref.shape
    n = -(-M // rows)
    p = torch.zeros(n * rows, N, dtype=ref.dtype, device=ref.device)
    p[:M] = ref
    return p.view(n, rows, N)


def stats_ref(ref, rows=128):
    """(ceil(M / rows), 2, N) fp64 column partials: sum z, sum z^2 per block."""
    z = _blocks(ref, rows)
    return torch.stack([z.sum(1), (z * z).sum(1)], dim=1)


def slab_refs(a, b, kchunk):
    """(S, M, N) fp64: slab s = the product over k in [s kchunk, (s + 1) kchunk)."""
    K = a.shape[1]
    S = max(1, -(-K // kchunk))
    pa = torch.zeros(a.shape[0], S * kchunk, dtype=torch.float64, device=a.device)
    pb = torch.zeros(b.shape[0], S * kchunk, dtype=torch.float64, device=a.device)
    pa[:, :K], pb[:, :K] = a.double(), b.double()
    return torch.einsum("msk,nsk->smn", pa.view(-1, S, kchunk), pb.view(-1, S, kchunk))


def split_kchunk(K, splits, bk):
    """k range of one slab, as include/dgx.h documents it: ceil(K / splits)
    rounded up to the kernel's K-step (the slab COUNT is asserted against the
    library's dgx_gemm*_slabs query by every case)."""
    return -(-(-(-K // splits)) // bk) * bk


# rounding probe: ties to even both ways, one just above a tie, and negatives
PROBE = [1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -20]
PROBE = PROBE + [-v for v in PROBE]
PROBE_BF16 = [1.0, 1 + 2.0 ** -6, 1 + 2.0 ** -7, -1.0, -(1 + 2.0 ** -6), -(1 + 2.0 ** -7)]   # RNE results


def probe_case(dev="cpu"):
    """(p (6, 4) of PROBE values, e (4, 4) exact partners): oracle(bf16(p), e) is
    exact in fp32 (<= 4 terms of <= 9 bits), and differs under truncation
    (1 + 3*2^-8 -> 1 + 2^-7) and round-half-up (1 + 2^-8 -> 1 + 2^-7)."""
    p = torch.tensor([[PROBE[(i + k) % 6] for k in range(4)] for i in range(6)], dtype=torch.float32, device=dev)
    e = torch.tensor([[1, 0, 0, 0], [0, 1, 0, 0], [1, 1, 0, 0], [1, -1, 2, 0.5]], dtype=torch.float32, device=dev)
    return p, e


def bf16_round(x):
    return x.to(torch.bfloat16).to(x.dtype)


# ---- guarded buffers ------------------------------------------------------------

LAYOUTS = ("dense", "slice", "odd")
# outputs and addends of the LDS path also isolate the two halves of `odd`:
# an aligned base with ld % 4 != 0, and ld % 4 == 0 with the base 4 bytes off
OUT_LAYOUTS = LAYOUTS + ("ldodd", "baseoff")


def layout_geometry(layout, cols, vec):
    """(ld, c0, off) of a (rows, cols) view: dense; a 16-byte aligned column
    slice of a wider buffer with ld a multiple of the vector width ``vec``; the
    scalar path's: odd ld and a base one element off the allocation; or (fp32)
    only ld % 4 != 0 ("ldodd") / only the base misaligned ("baseoff")."""
    if layout == "dense":
        return cols, 0, 0
    if layout == "slice":
        return -(-(cols + 2 * vec) // vec) * vec, vec, 0
    if layout == "ldodd":
        ld = cols + 1
        return (ld + 1 if ld % 4 == 0 else ld), 0, 0
    if layout == "baseoff":
        return -(-(cols + 1) // 4) * 4, 1, 0
    assert layout == "odd"
    return (cols + 5) | 1, 1, 1


class Buf:
    """(rows, cols) view with row stride ld at column c0 of a sentinel-filled
    allocation of rows + guard_rows rows, ``off`` elements into it."""

    def __init__(self, rows, cols, dev, dtype=torch.float32, fill=GUARD, ld=None, c0=0, off=0, guard_rows=2):
        ld = cols if ld is None else ld
        assert ld >= c0 + cols
        self.rows, self.cols, self.ld, self.c0, self.off, self.fill = rows, cols, ld, c0, off, fill
        self.flat = self._filled(off + (rows + guard_rows) * ld, dtype, dev)
        self.full = self.flat[off:].view(rows + guard_rows, ld)
        self.view = self.full[:rows, c0:c0 + cols]

    def _filled(self, n, dtype, dev):
        if self.fill is not GUARD:
            return torch.full((n,), self.fill, dtype=dtype, device=dev)
        t = torch.empty((n,), dtype=dtype, device=dev)
        self._bits(t).fill_(_GUARD_BITS[t.element_size()])
        return t

    @classmethod
    def of(cls, values, layout="dense", vec=4, fill=NAN, guard_rows=2, dtype=None):
        """Buf holding ``values`` (2-D) in the given layout."""
        rows, cols = values.shape
        ld, c0, off = layout_geometry(layout, cols, vec)
        b = cls(rows, cols, values.device, dtype or values.dtype, fill, ld, c0, off, guard_rows)
        b.view.copy_(values)
        return b

    def ptr(self):
        return self.view.data_ptr()

    def _bits(self, t):
        return t.view(torch.int16 if t.element_size() == 2 else torch.int32 if t.element_size() == 4 else torch.int64)

    def hit(self):
        """None if every guard element still holds the sentinel's bits, else a
        description of the first one that does not."""
        want = self._bits(self._filled(1, self.flat.dtype, self.flat.device))
        bad = self._bits(self.flat) != want
        if self.rows and self.cols:
            bad[self.off:].view(-1, self.ld)[:self.rows, self.c0:self.c0 + self.cols] = False
        if not bool(bad.any()):
            return None
        e = int(bad.nonzero()[0])
        if e < self.off:
            return f"front guard element {e} = {float(self.flat[e])}"
        r, c = divmod(e - self.off, self.ld)
        which = ("guard row after the last row" if r >= self.rows else
                 "ld padding left of the view" if c < self.c0 else "ld padding right of the view")
        return f"{which}: row {r} (of {self.rows}), buffer column {c} (view {self.c0}..{self.c0 + self.cols}) = " \
               f"{float(self.flat[e])} (bits {int(self._bits(self.flat)[e]):#x}), sentinel {self.fill}"


def where_in_tile(i, j, family, BM, BN):
    """Tile, wave and output round of element (i, j) for a kernel family:
    'reg' (gemm_bf16_kernel), 'lds' (gemm_lds_kernel), 'g256', 'f32'."""
    ii, jj = i % BM, j % BN
    if family == "g256":
        wave, rnd = (ii // 128) * 4 + jj // 64, ii // 64
    elif family == "f32":
        wave, rnd = (ii // 32) * 2 + jj // 32, 0
    else:
        wn = 2 if BN >= 128 else 1
        wm = 4 // wn
        wave = (ii // (BM // wm)) * wn + jj // (BN // wn)
        rnd = 0
        if family == "lds":
            nr = 1 if BM * (BN + 4) * 4 <= 2 * (BM + BN) * 64 * 2 else 2
            rnd = ii // (BM // nr)
    return f"tile ({i // BM}, {j // BN}) of {BM}x{BN}, in-tile ({ii}, {jj}), wave {wave}, round {rnd}"


def first_diff(got, want, family="reg", BM=128, BN=128, sentinel=NAN):
    """None if got == want everywhere (bitwise for finite values; no element is
    excluded, a NaN in ``got`` is a difference), else a localised description."""
    g, w = got.double(), want.double()
    if g.shape != w.shape:
        return f"shape {tuple(g.shape)} != {tuple(w.shape)}"
    bad = ~(g == w)
    if not bool(bad.any()):
        return None
    at = tuple(int(v) for v in bad.nonzero()[0])
    i, j = (at[-2] if len(at) > 1 else 0), at[-1]
    return f"{int(bad.sum())} of {bad.numel()} differ, first at {at}: got {float(g[at])}, want {float(w[at])}, " \
           f"sentinel {sentinel}; {where_in_tile(i, j, family, BM, BN)}"


def bound_violation(got, ref, bound, family="reg", BM=128, BN=128):
    """None if |got - ref| <= bound for EVERY element (NaN fails), else where."""
    err = (got.double() - ref).abs()
    bad = ~(err <= bound)
    if not bool(bad.any()):
        return None
    at = tuple(int(v) for v in bad.nonzero()[0])
    return f"{int(bad.sum())} of {bad.numel()} outside the bound, first at {at}: got {float(got[at])}, want " \
           f"{float(ref[at])}, |err| {float(err[at])} > {float(bound[at])}; " \
           f"{where_in_tile(at[-2] if len(at) > 1 else 0, at[-1], family, BM, BN)}"


# ---- grids: the smallest shapes that reach each instantiation -----------------

# register-staged path, dgx_gemm_bf16: (name, a_bf16, a_ic, b_ic, epi); B is fp32 in every arm
REG_ARMS = [("xwt_store", 0, 0, 0, STORE), ("xwt_stats", 0, 0, 0, STATS),
            ("xw_store_f32", 0, 0, 1, STORE), ("xw_accum_f32", 0, 0, 1, ACCUM),
            ("xw_store_bf16", 1, 0, 1, STORE), ("xw_accum_bf16", 1, 0, 1, ACCUM),
            ("atb_slab_f32", 0, 1, 1, SLAB), ("atb_slab_bf16", 1, 1, 1, SLAB)]
REG_M = (1, 127, 128, 129, 257)
REG_N = (1, 3, 63, 64, 65, 127, 128, 129, 200)
REG_K = (1, 3, 7, 31, 32, 33, 64, 65, 97)
REG_SLAB_R = (1, 31, 32, 33, 64, 65, 100, 257, 1000)
REG_SLAB_MN = ((1, 5), (127, 63), (129, 65), (257, 200), (128, 128))


def reg_slab_splits(R):
    s = -(-R // 32)
    return sorted({1, 2, 3, s, s + 3})


ATB_SMALL_N = (1, 2, 3, 4)
ATB_SMALL_M = (1, 255, 256, 257, 600)
ATB_SMALL_R = (1, 63, 64, 65, 255, 256, 257, 700)

# LDS-DMA NT path, dgx_gemm_lds_bf16(tn = 0)
LDS64_M = (1, 63, 64, 65, 129, 321)        # 321: 6 row tiles x 2 = a grid of 12
LDS64_N = (1, 3, 8, 63, 64, 65, 127, 128, 129, 200)
LDS64_K = (64, 128, 192, 320)
LDS_STATS_M = (1, 127, 128, 129, 255, 257, 385, 577)   # 577: 5 row tiles x 2 = a grid of 10
LDS_STATS_N = (8, 63, 64, 65, 200)
LDS_STATS_K = (64, 192)
LDS128_MN = ((65409, 64), (65535, 3), (65409, 8), (32641, 129), (32767, 200), (65601, 64))   # last: a grid of 513
LDS128_K = (64, 128)
LDS_SKINNY_EDGE = ((65408, 64, 64), (65409, 64, 128), (32640, 129, 64), (32641, 129, 128))   # (M, N, BM)
G256_MN = ((65281, 256), (65408, 256), (65409, 256), (65535, 256), (65536, 256), (16129, 1024),
           (65601, 256))               # last: a grid of 257 (no multiple of 8), 65 rows in the last tile
G256_K = (64, 128, 192, 448)            # nk = 1, 2, 3, 7
G256_SPLIT = ((128, 64), (384, 192))    # (Kw, a_k): Kw = 2 a_k
G256_EPIS = (STORE, ACCUM, STATS, STATS16)

# LDS-DMA TN path (tn = 1, SLAB)
TN_M = (8, 56, 64, 72, 128, 136, 200)
TN_N = (8, 56, 64, 72, 128, 136)
TN_R = (1, 63, 64, 65, 100, 129, 1000)
# (M, N, R, splits): R = 16421 / 5600 write 129 / 44 slabs and stay on 64-row tiles;
# R = 16363 / 5500 write 256 / 86 and reach 128 rows
TN_FORCED = ((136, 72, 16421, 256), (264, 136, 5600, 86), (136, 72, 16363, 256), (136, 56, 16363, 256),
             (264, 136, 5500, 86))


def tn_splits(R):
    return sorted({1, 2, 3, 5, -(-R // 64) + 2})


# dgx_gemm_edge_dz_bf16
EDZ_M = (1, 63, 64, 65, 129)
EDZ_N = (8, 24, 64, 72, 128)
EDZ_K = (64, 128, 192)
EDZ_BIG = ((65409, 64, 64), (65409, 128, 64))

# dgx_gemm_f32 (64 x 64 x 16): (a_ic, b_ic) x epilogue forms = the 12 instantiations
F32_M = (1, 63, 64, 65, 130)
F32_N = (1, 3, 63, 64, 65, 130)
F32_K = (1, 3, 15, 16, 17, 33, 64)
F32_LAYOUTS = ((0, 0), (0, 1), (1, 0), (1, 1))
F32_FORMS = ("store", "accum_self", "accum_addend", "slab")

# dgx_gemm_smallk*_f32: (N, K) pairs; N = 1008 at K = 16 is the largest the 64 KiB check admits
SMALLK_M = (1, 15, 16, 17, 77)
SMALLK_NK = tuple((n, k) for n in (4, 8, 24, 128) for k in (1, 3, 9, 16)) + ((1008, 16),)

# conversion kernels: rows and columns around the 32 x 32 tile
CONV_SIZES = (1, 31, 32, 33, 65)


def conversion_plane(rows, cols, dev="cpu"):
    """fp32 plane cycling through the RNE ties, the largest finite fp32 (rounds
    to inf), a subnormal, +-0 and ordinary values."""
    vals = PROBE + [3.4028234663852886e38, -3.4028234663852886e38, 1e-40, -1e-40, 0.0, -0.0, 0.3, -7.25, 1e-3,
                    65504.0, 2.0 ** -126, 1.0 + 2.0 ** -9]
    t = torch.tensor(vals, dtype=torch.float32)
    idx = (torch.arange(rows).view(-1, 1) * 7 + torch.arange(cols).view(1, -1) * 3) % len(vals)
    return t[idx].to(dev)


# ---- which layouts meet which shapes -------------------------------------------
# Small grids cross the layouts outright. The others rotate them: the layout of
# buffer j at grid index (i_0, i_1, ...) is choices_j[(sum_a c_ja i_a) % len],
# with coefficients such that every choice meets every value of every axis
# (``uncovered`` checks it on the CPU for every grid below).

def rotate(axes, picks):
    """[(values, chosen)]: values = one element per axis, chosen = one choice
    per (choices, coefficients) pick."""
    out = []
    for idx in itertools.product(*[range(len(a)) for a in axes]):
        out.append((tuple(a[i] for a, i in zip(axes, idx)),
                    tuple(ch[sum(c * i for c, i in zip(co, idx)) % len(ch)] for ch, co in picks)))
    return out


def uncovered(cases, picks):
    """(axis, value, pick, choice) combinations no case of ``rotate`` holds."""
    seen = {(a, v, p, c) for vals, ch in cases for a, v in enumerate(vals) for p, c in enumerate(ch)}
    return [(a, v, p, c) for a in range(len(cases[0][0])) for v in {vals[a] for vals, _ in cases}
            for p, (choices, _) in enumerate(picks) for c in choices if (a, v, p, c) not in seen]


OPS16 = ("dense", "slice")                       # LDS-path operands: `odd` is rejected
REG_PICKS = [(LAYOUTS, (1, 1, 1)), (LAYOUTS, (1, 2, 1)), (LAYOUTS, (2, 1, 1))]             # A, B, C over (M, N, K)
REG_SLAB_PICKS = [(LAYOUTS, (1, 1, 1)), (LAYOUTS, (1, 2, 2))]                              # A, B over (MN, R, split#)
ATB_SMALL_PICKS = [((0, 1, 2, 3), (1, 1, 1)), (LAYOUTS, (1, 1, 2)), (LAYOUTS, (2, 1, 1))]  # split kind, A, B
LDS64_ADD_PICK = [(OUT_LAYOUTS, (1, 1, 1, 1, 1, 2))]   # addend over (M, N, K, split, operand layout, C layout)
LDS128_FORMS = ("store", "accum_self", "accum_addend")
LDS128_PICKS = [(OUT_LAYOUTS, (1, 1, 1, 2)), (OUT_LAYOUTS, (2, 3, 1, 1))]   # C, addend over (MN, K, form, operand layout)
G256_KCFG = tuple((k, 0) for k in G256_K) + G256_SPLIT
G256_PICKS = [(OPS16, (1, 1)), (OUT_LAYOUTS, (1, 2)), (OUT_LAYOUTS, (2, 1)), (("accum_self", "accum_addend"), (1, 1)),
              (LAYOUTS, (1, 2))]                       # operands, C, addend, ACCUM form, bf16 C over (MN, K config)
F32_PICKS = [(LAYOUTS, (1, 1, 1, 1)), (LAYOUTS, (1, 2, 1, 2)), (LAYOUTS, (2, 1, 1, 1)), (OUT_LAYOUTS, (1, 1, 2, 1)),
             ((0, 1, 2, 3), (1, 1, 1, 2))]             # A, B, C, addend, split kind over (M, N, K, form)


def reg_cases():
    return rotate((REG_M, REG_N, REG_K), REG_PICKS)


def reg_slab_cases():
    """((M, N), R, splits) with the A and B layouts."""
    out = []
    for (iM, mn), (iR, r) in itertools.product(enumerate(REG_SLAB_MN), enumerate(REG_SLAB_R)):
        for iS, s in enumerate(reg_slab_splits(r)):
            out.append(((mn, r, s), tuple(ch[sum(c * i for c, i in zip(co, (iM, iR, iS))) % len(ch)]
                                          for ch, co in REG_SLAB_PICKS)))
    return out


def atb_small_cases():
    return rotate((ATB_SMALL_N, ATB_SMALL_M, ATB_SMALL_R), ATB_SMALL_PICKS)


def lds64_cases():
    """(M, N, K, split, operand layout, C layout) crossed outright; the addend's layout rotates."""
    return rotate((LDS64_M, LDS64_N, LDS64_K, (False, True), OPS16, OUT_LAYOUTS), LDS64_ADD_PICK)


def lds_stats_cases():
    """Crossed outright: (M, N, K, operand layout, output layout)."""
    return rotate((LDS_STATS_M, LDS_STATS_N, LDS_STATS_K, OPS16, LAYOUTS), [])


def lds128_cases():
    return rotate((LDS128_MN, LDS128_K, LDS128_FORMS, OPS16), LDS128_PICKS)


def g256_cases():
    return rotate((G256_MN, G256_KCFG), G256_PICKS)


def f32_cases():
    return rotate((F32_M, F32_N, F32_K, F32_FORMS), F32_PICKS)


ROTATED = {"reg": (reg_cases, REG_PICKS), "reg_slab": (reg_slab_cases, REG_SLAB_PICKS),
           "atb_small": (atb_small_cases, ATB_SMALL_PICKS), "lds64": (lds64_cases, LDS64_ADD_PICK),
           "lds128": (lds128_cases, LDS128_PICKS), "g256": (g256_cases, G256_PICKS), "f32": (f32_cases, F32_PICKS)}


def lds_tile_sets(L):
    """{(tn, BM, BN, epi)} the LDS grids above reach, by the library's own
    dgx_gemm_lds_tile / dgx_gemm_edge_dz_rows (host arithmetic, no GPU)."""
    got = set()

    def add(tn, M, N, K, a_k, epi, splits):
        t = L.dgx_gemm_lds_tile(tn, M, N, K, a_k, epi, splits)
        assert t > 0, (tn, M, N, K, a_k, epi, splits, t)
        got.add((tn, t // 1000, t % 1000, epi))

    for M in LDS64_M:
        for N in LDS64_N:
            for K in LDS64_K:
                for epi in (STORE, ACCUM):
                    add(0, M, N, K, 0, epi, 1)
                    add(0, M, N, 2 * K, K, epi, 1)
    for M in LDS_STATS_M:
        for N in LDS_STATS_N:
            for K in LDS_STATS_K:
                for epi in (STATS, STATS16):
                    add(0, M, N, K, 0, epi, 1)
    for M, N in LDS128_MN:
        for K in LDS128_K:
            for epi in (STORE, ACCUM):
                add(0, M, N, K, 0, epi, 1)
    for M, N in G256_MN:
        for K in G256_K:
            for epi in G256_EPIS:
                add(0, M, N, K, 0, epi, 1)
    for M in TN_M:
        for N in TN_N:
            for R in TN_R:
                for s in tn_splits(R):
                    add(1, M, N, R, 0, SLAB, s)
    for M, N, R, s in TN_FORCED:
        add(1, M, N, R, 0, SLAB, s)
    for M in EDZ_M:
        for N in EDZ_N:
            got.add((0, edz_bm(L, M, N), 128 if N > 64 else 64, EDZ))
    for M, N, _ in EDZ_BIG:
        got.add((0, edz_bm(L, M, N), 128 if N > 64 else 64, EDZ))
    return got


def edz_bm(L, M, N):
    """Rows per tile of dgx_gemm_edge_dz_bf16 from its own row count."""
    rows = L.dgx_gemm_edge_dz_rows(M, N)
    assert rows in (-(-M // 64), -(-M // 128)), (M, N, rows)
    return 64 if rows == -(-M // 64) else 128


LDS_TILES_EMITTED = (
    {(0, bm, bn, e) for bm in (64, 128) for bn in (64, 128) for e in (STORE, ACCUM, EDZ)}
    | {(0, 128, bn, e) for bn in (64, 128) for e in (STATS, STATS16)}
    | {(0, 256, 256, e) for e in G256_EPIS}
    | {(1, bm, bn, SLAB) for bm in (64, 128) for bn in (64, 128)})


def edz_ref(a, w, addend, ysel, arg, scale, shift, mean, invstd, slope, bm):
    """fp64 restatement of dgx_gemm_edge_dz_bf16: (packed words (M, N) int32,
    partials (ceil(M / bm), 2, N), |terms| sums for the exactness assertion)."""
    dY = addend.double() + oracle(a, w)
    z = scale.double() * ysel.double() + shift.double()
    d = dY * torch.where(z > 0, 1.0, float(slope))
    d32 = d.float()
    assert bool((d32.double() == d).all()), "edge dz case: d is not exact in fp32"
    words = (d32.view(torch.int32) & ~63) | arg.to(torch.int32)
    yhat = (ysel.double() - mean.double()) * invstd.double()
    M, N = d.shape
    n = -(-M // bm)
    part = torch.zeros(n, 2, N, dtype=torch.float64, device=d.device)
    mag = 0.0
    for t in range(n):
        dd, yy = d[t * bm:(t + 1) * bm], yhat[t * bm:(t + 1) * bm]
        part[t, 0], part[t, 1] = dd.sum(0), (dd * yy).sum(0)
        mag = max(mag, float(dd.abs().sum(0).max()), float((dd * yy).abs().sum(0).max()))
    return words, part, mag


def smallk_chain(x, w):
    """C = X W^T as the fp32 chain acc = fma(x_k, w_k, acc) over k in order, for
    operands whose products are exact in fp32 (<= 11 significant bits each):
    then fma(x, w, acc) = fl(acc + x w) and a plain fp32 running sum equals it."""
    acc = torch.zeros(x.shape[0], w.shape[0], dtype=torch.float32, device=x.device)
    for k in range(x.shape[1]):
        acc = acc + x[:, k:k + 1] * w[:, k].view(1, -1)
    return acc


def bits11(g, rows, cols, dev="cpu"):
    """Normal values rounded to 11 significant bits."""
    v = torch.randn(rows, cols, generator=g, device=dev)
    m, e = torch.frexp(v)
    return torch.ldexp((m * 2048).round() / 2048, e)
