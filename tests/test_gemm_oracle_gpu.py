"""Every GEMM instantiation of csrc/gemm.hip and csrc/gemm32.hip against the
fp64 oracle ``a.double() @ b.double().t()`` (tests/_gemm_ref.py, where the
exactness condition of the lattice cases and the bounds of the random cases
are derived): exact comparisons at every tile edge, guarded outputs, partials
and slabs, NaN-poisoned operand surrounds, the scalar fallbacks, every reject.

Each case asserts the tile the launcher takes by the library's own query
(dgx_gemm_lds_tile, dgx_gemm_edge_dz_rows, dgx_gemm*_slabs). Shapes loop inside
the tests. The layouts (dense / aligned column slice / odd = scalar path, and
for LDS-path outputs and addends also ld % 4 != 0 alone and a misaligned base
alone) are crossed outright with the small grids and rotated over the others by
the generators of _gemm_ref.py, whose coverage (every layout of every buffer
meets every value of every axis) test_gemm_ref_cpu.py asserts. A test collects
all failing cases and reports the first ones, each localised to element, tile,
wave and round."""
import ctypes
import itertools

import pytest
import torch

import _gemm_ref as R
from _gemm_ref import ACCUM, SLAB, STATS, STATS16, STORE, Buf

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16


def vp(x):
    return ctypes.c_void_p(x) if x else None


class Ctx:
    def __init__(self, dev, seed):
        from dgx import _native as nat
        self.nat, self.L, self.dev = nat, nat.lib(), dev
        self.g = torch.Generator(device=dev).manual_seed(seed)
        self.st = nat.stream_of(torch.empty(1, device=dev))
        self.fails, self.n, self.cnt = [], 0, 0

    def rot(self, *choices):
        """next combination of layouts for the few random cases (their layouts are not a grid)"""
        c, out = self.cnt, []
        for ch in choices:
            out.append(ch[c % len(ch)])
            c //= len(ch)
        self.cnt += 1
        return out

    def check(self, what, *problems):
        self.n += 1
        for p in problems:
            if p:
                self.fails.append(f"{what}: {p}")

    def done(self, at_least=1):
        assert self.n >= at_least, f"only {self.n} cases ran"
        assert not self.fails, f"{len(self.fails)} failures in {self.n} cases:\n" + "\n".join(self.fails[:12])


def operand(values, ic, dtype, layout):
    """Buf of a logical (rows, K) operand: stored as is (k contiguous) or
    transposed (ic: row index contiguous), NaN all round."""
    v = values.t() if ic else values
    return Buf.of(v.to(dtype), layout, vec=8 if dtype == BF16 else 4)


def out_buf(M, N, dev, layout, fill, dtype=F32, vec=4, guard_rows=2):
    ld, c0, off = R.layout_geometry(layout, N, vec)
    return Buf(M, N, dev, dtype, fill, ld, c0, off, guard_rows)


def slab_reduce(cx, slab, S, M, N):
    out = out_buf(M, N, cx.dev, "slice", R.GUARD)
    rc = cx.L.dgx_slab_reduce_f32(vp(slab.ptr()), S, M, N, M, vp(out.ptr()), out.ld, cx.st)
    return rc, out


# ---- register-staged path: dgx_gemm_bf16 -------------------------------------------

def reg_call(cx, arm, A, B, M, N, K, splits, C, ldc, part):
    _, a16, aic, bic, epi = arm
    return cx.L.dgx_gemm_bf16(vp(A.ptr()), a16, aic, A.ld, vp(B.ptr()), 0, bic, B.ld, M, N, K, epi, splits,
                              vp(C.ptr()), ldc, vp(part.ptr()) if part else None, cx.st)


@pytest.mark.parametrize("arm", [a for a in R.REG_ARMS if a[4] != SLAB], ids=lambda a: a[0])
def test_reg_lattice_every_tile_edge(cuda, arm):
    """dgx_gemm_bf16, STORE / ACCUM / STATS arms: M x N x K edges of the 128 x
    {64, 128} x 32 tile, exact; outputs and partials guarded; the three layouts
    (vector loads, and the scalar vec_a / vec_b fallbacks) rotate."""
    cx = Ctx(cuda, 11)
    name, a16, aic, bic, epi = arm
    lim, frac = (R.LIM_STATS, False) if epi == STATS else (R.LIM, epi == STORE)
    for (M, N, K), (la, lb, lc) in R.reg_cases():
        a, b = R.lattice(cx.g, M, K, lim, frac, cuda), R.lattice(cx.g, N, K, lim, frac, cuda)
        add = R.lattice(cx.g, M, N, R.LIM, False, cuda) if epi == ACCUM else None
        what = f"{name} M={M} N={N} K={K} A:{la} B:{lb} C:{lc}"
        ref = R.exact_or_raise(a, b, 64 if frac else 1, add, 128 if epi == STATS else 0, what)
        A, B = operand(a, aic, BF16 if a16 else F32, la), operand(b, bic, F32, lb)
        C = out_buf(M, N, cuda, lc, R.SENT if epi == ACCUM else R.GUARD)
        if add is not None:
            C.view.copy_(add)
        rows = cx.L.dgx_gemm_stats_rows(M)
        part = Buf(rows, 2 * N, cuda) if epi == STATS else None
        rc = reg_call(cx, arm, A, B, M, N, K, 1, C, C.ld, part)
        bn = 128 if N > 64 else 64
        probs = [rc and f"rc {rc}", R.first_diff(C.view, ref, "reg", 128, bn), C.hit()]
        if part:
            assert rows == -(-M // 128)
            probs += [R.first_diff(part.view.view(rows, 2, N), R.stats_ref(ref)), part.hit()]
        cx.check(what, *probs)
    cx.done(len(R.REG_M) * len(R.REG_N) * len(R.REG_K))


@pytest.mark.parametrize("arm", [a for a in R.REG_ARMS if a[4] == SLAB], ids=lambda a: a[0])
def test_reg_split_k_slabs(cuda, arm):
    """A^T B through the C entry with forced splits: every written slab equals
    its own k-range's product exactly, slabs past dgx_gemm_slabs stay NaN, and
    dgx_slab_reduce_f32 of them is the whole product."""
    cx = Ctx(cuda, 12)
    name, a16 = arm[0], arm[1]
    for ((M, N), Rr, splits), (la, lb) in R.reg_slab_cases():
        a, b = R.lattice(cx.g, M, Rr, R.LIM, True, cuda), R.lattice(cx.g, N, Rr, R.LIM, True, cuda)
        what = f"{name} M={M} N={N} R={Rr} splits={splits} A:{la} B:{lb}"
        ref = R.exact_or_raise(a, b, 64, what=what)
        S, kc = cx.L.dgx_gemm_slabs(Rr, splits), R.split_kchunk(Rr, splits, 32)
        assert S == -(-Rr // kc) <= splits, what
        A, B = operand(a, 1, BF16 if a16 else F32, la), operand(b, 1, F32, lb)
        slab = Buf(S * M, N, cuda, guard_rows=2 * M + 2)
        rc = reg_call(cx, arm, A, B, M, N, Rr, splits, slab, N, None)
        rc2, out = slab_reduce(cx, slab, S, M, N)
        cx.check(what, (rc or rc2) and f"rc {rc} {rc2}",
                 R.first_diff(slab.view.view(S, M, N), R.slab_refs(a, b, kc), "reg", 128, 128 if N > 64 else 64),
                 slab.hit(), R.first_diff(out.view, ref), out.hit())
    cx.done(190)


def test_reg_atb_small(cuda):
    """atb_small_kernel (bf16 A, N <= 4): exact slabs, guarded, and a second run
    is bit-identical."""
    cx = Ctx(cuda, 13)
    arm = ("atb_small", 1, 1, 1, SLAB)
    for (N, M, Rr), (kind, la, lb) in R.atb_small_cases():
        splits = (1, 3, cx.L.dgx_gemm_splits(M, N, Rr), -(-Rr // 32) + 3)[kind]
        a, b = R.lattice(cx.g, M, Rr, R.LIM, True, cuda), R.lattice(cx.g, N, Rr, R.LIM, True, cuda)
        what = f"atb_small M={M} N={N} R={Rr} splits={splits} A:{la} B:{lb}"
        ref = R.exact_or_raise(a, b, 64, what=what)
        S, kc = cx.L.dgx_gemm_slabs(Rr, splits), R.split_kchunk(Rr, splits, 32)
        A, B = operand(a, 1, BF16, la), operand(b, 1, F32, lb)
        slabs = []
        for _ in range(2):
            slab = Buf(S * M, N, cuda, guard_rows=2 * M + 2)
            rc = reg_call(cx, arm, A, B, M, N, Rr, splits, slab, N, None)
            slabs.append(slab)
            cx.check(what, rc and f"rc {rc}", R.first_diff(slab.view.view(S, M, N), R.slab_refs(a, b, kc)), slab.hit())
        rc2, out = slab_reduce(cx, slabs[0], S, M, N)
        cx.check(what, rc2 and f"rc {rc2}", R.first_diff(out.view, ref), out.hit(),
                 not torch.equal(slabs[0].view, slabs[1].view) and "two runs differ")
    cx.done(160)


def test_reg_rounding_probe(cuda):
    """fp32 operands are rounded to bf16 to nearest EVEN while staged: ties both
    ways and a just-above-tie, in A (where A is fp32) and in B (always fp32,
    atb_small's LDS staging included), against torch's .to(bfloat16)."""
    cx = Ctx(cuda, 14)
    p, e = R.probe_case(cuda)
    for arm in R.REG_ARMS + [("atb_small", 1, 1, 1, SLAB)]:
        name, a16, aic, bic, epi = arm
        for a, b in ((p, e), (e, p)):
            if a16 and a is p:
                continue
            for la in R.LAYOUTS:
                if name == "atb_small":
                    b = b[:4]
                M, N, K = a.shape[0], b.shape[0], 4
                ref = R.oracle(R.bf16_round(a), R.bf16_round(b))
                A, B = operand(a, aic, BF16 if a16 else F32, la), operand(b, bic, F32, la)
                C = out_buf(M, N, cuda, "dense" if epi == SLAB else la, R.SENT if epi == ACCUM else R.GUARD)
                if epi == ACCUM:
                    C.view.fill_(2.0)
                    ref = ref + 2.0
                part = Buf(1, 2 * N, cuda) if epi == STATS else None
                rc = reg_call(cx, arm, A, B, M, N, K, 1, C, C.ld, part)
                cx.check(f"probe {name} {'A' if a is p else 'B'} {la}", rc and f"rc {rc}", R.first_diff(C.view, ref),
                         C.hit())
    cx.done(40)


def test_reg_random_within_the_derived_bound(cuda):
    """Normal operands, every element within gamma_K(2^-23) |a||b|^T (+ the ACCUM
    rounding, + gamma_S for the slab sum) of the fp64 product of the
    bf16-rounded operands."""
    cx = Ctx(cuda, 15)
    for arm in R.REG_ARMS:
        name, a16, aic, bic, epi = arm
        for M, N, K in ((257, 200, 97), (129, 65, 33), (130, 3, 1000)):
            la, lb, lc = cx.rot(R.LAYOUTS, R.LAYOUTS, R.LAYOUTS)
            a = R.bf16_round(torch.randn(M, K, generator=cx.g, device=cuda))
            b = torch.randn(N, K, generator=cx.g, device=cuda)
            ref = R.oracle(a, R.bf16_round(b))
            mag = a.double().abs() @ R.bf16_round(b).double().abs().t()
            bound = R.gamma(K, R.U_MFMA16) * mag
            A, B = operand(a, aic, BF16 if a16 else F32, la), operand(b, bic, F32, lb)
            what = f"random {name} M={M} N={N} K={K}"
            if epi == SLAB:
                splits = 4
                S = cx.L.dgx_gemm_slabs(K, splits)
                slab = Buf(S * M, N, cuda, guard_rows=M + 1)
                rc = reg_call(cx, arm, A, B, M, N, K, splits, slab, N, None)
                rc2, C = slab_reduce(cx, slab, S, M, N)
                rc, bound = rc or rc2, bound + R.gamma(S, R.U32) * mag
            else:
                C = out_buf(M, N, cuda, lc, R.SENT if epi == ACCUM else R.GUARD)
                part = Buf(cx.L.dgx_gemm_stats_rows(M), 2 * N, cuda) if epi == STATS else None
                if epi == ACCUM:
                    add = torch.randn(M, N, generator=cx.g, device=cuda)
                    C.view.copy_(add)
                    ref = ref + add.double()
                    bound = bound + R.U32 * (add.double().abs() + mag) * (1 + R.gamma(K, R.U_MFMA16))
                rc = reg_call(cx, arm, A, B, M, N, K, 1, C, C.ld, part)
                if part:
                    z = C.view.double()
                    rows = part.rows
                    sb = torch.stack([R.gamma(128, R.U32) * R._blocks(z.abs(), 128).sum(1),
                                      R.gamma(129, R.U32) * R._blocks(z * z, 128).sum(1)], 1)
                    cx.check(what + " stats", R.bound_violation(part.view.view(rows, 2, N), R.stats_ref(z), sb),
                             part.hit())
            cx.check(what, rc and f"rc {rc}", R.bound_violation(C.view, ref, bound), C.hit())
    cx.done(24)


# ---- LDS-DMA path: dgx_gemm_lds_bf16 ----------------------------------------------

def nt_case(cx, M, N, K, split, epi, form, lo, lc, want_bm, lim=None, random=False, ab=None, what="", ld=None):
    """One NT launch. split: B = [W_hi | W_lo] (Kw = 2K, a_k = K). form: 'store',
    'accum_self' (C += ..), 'accum_addend' (C = addend + ..), 'stats',
    'stats16'. lo: operand layout (dense / slice), lc: output (and addend)
    layout unless ``ld`` names the addend's own. Records into cx; returns the partials."""
    dev = cx.dev
    stats = epi in (STATS, STATS16)
    Kw = 2 * K if split else K
    ld = ld or lc
    what = f"lds nt {form} M={M} N={N} K={K}{' split' if split else ''} ops:{lo} C:{lc} addend:{ld} {what}"
    tile = cx.L.dgx_gemm_lds_tile(0, M, N, Kw, K if split else 0, epi, 1)
    bm, bn = tile // 1000, tile % 1000
    if bm != want_bm:
        cx.check(what, f"dgx_gemm_lds_tile = {tile}, the grid is meant to reach {want_bm}-row tiles")
        return
    family = "g256" if bm == 256 else "lds"
    if ab is not None:
        a, b = ab
    elif random:
        a = R.bf16_round(torch.randn(M, K, generator=cx.g, device=dev))
        b = R.bf16_round(torch.randn(N, Kw, generator=cx.g, device=dev))
    else:
        lim = lim or (R.LIM_STATS if stats else R.LIM)
        frac = form == "store"
        a, b = R.lattice(cx.g, M, K, lim, frac, dev), R.lattice(cx.g, N, Kw, lim, frac, dev)
    a2 = torch.cat([a, a], 1) if split else a
    add = None
    if epi == ACCUM:
        add = torch.randn(M, N, generator=cx.g, device=dev) if random else R.lattice(cx.g, M, N, R.LIM, False, dev)
    if random:
        ref = R.oracle(a2, b)
        mag = a2.double().abs() @ b.double().abs().t()
        bound = R.gamma(Kw, R.U_MFMA16) * mag
        if add is not None:
            ref = ref + add.double()
            bound = bound + R.U32 * (add.double().abs() + mag) * (1 + R.gamma(Kw, R.U_MFMA16))
    else:
        ref = R.exact_or_raise(a2, b, 64 if form == "store" else 1, add, 128 if stats else 0, what)
    A, B = operand(a, 0, BF16, lo), operand(b, 0, BF16, lo)
    o16 = epi == STATS16
    C = out_buf(M, N, dev, lc, R.SENT if form == "accum_self" else R.GUARD, BF16 if o16 else F32, 8 if o16 else 4)
    D = None
    if form == "accum_self":
        C.view.copy_(add)
    elif form == "accum_addend":
        D = Buf.of(add, ld, 4)
    rows = cx.L.dgx_gemm_stats_rows(M)
    part = Buf(rows, 2 * N, dev) if stats else None
    rc = cx.L.dgx_gemm_lds_bf16(vp(A.ptr()), A.ld, vp(B.ptr()), B.ld, 0, M, N, Kw, K if split else 0, epi, 1,
                                vp(C.ptr()), C.ld, vp(part.ptr()) if part else None, vp(D.ptr()) if D else None,
                                D.ld if D else 0, cx.st)
    if random:
        probs = [R.bound_violation(C.view, ref, bound, family, bm, bn)]
    elif o16:
        probs = [R.first_diff(C.view, ref.to(BF16), family, bm, bn)]   # one RNE of the exact fp32 sum
    else:
        probs = [R.first_diff(C.view, ref, family, bm, bn)]
    if part and not random:
        probs += [R.first_diff(part.view.view(rows, 2, N), R.stats_ref(ref)), part.hit()]
    cx.check(what, rc and f"rc {rc}", C.hit(), D and D.hit(), *probs)
    return part


NT_FORMS = {"store": STORE, "accum_self": ACCUM, "accum_addend": ACCUM}


@pytest.mark.parametrize("form", list(NT_FORMS))
def test_lds_nt_64_row_tiles(cuda, form):
    """gemm_lds_kernel<false, 64, {64, 128}, STORE / ACCUM>: every small or
    ragged shape takes 64-row tiles; plain and split weight (Kw = 2K, a_k = K);
    operands dense and as column slices, C in all five output layouts, all
crossed; the addend's own layout rotates (ldd % 4 and its base alone too)."""
    cx = Ctx(cuda, 21)
    for (M, N, K, split, lo, lc), (ld,) in R.lds64_cases():
        nt_case(cx, M, N, K, split, NT_FORMS[form], form, lo, lc, 64, ld=ld)
    cx.done(20 * len(R.LDS64_M) * len(R.LDS64_N) * len(R.LDS64_K))


def test_lds_nt_stats_and_bf16_output(cuda):
    """STATS and STATS16 (always 128-row tiles): every partial row exact and
    guarded; the bf16 output equals ref.to(bfloat16) at ldc % 8 == 0 and not;
    STATS16's partials equal STATS's bit for bit."""
    cx = Ctx(cuda, 22)
    for (M, N, K, lo, lc), _ in R.lds_stats_cases():
        ab = (R.lattice(cx.g, M, K, R.LIM_STATS, False, cuda), R.lattice(cx.g, N, K, R.LIM_STATS, False, cuda))
        p32 = nt_case(cx, M, N, K, False, STATS, "stats", lo, lc, 128, ab=ab)
        p16 = nt_case(cx, M, N, K, False, STATS16, "stats16", lo, lc, 128, ab=ab)
        if p32 and p16:
            cx.check(f"M={M} N={N} K={K}", not torch.equal(p32.view, p16.view) and "STATS16 partials differ from STATS")
    cx.done(6 * 3 * len(R.LDS_STATS_M) * len(R.LDS_STATS_N) * len(R.LDS_STATS_K))


def test_lds_nt_128_row_tiles_at_ragged_m(cuda):
    """gemm_lds_kernel<false, 128, {64, 128}, STORE / ACCUM> with a ragged last
    tile: M just past the skinny rule's threshold (the query confirms 64 rows
    one row earlier), reference computed and compared on the device."""
    cx = Ctx(cuda, 23)
    for M, N, bm in R.LDS_SKINNY_EDGE:
        assert cx.L.dgx_gemm_lds_tile(0, M, N, 64, 0, STORE, 1) // 1000 == bm
    for ((M, N), K, form, lo), (lc, ld) in R.lds128_cases():
        nt_case(cx, M, N, K, False, NT_FORMS[form], form, lo, lc, 128, ld=ld)
    nt_case(cx, 65409, 64, 64, True, STORE, "store", "dense", "odd", 128)
    cx.done(6 * len(R.LDS128_MN) * len(R.LDS128_K))


@pytest.mark.parametrize("epi", R.G256_EPIS, ids=["store", "accum", "stats", "stats16"])
def test_lds_nt_256x256_kernel(cuda, epi):
    """gemm256_nt_kernel: last tiles of 1, 128, 129, 255, 256 (and 65) rows, nk =
    1, 2, 3, 7 (ring prologue and wrap-arounds), the split weight at a_k = 64 and
    192, every partial row exact and the row after the last untouched."""
    cx = Ctx(cuda, 24)
    A_all = R.lattice(cx.g, max(m for m, _ in R.G256_MN), max(R.G256_K), R.LIM_STATS, False, cuda)
    B_all = R.lattice(cx.g, max(n for _, n in R.G256_MN), max(max(R.G256_K), max(k for k, _ in R.G256_SPLIT)),
                      R.LIM_STATS, False, cuda)
    form = {STORE: "store", ACCUM: "accum", STATS: "stats", STATS16: "stats16"}[epi]
    for ((M, N), (Kw, ak)), (lo, lc, ld, fa, lc16) in R.g256_cases():
        f = form if epi != ACCUM else fa
        K = ak or Kw
        nt_case(cx, M, N, K, bool(ak), epi, f, lo, lc16 if epi == STATS16 else lc, 256,
                ab=(A_all[:M, :K], B_all[:N, :Kw]), ld=ld)
    cx.done(len(R.G256_MN) * (len(R.G256_K) + len(R.G256_SPLIT)))


def test_lds_nt_random_within_the_derived_bound(cuda):
    cx = Ctx(cuda, 25)
    for (M, N, K, bm), form in itertools.product(((129, 200, 320, 64), (65409, 64, 128, 128), (65281, 256, 448, 256)),
                                                 NT_FORMS):
        lo, lc = cx.rot(("dense", "slice"), R.LAYOUTS)
        nt_case(cx, M, N, K, False, NT_FORMS[form], form, lo, lc, bm, random=True)
        nt_case(cx, M, N, K // 2 if K % 128 == 0 else K, K % 128 == 0, NT_FORMS[form], form, lo, lc, bm, random=True)
    # TN: the slab sum adds gamma_S(2^-24)
    for M, N, Rr, splits in ((200, 136, 1000, 5), (72, 56, 129, 2), (136, 72, 16363, 256)):
        a = R.bf16_round(torch.randn(M, Rr, generator=cx.g, device=cuda))
        b = R.bf16_round(torch.randn(N, Rr, generator=cx.g, device=cuda))
        mag = a.double().abs() @ b.double().abs().t()
        S = cx.L.dgx_gemm_lds_slabs(Rr, splits)
        A, B = operand(a, 1, BF16, "slice"), operand(b, 1, BF16, "dense")
        slab = Buf(S * M, N, cuda, guard_rows=M + 1)
        rc = cx.L.dgx_gemm_lds_bf16(vp(A.ptr()), A.ld, vp(B.ptr()), B.ld, 1, M, N, Rr, 0, SLAB, splits, vp(slab.ptr()),
                                    N, None, None, 0, cx.st)
        rc2, out = slab_reduce(cx, slab, S, M, N)
        cx.check(f"random tn M={M} N={N} R={Rr}", (rc or rc2) and f"rc {rc} {rc2}", slab.hit(), out.hit(),
                 R.bound_violation(out.view, R.oracle(a, b), (R.gamma(Rr, R.U_MFMA16) + R.gamma(S, R.U32)) * mag))
    cx.done(21)


def tn_case(cx, M, N, Rr, splits, lo, want_bm=None):
    dev = cx.dev
    what = f"lds tn M={M} N={N} R={Rr} splits={splits} ops:{lo}"
    tile = cx.L.dgx_gemm_lds_tile(1, M, N, Rr, 0, SLAB, splits)
    bm, bn = tile // 1000, tile % 1000
    if tile < 0 or (want_bm and bm != want_bm):
        cx.check(what, f"dgx_gemm_lds_tile = {tile}, wanted {want_bm}-row tiles")
        return
    a, b = R.lattice(cx.g, M, Rr, R.LIM, True, dev), R.lattice(cx.g, N, Rr, R.LIM, True, dev)
    ref = R.exact_or_raise(a, b, 64, what=what)
    S, kc = cx.L.dgx_gemm_lds_slabs(Rr, splits), R.split_kchunk(Rr, splits, 64)
    assert S == -(-Rr // kc) <= splits, what
    A, B = operand(a, 1, BF16, lo), operand(b, 1, BF16, lo)
    slab = Buf(S * M, N, dev, guard_rows=2 * M + 2)
    rc = cx.L.dgx_gemm_lds_bf16(vp(A.ptr()), A.ld, vp(B.ptr()), B.ld, 1, M, N, Rr, 0, SLAB, splits, vp(slab.ptr()), N,
                                None, None, 0, cx.st)
    rc2, out = slab_reduce(cx, slab, S, M, N)
    cx.check(what, (rc or rc2) and f"rc {rc} {rc2}",
             R.first_diff(slab.view.view(S, M, N), R.slab_refs(a, b, kc), "lds", bm, bn), slab.hit(),
             R.first_diff(out.view, ref, "lds", bm, bn), out.hit())
    return bm, bn


@pytest.mark.parametrize("lo", ["dense", "slice"])
def test_lds_tn_slabs(cuda, lo):
    """gemm_lds_kernel<true, *, *, SLAB>: M and N multiples of 8 that are no
    multiples of the tile (the clamped last 16-byte chunk), reduction lengths
    with a partial last K-step (its zeroed k-rows), forced splits; every slab
    exact, unwritten slabs untouched."""
    cx = Ctx(cuda, 31)
    for M, N, Rr in itertools.product(R.TN_M, R.TN_N, R.TN_R):
        for splits in R.tn_splits(Rr):
            tn_case(cx, M, N, Rr, splits, lo)
    got = {tn_case(cx, M, N, Rr, splits, lo) for M, N, Rr, splits in R.TN_FORCED}
    assert got >= {(128, 128), (128, 64), (64, 128)}, got
    cx.done(1000)


def test_atb_wrappers_unstack_into_a_strided_guarded_destination(cuda):
    """lds_atb / mm_atb(split_rows=) end to end at ragged sizes: the [W1; W2] ->
    [W1 | W2] un-stacking into a column slice, exact, surround untouched."""
    from dgx import gemm as G
    cx = Ctx(cuda, 32)
    for fn, dt, Rr, co, N in ((G.lds_atb, BF16, 1000, 36, 40), (G.lds_atb, BF16, 129, 68, 136),
                              (G.mm_atb, F32, 257, 5, 7), (G.mm_atb, BF16, 1000, 65, 3), (G.mm_atb, F32, 100, 64, 130)):
        M = 2 * co
        a, b = R.lattice(cx.g, M, Rr, R.LIM, True, cuda), R.lattice(cx.g, N, Rr, R.LIM, True, cuda)
        what = f"{fn.__name__} {dt} R={Rr} co={co} N={N}"
        full = R.exact_or_raise(a, b, 64, what=what)
        A = operand(a, 1, dt, "slice")
        B = operand(b, 1, BF16 if fn is G.lds_atb else F32, "slice")
        out = out_buf(co, 2 * N, cuda, "slice", R.GUARD)
        fn(A.view, B.view, out.view, split_rows=co)
        cx.check(what, R.first_diff(out.view, torch.cat([full[:co], full[co:]], 1)), out.hit())
    cx.done(5)


# ---- dgx_gemm_edge_dz_bf16 ------------------------------------------------------------

def edz_case(cx, M, N, K, ldd_layout, want_bm=None):
    dev, g = cx.dev, cx.g
    what = f"edge dz M={M} N={N} K={K} addend:{ldd_layout}"
    rows = cx.L.dgx_gemm_edge_dz_rows(M, N)
    bm = R.edz_bm(cx.L, M, N)
    if want_bm and bm != want_bm:
        cx.check(what, f"{rows} partial rows: {bm}-row tiles, wanted {want_bm}")
        return
    a, w = R.lattice(g, M, K, R.LIM_STATS, False, dev), R.lattice(g, N, K, R.LIM_STATS, False, dev)
    add, ysel = R.lattice(g, M, N, R.LIM, False, dev), R.lattice(g, M, N, 3, False, dev)
    arg = torch.randint(0, 64, (M + 2, N), generator=g, device=dev, dtype=torch.uint8)
    scale, shift, mean = (R.lattice(g, 1, N, 2, False, dev).view(N).contiguous() for _ in range(3))
    invstd = torch.tensor([0.5, 1.0, 2.0, 0.25], device=dev)[torch.randint(0, 4, (N,), generator=g, device=dev)]
    slope = 0.25
    R.exact_or_raise(a, w, 1, add, what=what)
    words, pref, mag = R.edz_ref(a, w, add, ysel, arg[:M], scale, shift, mean, invstd, slope, bm)
    assert mag * 16 < R.TWO24, what                      # d in 1/4, yhat in 1/4: sums of 1/16 below 2^24
    assert bool(((scale * ysel + shift) == 0).any()) or M * N < 16, what   # z = 0 is on the slope side
    A, W = operand(a, 0, BF16, "dense"), operand(w, 0, BF16, "slice")
    D, Y = Buf.of(add, ldd_layout, 4), Buf.of(ysel, "dense")
    dz, part = Buf(M, N, dev), Buf(rows, 2 * N, dev)
    rc = cx.L.dgx_gemm_edge_dz_bf16(vp(A.ptr()), A.ld, vp(W.ptr()), W.ld, M, N, K, vp(D.ptr()), D.ld, vp(Y.ptr()),
                                    vp(arg.data_ptr()), vp(scale.data_ptr()), vp(shift.data_ptr()),
                                    vp(mean.data_ptr()), vp(invstd.data_ptr()), slope, vp(dz.ptr()), vp(part.ptr()),
                                    rows, cx.st)
    bn = 128 if N > 64 else 64
    cx.check(what, rc and f"rc {rc}", R.first_diff(dz.view.view(torch.int32), words, "lds", bm, bn), dz.hit(),
             R.first_diff(part.view.view(rows, 2, N), pref), part.hit(), D.hit())


def edz_lowbits_case(cx, M, N, K, positive):
    """Addends with full 24-bit mantissas, so d has its six low mantissa bits
    set: the word must be (bits(d) & ~63) | slot with d = fl(product + addend)
    * factor (one fp32 addition of an exact product, an exact scaling: the
    reference forms the same fp32 value), and the partials must sum the
    UNMASKED d. ``positive``: every d > 0, z > 0, yhat = 1, so masking before
    the sum would lose about 31 ulp per element, all in one direction (42 u
    relative, u = 2^-24), while a sum of M <= 8 fp32 terms is within gamma_M(u)
    sum|d| <= 8 u sum|d| of the fp64 one: the bound tells the two apart."""
    dev, g = cx.dev, cx.g
    what = f"edge dz low bits M={M} N={N} K={K} positive={positive}"
    rows, bm = cx.L.dgx_gemm_edge_dz_rows(M, N), R.edz_bm(cx.L, M, N)
    a, w = R.lattice(g, M, K, 1, False, dev), R.lattice(g, N, K, 1, False, dev)
    prod = R.exact_or_raise(a, w, 1, what=what)
    add = torch.randn(M, N, generator=g, device=dev)
    arg = torch.randint(0, 64, (M + 2, N), generator=g, device=dev, dtype=torch.uint8)
    if positive:
        add = add.abs() + float(prod.abs().max()) + 1.0
        ysel, scale, shift = (torch.ones(M, N, device=dev), torch.ones(N, device=dev), torch.zeros(N, device=dev))
        mean, invstd = torch.zeros(N, device=dev), torch.ones(N, device=dev)
    else:
        ysel = R.lattice(g, M, N, 3, False, dev)
        scale, shift, mean = (R.lattice(g, 1, N, 2, False, dev).view(N).contiguous() for _ in range(3))
        invstd = torch.tensor([0.5, 1.0, 2.0, 0.25], device=dev)[torch.randint(0, 4, (N,), generator=g, device=dev)]
    slope = 0.25
    dY = prod.float() + add                                  # the epilogue's one fp32 addition
    d = dY * torch.where(scale * ysel + shift > 0, 1.0, slope).float()
    words = (d.view(torch.int32) & ~63) | arg[:M].to(torch.int32)
    assert bool((d.view(torch.int32) & 63 != 0).any()), what
    yhat = (ysel.double() - mean.double()) * invstd.double()
    assert M <= bm
    pref = torch.stack([d.double().sum(0), (d.double() * yhat).sum(0)]).view(1, 2, N)
    bound = torch.stack([R.gamma(M, R.U32) * d.double().abs().sum(0),
                         R.gamma(M + 1, R.U32) * (d.double() * yhat).abs().sum(0)]).view(1, 2, N)
    A, W = operand(a, 0, BF16, "dense"), operand(w, 0, BF16, "dense")
    D, Y = Buf.of(add, "slice", 4), Buf.of(ysel, "dense")
    dz, part = Buf(M, N, dev), Buf(rows, 2 * N, dev)
    rc = cx.L.dgx_gemm_edge_dz_bf16(vp(A.ptr()), A.ld, vp(W.ptr()), W.ld, M, N, K, vp(D.ptr()), D.ld, vp(Y.ptr()),
                                    vp(arg.data_ptr()), vp(scale.data_ptr()), vp(shift.data_ptr()),
                                    vp(mean.data_ptr()), vp(invstd.data_ptr()), slope, vp(dz.ptr()), vp(part.ptr()),
                                    rows, cx.st)
    cx.check(what, rc and f"rc {rc}", R.first_diff(dz.view.view(torch.int32), words, "lds", bm, 128 if N > 64 else 64),
             dz.hit(), R.bound_violation(part.view.view(rows, 2, N), pref, bound), part.hit())
    if positive:   # the check can tell: partials of the masked d lie outside the bound
        masked = (d.view(torch.int32) & ~63).view(torch.float32).double().sum(0)
        assert float(((masked - pref[0, 0]).abs() > bound[0, 0]).float().mean()) > 0.9, what


def test_edge_dz_epilogue_against_its_fp64_restatement(cuda):
    """dY = addend + A W^T; d = dY * (fma(scale, ysel, shift) > 0 ? 1 : slope);
    word = (bits(d) & ~63) | slot; partials sum d and sum d (ysel - mean) invstd
    per tile — all exact on integer / dyadic data, 64- and 128-row tiles, both
    addend layouts; and cases whose d has low mantissa bits for the mask to
    clear, with the partials held to the unmasked sum."""
    cx = Ctx(cuda, 41)
    for M, N, K in itertools.product(R.EDZ_M, R.EDZ_N, R.EDZ_K):
        for lay in ("dense", "slice"):
            edz_case(cx, M, N, K, lay, 64)
    for (M, N, K), lay in itertools.product(R.EDZ_BIG, ("dense", "slice")):
        edz_case(cx, M, N, K, lay, 128)
    for M, N, positive in itertools.product((5, 8), (8, 72), (True, False)):
        edz_lowbits_case(cx, M, N, 64, positive)
    cx.done(2 * len(R.EDZ_M) * len(R.EDZ_N) * len(R.EDZ_K) + 4)


# ---- fp32 MFMA: dgx_gemm_f32 ---------------------------------------------------------

def f32_case(cx, aic, bic, form, M, N, K, la, lb, lc, random=False, splits=1, ld=None):
    dev = cx.dev
    ld = ld or lc
    what = f"gemm32 a_ic={aic} b_ic={bic} {form} M={M} N={N} K={K} splits={splits} A:{la} B:{lb} C:{lc} addend:{ld}"
    if random:
        a, b = torch.randn(M, K, generator=cx.g, device=dev), torch.randn(N, K, generator=cx.g, device=dev)
    else:
        a, b = R.lattice(cx.g, M, K, R.LIM, True, dev), R.lattice(cx.g, N, K, R.LIM, True, dev)
    add = None
    if form.startswith("accum"):
        add = torch.randn(M, N, generator=cx.g, device=dev) if random else R.lattice(cx.g, M, N, R.LIM, True, dev)
    mag = a.double().abs() @ b.double().abs().t()
    if random:
        ref = R.oracle(a, b) + (add.double() if add is not None else 0)
        bound = R.gamma(K, R.U32) * mag + (R.U32 * (add.double().abs() + mag) * (1 + R.gamma(K, R.U32))
                                            if add is not None else 0)
    else:
        ref = R.exact_or_raise(a, b, 64, add, what=what)
    A, B = operand(a, aic, F32, la), operand(b, bic, F32, lb)
    if form == "slab":
        S, kc = cx.L.dgx_gemm_f32_slabs(K, splits), R.split_kchunk(K, splits, 16)
        assert S == -(-K // kc) <= splits, what
        slab = Buf(S * M, N, dev, guard_rows=2 * M + 2)
        rc = cx.L.dgx_gemm_f32(vp(A.ptr()), aic, A.ld, vp(B.ptr()), bic, B.ld, M, N, K, SLAB, splits, vp(slab.ptr()),
                               N, None, 0, cx.st)
        rc2, C = slab_reduce(cx, slab, S, M, N)
        if random:
            cx.check(what, (rc or rc2) and f"rc {rc} {rc2}", slab.hit(), C.hit(),
                     R.bound_violation(C.view, ref, bound + R.gamma(S, R.U32) * mag, "f32", 64, 64))
        else:
            cx.check(what, (rc or rc2) and f"rc {rc} {rc2}", slab.hit(), C.hit(),
                     R.first_diff(slab.view.view(S, M, N), R.slab_refs(a, b, kc), "f32", 64, 64),
                     R.first_diff(C.view, ref, "f32", 64, 64))
        return
    C = out_buf(M, N, dev, lc, R.SENT if form == "accum_self" else R.GUARD)
    D = None
    if form == "accum_self":
        C.view.copy_(add)
    elif form == "accum_addend":
        D = Buf.of(add, ld, 4)
    rc = cx.L.dgx_gemm_f32(vp(A.ptr()), aic, A.ld, vp(B.ptr()), bic, B.ld, M, N, K, STORE if form == "store" else ACCUM,
                           1, vp(C.ptr()), C.ld, vp(D.ptr()) if D else None, D.ld if D else 0, cx.st)
    cx.check(what, rc and f"rc {rc}", C.hit(), D and D.hit(),
             R.bound_violation(C.view, ref, bound, "f32", 64, 64) if random else
             R.first_diff(C.view, ref, "f32", 64, 64))


@pytest.mark.parametrize("aic,bic", R.F32_LAYOUTS)
def test_gemm32_lattice_every_tile_edge(cuda, aic, bic):
    """All 12 gemm32_kernel instantiations (4 layouts x STORE / ACCUM / SLAB),
    ACCUM both as C += and as C = addend +, SLAB with forced splits, vector and
    scalar loads, at the edges of the 64 x 64 x 16 tile: exact."""
    cx = Ctx(cuda, 51 + 2 * aic + bic)
    for (M, N, K, form), (la, lb, lc, ld, kind) in R.f32_cases():
        splits = (1, 2, 3, -(-K // 16) + 1)[kind] if form == "slab" else 1
        f32_case(cx, aic, bic, form, M, N, K, la, lb, lc, splits=splits, ld=ld)
    cx.done(4 * len(R.F32_M) * len(R.F32_N) * len(R.F32_K))


def test_gemm32_random_within_the_fmaf_chain_bound(cuda):
    """u = 2^-24: gamma_K(2^-24) |a||b|^T per element (+ ACCUM rounding, + slab sum)."""
    cx = Ctx(cuda, 55)
    for (aic, bic), form in itertools.product(R.F32_LAYOUTS, R.F32_FORMS):
        la, lb, lc = cx.rot(R.LAYOUTS, R.LAYOUTS, R.LAYOUTS)
        f32_case(cx, aic, bic, form, 130, 65, 1000 if form == "slab" else 64, la, lb, lc, random=True,
                 splits=5 if form == "slab" else 1)
    cx.done(16)


# ---- small-K exact fp32: dgx_gemm_smallk_f32 / _split_f32 -------------------------------

def smallk_case(cx, M, N, K, ldx_kind, pad_c, split, x=None, w=None, want=None):
    dev = cx.dev
    what = f"smallk{'_split' if split else ''} M={M} N={N} K={K} ldx:{ldx_kind} ldc=N+{pad_c}"
    if x is None:
        x, w = R.lattice(cx.g, M, K, R.LIM, True, dev), R.lattice(cx.g, N, K, R.LIM, True, dev)
        want = R.exact_or_raise(x, w, 64, what=what)
    ld, c0 = {"K": (K, 0), "K+1": (K + 1, 0), "slice": (K + 24, 8)}[ldx_kind]
    X = Buf(M, K, dev, F32, R.NAN, ld, c0)
    X.view.copy_(x)
    C = Buf(M, N, dev, F32, R.GUARD, N + pad_c, 0)
    if split:     # the reference conv weight (Co, 2K) = [W1 | W2] of the stacked [W1; W2]
        co = N // 2
        W = Buf.of(torch.cat([w[:co], w[co:]], 1), "dense")
        rc = cx.L.dgx_gemm_smallk_split_f32(vp(X.ptr()), X.ld, vp(W.ptr()), M, co, K, vp(C.ptr()), C.ld, cx.st)
    else:
        W = Buf.of(w, "dense")
        rc = cx.L.dgx_gemm_smallk_f32(vp(X.ptr()), X.ld, vp(W.ptr()), M, N, K, vp(C.ptr()), C.ld, cx.st)
    cx.check(what, rc and f"rc {rc}", R.first_diff(C.view, want), C.hit())


def test_smallk_lattice_and_fmaf_chain(cuda):
    """Exact on the lattice at every M / N / K / ldx / ldc edge, plain and split
    weight; and for operands of <= 11 significant bits (exact fp32 products)
    bit-equal to a plain fp32 running sum over k computed on the CPU: the
    documented fmaf chain in k order."""
    cx = Ctx(cuda, 61)
    for M, (N, K) in itertools.product(R.SMALLK_M, R.SMALLK_NK):
        for split in (False, True):
            for ldx_kind, pad_c in itertools.product(("K", "K+1", "slice"), (0, 4)):
                smallk_case(cx, M, N, K, ldx_kind, pad_c, split)
    gc = torch.Generator().manual_seed(62)
    for M, (N, K) in itertools.product((17, 77), ((24, 3), (128, 9), (1008, 16), (8, 16))):
        x, w = R.bits11(gc, M, K), R.bits11(gc, N, K)
        want = R.smallk_chain(x, w).double().to(cuda)
        for split in (False, True):
            smallk_case(cx, M, N, K, "K+1", 4, split, x.to(cuda), w.to(cuda), want)
    cx.done(12 * len(R.SMALLK_M) * len(R.SMALLK_NK))


# ---- conversion kernels -----------------------------------------------------------------

def bits_diff(got, want):
    """first_diff on the raw bits (tells -0 from +0, compares inf)."""
    iv = torch.int16 if got.element_size() == 2 else torch.int32
    g, w = got.contiguous().view(iv), want.to(got.device).contiguous().view(iv)
    if torch.equal(g, w):
        return None
    at = tuple(int(v) for v in (g != w).nonzero()[0])
    return f"{int((g != w).sum())} differ, first at {at}: got {float(got[at])} ({int(g[at]):#x}), want " \
           f"{float(want[at])} ({int(w[at]):#x})"


def stacked_rows(w, C, stacked):
    return torch.cat([w[:, :C], w[:, C:]], 0) if stacked else w


def test_weight_prep_and_split_round_like_torch(cuda):
    """dgx_weight_prep_bf16, dgx_weight_prep_multi_bf16 (plain, stacked, split,
    transposed split), dgx_weight_stack_multi_f32 and dgx_split_bf16 on a plane
    of RNE ties, the largest finite fp32, a subnormal and +-0, around the
    32 x 32 tile: bit for bit torch's .to(bfloat16), outputs guarded."""
    cx = Ctx(cuda, 71)
    L = cx.L
    for Co, C in itertools.product(R.CONV_SIZES, R.CONV_SIZES):
        for stacked in (0, 1):
            w = R.conversion_plane(Co, C * (2 if stacked else 1))
            exp = stacked_rows(w, C, stacked)
            rows = exp.shape[0]
            W = Buf.of(w.to(cuda), "dense")
            nt, tn = Buf(rows, C, cuda, BF16), Buf(C, rows, cuda, BF16)
            rc = L.dgx_weight_prep_bf16(vp(W.ptr()), Co, C, stacked, vp(nt.ptr()), vp(tn.ptr()), cx.st)
            cx.check(f"weight_prep Co={Co} C={C} stacked={stacked}", rc and f"rc {rc}",
                     bits_diff(nt.view, exp.to(BF16)), bits_diff(tn.view, exp.to(BF16).t()), nt.hit(), tn.hit())
    # multi: up to 8 jobs per launch, flags bit 0 stacked, bit 1 split nt, bit 2 split tn
    shapes = [(Co, C, f) for (Co, C), f in zip(itertools.product(R.CONV_SIZES, R.CONV_SIZES),
                                               itertools.cycle((0, 1, 2, 3, 7, 6, 4, 5)))]
    for j0 in range(0, len(shapes), 8):
        jobs = shapes[j0:j0 + 8]
        n = len(jobs)
        ws, nts, tns, exps = [], [], [], []
        for Co, C, f in jobs:
            w = R.conversion_plane(Co, C * (2 if f & 1 else 1))
            exp = stacked_rows(w, C, f & 1)
            rows = exp.shape[0]
            ws.append(Buf.of(w.to(cuda), "dense"))
            nts.append(Buf(rows, 2 * C if f & 2 else C, cuda, BF16))
            tns.append(Buf(C, 2 * rows if f & 4 else rows, cuda, BF16))
            exps.append(exp)
        arr, ints = ctypes.c_void_p * n, ctypes.c_int * n
        rc = L.dgx_weight_prep_multi_bf16(n, arr(*[b.ptr() for b in ws]), ints(*[j[0] for j in jobs]),
                                          ints(*[j[1] for j in jobs]), ints(*[j[2] for j in jobs]),
                                          arr(*[b.ptr() for b in nts]), arr(*[b.ptr() for b in tns]), cx.st)
        for (Co, C, f), nt, tn, exp in zip(jobs, nts, tns, exps):
            hi = exp.to(BF16)
            lo = (exp - hi.float()).to(BF16)
            rows = exp.shape[0]
            cx.check(f"weight_prep_multi Co={Co} C={C} flags={f}", rc and f"rc {rc}", nt.hit(), tn.hit(),
                     bits_diff(nt.view[:, :C], hi), f & 2 and bits_diff(nt.view[:, C:], lo),
                     bits_diff(tn.view[:, :rows], hi.t()), f & 4 and bits_diff(tn.view[:, rows:], lo.t()))
    # fp32 stacking: a pure permutation
    jobs = list(itertools.product(R.CONV_SIZES, R.CONV_SIZES))
    for j0 in range(0, len(jobs), 8):
        js = jobs[j0:j0 + 8]
        n = len(js)
        ws = [Buf.of(R.conversion_plane(Co, 2 * C).to(cuda), "dense") for Co, C in js]
        outs = [Buf(2 * Co, C, cuda) for Co, C in js]
        arr, ints = ctypes.c_void_p * n, ctypes.c_int * n
        rc = L.dgx_weight_stack_multi_f32(n, arr(*[b.ptr() for b in ws]), ints(*[j[0] for j in js]),
                                          ints(*[j[1] for j in js]), arr(*[b.ptr() for b in outs]), cx.st)
        for (Co, C), w, o in zip(js, ws, outs):
            cx.check(f"weight_stack Co={Co} C={C}", rc and f"rc {rc}", o.hit(),
                     bits_diff(o.view, stacked_rows(w.view, C, 1)))
    # hi / lo planes; hi is optional
    for rows, cols in itertools.product(R.CONV_SIZES, (4, 28, 32, 36, 68)):
        for lay, with_hi in itertools.product(("dense", "slice"), (True, False)):
            src = R.conversion_plane(rows, cols)
            S = Buf.of(src.to(cuda), lay, 4)
            ld, c0, _ = R.layout_geometry(lay, cols, 4)
            hi, lo = Buf(rows, cols, cuda, BF16, R.GUARD, ld, c0), Buf(rows, cols, cuda, BF16, R.GUARD, ld, c0)
            rc = L.dgx_split_bf16(vp(S.ptr()), S.ld, rows, cols, vp(hi.ptr()) if with_hi else None, vp(lo.ptr()), ld,
                                  cx.st)
            h = src.to(BF16)
            cx.check(f"split_bf16 rows={rows} cols={cols} {lay} hi={with_hi}", rc and f"rc {rc}", hi.hit(), lo.hit(),
                     with_hi and bits_diff(hi.view, h), bits_diff(lo.view, (src - h.float()).to(BF16)),
                     not with_hi and not bool(torch.isnan(hi.view).all()) and "hi written though NULL")
    cx.done(150)


# ---- rejects ----------------------------------------------------------------------------

class Pool:
    """Valid device buffers of 64 Ki elements each, large enough for every
    shape the reject cases name; the outputs are NaN-filled and must stay so."""

    def __init__(self, dev):
        n = 1 << 16
        self.a16, self.b16 = (torch.ones(n, dtype=BF16, device=dev) for _ in range(2))
        self.a32, self.b32, self.add, self.ysel = (torch.ones(n, device=dev) for _ in range(4))
        self.vec = [torch.ones(256, device=dev) for _ in range(4)]
        self.arg = torch.zeros(n, dtype=torch.uint8, device=dev)
        self.C, self.part = Buf(0, 1, dev, guard_rows=n), Buf(0, 1, dev, guard_rows=n)

    def untouched(self):
        return self.C.hit() or self.part.hit()


def p(t, byte_off=0):
    return (t.flat if isinstance(t, Buf) else t).data_ptr() + byte_off


def expect(cx, P, what, rc, want):
    cx.check(what, rc != want and f"rc {rc}, want {want}", P.untouched())


def test_rejects_of_every_gemm_entry(cuda):
    """One call per documented DGX_EINVAL / DGX_EUNSUPPORTED condition of the six
    GEMM entries, every buffer valid and large enough, outputs untouched; empty
    outputs (M == 0, N == 0) return DGX_OK and write nothing."""
    cx = Ctx(cuda, 81)
    L, P, st = cx.L, Pool(cuda), cx.st
    EI, EU, OK = R.EINVAL, R.EUNSUPPORTED, R.OK

    # dgx_gemm_bf16(A, a_bf16, a_ic, lda, B, b_bf16, b_ic, ldb, M, N, K, epi, splits, C, ldc, partials, stream)
    def gb(want, note, A=p(P.a32), a16=0, aic=0, lda=64, B=p(P.b32), b16=0, bic=0, ldb=64, M=16, N=16, K=16, epi=STORE,
           splits=1, C=p(P.C), ldc=64, part=p(P.part)):
        expect(cx, P, f"dgx_gemm_bf16 {note}", L.dgx_gemm_bf16(vp(A), a16, aic, lda, vp(B), b16, bic, ldb, M, N, K,
                                                                epi, splits, vp(C), ldc, vp(part), st), want)
    for note, kw in (("A null", dict(A=0)), ("B null", dict(B=0)), ("C null", dict(C=0)), ("M < 0", dict(M=-1)),
                     ("N < 0", dict(N=-1)), ("K < 0", dict(K=-1)), ("lda < 1", dict(lda=0)), ("ldb < 1", dict(ldb=0)),
                     ("ldc < 1", dict(ldc=0)), ("splits < 1", dict(splits=0)),
                     ("STATS without partials", dict(epi=STATS, part=0))):
        gb(EI, note, **kw)
    gb(OK, "M == 0", M=0)
    gb(OK, "N == 0", N=0)
    for note, kw in (("bf16 B", dict(b16=1, B=p(P.b16))), ("X W^T accumulate", dict(epi=ACCUM)),
                     ("X W^T slab", dict(epi=SLAB)), ("X W^T bf16 A", dict(a16=1, A=p(P.a16))),
                     ("X W statistics", dict(bic=1, epi=STATS)), ("X W slab", dict(bic=1, epi=SLAB)),
                     ("A^T B^T", dict(aic=1, bic=0, epi=SLAB)), ("A^T B store", dict(aic=1, bic=1, epi=STORE)),
                     ("A^T B accumulate", dict(aic=1, bic=1, epi=ACCUM)), ("epi 4", dict(epi=STATS16)),
                     ("epi 9", dict(epi=9))):
        gb(EU, note, **kw)

    # dgx_gemm_lds_bf16(A, lda, B, ldb, tn, M, N, K, a_k, epi, splits, C, ldc, partials, addend, ldd, stream)
    def gl(want, note, A=p(P.a16), lda=256, B=p(P.b16), ldb=256, tn=0, M=16, N=16, K=64, ak=0, epi=STORE, splits=1,
           C=p(P.C), ldc=64, part=p(P.part), add=0, ldd=0):
        expect(cx, P, f"dgx_gemm_lds_bf16 {note}", L.dgx_gemm_lds_bf16(vp(A), lda, vp(B), ldb, tn, M, N, K, ak, epi,
                                                                        splits, vp(C), ldc, vp(part), vp(add), ldd, st),
               want)
        if want != OK and A and B and C and part:   # the query gives the launcher's code for every shape reject
            q = L.dgx_gemm_lds_tile(tn, M, N, K, ak, epi, splits)
            if A % 16 == 0 and B % 16 == 0 and lda % 8 == 0 and ldb % 8 == 0:
                cx.check(f"dgx_gemm_lds_tile {note}", q != want and f"query {q}, launcher {want}")
    for note, kw in (("A null", dict(A=0)), ("B null", dict(B=0)), ("C null", dict(C=0)), ("M < 0", dict(M=-1)),
                     ("N < 0", dict(N=-1)), ("K < 0", dict(K=-1)), ("splits < 1", dict(splits=0)),
                     ("STATS without partials", dict(epi=STATS, part=0)),
                     ("STATS16 without partials", dict(epi=STATS16, part=0))):
        gl(EI, note, **kw)
    gl(OK, "M == 0", M=0)
    gl(OK, "N == 0", N=0)
    gl(OK, "tn M == 0", tn=1, M=0, epi=SLAB)
    for note, kw in (("a_k with tn", dict(tn=1, K=128, ak=64, epi=SLAB)), ("a_k < 64", dict(K=128, ak=32)),
                     ("a_k % 64", dict(K=192, ak=96)), ("K % a_k", dict(K=192, ak=128)),
                     ("A misaligned", dict(A=p(P.a16, 2))), ("B misaligned", dict(B=p(P.b16, 8))),
                     ("lda % 8", dict(lda=260)), ("ldb % 8", dict(ldb=68)), ("tn M < 8", dict(tn=1, M=4, epi=SLAB)),
                     ("tn N < 8", dict(tn=1, N=4, epi=SLAB)), ("tn M % 8", dict(tn=1, M=20, epi=SLAB)),
                     ("tn N % 8", dict(tn=1, N=20, epi=SLAB)), ("tn store", dict(tn=1, epi=STORE)),
                     ("K % 64", dict(K=96)), ("nt slab", dict(epi=SLAB)), ("epi 5", dict(epi=5)),
                     ("epi 6", dict(epi=6)), ("epi 7", dict(epi=7))):
        gl(EU, note, **kw)

    # dgx_gemm_edge_dz_bf16(A, lda, W, ldw, M, N, K, addend, ldd, ysel, arg, scale, shift, mean, invstd, slope,
    #                       dz, partials, nrows, stream)
    def ge(want, note, A=p(P.a16), lda=256, W=p(P.b16), ldw=256, M=16, N=16, K=64, add=p(P.add), ldd=160,
           ysel=p(P.ysel), arg=p(P.arg), sc=p(P.vec[0]), sh=p(P.vec[1]), me=p(P.vec[2]), iv=p(P.vec[3]), dz=p(P.C),
           part=p(P.part), nrows=None):
        nrows = L.dgx_gemm_edge_dz_rows(M, N) if nrows is None else nrows
        expect(cx, P, f"dgx_gemm_edge_dz_bf16 {note}",
               L.dgx_gemm_edge_dz_bf16(vp(A), lda, vp(W), ldw, M, N, K, vp(add), ldd, vp(ysel), vp(arg), vp(sc), vp(sh),
                                       vp(me), vp(iv), 0.25, vp(dz), vp(part), nrows, st), want)
    for name in ("A", "W", "add", "ysel", "arg", "sc", "sh", "me", "iv", "dz", "part"):
        ge(EI, f"{name} null", **{name: 0})
    for note, kw in (("M < 1", dict(M=0, nrows=1)), ("N < 1", dict(N=0, nrows=1)), ("K < 1", dict(K=-64)),
                     ("nrows wrong", dict(nrows=2))):
        ge(EI, note, **kw)
    assert L.dgx_gemm_edge_dz_rows(0, 16) == EI and L.dgx_gemm_edge_dz_rows(16, 0) == EI
    for note, kw in (("N % 8", dict(N=20)), ("N > 128", dict(N=136)), ("K % 64", dict(K=96)), ("ldd % 4", dict(ldd=162)),
                     ("A misaligned", dict(A=p(P.a16, 8))), ("W misaligned", dict(W=p(P.b16, 2))),
                     ("lda % 8", dict(lda=260)), ("ldw % 8", dict(ldw=68)), ("addend misaligned", dict(add=p(P.add, 4))),
                     ("ysel misaligned", dict(ysel=p(P.ysel, 8))), ("arg misaligned", dict(arg=p(P.arg, 2))),
                     ("dz misaligned", dict(dz=p(P.C, 4))), ("scale misaligned", dict(sc=p(P.vec[0], 4))),
                     ("shift misaligned", dict(sh=p(P.vec[1], 8))), ("mean misaligned", dict(me=p(P.vec[2], 4))),
                     ("invstd misaligned", dict(iv=p(P.vec[3], 12)))):
        ge(EU, note, **kw)

    # dgx_gemm_smallk_f32(X, ldx, W, M, N, K, C, ldc, stream) and the split form (Co = N / 2)
    for split in (0, 1):
        def gs(want, note, X=p(P.a32), ldx=32, W=p(P.b32), M=16, N=16, K=8, C=p(P.C), ldc=1024):
            fn = L.dgx_gemm_smallk_split_f32 if split else L.dgx_gemm_smallk_f32
            expect(cx, P, f"{'dgx_gemm_smallk_split_f32' if split else 'dgx_gemm_smallk_f32'} {note}",
                   fn(vp(X), ldx, vp(W), M, N // 2 if split else N, K, vp(C), ldc, st), want)
        for note, kw in (("X null", dict(X=0)), ("W null", dict(W=0)), ("C null", dict(C=0)), ("M < 1", dict(M=0)),
                         ("N < 4 / Co < 2", dict(N=2)), ("K < 1", dict(K=-1)), ("ldx < K", dict(ldx=4)),
                         ("ldc < N", dict(ldc=12))):
            gs(EI, note, **kw)
        for note, kw in (("K > 16", dict(K=17)), ("N % 4", dict(N=18)), ("ldc % 4", dict(ldc=1026)),
                         ("C misaligned", dict(C=p(P.C, 4))), ("W and X past 64 KiB of LDS", dict(N=1012, K=16))):
            gs(EU, note, **kw)

    # dgx_gemm_f32(A, a_ic, lda, B, b_ic, ldb, M, N, K, epi, splits, C, ldc, addend, ldd, stream)
    def gf(want, note, A=p(P.a32), aic=0, lda=64, B=p(P.b32), bic=0, ldb=64, M=16, N=16, K=64, epi=STORE, splits=1,
           C=p(P.C), ldc=64, add=0, ldd=0):
        expect(cx, P, f"dgx_gemm_f32 {note}", L.dgx_gemm_f32(vp(A), aic, lda, vp(B), bic, ldb, M, N, K, epi, splits,
                                                              vp(C), ldc, vp(add), ldd, st), want)
    for note, kw in (("A null", dict(A=0)), ("B null", dict(B=0)), ("C null", dict(C=0)), ("M < 0", dict(M=-1)),
                     ("N < 0", dict(N=-1)), ("K < 0", dict(K=-1)), ("lda < 1", dict(lda=0)), ("ldb < 1", dict(ldb=0)),
                     ("splits < 1", dict(splits=0)), ("epi 2", dict(epi=STATS)), ("epi 4", dict(epi=STATS16)),
                     ("ldc < N", dict(ldc=8)), ("store with 2 slabs", dict(splits=2)),
                     ("accumulate with 2 slabs", dict(epi=ACCUM, splits=2))):
        gf(EI, note, **kw)
    gf(OK, "M == 0", M=0)
    gf(OK, "N == 0", N=0)
    cx.done(100)
