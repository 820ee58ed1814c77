"""CPU checks of tests/_gemm_ref.py: the lattice really is exact, the rounding
probe really tells the rounding modes apart, the guards really notice, and the
grids really reach every instantiation — by the library's own host queries
(dgx_gemm_lds_tile, dgx_gemm_edge_dz_rows, dgx_gemm*_slabs), not a restatement."""
import pytest
import torch

import _gemm_ref as R


def _lib():
    from dgx import _native
    return _native.lib()


def test_lattice_is_bf16_exact_and_condition_holds_with_room():
    g = torch.Generator().manual_seed(0)
    for lim, frac in ((R.LIM, True), (R.LIM, False), (R.LIM_STATS, False)):
        v = R.lattice(g, 300, 1024, lim, frac)
        assert torch.equal(R.bf16_round(v), v)
        assert float(v.abs().max()) <= (4.0 if frac else lim)
        assert bool((v * 8 == (v * 8).round()).all())
    a = R.lattice(g, 257, 1024, R.LIM_STATS)
    b = R.lattice(g, 200, 1024, R.LIM_STATS)
    ref = R.exact_or_raise(a, b, 1, stats_rows=128, what="K=1024 statistics")
    assert float((a.abs() @ b.abs().t()).max()) < 2 ** 13       # orders of magnitude of room
    assert float(R.stats_ref(ref)[:, 1].max()) < 2 ** 21
    # the exact result survives ANY summation order: fp32 sums over shuffled k agree bit for bit
    perm = torch.randperm(1024, generator=g)
    for order in (torch.arange(1024), perm, perm.flip(0)):
        acc = torch.zeros(257, 200)
        for k0 in range(0, 1024, 64):
            ks = order[k0:k0 + 64]
            acc = acc + a[:, ks] @ b[:, ks].t()
        assert torch.equal(acc.double(), ref)


def test_exactness_assertion_can_fail():
    a = torch.full((2, 70000), 4.0)
    with pytest.raises(AssertionError, match="not exact"):
        R.exact_or_raise(a, a, 64)
    z = torch.full((128, 1), 400.0)
    with pytest.raises(AssertionError, match="statistics"):
        R.exact_or_raise(z, torch.ones(1, 1), 1, stats_rows=128)
    with pytest.raises(AssertionError, match="multiples"):
        R.exact_or_raise(torch.full((1, 1), 0.125), torch.full((1, 1), 0.125), 1)


def test_rounding_probe_separates_rne_from_truncation_and_half_up():
    p, e = R.probe_case()
    rne = p.to(torch.bfloat16).float()
    assert rne[:, 0].tolist() == R.PROBE_BF16
    assert sorted(set(rne.flatten().tolist())) == sorted(set(R.PROBE_BF16))
    bits = p.view(torch.int32)
    trunc = (bits & ~0xFFFF).view(torch.float32)
    half_up = ((bits + 0x8000) & ~0xFFFF).view(torch.float32)
    want = R.oracle(rne, e)
    assert not torch.equal(R.oracle(trunc, e), want)
    assert not torch.equal(R.oracle(half_up, e), want)
    assert torch.equal(want.float().double(), want)             # exact in fp32
    # each of the three modes differs from the other two on some single entry
    assert bool((trunc != rne).any()) and bool((half_up != rne).any()) and bool((half_up != trunc).any())


def test_gamma_bounds():
    assert R.gamma(1024, R.U_MFMA16) == pytest.approx(1024 * 2.0 ** -23, rel=1e-3)
    assert R.gamma(16, R.U32) < R.gamma(16, R.U_MFMA16) < 2e-6


def test_buf_guards_notice_every_kind_of_stray_write():
    for dtype in (torch.float32, torch.bfloat16):
        vec = 8 if dtype == torch.bfloat16 else 4
        for fill in (R.GUARD, R.NAN, R.SENT):
            for layout in (R.LAYOUTS if dtype == torch.bfloat16 else R.OUT_LAYOUTS):
                v = torch.arange(15, dtype=torch.float32).view(3, 5).to(dtype)
                b = R.Buf.of(v, layout, vec=vec, fill=fill)
                ld, c0, off = R.layout_geometry(layout, 5, vec)
                assert (b.ld, b.c0, b.off) == (ld, c0, off) and torch.equal(b.view, v)
                assert b.ptr() == b.flat.data_ptr() + (off + c0) * b.flat.element_size()
                assert b.hit() is None
                b.view.fill_(1.0)                     # writes inside the view are not hits
                assert b.hit() is None
                clean = b.flat.clone()

                def stray(t, idx, value, where):
                    t[idx] = value
                    assert where in b.hit(), (layout, fill, where)
                    b.flat.copy_(clean)
                    assert b.hit() is None

                stray(b.full, (3, c0), 1.0, "guard row")
                if ld > c0 + 5:
                    stray(b.full, (1, c0 + 5), 2.0, "right of the view")
                if c0:
                    stray(b.full, (2, c0 - 1), 2.0, "left of the view")
                if off:
                    stray(b.flat, 0, 0.0, "front")
                if fill is R.GUARD:   # what a store of a value computed from an over-read operand NaN leaves
                    assert bool(torch.isnan(b.flat[-1]))
                    stray(b.full, (4, 0), R.NAN, "guard row")
    z = R.Buf(0, 4, "cpu", guard_rows=2)
    assert z.hit() is None


def test_layouts_are_vector_or_scalar_as_named():
    for vec in (4, 8):
        for cols in (1, 3, 64, 65, 200):
            ld, c0, off = R.layout_geometry("slice", cols, vec)
            assert ld % vec == 0 and c0 % vec == 0 and off == 0 and ld >= c0 + cols
            ld, c0, off = R.layout_geometry("odd", cols, vec)
            assert ld % 2 == 1 and (c0 + off) % 4 != 0 and ld >= c0 + cols
    for cols in (1, 3, 8, 63, 64, 65, 200, 256):          # fp32: one half of `odd` at a time
        ld, c0, off = R.layout_geometry("ldodd", cols, 4)
        assert ld % 4 != 0 and c0 == 0 and off == 0 and ld >= cols
        ld, c0, off = R.layout_geometry("baseoff", cols, 4)
        assert ld % 4 == 0 and (c0 + off) % 4 != 0 and ld >= c0 + cols


def test_every_layout_meets_every_value_of_every_axis():
    """The rotated grids of the GPU file: each layout of each buffer (and each
    split kind / ACCUM form that rotates with them) meets each value of each
    axis, both split-weight settings and both operand layouts included; the
    crossed grids hold the full product."""
    for name, (cases, picks) in R.ROTATED.items():
        cs = cases()
        assert R.uncovered(cs, picks) == [], name
        assert len({vals for vals, _ in cs}) == len(cs), name
    c64 = {vals for vals, _ in R.lds64_cases()}
    assert len(c64) == len(R.LDS64_M) * len(R.LDS64_N) * len(R.LDS64_K) * 2 * 2 * 5
    for split in (False, True):
        for lo in R.OPS16:
            for lc in R.OUT_LAYOUTS:
                assert (65, 63, 192, split, lo, lc) in c64
    st = {vals for vals, _ in R.lds_stats_cases()}
    assert len(st) == len(R.LDS_STATS_M) * len(R.LDS_STATS_N) * len(R.LDS_STATS_K) * 2 * 3
    # a rotation can fail the check: tied to the innermost axis it leaves holes
    bad = R.rotate((R.REG_M, R.REG_N, R.REG_K), [(R.LAYOUTS, (0, 0, 1))])
    assert R.uncovered(bad, [(R.LAYOUTS, (0, 0, 1))])


def test_first_diff_and_bound_report_and_exclude_nothing():
    a = torch.zeros(300, 200)
    assert R.first_diff(a, a.double()) is None
    b = a.clone()
    b[257, 130] = 1.0
    msg = R.first_diff(b, a.double(), "lds", 128, 128)
    assert "(257, 130)" in msg and "tile (2, 1)" in msg and "in-tile (1, 2)" in msg and "wave 0" in msg
    assert "wave 3" in R.where_in_tile(70, 70, "lds", 128, 128) and "wave 2" in R.where_in_tile(70, 3, "lds", 128, 64)
    b[257, 130] = R.NAN
    assert "(257, 130)" in R.first_diff(b, a.double())
    assert "(257, 130)" in R.bound_violation(b, a.double(), torch.ones(300, 200, dtype=torch.float64))
    assert R.bound_violation(a + 0.5, a.double(), torch.ones(300, 200, dtype=torch.float64)) is None
    assert "wave 5" in R.where_in_tile(130, 70, "g256", 256, 256) and "round 2" in R.where_in_tile(130, 70, "g256", 256, 256)
    assert "round 1" in R.where_in_tile(100, 3, "lds", 128, 128) and "round 0" in R.where_in_tile(100, 3, "lds", 128, 64)


def test_one_hot_names_the_source_element():
    g = torch.Generator().manual_seed(1)
    a, k = R.one_hot_rows(g, 9, 70)
    b = R.lattice(g, 5, 70)
    assert torch.equal(R.oracle(a, b), b[:, k].t().double())


def test_lds_tile_query_follows_the_documented_rule_at_its_edges():
    L = _lib()
    for M, N, bm in R.LDS_SKINNY_EDGE:
        bn = 128 if N > 64 else 64
        assert L.dgx_gemm_lds_tile(0, M, N, 64, 0, R.STORE, 1) == bm * 1000 + bn
        assert L.dgx_gemm_lds_tile(0, M, N, 64, 0, R.STATS, 1) == 128 * 1000 + bn   # statistics: always 128 rows
    assert L.dgx_gemm_lds_tile(0, 65281, 256, 64, 0, R.STORE, 1) == 256256
    assert L.dgx_gemm_lds_tile(0, 65280, 256, 64, 0, R.STORE, 1) == 128128          # 255 tiles only
    assert L.dgx_gemm_lds_tile(0, 65281, 256, 128, 64, R.STATS16, 1) == 256256
    assert L.dgx_gemm_lds_tile(0, 65281, 384, 64, 0, R.STORE, 1) == 128128          # N % 256
    assert L.dgx_gemm_lds_tile(0, 0, 8, 64, 0, R.STORE, 1) == 0
    # rejects, in the launcher's order
    assert L.dgx_gemm_lds_tile(0, -1, 8, 64, 0, R.STORE, 1) == R.EINVAL
    assert L.dgx_gemm_lds_tile(0, 8, 8, 64, 0, R.STORE, 0) == R.EINVAL
    assert L.dgx_gemm_lds_tile(0, 8, 8, 100, 0, R.STORE, 1) == R.EUNSUPPORTED       # K % 64
    assert L.dgx_gemm_lds_tile(0, 8, 8, 64, 0, R.SLAB, 1) == R.EUNSUPPORTED
    assert L.dgx_gemm_lds_tile(0, 8, 8, 64, 0, 5, 1) == R.EUNSUPPORTED
    assert L.dgx_gemm_lds_tile(0, 8, 8, 128, 32, R.STORE, 1) == R.EUNSUPPORTED      # a_k < 64
    assert L.dgx_gemm_lds_tile(0, 8, 8, 192, 128, R.STORE, 1) == R.EUNSUPPORTED     # K % a_k
    assert L.dgx_gemm_lds_tile(1, 8, 8, 128, 64, R.SLAB, 1) == R.EUNSUPPORTED       # a_k with tn
    assert L.dgx_gemm_lds_tile(1, 12, 8, 64, 0, R.SLAB, 1) == R.EUNSUPPORTED        # M % 8
    assert L.dgx_gemm_lds_tile(1, 8, 4, 64, 0, R.SLAB, 1) == R.EUNSUPPORTED
    assert L.dgx_gemm_lds_tile(1, 8, 8, 64, 0, R.STORE, 1) == R.EUNSUPPORTED
    # the TN choice counts the slabs the launch really writes
    assert L.dgx_gemm_lds_tile(1, 136, 72, 16363, 0, R.SLAB, 256) == 128128 and L.dgx_gemm_lds_slabs(16363, 256) == 256
    assert L.dgx_gemm_lds_tile(1, 136, 72, 16421, 0, R.SLAB, 256) == 64128 and L.dgx_gemm_lds_slabs(16421, 256) == 129
    # the edge-dz launcher shares the rule
    for M, N in ((65408, 64), (65409, 64), (65409, 128), (129, 72)):
        assert R.edz_bm(L, M, N) == L.dgx_gemm_lds_tile(0, M, N, 64, 0, R.STORE, 1) // 1000


def test_grids_reach_every_instantiation():
    L = _lib()
    assert R.lds_tile_sets(L) == R.LDS_TILES_EMITTED
    # dgx_gemm_bf16's layout table (gemm.hip, "the operand layouts the engine uses"), plus atb_small
    assert {(a, ai, bi, e) for _, a, ai, bi, e in R.REG_ARMS} == {
        (0, 0, 0, R.STORE), (0, 0, 0, R.STATS), (0, 0, 1, R.ACCUM), (0, 0, 1, R.STORE), (1, 0, 1, R.ACCUM),
        (1, 0, 1, R.STORE), (1, 1, 1, R.SLAB), (0, 1, 1, R.SLAB)}
    assert max(R.ATB_SMALL_N) == 4 and min(R.REG_N) <= 64 < max(R.REG_N)             # both BN of the register path
    # gemm32: the launcher switches on (a_ic, b_ic) and on epi in {STORE, ACCUM, SLAB}; the grid lists all of both
    assert set(R.F32_LAYOUTS) == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert set(R.F32_FORMS) == {"store", "accum_self", "accum_addend", "slab"}
    # row-tile counts and grid sizes, from the library's own tile (LDS path) or partial-row count (register path)
    def lds_grids(tn, ms, ns, k, epi):
        out = set()
        for m in ms:
            for n in ns:
                t = L.dgx_gemm_lds_tile(tn, m, n, k, 0, epi, 1)
                assert t > 0
                ni = -(-m // (t // 1000))
                out.add((ni, ni * -(-n // (t % 1000))))
        return out
    families = {"reg": {(L.dgx_gemm_stats_rows(m), None) for m in R.REG_M},
                "lds64": lds_grids(0, R.LDS64_M, R.LDS64_N, 64, R.STORE),
                "stats": lds_grids(0, R.LDS_STATS_M, R.LDS_STATS_N, 64, R.STATS),
                "tn": lds_grids(1, R.TN_M, R.TN_N, 64, R.SLAB)}
    for name, got in families.items():
        nis = {ni for ni, _ in got}
        assert any(ni % 2 for ni in nis if ni > 1) and any(ni % 2 == 0 for ni in nis), (name, nis)
        if name != "reg":
            assert any(gs % 8 for _, gs in got), name
        if name in ("lds64", "stats"):                  # and one that wraps round the 8 XCDs
            assert any(gs % 8 and gs > 8 for _, gs in got), name
    for mn, k, epi in ((R.LDS128_MN, 64, R.STORE), (R.G256_MN, 64, R.STORE)):
        big = set().union(*[lds_grids(0, [m], [n], k, epi) for m, n in mn])
        assert any(gs % 8 for _, gs in big) and any(gs % 8 == 0 for _, gs in big)
    # nk of the 256 x 256 kernel's rings: prologue only, wrap-around of the B ring, of the A ring, and a long loop
    assert {k // 64 for k in R.G256_K} >= {1, 2, 3, 7}
    assert {(kw // 64, ak // 64) for kw, ak in R.G256_SPLIT} == {(2, 1), (6, 3)}
    # last 256-row tile holds 1, 128, 129, 255 and 256 rows
    assert [m - (-(-m // 256) - 1) * 256 for m, n in R.G256_MN if n == 256][:5] == [1, 128, 129, 255, 256]
    # split-K: forced split lists reach one slab, fewer slabs than asked, and more splits than K-steps
    for Rr in R.REG_SLAB_R:
        used = {L.dgx_gemm_slabs(Rr, s) for s in R.reg_slab_splits(Rr)}
        assert 1 in used and max(used) == -(-Rr // 32)
    for Rr in R.TN_R:
        used = {L.dgx_gemm_lds_slabs(Rr, s) for s in R.tn_splits(Rr)}
        assert 1 in used and max(used) == -(-Rr // 64)
    # smallk: 1008 x 16 is the largest N the 64 KiB check admits at K = 16
    assert (1008 + 16) * 16 * 4 <= 64 * 1024 < (1012 + 16) * 16 * 4


def test_edz_ref_by_hand():
    a = torch.tensor([[1.0, 2.0]])
    w = torch.tensor([[3.0, -1.0], [0.0, 1.0]])
    add = torch.tensor([[1.0, -5.0]])
    ysel = torch.tensor([[2.0, 0.0]])
    arg = torch.tensor([[7, 63]], dtype=torch.uint8)
    words, part, mag = R.edz_ref(a, w, add, ysel, arg, torch.tensor([1.0, 1.0]), torch.tensor([0.0, 0.0]),
                                 torch.tensor([1.0, 1.0]), torch.tensor([0.5, 2.0]), 0.25, 64)
    # dY = [1 + 1, -5 + 2] = [2, -3]; z = [2, 0]: z = 0 takes the slope side; d = [2, -0.75]
    d = torch.tensor([2.0, -0.75])
    assert words.tolist() == [[int(d.view(torch.int32)[0]) | 7, int(d.view(torch.int32)[1]) | 63]]
    assert part[0, 0].tolist() == [2.0, -0.75] and part[0, 1].tolist() == [2.0 * 0.5, -0.75 * -2.0]
    assert mag == 2.0


def test_smallk_chain_is_the_fmaf_chain_for_11_bit_operands():
    g = torch.Generator().manual_seed(3)
    x, w = R.bits11(g, 40, 16), R.bits11(g, 24, 16)
    assert torch.equal((x[:, None, :] * w[None, :, :]).double(), x.double()[:, None, :] * w.double()[None, :, :])
    got = R.smallk_chain(x, w)
    ref = R.oracle(x, w)
    assert R.bound_violation(got, ref, R.gamma(16, R.U32) * (x.abs().double() @ w.abs().double().t())) is None


def test_conversion_plane_holds_the_crafted_values():
    p = R.conversion_plane(65, 33)
    b = p.to(torch.bfloat16)
    assert bool(torch.isinf(b).any()) and bool(torch.isfinite(p).all())
    assert bool(((p != 0) & (p.abs() < 2.0 ** -126)).any())            # a subnormal
    assert bool((p.view(torch.int32) == -2 ** 31).any())                # -0
    for v in R.PROBE:
        assert bool((p == v).any())
