"""The backward-scatter oracle (tests/_scatter_ref.py) checked on the CPU: the
lattice bound and its ties, the restatements against brute-force loops on tiny
graphs, and — with the library loaded — every table entry's stated launch form
against dgx_edge_bwd_scatter_geometry, the launcher's own rules, and the
table's cover of every reachable launch form."""
import ctypes

import pytest
import torch

import _scatter_ref as R


def _lib():
    from dgx import _native
    return _native.lib()


def _geometry(B, N, Co, packed):
    """(rc, cs, parts, tpp, lds) from the library"""
    cs, parts, tpp, lds = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int64(-1)
    rc = _lib().dgx_edge_bwd_scatter_geometry(B, N, Co, int(packed), ctypes.byref(cs), ctypes.byref(parts),
                                              ctypes.byref(tpp), ctypes.byref(lds))
    return rc, cs.value, parts.value, tpp.value, lds.value


TINY = [("random", 2, 7, 3, 5), ("dups", 1, 9, 4, 3), ("all0", 2, 5, 2, 1), ("hubs", 1, 40, 6, 2)]


@pytest.mark.parametrize("kind,B,N,k,Co", TINY)
def test_reverse_graph_and_refs_equal_brute_force(kind, B, N, k, Co):
    idx = R.make_idx(kind, B, N, k, seed=1)
    c = R.make_lattice(B, N, k, Co, idx, ldpq=2 * Co + 1, seed=2)
    rowptr, edges = R.reverse_graph_brute(idx, B, N, k)
    assert torch.equal(c.rowptr, rowptr) and torch.equal(c.edges, edges)
    for packed in (False, True):
        assert torch.equal(R.ref64(c, packed), R.ref_brute(c, packed))
    r = R.make_random(B, N, k, Co, idx, seed=3)
    for packed in (False, True):
        assert float((R.ref64(r, packed) - R.ref_brute(r, packed)).abs().max()) < 1e-12
        for tpp in (1, 2, 4):
            got, want = R.ordered_sums(r, packed, tpp), R.ordered_brute(r, packed, tpp)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    # the order matters on random data (else the GPU's order test would pin nothing) ...
    big = R.make_random(1, 64, 8, 4, R.make_idx("all0", 1, 64, 8), seed=4)
    s1, s4 = R.ordered_sums(big, False, 1), R.ordered_sums(big, False, 4)
    assert not torch.equal(s1[1], s4[1])
    # ... and not on the lattice: any order gives the fp64 sums exactly
    for tpp in (1, 2, 4):
        sd, sq = R.ordered_sums(c, False, tpp)
        deg = R.in_degrees(c).float().unsqueeze(1)
        P = c.PQ[:, :Co]
        dP = c.a * sd + c.c0 * deg + c.c1 * (deg * P + sq)          # fp32 throughout
        assert torch.equal(dP.double(), R.ref64(c)[:, :Co])


def test_duplicate_neighbours_carry_dz_on_the_selected_slot_only():
    """Point 0 lists point 1 three times; arg picks slot 1: point 1 gets dz once, and Q three times."""
    idx = torch.tensor([[[1, 1, 1], [0, 0, 0]]])
    c = R.make_lattice(1, 2, 3, 1, idx, arg=torch.tensor([[1], [2]], dtype=torch.uint8))
    a, c0, c1 = (float(x[0]) for x in (c.a, c.c0, c.c1))
    P, Q, dz = c.PQ[:, 0].double(), c.PQ[:, 1].double(), c.dz[:, 0].double()
    want = a * dz[0] + 3 * c0 + c1 * (3 * P[1] + 3 * Q[0])
    assert float(R.ref64(c)[1, 0]) == float(want)


def test_lattice_bound_and_ties():
    idx = R.make_idx("random", 1, 200, 4)
    c = R.make_lattice(1, 200, 4, 8, idx)
    ref = R.ref64(c)
    assert float(ref.abs().max()) <= c.bound < R.LIM
    assert bool(((2 * ref) == (2 * ref).round()).all())
    R.exact_f32(ref)
    dQ = ref[:, 8:]
    for v in (257., 259., 385., 387., 256., 258., 256.5, 257.5):
        assert bool((dQ == v).any()), v
    # ties round to even, their neighbours to nearest: truncation would give 256, 258, 384, 386 / 256, 256
    t = torch.tensor([257., 259., 385., 387., 256.5, 257.5])
    assert R.expected_planes(t, 1)[0].float().tolist() == [256., 260., 384., 388., 256., 258.]
    hi, lo, third = R.expected_planes(t, 2)
    assert third is None and (hi.float() + lo.float()).tolist() == t.tolist()
    # the largest graphs of the GPU file: every edge on one point, and the ladder's hub
    for kind, N in (("all0", 9217), ("ladder", 200)):
        h = R.make_lattice(1, N, 4, 8, R.make_idx(kind, 1, N, 4))
        assert h.maxdeg == (4 * N if kind == "all0" else 4 * N - sum(R.LADDER)) and h.bound < R.LIM
    assert sorted(R.in_degrees(h)[1:12].tolist()) == sorted(R.LADDER)
    # the bound trips: the same graph with values 2^12 times larger
    big = R.make_lattice(1, 9217, 4, 8, R.make_idx("all0", 1, 9217, 4))
    big.dz = big.dz * 4096
    assert R.lattice_bound(big) >= R.LIM


def test_finalize_reference_is_exact():
    for cs in (8, 4, 2, 1):
        for nrows in R.fin_nrows(cs):
            part, count, mean, invstd = R.make_finalize(20, nrows)
            a = torch.tensor([R.TRIPLES[o % 9][0] for o in range(20)], dtype=torch.float32)
            dgamma, dbeta, c0, c1 = R.finalize_ref(part, count, a, mean, invstd, False)
            assert torch.equal(dbeta, part[:, 0].sum(0)) and torch.equal(dgamma, part[:, 1].sum(0))
            z = R.finalize_ref(part, count, a, mean, invstd, True)
            assert not bool(z[2].any()) and not bool(z[3].any()) and torch.equal(z[0], dgamma)
    assert [R.fin_nrows(cs)[2] for cs in (8, 4, 2, 1)] == [64, 128, 256, 512]


def test_table_entries_hit_their_launch_forms():
    """every stated (cs, tpp) is the library's answer, and the restated rule agrees in full"""
    entries = R.all_table_entries()
    assert len(entries) > 40
    for (B, N, k, Co), packed, (cs, tpp) in entries:
        rc, qcs, qparts, qtpp, lds = _geometry(B, N, Co, packed)
        assert rc == 0 and (qcs, qtpp) == (cs, tpp), (B, N, Co, packed, qcs, qtpp)
        assert R.form_of(B, N, Co, packed) == (qcs, qparts, qtpp)
        assert 0 < lds <= 160 * 1024
    for (B, N, k, Co), packed, (cs, tpp), passes, last in R.PASSES:
        _, _, parts, qtpp, _ = _geometry(B, N, Co, packed)
        ppb = R.EC_THREADS // qtpp
        assert parts == 1 and -(-N // ppb) == passes and N - (passes - 1) * ppb == last
    # a partly filled reversed (odd) pass, two full passes, and a partly filled third, with and without lanes
    assert {(pk, p, last == R.EC_THREADS // t[1]) for _, pk, t, p, last in R.PASSES} == {
        (False, 2, False), (False, 2, True), (False, 3, False), (True, 2, False), (True, 2, True), (True, 3, False)}


def test_table_covers_every_reachable_form():
    """36 launch forms: (slices, cs, tpp) x output mode; a form that loses its case fails here"""
    have = {(packed, cs, tpp) for _, packed, (cs, tpp) in R.FORMS.values()}
    assert have == set(R.REACHABLE) and len(R.FORMS) == len(R.REACHABLE) == 9
    assert len({(f, m) for f in have for m in R.MODES}) == 36
    # nothing else is reachable: every (B, N, Co) of a wide sweep lands in REACHABLE
    seen = set()
    for packed in (False, True):
        for B in (1, 2, 16, 64):
            for Co in (1, 8, 64):
                for N in list(range(1, 1300, 37)) + [2048, 2305, 4097, 4609, 9217, 17000]:
                    rc, cs, parts, tpp, _ = _geometry(B, N, Co, packed)
                    assert rc == 0
                    seen.add((packed, cs, tpp))
    assert seen == set(R.REACHABLE)
    # the finalize table reaches every CS in both dz forms
    assert {(R.FORMS[n][1], R.FORMS[n][2][0]) for n, _ in R.FIN_FORMS} == {(pk, cs) for pk in (False, True)
                                                                          for cs in (8, 4, 2, 1)}
    assert all(R.FORMS[n][2][0] == cs for n, cs in R.FIN_FORMS)


def test_boundaries_change_what_they_claim():
    b = R.BOUNDARIES
    for lo, hi in zip(b[0::2], b[1::2]):
        (B, N0, _, Co), pk, f0 = lo
        (_, N1, _, _), _, f1 = hi
        g0, g1 = _geometry(B, N0, Co, pk), _geometry(B, N1, Co, pk)
        if N0 in (8192, 9216):   # the last N whose one-channel slices fit 72 KiB | the 160 KiB mode
            assert N1 == N0 + 1 and (8 if pk else 9) * N0 == 72 * 1024 and g0[1] == g1[1] == 1
        elif N0 == 512:          # 128 | 129 points per part
            assert (-(-N0 // g0[2]), -(-N1 // g1[2])) == (128, 129) and (g0[3], g1[3]) == (4, 2)
        else:
            assert N1 == N0 + 1 and g0[1] == 2 * g1[1]
    # the parts * 64 < N rule around N = 64
    assert [_geometry(1, N, 8, 0)[2] for N in (1, 2, 63, 64, 65)] == [1, 1, 1, 1, 2]
    for B in R.XCD_BS:
        for pk in (False, True):
            rc, cs, parts, tpp, _ = _geometry(B, R.XCD_SHAPE["N"], R.XCD_SHAPE["Co"], pk)
            assert (cs, parts) == (8, 1) and (parts * -(-R.XCD_SHAPE["Co"] // cs)) % 2 == 1


def test_query_refuses_exactly_where_fits_does():
    L = _lib()
    for packed in (0, 1):
        nmax = L.dgx_edge_bwd_scatter_max_n(1, 8, packed)
        for B, N, Co in [(1, nmax, 8), (1, nmax + 1, 8), (1, 0, 8), (1, 65535, 8), (1, 65536, 8), (0, 100, 8),
                         (1, 100, 0), (4, 17000, 64), (4, 21000, 64)] + [(1, N, 8) for N in range(17000, 21000, 97)]:
            rc, cs, parts, tpp, lds = _geometry(B, N, Co, packed)
            fits = L.dgx_edge_bwd_scatter_fits(B, N, Co, packed)
            assert (rc == 0) == (fits == 1)
            if rc != 0:
                assert rc == -2 and (cs, parts, tpp, lds) == (-1, -1, -1, -1)
    assert L.dgx_edge_bwd_scatter_geometry(1, 200, 8, 1, None, None, None, None) == 0
