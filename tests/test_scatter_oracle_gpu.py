"""The EdgeConv backward scatter (edge_bwd_scatter_kernel<CS, OUT16, PACKED,
SPLIT, TPP>, csrc/edgeconv.hip) against the host oracle tests/_scatter_ref.py,
through the C entries with hand-built inputs and a host-built reverse graph:

* every reachable launch form (36: slices x cs x lanes x output mode) on
  lattice inputs, where fp32 is exact in any order: fp32 output equal to the
  fp64 reference bit for bit, bf16 to its round-to-nearest-even cast, the
  split planes to hi = bf16(v), lo = bf16(v - hi);
* both sides of every boundary of the slice-width, LDS-mode and lane rules,
  N around 64, the XCD map's repeated and padded forms;
* second and third passes of the boustrophedon deal, full and partly filled;
* channel counts and PQ strides off every vector form, NaN in PQ's padding;
* k = 1 .. 64 (slot 63), in-degrees at each batch edge and at the bucket clamp,
  a cloud whose every edge enters one point, repeated neighbour ids;
* the summation order itself, on random data, and the project's 2e-6 bar;
* the folded-in BatchNorm finalize at every CS around its row-loop edges.

Every output lies inside a NaN-filled buffer whose guards (and, in mode 2, third
plane) must stay NaN. The launch form of every case is asked from
dgx_edge_bwd_scatter_geometry before the launch."""
import ctypes
import functools

import pytest
import torch

import _scatter_ref as R
from dgx import _native as nat
from dgx import schedule

pytestmark = pytest.mark.gpu


def _geometry(B, N, Co, packed):
    cs, parts, tpp, lds = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int64(-1)
    nat.check(nat.lib().dgx_edge_bwd_scatter_geometry(B, N, Co, int(packed), ctypes.byref(cs), ctypes.byref(parts),
                                                      ctypes.byref(tpp), ctypes.byref(lds)), "geometry")
    return cs.value, parts.value, tpp.value


def _expect_form(c, packed, form):
    cs, parts, tpp = _geometry(c.B, c.N, c.Co, packed)
    assert (cs, tpp) == tuple(form), (c.B, c.N, c.Co, packed, cs, parts, tpp)
    return cs, parts, tpp


@functools.lru_cache(maxsize=4)
def _lattice(shape, graph="random", extra=0, seed=0, arg_all_slots=False):
    """the lattice case of a shape with its exact fp32 reference (shared by the tests of that shape)"""
    B, N, k, Co = shape
    arg = None
    if arg_all_slots:   # every slot 0 .. k-1, in every channel
        arg = ((torch.arange(B * N).view(-1, 1) + torch.arange(Co).view(1, -1)) % k).to(torch.uint8)
    c = R.make_lattice(B, N, k, Co, R.make_idx(graph, B, N, k, seed), ldpq=2 * Co + extra, seed=seed, arg=arg)
    c.ref = R.exact_f32(R.ref64(c))
    return c


def _dev(c, dev):
    """the case's inputs on the device (once)"""
    if getattr(c, "_d", None) is None:
        c._d = {n: getattr(c, n).to(dev) for n in ("PQ", "dz", "arg", "sumP", "a", "c0", "c1", "rowptr", "edges")}
        c._d["words"] = c.dz_words().to(dev)
    return c._d


def _guarded(n, dtype, dev):
    full = torch.full((R.GUARD + n + R.GUARD,), R.NAN, dtype=dtype, device=dev)
    return full, full[R.GUARD:R.GUARD + n]


def _guards_nan(full):
    return bool(full[:R.GUARD].isnan().all()) and bool(full[-R.GUARD:].isnan().all())


def _launch(c, dev, packed, mode, over=None, fin=None):
    """One scatter launch into a guarded buffer -> the whole buffer. ``over``:
    replacement device tensors (PQ, sumP, a, c0, c1); ``fin``: (partials, nrows,
    count, mean, invstd, eval, dgamma, dbeta) for dgx_edge_bwd_scatter_fin_f32,
    which then writes c0 / c1."""
    D = dict(_dev(c, dev), **(over or {}))
    L = nat.lib()
    n = c.M * 2 * c.Co * (1 if mode < 2 else 3)
    full, out = _guarded(n, torch.float32 if mode == 0 else torch.bfloat16, dev)
    stream = nat.stream_of(out)
    head = (nat.f32(D["PQ"]), c.ldpq, nat.i32(D["rowptr"]), nat.i32(D["edges"]))
    if fin is not None:
        part, nrows, count, mean, invstd, ev, dgamma, dbeta = fin
        nat.check(L.dgx_edge_bwd_scatter_fin_f32(
            *head, nat.f32(D["words"] if packed else D["dz"]), None if packed else nat.u8(D["arg"]),
            nat.f32(D["sumP"]), c.B, c.N, c.k, c.Co, nat.f32(part), nrows, count, nat.f32(D["a"]), nat.f32(mean),
            nat.f32(invstd), int(ev), nat.f32(dgamma), nat.f32(dbeta), nat.f32(D["c0"]), nat.f32(D["c1"]),
            nat.ptr(out, nat.F32, nat.BF16), mode, int(packed), stream), "scatter fin")
        return full
    tail = (nat.f32(D["sumP"]), c.B, c.N, c.k, c.Co, nat.f32(D["a"]), nat.f32(D["c0"]), nat.f32(D["c1"]),
            nat.ptr(out, nat.F32, nat.BF16), mode, stream)
    if packed:
        nat.check(L.dgx_edge_bwd_scatter_packed_f32(*head, nat.f32(D["words"]), *tail), "scatter packed")
    else:
        nat.check(L.dgx_edge_bwd_scatter_f32(*head, nat.f32(D["dz"]), nat.u8(D["arg"]), *tail), "scatter")
    return full


def _planes(full, c, mode):
    return full[R.GUARD:-R.GUARD].view(1 if mode < 2 else 3, c.M, 2 * c.Co)


def _assert_exact(full, c, ref, mode, what=""):
    """guards NaN; the planes equal to what the exact fp32 result ``ref`` gives in this mode, bit for bit"""
    torch.cuda.synchronize()
    assert _guards_nan(full), ("guard overwritten", what, mode)
    got = _planes(full, c, mode).cpu()
    for p, want in enumerate(R.expected_planes(ref, mode)):
        if want is None:
            assert bool(got[p].isnan().all()), ("mode 2 wrote its third plane", what)
            continue
        assert bool(torch.isfinite(got[p].float()).all()), ("not finite", what, mode, p)
        if not torch.equal(got[p], want):
            bad = (got[p].float() != want.float()).nonzero()
            r, o = (int(x) for x in bad[0])
            raise AssertionError(f"{what} mode {mode} plane {p}: {len(bad)} of {want.numel()} differ, first at row "
                                 f"{r} (point {r % c.N} of cloud {r // c.N}) column {o}: got {float(got[p][r, o])}, "
                                 f"want {float(want[r, o])}")


def _run_exact(c, dev, packed, modes, what=""):
    for mode in modes:
        _assert_exact(_launch(c, dev, packed, mode), c, c.ref, mode, what)


# ---- the host graph is the engine's ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,B,N,k", [("hubs", 4, 777, 11), ("ladder", 2, 200, 4), ("dups", 3, 65, 64)])
def test_engine_reverse_graph_equals_host_graph(cuda, kind, B, N, k):
    idx = R.make_idx(kind, B, N, k, seed=3)
    rowptr, edges = R.reverse_graph(idx, B, N, k)
    (rp, ed), = schedule.reverse_graphs([idx.to(torch.int32).to(cuda).contiguous()])
    torch.cuda.synchronize()
    assert torch.equal(rp.cpu(), rowptr) and torch.equal(ed.cpu(), edges)


# ---- a. every launch form, exact ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("name", list(R.FORMS))
def test_every_launch_form_exact(cuda, name, mode):
    shape, packed, form = R.FORMS[name]
    c = _lattice(shape, "hubs")
    _expect_form(c, packed, form)
    _run_exact(c, cuda, packed, (mode,), name)


# ---- b. both sides of every boundary --------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,packed,form", R.BOUNDARIES, ids=lambda v: str(v).replace(" ", ""))
def test_boundaries_exact(cuda, shape, packed, form):
    c = _lattice(shape)
    _expect_form(c, packed, form)
    _run_exact(c, cuda, packed, (0, 1) if packed else (0, 3), f"N{shape[1]}")


@pytest.mark.parametrize("shape,packed", R.SMALL_N, ids=lambda v: str(v).replace(" ", ""))
def test_small_clouds_exact(cuda, shape, packed):
    """N = 1 (k = 1), 2, 63, 64 — one part — and 65, the first with two (parts * 64 < N)"""
    c = _lattice(shape)
    _, parts, _ = _geometry(c.B, c.N, c.Co, packed)
    assert parts == (2 if c.N == 65 else 1)
    _run_exact(c, cuda, packed, R.MODES, f"N{shape[1]}")


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("B", R.XCD_BS)
def test_xcd_map_forms_exact(cuda, B, packed):
    """an odd number of (part x slice) tiles per cloud at B = 2, 3 (each cloud on 4 / 2
    XCDs, the last range short or empty), 5, 9 (padding blocks) and 8"""
    s = R.XCD_SHAPE
    c = _lattice((B, s["N"], s["k"], s["Co"]))
    cs, parts, _ = _geometry(B, c.N, c.Co, packed)
    assert (parts * -(-c.Co // cs)) % 2 == 1
    _run_exact(c, cuda, packed, (0, 2), f"B{B}")


# ---- c. several passes ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,packed,form,passes,last", R.PASSES, ids=lambda v: str(v).replace(" ", ""))
def test_several_passes_exact(cuda, shape, packed, form, passes, last):
    c = _lattice(shape, "hubs")
    _, parts, tpp = _expect_form(c, packed, form)
    ppb = R.EC_THREADS // tpp
    assert parts == 1 and -(-c.N // ppb) == passes and c.N - (passes - 1) * ppb == last
    _run_exact(c, cuda, packed, (1,) if packed else (0,), f"N{shape[1]}")


# ---- d. channels and strides ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("extra", R.LDPQ_EXTRA)
@pytest.mark.parametrize("Co", R.CS8_COS + (8,))
def test_channels_and_strides_exact(cuda, Co, extra, packed):
    """Co off the slice width and off 4 at 8-channel slices; ldpq = 2Co, 2Co + 4,
    2Co + 1 with NaN in PQ's padding columns"""
    c = _lattice((1, 200, 4, Co), "hubs", extra)
    assert bool(c.PQ[:, 2 * Co:].isnan().all()) and c.PQ.shape[1] == 2 * Co + extra
    _expect_form(c, packed, (8, 4 if packed else 1))
    _run_exact(c, cuda, packed, R.MODES, f"Co{Co} ldpq{c.ldpq}")


@pytest.mark.parametrize("extra", (0, 1))
@pytest.mark.parametrize("shape,packed,form", R.PARTIAL_SLICES, ids=lambda v: str(v).replace(" ", ""))
def test_partial_last_slice_exact(cuda, shape, packed, form, extra):
    c = _lattice(shape, "random", extra)
    cs, _, _ = _expect_form(c, packed, form)
    assert c.Co % cs != 0 and c.Co > cs
    _run_exact(c, cuda, packed, R.MODES, f"Co{c.Co} cs{cs}")


# ---- e. k and in-degrees --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", (1, 4, 2))
@pytest.mark.parametrize("k", R.KS)
def test_k_extremes_exact(cuda, k, lanes):
    """k = 1, 16, 17 and 64: arg takes every slot up to 63, the top of the 6-bit field"""
    (B, N, _, Co), packed, form = R.LANE_FORMS[lanes]
    c = _lattice((B, N, k, Co), "random", 0, 0, True)
    assert sorted(c.arg.unique().tolist()) == list(range(k))
    _expect_form(c, packed, form)
    _run_exact(c, cuda, packed, (0,), f"k{k}")
    if lanes == 1:   # the slot bytes' form of the same, and the packed words at one lane
        c4 = _lattice((1, 1200, k, 8), "random", 0, 0, True)
        _expect_form(c4, True, (4, 1))
        _run_exact(c4, cuda, True, (0,), f"k{k} packed cs4")


@pytest.mark.parametrize("lanes", (1, 4, 2, "p1"))
@pytest.mark.parametrize("graph", ("ladder", "all0", "dups"))
def test_in_degree_edges_exact(cuda, graph, lanes):
    """in-degrees 0, 1, 15, 16, 17, 31, 32, 33 (the 16-id batch, 8 and 4 per lane)
    and 63, 64, 65 (the bucket clamp) with a hub; one point holding every edge;
    rows that repeat a neighbour"""
    shape, packed, form = R.LANE_FORMS[lanes]
    c = _lattice(shape, graph, 0, 1)
    if graph == "ladder":
        assert sorted(R.in_degrees(c)[1:12].tolist()) == sorted(R.LADDER)
    if graph == "all0":
        assert c.maxdeg == c.N * c.k
    _expect_form(c, packed, form)
    _run_exact(c, cuda, packed, (0, 1), f"{graph} lanes {lanes}")


# ---- f. the summation order -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", (1, 4, 2))
def test_summation_order_on_random_data(cuda, lanes):
    """Random data with hubs. c0 = c1 = 0, a = +-2^e: dP = a x the fp32 sum of the
    selected dz over the in-edges in CSR order (lane s of TPP taking edges beg + s
    + TPP v, lanes combined (s0 + s1) + (s2 + s3)), bit for bit; a = c0 = 0, c1 =
    1, P = sumP = 0: dP = that sum of Q, dQ = k Q. The general case: 2e-6 of the
    output's largest value from fp64, and the bf16 and split-plane outputs equal
    to the roundings of that fp32 output (lo = bf16(v - hi) needs rounding here,
    as it never does on the lattice)."""
    shape, packed, form = R.LANE_FORMS[lanes]
    B, N, k, Co = shape
    c = R.make_random(B, N, k, Co, R.make_idx("hubs", B, N, k, 5), seed=5)
    _, _, tpp = _expect_form(c, packed, form)
    assert tpp == lanes
    sd, sq = R.ordered_sums(c, packed, tpp)
    zero = torch.zeros(Co, device=cuda)
    a = torch.tensor([(-1.0) ** o * 2.0 ** (o % 5 - 2) for o in range(Co)])
    full = _launch(c, cuda, packed, 0, dict(a=a.to(cuda), c0=zero, c1=zero))
    torch.cuda.synchronize()
    got = _planes(full, c, 0)[0].cpu()
    assert _guards_nan(full)
    assert torch.equal(got[:, :Co], a * sd)
    assert torch.equal(got[:, Co:], a * c.dz_values(packed))
    PQ0 = c.PQ.clone()
    PQ0[:, :Co] = 0
    full = _launch(c, cuda, packed, 0, dict(PQ=PQ0.to(cuda), sumP=torch.zeros(c.M, Co, device=cuda), a=zero, c0=zero,
                                           c1=torch.ones(Co, device=cuda)))
    torch.cuda.synchronize()
    got = _planes(full, c, 0)[0].cpu()
    assert _guards_nan(full)
    assert torch.equal(got[:, :Co], sq)
    assert torch.equal(got[:, Co:], float(k) * c.PQ[:, Co:2 * Co])
    ref = R.ref64(c, packed)
    full = _launch(c, cuda, packed, 0)
    torch.cuda.synchronize()
    err = float((_planes(full, c, 0)[0].cpu().double() - ref).abs().max() / ref.abs().max())
    print(f"lanes {lanes}: general random case {err:.2e} of the output scale")
    assert _guards_nan(full) and err < 2e-6
    # the bf16 forms of the same (full-mantissa) result: its round-to-nearest-even cast and split planes
    v = _planes(full, c, 0)[0].cpu()
    for mode in (1, 2, 3):
        _assert_exact(_launch(c, cuda, packed, mode), c, v, mode, f"random, lanes {lanes}")


# ---- g. the finalize form at every CS -------------------------------------------------------------------------------
@pytest.mark.parametrize("name,cs", R.FIN_FORMS)
def test_finalize_form_exact(cuda, name, cs):
    """dgx_edge_bwd_scatter_fin_f32: lattice partial rows and power-of-two count,
    mean, invstd make dgamma, dbeta, c0, c1 exact; nrows on both sides of G = 512 /
    CS rows per trip and of the 4 G unroll; dPQ equal to the plain entry's with
    those constants, bit for bit. Co = 12: at CS = 8 the second slice is partial."""
    (B, N, k, _), packed, _ = R.FORMS[name]
    Co = 12
    c = _lattice((B, N, k, Co), "hubs")
    assert _geometry(B, N, Co, packed)[0] == cs
    for nrows in R.fin_nrows(cs):
        part, count, mean, invstd = R.make_finalize(Co, nrows)
        dpart, dmean, dinv = part.to(cuda), mean.to(cuda), invstd.to(cuda)
        for ev in (0, 1):
            bufs = [_guarded(Co, torch.float32, cuda) for _ in range(4)]     # dgamma, dbeta, c0, c1
            (_, dgamma), (_, dbeta), (_, c0), (_, c1) = bufs
            full = _launch(c, cuda, packed, 0, dict(c0=c0, c1=c1),
                           fin=(dpart, nrows, count, dmean, dinv, ev, dgamma, dbeta))
            plain = _launch(c, cuda, packed, 0, dict(c0=c0, c1=c1))
            torch.cuda.synchronize()
            want = R.finalize_ref(part, count, c.a, mean, invstd, ev)
            for (fb, got), w, nm in zip(bufs, want, ("dgamma", "dbeta", "c0", "c1")):
                assert _guards_nan(fb), nm
                assert torch.equal(got.cpu(), w), (nm, nrows, ev, got.cpu(), w)
            assert _guards_nan(full) and _guards_nan(plain)
            out = _planes(full, c, 0)[0]
            assert bool(torch.isfinite(out).all()) and torch.equal(out, _planes(plain, c, 0)[0]), (nrows, ev)
            if ev:   # c0 = c1 = 0: dPQ = a x the sums, exact on the lattice
                assert torch.equal(out.cpu(), R.exact_f32(R.ref64(c, packed, c0=want[2], c1=want[3])))
