"""The split-K weight-gradient GEMM (gemm_lds_kernel<true, ...>, csrc/gemm.hip)
where its operand ring and its chunk-major workgroup map can go wrong: every
number of K-steps from one to past the ring's depth (fill, steady state and
drain), whole and partial last steps, a last chunk shorter than the ring, and
grids whose (tile, chunk) decode is ragged over the 8 XCDs. Through the C ABI
(dgx_gemm_lds_bf16 with tn = 1 and SLAB, then dgx_slab_reduce_f32), with the
lattice operands, the slab references and the guarded buffers of _gemm_ref.py:
every slab and every sum is compared exactly. Operands are redrawn for every
case, so a slab left over from an earlier case never equals the expected one."""
import ctypes

import pytest
import torch

import _gemm_ref as R
from _gemm_ref import SLAB, Buf

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
D = 3          # the deepest ring of the TN tiles (tn_depth in gemm.hip; 128 x 128 tiles run 2 stages)

# (M, N, R, splits, tile): the tile is asserted against dgx_gemm_lds_tile
FILL_DRAIN = [(M, N, 64 * nk - cut, 1, tile) for (M, N, tile) in ((72, 56, (64, 64)), (136, 136, (64, 128)))
              for nk in range(1, D + 3) for cut in (0, 27)]
# chunks of 4 steps (> D; S >= 4 keeps kchunk at 256), the last of 1 row, D - 1 steps, D steps less 5 rows
SHORT_LAST = [(M, N, 256 * (S - 1) + r, S, tile)
              for (M, N, S, tile) in ((72, 56, 4, (64, 64)), (136, 136, 5, (64, 128)), (136, 56, 256, (128, 64)))
              for r in (1, 64 * (D - 1), 64 * D - 5)]
# (row tiles, column tiles, slabs) -> (M, N): 64-row tiles, 64 or 128 columns, both edges ragged
MAP_GRIDS = [((1, 1, 17), (64, 64)), ((3, 1, 5), (184, 56)), ((5, 1, 3), (320, 64)), ((3, 3, 7), (192, 376)),
             ((5, 2, 9), (312, 200)), ((5, 3, 8), (320, 384)), ((3, 2, 16), (136, 256))]
MAP = [(M, N, 128 * S - 27, S, (64, 128 if N > 64 else 64)) for ((_, _, S), (M, N)) in MAP_GRIDS]
WORKLOAD = (1024, 512, 2048, 16, (128, 128))      # conv5's dW grid in miniature: 32 tiles x 16 chunks of 2 steps


def vp(x):
    return ctypes.c_void_p(x) if x else None


class Ctx:
    def __init__(self, dev, seed):
        from dgx import _native as nat
        self.L, self.dev = nat.lib(), dev
        self.g = torch.Generator(device=dev).manual_seed(seed)
        self.st = nat.stream_of(torch.empty(1, device=dev))
        self.fails, self.n = [], 0

    def check(self, what, *problems):
        self.n += 1
        self.fails += [f"{what}: {p}" for p in problems if p]

    def done(self, n):
        assert self.n == n, f"{self.n} cases ran, {n} expected"
        assert not self.fails, f"{len(self.fails)} failures in {self.n} cases:\n" + "\n".join(self.fails[:12])


def launch(cx, A, B, M, N, Rr, splits, slab):
    return cx.L.dgx_gemm_lds_bf16(vp(A.ptr()), A.ld, vp(B.ptr()), B.ld, 1, M, N, Rr, 0, SLAB, splits, vp(slab.ptr()),
                                  N, None, None, 0, cx.st)


def tn_case(cx, case, layout="dense", twice=False):
    M, N, Rr, splits, (bm, bn) = case
    dev = cx.dev
    what = f"tn M={M} N={N} R={Rr} splits={splits} ops:{layout}"
    assert cx.L.dgx_gemm_lds_tile(1, M, N, Rr, 0, SLAB, splits) == bm * 1000 + bn, what
    frac = Rr <= 4096                    # longer reductions stay exact with integers only
    a, b = R.lattice(cx.g, M, Rr, R.LIM, frac, dev), R.lattice(cx.g, N, Rr, R.LIM, frac, dev)
    ref = R.exact_or_raise(a, b, 64 if frac else 1, what=what)
    S, kc = cx.L.dgx_gemm_lds_slabs(Rr, splits), R.split_kchunk(Rr, splits, 64)
    assert S == -(-Rr // kc) <= splits, what
    A, B = Buf.of(a.t().to(BF16), layout, vec=8), Buf.of(b.t().to(BF16), layout, vec=8)
    slab = Buf(S * M, N, dev, guard_rows=2 * M + 2)
    rc = launch(cx, A, B, M, N, Rr, splits, slab)
    out = Buf(M, N, dev, ld=N + 8, c0=4)
    rc2 = cx.L.dgx_slab_reduce_f32(vp(slab.ptr()), S, M, N, M, vp(out.ptr()), out.ld, cx.st)
    probs = [(rc or rc2) and f"rc {rc} {rc2}",
             R.first_diff(slab.view.view(S, M, N), R.slab_refs(a, b, kc), "lds", bm, bn), slab.hit(),
             R.first_diff(out.view, ref, "lds", bm, bn), out.hit()]
    if twice:
        again = Buf(S * M, N, dev, guard_rows=2 * M + 2)
        rc3 = launch(cx, A, B, M, N, Rr, splits, again)
        probs += [rc3 and f"rc {rc3}", not torch.equal(slab.flat.view(torch.int32), again.flat.view(torch.int32))
                  and "two calls on the same operands differ", again.hit()]
    cx.check(what, *probs)
    return S


def test_cases_reach_every_tile_and_grid(cuda):
    """The cases below take the tiles and the (tiles x slabs) grids they are
    meant to, by the library's own queries."""
    L = Ctx(cuda, 0).L
    cases = FILL_DRAIN + SHORT_LAST + MAP + [WORKLOAD]
    tiles = {divmod(L.dgx_gemm_lds_tile(1, M, N, Rr, 0, SLAB, s), 1000) for M, N, Rr, s, _ in cases}
    assert tiles >= {(128, 128), (128, 64), (64, 128), (64, 64)}, tiles
    assert {c[4] for c in cases} == tiles
    for ((ni, nj, S), (M, N)), (_, _, Rr, s, (bm, bn)) in zip(MAP_GRIDS, MAP):
        assert (-(-M // bm), -(-N // bn), L.dgx_gemm_lds_slabs(Rr, s)) == (ni, nj, S), (M, N, Rr, s)
    assert sorted(ni * nj * S for (ni, nj, S), _ in MAP_GRIDS) == sorted([17, 15, 15, 63, 90, 120, 96])
    M, N, Rr, s, _ = WORKLOAD
    assert (M // 128) * (N // 128) == 32 and L.dgx_gemm_lds_slabs(Rr, s) == 16 and R.split_kchunk(Rr, s, 64) == 128


@pytest.mark.parametrize("layout", ["dense", "slice"])
def test_ring_fill_and_drain(cuda, layout):
    """1 .. D + 2 K-steps in one chunk: the ring never fills (1, 2 steps), fills
    exactly, and runs one and two steps of steady state before it drains; with a
    whole and with a partial last step (its k-rows zeroed in the landed stage)."""
    cx = Ctx(cuda, 41)
    for case in FILL_DRAIN:
        assert tn_case(cx, case, layout) == 1
    cx.done(len(FILL_DRAIN))


def test_short_last_chunk(cuda):
    """Chunks of four steps with a last chunk of one k-row, of D - 1 steps and of
    D steps with a partial one: the last chunk's ring is shorter than the others'."""
    cx = Ctx(cuda, 42)
    for case in SHORT_LAST:
        assert R.split_kchunk(case[2], case[3], 64) == 256, case
        assert tn_case(cx, case) == case[3]
    cx.done(len(SHORT_LAST))


def test_chunk_major_map_writes_every_tile_of_every_slab(cuda):
    """Grids of fewer than 8 workgroups per chunk, totals that are no multiple
    of 8 and a shorter last XCD range: every (tile, slab) holds its own product
    and nothing else is written; then conv5's grid in miniature."""
    cx = Ctx(cuda, 43)
    for case in MAP + [WORKLOAD]:
        assert tn_case(cx, case) == case[3]
    cx.done(len(MAP) + 1)


def test_two_calls_give_bit_equal_slabs(cuda):
    cx = Ctx(cuda, 44)
    for case in (WORKLOAD, MAP[4], SHORT_LAST[2], FILL_DRAIN[-1]):
        tn_case(cx, case, twice=True)
    cx.done(4)
