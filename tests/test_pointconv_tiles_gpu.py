"""The three bf16 conv5 BatchNorm passes of csrc/pointconv.hip (apply16_lt,
bwd16_stats_lt, bwd16_dz_lt) at the edges of the geometry they ship with, through
the C ABI against the fp64 restatement of tests/_pointconv_ref.py, with the
bounds, guard rows and sentinels of test_pointconv_oracle_gpu.py (outputs
2 u |ref|, sums 32 u sum|.|, dZ 4 u mag + 2^-8 |ref|).

Geometry: every kernel works on tiles of T_n = 128 points x T_c = 64 channels;
the stats pass sums two consecutive point tiles into one partial row per (cloud,
256-point block). A workgroup does not take the tile of its blockIdx: tile_map
deals the tiles cloud by cloud (point blocks fastest inside a cloud), and the dz
pass walks that order backwards. So the cases are

  N (at C = 72: two channel blocks, the second nearly empty)
     126  T_n - 2, N % 4 != 0          128  T_n           132  T_n + 4
     258  2 T_n + 2                    257  the 256-point stats block + 1 point
     516  three stats blocks (the third nearly empty), five point tiles
  C (at N = 258: three point tiles, two stats blocks per cloud)
      56  T_c - 8      64  T_c      72  T_c + 8
     132  2 T_c + 4, % 8 != 0, % 4 == 0: scalar staging
      70  % 4 != 0: scalar staging
  C = 1024 at N = 132, B = 1: sixteen channel blocks against two point tiles

each with B in {1, 3} (3: the batch stride, and a block order in which clouds,
point blocks and channel blocks all differ from the launch order) and slope in
{0.2, 0.0}. Every element of every output is compared; the partial rows are
compared row by row (a row is one cloud's 256-point block: column sums alone
would not see two rows exchanged). Two launches of each pass are bit-equal, and
the dz pass is bit-equal to dgx_pointconv_input_grad (bf16 output) fed the d that
torch computes with the same single fp32 multiply, where both evaluate
fmaf(a, d, fmaf(c1, z, c0)) and round to bf16 once.

Each test was run against libraries with value-only mutations of the new code
(every mutated index stays inside the grid, so nothing is written out of bounds)
and failed as it should:
  tile_map's point block taken as (r % gy) % per_cloud (a wrong tile index
  under the remap)                       test_apply_tiles, test_bwd_tiles, test_dz_bit_equal_unfused
  the reversed order off by one tile (id = max(total - 2 - id, 0))
                                         test_bwd_tiles (dZ), test_dz_bit_equal_unfused
  the stats partial row taken from blockIdx.x, not from the mapped block
                                         test_bwd_tiles (B = 3, row by row)"""
import itertools

import pytest
import torch

import _pointconv_ref as P
from dgx import _native as nat

pytestmark = pytest.mark.gpu
f32, bf16 = nat.f32, nat.bf16

T_N, T_C, STATS_N = 128, 64, 256
N_CASES = [(n, T_C + 8) for n in (T_N - 2, T_N, T_N + 4, 2 * T_N + 2, 257, 516)]
C_CASES = [(2 * T_N + 2, c) for c in (T_C - 8, T_C, 2 * T_C + 4, 70)]   # (258, 72) is among the N cases
SHAPES = N_CASES + C_CASES
WIDE = (T_N + 4, 1024)   # more channel blocks than point blocks: B = 1 only


def _cases(cuda, N, C):
    for B, slope in itertools.product((1,) if (N, C) == WIDE else P.BS, P.SLOPES):
        yield P.make_case(cuda, B, N, C, 1000 * N + 10 * C + B), slope


def _assert_within(got, ref, bound, what):
    assert P.within(got, ref, bound), (what, "worst error / bound", P.worst(got, ref, bound))


def _apply(L, c, slope, cuda):
    full, out = P.guarded(c.B * c.C, c.N, cuda)
    nat.check(L.dgx_pointconv_apply_bf16(bf16(c.Zb), c.B, c.N, c.C, f32(c.scale), f32(c.shift), slope, f32(out),
                                         nat.stream_of(c.Z)), "apply bf16")
    return full, out


def _stats(L, c, slope, cuda):
    rows = L.dgx_pointconv_bf16_rows(c.B, c.N)
    assert rows == c.B * ((c.N + STATS_N - 1) // STATS_N)
    full, part = P.guarded(rows, 2 * c.C, cuda)
    nat.check(L.dgx_pointconv_bwd_bf16(f32(c.dout), bf16(c.Zb), c.B, c.N, c.C, f32(c.scale), f32(c.shift),
                                       f32(c.mean), f32(c.invstd), slope, None, None, f32(part), None, 0,
                                       nat.stream_of(c.Z)), "bwd16 stats")
    return full, part


def _dz(L, c, slope, cuda):
    full, dZ = P.guarded(c.M, c.C, cuda, torch.bfloat16)
    nat.check(L.dgx_pointconv_bwd_bf16(f32(c.dout), bf16(c.Zb), c.B, c.N, c.C, f32(c.scale), f32(c.shift), None, None,
                                       slope, f32(c.c0), f32(c.c1), None, bf16(dZ), 1, nat.stream_of(c.Z)),
              "bwd16 dZ")
    return full, dZ


def _row_sums(c, r):
    """fp64 (sum d, sum |d|, sum d zhat, sum |d zhat|) of each partial row: (cloud, 256-point block) x channel"""
    zhat = (r.z - c.mean.double()) * c.invstd.double()
    t2 = r.d * zhat
    out = [[], [], [], []]
    for b in range(c.B):
        for n0 in range(0, c.N, STATS_N):
            sl = slice(b * c.N + n0, b * c.N + min(n0 + STATS_N, c.N))
            for acc, t in zip(out, (r.d[sl], r.d[sl].abs(), t2[sl], t2[sl].abs())):
                acc.append(t.sum(0))
    return [torch.stack(a) for a in out]


@pytest.mark.parametrize("N,C", SHAPES + [WIDE])
def test_apply_tiles(cuda, N, C):
    L = nat.lib()
    for c, slope in _cases(cuda, N, C):
        r = P.Ref(c, c.Zb, slope)
        full, out = _apply(L, c, slope, cuda)
        torch.cuda.synchronize()
        assert P.guard_intact(full)
        _assert_within(out.view(c.B, C, N), r.out, 2 * P.U * r.out.abs(), ("apply bf16", c.B, slope))


@pytest.mark.parametrize("N,C", SHAPES + [WIDE])
def test_bwd_tiles(cuda, N, C):
    """pass 0: every partial row against its own (cloud, 256-point block); pass 1: dZ"""
    L = nat.lib()
    for c, slope in _cases(cuda, N, C):
        r = P.Ref(c, c.Zb, slope)
        fp, part = _stats(L, c, slope, cuda)
        fz, dZ = _dz(L, c, slope, cuda)
        torch.cuda.synchronize()
        assert P.guard_intact(fp) and P.guard_intact(fz)
        s1, s1_abs, s2, s2_abs = _row_sums(c, r)
        _assert_within(part[:, :C], s1, 32 * P.U * s1_abs, ("sum d by row", c.B, slope))
        _assert_within(part[:, C:], s2, 32 * P.U * s2_abs, ("sum d zhat by row", c.B, slope))
        ref, mag = r.dZ(r.d)
        _assert_within(dZ, ref, 4 * P.U * mag + 2.0 ** -8 * ref.abs(), ("dZ bf16", c.B, slope))


def test_two_launches_bit_equal(cuda):
    """out, the partial rows and dZ of two launches on the same inputs, bit for bit"""
    L = nat.lib()
    c = P.make_case(cuda, 3, 516, 2 * T_C + 4, 5)
    for fn, view in ((_apply, torch.int32), (_stats, torch.int32), (_dz, torch.int16)):
        a, b = fn(L, c, 0.2, cuda)[0], fn(L, c, 0.2, cuda)[0]
        torch.cuda.synchronize()
        assert torch.equal(a.view(view), b.view(view)), fn.__name__


@pytest.mark.parametrize("slope", P.SLOPES)
def test_dz_bit_equal_unfused(cuda, slope):
    """C % 8 == 0: dZ of the fused pass == dgx_pointconv_input_grad (bf16 out) on d = dout * (y > 0 ? 1 : slope),
    d formed in torch by one fp32 multiply (the decision is the sign of the exact a z + b, as in the kernel's
    correctly rounded fmaf); both then evaluate fmaf(a, d, fmaf(c1, z, c0)) and round to nearest even once."""
    L = nat.lib()
    B, N, C = 3, 2 * T_N + 2, T_C + 8
    c = P.make_case(cuda, B, N, C, 77)
    st = nat.stream_of(c.Z)
    z32 = c.Zb.float().contiguous()
    pos = (c.scale.double() * z32.double() + c.shift.double()) > 0
    factor = torch.where(pos, torch.tensor(1.0, device=cuda), torch.tensor(slope, dtype=torch.float32, device=cuda))
    d = (P.to_mc(c.dout, B, N, C) * factor).contiguous()
    assert d.dtype == torch.float32
    fw, want = P.guarded(c.M, C, cuda, torch.bfloat16)
    nat.check(L.dgx_pointconv_input_grad(f32(d), f32(z32), C, c.M, C, f32(c.scale), f32(c.c0), f32(c.c1),
                                         nat.ptr(want), 1, st), "dZ unfused")
    fz, dZ = _dz(L, c, slope, cuda)
    torch.cuda.synchronize()
    assert P.guard_intact(fw) and P.guard_intact(fz)
    assert torch.equal(dZ.view(torch.int16), want.view(torch.int16))
