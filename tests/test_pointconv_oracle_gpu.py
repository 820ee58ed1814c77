"""Every entry point of csrc/pointconv.hip (conv5's BatchNorm + LeakyReLU passes,
reference models/dgcnn.py:74-78, 100-102) against the fp64 restatement of
tests/_pointconv_ref.py, through the C ABI, at the smallest shapes that reach
each tile edge:

  N    3  less than one float4, N % 4 != 0      C    4  one vector
     130  crosses the 128-point tile, N % 4 == 2     68  % 8 != 0, % 4 == 0, second 64-channel group nearly empty
     257  odd, second tile of the 256-point stats    70  % 4 != 0: 64x64 transpose route (fp32), scalar staging
          block nearly empty                             (bf16), the split passes answer DGX_EUNSUPPORTED
     384  N % 4 == 0, odd tile count                 96  % 8 == 0, % 64 != 0
                                                    128  whole channel groups
each with B in {1, 3} and slope in {0.2, 0.0}. Every element of every output is
compared (outputs start as a sentinel and carry a guard row, inputs carry a NaN
guard row), with the derived bounds of _pointconv_ref. dgx_to_bf16 /
dgx_split_bf16 are held bit-equal to torch's round-to-nearest-even on a crafted
vector, and the argument checks of the entry points return DGX_EINVAL without
touching their outputs.

Each test was run against libraries with value-only mutations of pointconv.hip
and failed as it should (none of them changes an address):
  ``>=`` for ``>`` in the five backward LeakyReLU decisions   test_bwd_f32, test_bwd_bf16, test_bwd_split_f32
  colstats skipping the first 4 rows of each 128-row block   test_colstats
  store_row4's scalar tail one element short                 test_apply_f32, test_apply_bf16 (N % 4 != 0)
  round-half-away in f32_to_bf16_rne                         test_to_bf16_and_split_bit_equal
  ``ldz < 1`` for ``ldz < C`` in dgx_colstats_f32            test_argument_checks
  c0 and c1 swapped in the three dZ kernels                  test_input_grad, test_bwd_bf16, test_bwd_split_f32
  load_row4's tail padded with 1 instead of 0                test_bwd_bf16, test_bwd_split_f32 (pass 0)
  scale and shift swapped in apply_T_kernel                  test_apply_f32 (strided rows, C % 4 != 0)"""
import itertools

import pytest
import torch

import _pointconv_ref as P
from dgx import _native as nat

pytestmark = pytest.mark.gpu
EINVAL, EUNSUPPORTED = -1, -2
f32, bf16 = nat.f32, nat.bf16


def _cases(cuda, N, C):
    for B, slope in itertools.product(P.BS, P.SLOPES):
        yield P.make_case(cuda, B, N, C, 1000 * N + 10 * C + B), slope


def _ok(rc, what):
    nat.check(rc, what)


def _assert_within(got, ref, bound, what):
    assert P.within(got, ref, bound), (what, "worst error / bound", P.worst(got, ref, bound))


def _assert_sums(part, ref, ref_abs, what):
    """column sums of the partial rows (reduced here in fp64; the row layout is the kernel's own)"""
    _assert_within(part.double().sum(0), ref, 32 * P.U * ref_abs, what)


@pytest.mark.parametrize("C", P.CS)
@pytest.mark.parametrize("N", P.NS)
def test_colstats(cuda, N, C):
    L = nat.lib()
    for B in P.BS:
        c = P.make_case(cuda, B, N, C, 7 * N + C + B)
        st = nat.stream_of(c.Z)
        z = c.Z.double()
        rows = L.dgx_colstats_rows(c.M)
        assert rows == (c.M + 127) // 128
        Zs = torch.full((c.M + 1, C + 4), float("nan"), device=cuda)
        Zs[:c.M, :C] = c.Z
        for src, ldz in ((c.Z, C), (Zs, C + 4)):
            full, part = P.guarded(rows, 2 * C, cuda)
            _ok(L.dgx_colstats_f32(f32(src), ldz, c.M, C, f32(part), rows, st), "colstats")
            torch.cuda.synchronize()
            assert P.guard_intact(full)
            _assert_sums(part[:, :C], z.sum(0), z.abs().sum(0), ("sum z", B, ldz))
            _assert_sums(part[:, C:], (z * z).sum(0), (z * z).sum(0), ("sum z^2", B, ldz))


@pytest.mark.parametrize("C", P.CS)
@pytest.mark.parametrize("N", P.NS)
def test_apply_f32(cuda, N, C):
    """dense rows (the 128-point LDS tile kernel when C % 4 == 0) and strided rows
    (ldz = C + 4, the 64x64 transpose kernel), bit-equal to each other"""
    L = nat.lib()
    for c, slope in _cases(cuda, N, C):
        B, st = c.B, nat.stream_of(c.Z)
        r = P.Ref(c, c.Z, slope)
        Zs = torch.full((c.M + 1, C + 4), float("nan"), device=cuda)
        Zs[:c.M, :C] = c.Z
        outs = []
        for src, ldz in ((c.Z, C), (Zs, C + 4)):
            full, out = P.guarded(B * C, N, cuda)
            _ok(L.dgx_pointconv_apply_f32(f32(src), ldz, B, N, C, f32(c.scale), f32(c.shift), slope, f32(out), st),
                "apply")
            torch.cuda.synchronize()
            assert P.guard_intact(full)
            _assert_within(out.view(B, C, N), r.out, 2 * P.U * r.out.abs(), ("apply", B, slope, ldz))
            outs.append(out)
        assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("C", P.CS)
@pytest.mark.parametrize("N", P.NS)
def test_apply_bf16(cuda, N, C):
    L = nat.lib()
    for c, slope in _cases(cuda, N, C):
        B, st = c.B, nat.stream_of(c.Z)
        r = P.Ref(c, c.Zb, slope)
        full, out = P.guarded(B * C, N, cuda)
        _ok(L.dgx_pointconv_apply_bf16(bf16(c.Zb), B, N, C, f32(c.scale), f32(c.shift), slope, f32(out), st),
            "apply bf16")
        torch.cuda.synchronize()
        assert P.guard_intact(full)
        _assert_within(out.view(B, C, N), r.out, 2 * P.U * r.out.abs(), ("apply bf16", B, slope))


@pytest.mark.parametrize("C", P.CS)
@pytest.mark.parametrize("N", P.NS)
def test_bwd_f32(cuda, N, C):
    """dz and the (sum d, sum d zhat) partials of the 64-point-tile pass, dense and strided Z"""
    L = nat.lib()
    for c, slope in _cases(cuda, N, C):
        B, M, st = c.B, c.M, nat.stream_of(c.Z)
        r = P.Ref(c, c.Z, slope)
        rows = L.dgx_pointconv_bwd_rows(B, N)
        assert rows == B * ((N + 63) // 64)
        Zs = torch.full((M + 1, C + 4), float("nan"), device=cuda)
        Zs[:M, :C] = c.Z
        for src, ldz in ((c.Z, C), (Zs, C + 4)):
            fdz, dz = P.guarded(M, C, cuda)
            fp, part = P.guarded(rows, 2 * C, cuda)
            _ok(L.dgx_pointconv_bwd_f32(f32(c.dout), f32(src), ldz, B, N, C, f32(c.scale), f32(c.shift), f32(c.mean),
                                        f32(c.invstd), slope, f32(dz), f32(part), st), "bwd")
            torch.cuda.synchronize()
            assert P.guard_intact(fdz) and P.guard_intact(fp)
            _assert_within(dz, r.d, 2 * P.U * r.d.abs(), ("dz", B, slope, ldz))
            _assert_sums(part[:, :C], r.s1, r.s1_abs, ("sum d", B, slope, ldz))
            _assert_sums(part[:, C:], r.s2, r.s2_abs, ("sum d zhat", B, slope, ldz))


@pytest.mark.parametrize("C", P.CS)
@pytest.mark.parametrize("N", P.NS)
def test_input_grad(cuda, N, C):
    """dZ = a dz + c0 + c1 z from a given dz, fp32 and bf16 output, dense and strided Z"""
    L = nat.lib()
    for B in P.BS:
        c = P.make_case(cuda, B, N, C, 3 * N + C + B)
        M, st = c.M, nat.stream_of(c.Z)
        r = P.Ref(c, c.Z, 0.2)
        ref, mag = r.dZ(c.dz_in.double())
        Zs = torch.full((M + 1, C + 4), float("nan"), device=cuda)
        Zs[:M, :C] = c.Z
        for (src, ldz), as16 in itertools.product(((c.Z, C), (Zs, C + 4)), (0, 1)):
            full, dZ = P.guarded(M, C, cuda, torch.bfloat16 if as16 else torch.float32)
            _ok(L.dgx_pointconv_input_grad(f32(c.dz_in), f32(src), ldz, M, C, f32(c.scale), f32(c.c0), f32(c.c1),
                                           nat.ptr(dZ), as16, st), "dZ")
            torch.cuda.synchronize()
            assert P.guard_intact(full)
            bound = 4 * P.U * mag + (2.0 ** -8 * ref.abs() if as16 else 0.0)
            _assert_within(dZ, ref, bound, ("dZ", B, ldz, as16))


@pytest.mark.parametrize("C", P.CS)
@pytest.mark.parametrize("N", P.NS)
def test_bwd_bf16(cuda, N, C):
    """bf16 Z: pass 0 (partials over 256-point blocks) and pass 1 (dZ in bf16)"""
    L = nat.lib()
    for c, slope in _cases(cuda, N, C):
        B, M, st = c.B, c.M, nat.stream_of(c.Z)
        r = P.Ref(c, c.Zb, slope)
        rows = L.dgx_pointconv_bf16_rows(B, N)
        assert rows == B * ((N + 255) // 256)
        fp, part = P.guarded(rows, 2 * C, cuda)
        _ok(L.dgx_pointconv_bwd_bf16(f32(c.dout), bf16(c.Zb), B, N, C, f32(c.scale), f32(c.shift), f32(c.mean),
                                     f32(c.invstd), slope, None, None, f32(part), None, 0, st), "bwd16 stats")
        fz, dZ = P.guarded(M, C, cuda, torch.bfloat16)
        _ok(L.dgx_pointconv_bwd_bf16(f32(c.dout), bf16(c.Zb), B, N, C, f32(c.scale), f32(c.shift), None, None, slope,
                                     f32(c.c0), f32(c.c1), None, bf16(dZ), 1, st), "bwd16 dZ")
        torch.cuda.synchronize()
        assert P.guard_intact(fp) and P.guard_intact(fz)
        _assert_sums(part[:, :C], r.s1, r.s1_abs, ("sum d", B, slope))
        _assert_sums(part[:, C:], r.s2, r.s2_abs, ("sum d zhat", B, slope))
        ref, mag = r.dZ(r.d)
        _assert_within(dZ, ref, 4 * P.U * mag + 2.0 ** -8 * ref.abs(), ("dZ bf16", B, slope))


@pytest.mark.parametrize("C", P.CS)
@pytest.mark.parametrize("N", P.NS)
def test_bwd_split_f32(cuda, N, C):
    """fp32 Z on the 128-point tiles: pass 0 partials; pass 1 writes the split-bf16
    planes of v = the fp32 dZ: hi = bf16(v), lo = bf16(v - hi) bit for bit, with v
    taken from the unfused pair (dgx_pointconv_bwd_f32 + dgx_pointconv_input_grad,
    themselves held to the oracle above), the planes of dgx_split_bf16 on that v
    bit-equal too, and hi + lo within the fp32 bound + 2^-17 |ref| of the fp64 dZ
    (|v - hi| <= 2^-9 |v|, lo rounds that to 2^-9 relative). C % 4 != 0 is refused."""
    L = nat.lib()
    for c, slope in _cases(cuda, N, C):
        B, M, st = c.B, c.M, nat.stream_of(c.Z)
        rows = L.dgx_pointconv_bf16_rows(B, N)
        fp, part = P.guarded(rows, 2 * C, cuda)
        fh, hi = P.guarded(M, C, cuda, torch.bfloat16)
        fl, lo = P.guarded(M, C, cuda, torch.bfloat16)
        rc0 = L.dgx_pointconv_bwd_split_f32(f32(c.dout), f32(c.Z), B, N, C, f32(c.scale), f32(c.shift), f32(c.mean),
                                            f32(c.invstd), slope, None, None, f32(part), None, None, 0, st)
        rc1 = L.dgx_pointconv_bwd_split_f32(f32(c.dout), f32(c.Z), B, N, C, f32(c.scale), f32(c.shift), None, None,
                                            slope, f32(c.c0), f32(c.c1), None, bf16(hi), bf16(lo), 1, st)
        torch.cuda.synchronize()
        assert P.guard_intact(fp) and P.guard_intact(fh) and P.guard_intact(fl)
        if C % 4:
            assert rc0 == EUNSUPPORTED and rc1 == EUNSUPPORTED
            for t in (part, hi, lo):
                assert bool((t.float() == P.SENT).all())
            continue
        _ok(rc0, "split stats")
        _ok(rc1, "split dZ")
        r = P.Ref(c, c.Z, slope)
        _assert_sums(part[:, :C], r.s1, r.s1_abs, ("sum d", B, slope))
        _assert_sums(part[:, C:], r.s2, r.s2_abs, ("sum d zhat", B, slope))
        # v from the unfused pair
        dz = torch.empty(M, C, device=cuda)
        p0 = torch.empty(L.dgx_pointconv_bwd_rows(B, N), 2 * C, device=cuda)
        _ok(L.dgx_pointconv_bwd_f32(f32(c.dout), f32(c.Z), C, B, N, C, f32(c.scale), f32(c.shift), f32(c.mean),
                                    f32(c.invstd), slope, f32(dz), f32(p0), st), "bwd")
        v = torch.empty(M, C, device=cuda)
        _ok(L.dgx_pointconv_input_grad(f32(dz), f32(c.Z), C, M, C, f32(c.scale), f32(c.c0), f32(c.c1), f32(v), 0, st),
            "dZ")
        hi0, lo0 = torch.empty_like(hi), torch.empty_like(lo)
        _ok(L.dgx_split_bf16(f32(v), C, M, C, bf16(hi0), bf16(lo0), C, st), "split")
        torch.cuda.synchronize()
        want_hi = v.bfloat16()
        want_lo = (v - want_hi.float()).bfloat16()
        assert torch.equal(hi.view(torch.int16), want_hi.view(torch.int16)), ("hi", B, slope)
        assert torch.equal(lo.view(torch.int16), want_lo.view(torch.int16)), ("lo", B, slope)
        assert torch.equal(hi, hi0) and torch.equal(lo, lo0)
        ref, mag = r.dZ(r.d)
        _assert_within(hi.double() + lo.double(), ref, 4 * P.U * mag + 2.0 ** -17 * ref.abs(), ("hi + lo", B, slope))


def _crafted():
    """fp32 bit patterns: ties to even in both directions (and one ulp either
    side), both signs; the largest finite (rounds to inf); subnormals (ties,
    the largest); +-0; +-inf; quiet and signalling NaNs."""
    pos = [0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0x3F817FFF, 0x3F818001, 0x3F800000, 0x40490FDB,
           0x7F7FFFFF, 0x7F7F8000, 0x7F7F7FFF, 0x00000001, 0x00008000, 0x00008001, 0x00018000, 0x007FFFFF,
           0x00800000, 0x00000000, 0x7F800000, 0x7FC00000, 0x7F800001, 0x7FFFFFFF]
    words = pos + [w | 0x80000000 for w in pos]
    words += [0x3F800000] * (-len(words) % 4)
    t = torch.tensor([w - (1 << 32) if w >= (1 << 31) else w for w in words], dtype=torch.int32)
    return t.view(torch.float32)


def _same_bf16(got, want):
    """bit-equal, except that any NaN matches any NaN"""
    nan = want.float().isnan()
    assert torch.equal(got.float().isnan(), nan)
    assert torch.equal(got.view(torch.int16)[~nan], want.view(torch.int16)[~nan])


def test_to_bf16_and_split_bit_equal(cuda):
    L = nat.lib()
    v = _crafted()
    n = v.numel()
    src = torch.full((3, n + 4), float("nan"))
    src[:, :n] = torch.stack([v, -v, v.flip(0)])
    host = src[:, :n].contiguous()
    want = host.bfloat16()                                   # torch's host conversion: round to nearest even
    want_lo = (host - want.float()).bfloat16().to(cuda)
    want = want.to(cuda)
    src = src.to(cuda)
    dense = src[:, :n].contiguous()
    st = nat.stream_of(src)
    for s, ld in ((dense, n), (src, n + 4)):   # dense and strided source
        full, dst = P.guarded(3, n, cuda, torch.bfloat16)
        _ok(L.dgx_to_bf16(f32(s), ld, 3, n, bf16(dst), st), "to_bf16")
        fh, hi = P.guarded(3, n, cuda, torch.bfloat16)
        fl, lo = P.guarded(3, n, cuda, torch.bfloat16)
        _ok(L.dgx_split_bf16(f32(s), ld, 3, n, bf16(hi), bf16(lo), n, st), "split")
        torch.cuda.synchronize()
        assert P.guard_intact(full) and P.guard_intact(fh) and P.guard_intact(fl)
        _same_bf16(dst, want)
        _same_bf16(hi, want)
        _same_bf16(lo, want_lo)


def test_argument_checks(cuda):
    """ldz < C, a null pointer and B < 1 (M < 1) answer DGX_EINVAL and leave the outputs alone"""
    L = nat.lib()
    B, N, C = 2, 5, 8
    c = P.make_case(cuda, B, N, C, 1)
    M, st = c.M, nat.stream_of(c.Z)
    fo, out = P.guarded(max(M, B * C), max(2 * C, N) + 8, cuda)
    fb, out16 = P.guarded(M, C, cuda, torch.bfloat16)
    o, o16 = f32(out), bf16(out16)
    Z, Zb, dout, a, b, mu, iv, c0, c1 = (f32(c.Z), bf16(c.Zb), f32(c.dout), f32(c.scale), f32(c.shift), f32(c.mean),
                                         f32(c.invstd), f32(c.c0), f32(c.c1))
    rows = L.dgx_colstats_rows(M)
    bad = [
        L.dgx_colstats_f32(Z, C - 1, M, C, o, rows, st), L.dgx_colstats_f32(None, C, M, C, o, rows, st),
        L.dgx_colstats_f32(Z, C, M, C, None, rows, st), L.dgx_colstats_f32(Z, C, 0, C, o, rows, st),
        L.dgx_colstats_f32(Z, C, M, C, o, rows + 1, st),
        L.dgx_pointconv_apply_f32(Z, C - 1, B, N, C, a, b, 0.2, o, st),
        L.dgx_pointconv_apply_f32(None, C, B, N, C, a, b, 0.2, o, st),
        L.dgx_pointconv_apply_f32(Z, C, B, N, C, a, None, 0.2, o, st),
        L.dgx_pointconv_apply_f32(Z, C, B, N, C, a, b, 0.2, None, st),
        L.dgx_pointconv_apply_f32(Z, C, 0, N, C, a, b, 0.2, o, st),
        L.dgx_pointconv_bwd_f32(dout, Z, C - 1, B, N, C, a, b, mu, iv, 0.2, o, o, st),
        L.dgx_pointconv_bwd_f32(None, Z, C, B, N, C, a, b, mu, iv, 0.2, o, o, st),
        L.dgx_pointconv_bwd_f32(dout, Z, C, B, N, C, a, b, None, iv, 0.2, o, o, st),
        L.dgx_pointconv_bwd_f32(dout, Z, C, B, N, C, a, b, mu, iv, 0.2, o, None, st),
        L.dgx_pointconv_bwd_f32(dout, Z, C, 0, N, C, a, b, mu, iv, 0.2, o, o, st),
        L.dgx_pointconv_input_grad(Z, Z, C - 1, M, C, a, c0, c1, o, 0, st),
        L.dgx_pointconv_input_grad(None, Z, C, M, C, a, c0, c1, o, 0, st),
        L.dgx_pointconv_input_grad(Z, Z, C, M, C, a, c0, None, o, 0, st),
        L.dgx_pointconv_input_grad(Z, Z, C, M, C, a, c0, c1, None, 1, st),
        L.dgx_pointconv_input_grad(Z, Z, C, 0, C, a, c0, c1, o, 0, st),
        L.dgx_pointconv_apply_bf16(None, B, N, C, a, b, 0.2, o, st),
        L.dgx_pointconv_apply_bf16(Zb, B, N, C, None, b, 0.2, o, st),
        L.dgx_pointconv_apply_bf16(Zb, B, N, C, a, b, 0.2, None, st),
        L.dgx_pointconv_apply_bf16(Zb, 0, N, C, a, b, 0.2, o, st),
        L.dgx_pointconv_bwd_bf16(None, Zb, B, N, C, a, b, mu, iv, 0.2, None, None, o, None, 0, st),
        L.dgx_pointconv_bwd_bf16(dout, Zb, B, N, C, a, b, None, iv, 0.2, None, None, o, None, 0, st),
        L.dgx_pointconv_bwd_bf16(dout, Zb, B, N, C, a, b, mu, iv, 0.2, None, None, None, None, 0, st),
        L.dgx_pointconv_bwd_bf16(dout, Zb, B, N, C, a, b, None, None, 0.2, c0, None, None, o16, 1, st),
        L.dgx_pointconv_bwd_bf16(dout, Zb, B, N, C, a, b, None, None, 0.2, c0, c1, None, None, 1, st),
        L.dgx_pointconv_bwd_bf16(dout, Zb, 0, N, C, a, b, mu, iv, 0.2, None, None, o, None, 0, st),
        L.dgx_pointconv_bwd_split_f32(dout, None, B, N, C, a, b, mu, iv, 0.2, None, None, o, None, None, 0, st),
        L.dgx_pointconv_bwd_split_f32(dout, Z, B, N, C, a, b, mu, None, 0.2, None, None, o, None, None, 0, st),
        L.dgx_pointconv_bwd_split_f32(dout, Z, B, N, C, a, b, None, None, 0.2, c0, c1, None, o16, None, 1, st),
        L.dgx_pointconv_bwd_split_f32(dout, Z, B, N, C, a, b, None, None, 0.2, None, c1, None, o16, o16, 1, st),
        L.dgx_pointconv_bwd_split_f32(dout, Z, 0, N, C, a, b, mu, iv, 0.2, None, None, o, None, None, 0, st),
        L.dgx_to_bf16(Z, C - 1, M, C, o16, st), L.dgx_to_bf16(None, C, M, C, o16, st),
        L.dgx_to_bf16(Z, C, M, C, None, st),
        L.dgx_split_bf16(Z, C - 4, M, C, o16, o16, C, st), L.dgx_split_bf16(None, C, M, C, o16, o16, C, st),
        L.dgx_split_bf16(Z, C, M, C, o16, None, C, st),
    ]
    torch.cuda.synchronize()
    assert [i for i, rc in enumerate(bad) if rc != EINVAL] == []
    assert bool((fo == P.SENT).all()) and bool((fb.float() == P.SENT).all())
    assert L.dgx_colstats_rows(0) == EINVAL and L.dgx_pointconv_bwd_rows(0, N) == EINVAL
    assert L.dgx_pointconv_bf16_rows(B, 0) == EINVAL
