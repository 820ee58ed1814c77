"""The EdgeConv forward gather (csrc/edgeconv.hip edge_gather_lds_kernel<CS,
EVAL>, reference models/dgcnn.py:84-98: max over the k neighbours of the
pre-BN edge value) called directly, at every launch geometry gather_geom can
choose: the channel slice CS follows N (32 up to N = 512, halved at each
doubling down to 1 above 8192, more than 64 KiB of LDS per one-channel slice
above 16384), the CS < 4 thread split, a partial last slice, Co % 4 != 0,
ldpq % 4 != 0, short idx passes at large k, and point_parts from 1 upwards.

Integer-valued P and Q make every fp32 sum of the kernel exact in any order,
so the selected value, its FIRST extremal slot, sum_k P and the BatchNorm
partial sums are compared bit for bit with an integer restatement; randn data
then checks the same kernel against an fp32 / fp64 restatement."""
import pytest
import torch

pytestmark = pytest.mark.gpu

# each side of every CS boundary, and two clouds in the large-LDS mode (a
# one-channel slice of N floats + the idx pass buffer stays under the entry's
# 160 KiB check up to N = 36864)
NS = [512, 513, 1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193, 16384, 16385, 30000]
COS = [6, 8, 40]     # partial last slice + Co % 4 != 0 | whole vectors, one slice at CS >= 8 | several slices
BUDGET = 80 * 10 ** 6   # gathered (B, N, k, Co) elements of the restatement


def _cs(N):
    """slice_channels(N, 1): the widest power-of-two slice of N floats per channel in 64 KiB."""
    cs = 32
    while cs > 1 and N * cs * 4 > 64 * 1024:
        cs //= 2
    return cs


def _geometry_cases():
    """Every N meets every Co; every N meets k = 64 once; B, ldpq and k rotate."""
    out = []
    for i, N in enumerate(NS):
        for j, Co in enumerate(COS):
            k = 64 if j == i % 3 else (1, 7, 20)[(i + j) % 3]
            B = (1, 3, 9)[(i + 2 * j) % 3]
            while B > 1 and B * N * k * Co > BUDGET:
                B = {9: 3, 3: 1}[B]
            pad = (0, 4, 1)[(i + j) % 3]      # PQ rows of a wider buffer: ldpq = 2 Co + pad
            out.append((B, N, k, Co, pad))
    # many small clouds: B * slices >= 512 (and N <= 64), one part per cloud
    out += [(600, 40, 7, 8, 4), (520, 33, 20, 40, 1)]
    return out


CASES = _geometry_cases()


def _ids(c):
    B, N, k, Co, pad = c
    return f"B{B}N{N}k{k}Co{Co}ld{2 * Co + pad}cs{_cs(N)}"


def _inputs(case, cuda, integer):
    B, N, k, Co, pad = case
    g = torch.Generator(device="cpu").manual_seed(N * 131 + Co * 7 + k)
    M, ld = B * N, 2 * Co + pad
    buf = torch.full((M, ld), float("nan"))            # the padding columns are never read
    if integer:
        buf[:, :2 * Co] = torch.randint(-4, 5, (M, 2 * Co), generator=g).float()
    else:
        buf[:, :2 * Co] = torch.randn(M, 2 * Co, generator=g)
    idx = torch.randint(0, N, (B, N, k), generator=g, dtype=torch.int32)
    gamma = torch.randn(Co, generator=g).abs() + 0.1
    gamma[::2] *= -1.0                                 # both signs
    gamma[Co // 2] = 0.0                               # gamma = 0 selects the max, as gamma > 0 does
    assert bool((gamma < 0).any()) and bool((gamma > 0).any())
    PQ = buf.to(cuda)[:, :2 * Co] if pad == 0 else buf.to(cuda)
    assert PQ.data_ptr() % 16 == 0 and PQ.stride(0) == ld
    return PQ, idx.to(cuda), gamma.to(cuda)


def _gathered(PQ, idx, B, N, k, Co, dtype):
    """P of every edge (B, N, k, Co), Q of every centre (B, N, Co)."""
    P = PQ[:, :Co].reshape(B, N, Co).to(dtype)
    Q = PQ[:, Co:2 * Co].reshape(B, N, Co).to(dtype)
    b = torch.arange(B, device=PQ.device).view(B, 1, 1)
    return P[b, idx.long()], Q


def _select(Pn, neg):
    """(extremal P, FIRST extremal slot) per (cloud, point, channel): max over
    the k slots where the channel's sign is >= 0, min where ``neg`` (Co,) says < 0."""
    k = Pn.shape[2]
    v = torch.where(neg.view(1, 1, 1, -1), -Pn, Pn)
    best = v.max(dim=2).values
    slots = torch.arange(k, device=Pn.device).view(1, 1, k, 1)
    arg = torch.where(v == best.unsqueeze(2), slots, k).min(dim=2).values
    return torch.where(neg, -best, best), arg


def _run_gather(PQ, idx, gamma, B, N, k, Co):
    from dgx import _native as nat
    from dgx.edgeconv import edge_select
    ysel, arg, sumP, partials, prow = edge_select(PQ, idx, B, N, k, Co, gamma, nat.stream_of(PQ))
    torch.cuda.synchronize()
    return ysel.view(B, N, Co), arg.view(B, N, Co), sumP.view(B, N, Co), partials, prow


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_gather_exact_on_integer_data(cuda, case):
    B, N, k, Co, pad = case
    PQ, idx, gamma = _inputs(case, cuda, integer=True)
    ysel, arg, sumP, partials, prow = _run_gather(PQ, idx, gamma, B, N, k, Co)
    Pn, Q = _gathered(PQ, idx, B, N, k, Co, torch.int32)
    best, slot = _select(Pn, gamma < 0)
    sP = Pn.sum(dim=2, dtype=torch.int64)
    y = Pn + Q.unsqueeze(2)
    s1 = y.sum(dim=2, dtype=torch.int64)                       # per point
    s2 = (y * y).sum(dim=2, dtype=torch.int64)
    a1 = y.abs().sum(dim=2, dtype=torch.int64)
    # exactness: every partial row (a part of one cloud: `per` consecutive
    # points) sums integers whose absolute total stays below 2^24, so each fp32
    # partial sum of the kernel is exact whatever its order
    parts = prow // B
    assert prow == B * parts
    per = (N + parts - 1) // parts
    padn = parts * per - N
    for tot in (a1, s2):
        rows = torch.nn.functional.pad(tot, (0, 0, 0, padn)).view(B, parts, per, Co).sum(dim=2)
        assert int(rows.max()) < 2 ** 24
    assert torch.equal(_bits(ysel), _bits((best + Q).float()))
    assert torch.equal(arg.long(), slot)
    # by value: a zero sum of a min channel is -0.0 (the kernel sums dir * P and
    # flips the sign back), which equals the restatement's +0.0
    assert torch.equal(sumP, sP.float())
    got = partials.double().sum(dim=0)                         # (2, Co): exact integers below 2^53
    assert torch.equal(got[0], s1.sum(dim=(0, 1)).double())
    assert torch.equal(got[1], s2.sum(dim=(0, 1)).double())


def _generic_cases():
    """One run per N; Co, k and B rotate (k = 64 is covered above)."""
    return [((1, 3)[i % 2], N, (20, 7, 40)[i % 3], COS[(i + 1) % 3], (1, 0, 4)[i % 3]) for i, N in enumerate(NS)]


@pytest.mark.parametrize("case", _generic_cases(), ids=_ids)
def test_gather_generic_data(cuda, case):
    """randn values: the selected value is a max of fp32 values and one fp32 add
    (exact against the same two operations), the slot the first extremal one;
    sum_k P within k 2^-24 sum_k |P_j| of the fp64 sum, the rounding bound of
    any order of k - 1 fp32 additions."""
    B, N, k, Co, pad = case
    PQ, idx, gamma = _inputs(case, cuda, integer=False)
    ysel, arg, sumP, _, _ = _run_gather(PQ, idx, gamma, B, N, k, Co)
    Pn, Q = _gathered(PQ, idx, B, N, k, Co, torch.float32)
    best, slot = _select(Pn, gamma < 0)
    assert torch.equal(_bits(ysel), _bits(best + Q))
    assert torch.equal(arg.long(), slot)
    ref = Pn.double().sum(dim=2)
    bound = k * 2.0 ** -24 * Pn.double().abs().sum(dim=2)
    assert bool(((sumP.double() - ref).abs() <= bound).all())


def _run_eval(PQ, idx, scale, shift, slope, B, N, k, Co, ldo):
    from dgx import _native as nat
    buf = torch.full((B * N, ldo), float("nan"), device=PQ.device)
    nat.check(nat.lib().dgx_edge_fwd_eval_f32(nat.f32(PQ), PQ.stride(0), nat.i32(idx), B, N, k, Co, nat.f32(scale),
                                              nat.f32(shift), slope, nat.f32(buf), ldo, nat.stream_of(PQ)),
              "edge eval")
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[:, Co:]).all())                # columns beyond Co are not written
    return buf[:, :Co].reshape(B, N, Co)


SLOPE = 0.25   # a power of two: the LeakyReLU product adds no rounding to the bounds below


# the six EVAL instantiations (CS 32, 16, 8, 4, 2, 1) and the large-LDS mode
EVAL_NS = [512, 1024, 1025, 4096, 4097, 8193, 16385]
assert sorted(_cs(N) for N in EVAL_NS) == [1, 1, 2, 4, 8, 16, 32] and max(EVAL_NS) > 16384


def _eval_cases():
    """Every EVAL instantiation once and the large-LDS mode, each Co, ldo a multiple of 4 and not."""
    return [((3, 1)[i % 2], N, (7, 20, 64)[i % 3], COS[i % 3], (4, 1, 0)[i % 3]) for i, N in enumerate(EVAL_NS)]


@pytest.mark.parametrize("integer", [True, False], ids=["integer", "randn"])
@pytest.mark.parametrize("case", _eval_cases(), ids=_ids)
def test_eval_form(cuda, case, integer):
    """out = LeakyReLU(fma(scale, extremal P + Q, shift)), the extremum chosen
    by the sign of scale. Integer data with scale and shift small integers
    times a power of two: every step is exact. randn data: within
    2^-23 (|scale y| + |shift|) of the fp64 value (the fp32 add y = P + Q and
    the fma's one rounding)."""
    B, N, k, Co, pad = case
    PQ, idx, _ = _inputs(case, cuda, integer)
    g = torch.Generator().manual_seed(N + Co)
    if integer:
        scale = torch.randint(-3, 4, (Co,), generator=g).float() * 0.25
        shift = torch.randint(-5, 6, (Co,), generator=g).float() * 0.125
        scale[0], scale[1] = -0.5, 0.75
    else:
        scale, shift = torch.randn(Co, generator=g), torch.randn(Co, generator=g)
    assert bool((scale < 0).any()) and bool((scale > 0).any())
    scale, shift = scale.to(cuda), shift.to(cuda)
    ldo = Co + (4 - Co % 4) % 4 + (4 if pad != 1 else 1)       # % 4 == 0 unless pad == 1
    out = _run_eval(PQ, idx, scale, shift, SLOPE, B, N, k, Co, ldo)
    Pn, Q = _gathered(PQ, idx, B, N, k, Co, torch.float32)
    best, _ = _select(Pn, scale < 0)
    y = (best + Q).double() if integer else best.double() + Q.double()
    z = scale.double() * y + shift.double()
    ref = torch.where(z > 0, z, z * SLOPE)
    if integer:
        assert torch.equal(_bits(out), _bits(ref.float()))
    else:
        bound = 2.0 ** -23 * ((scale.double() * y).abs() + shift.double().abs())
        assert bool(((out.double() - ref).abs() <= bound).all())


@pytest.mark.parametrize("N", [1024, 1025, 4096, 8193])
def test_eval_form_returns_nan_neighbour(cuda, N):
    """The ordered '>' passes over a NaN neighbour; the reference's max returns
    it. At CS 16, 8 (two channels per thread), 4 and 1 (the TPP = CS split): every
    centre that lists the NaN point gets NaN in that channel only."""
    B, k, Co = 1, 7, 6
    PQ, idx, _ = _inputs((B, N, k, Co, 0), cuda, integer=True)
    PQ = PQ.clone()
    PQ[N // 3, 4] = float("nan")
    scale = torch.tensor([1.0, -1.0, 0.5, 2.0, -0.5, 1.0], device=cuda)
    out = _run_eval(PQ, idx, scale, torch.zeros(Co, device=cuda), SLOPE, B, N, k, Co, Co)
    hit = (idx.long() == N // 3).any(dim=2)                     # (B, N)
    assert bool(hit.any()) and not bool(hit.all())
    want = torch.zeros(B, N, Co, dtype=torch.bool, device=cuda)
    want[..., 4] = hit
    assert torch.equal(torch.isnan(out), want)
