"""The EdgeConv BatchNorm oracle (tests/_edgebn_ref.py) checked on the CPU: fed
exact per-block sums of a tiny fp64 edge tensor y (B, Co, N, k), its finalize
reproduces the batch statistics and the running-statistics update of
nn.BatchNorm2d in double, and its dz / bwd_consts chain reproduces autograd's
gradients of BatchNorm2d -> LeakyReLU(0.2) -> max(dim=-1) (reference
models/dgcnn.py:54-98), in train and in eval mode, to 1e-12; the rounding
helpers and the lattice data the GPU file uses meet their stated properties."""
import itertools

import pytest
import torch

import _edgebn_ref as R

TOL = 1e-12
F64 = torch.float64


def _rel(got, want):
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-300))


def _edges(y):
    """(B, Co, N, k) -> edge-major (B N k, Co)"""
    return y.permute(0, 2, 3, 1).reshape(-1, y.shape[1])


def _block_sums(y, rows=5):
    """exact-in-fp64-terms per-block (sum y, sum y^2) partial rows of the edge tensor"""
    e = _edges(y.detach())
    nblk = -(-e.shape[0] // rows)
    blk = torch.arange(e.shape[0]) // rows
    return torch.stack([R.rowsum(e, blk, nblk), R.rowsum(e * e, blk, nblk)], 1)


def _module(Co, g, momentum=0.1, track=True, eps=1e-5):
    bn = torch.nn.BatchNorm2d(Co, eps=eps, momentum=momentum, track_running_stats=track).double()
    with torch.no_grad():
        bn.weight.copy_(torch.randn(Co, generator=g, dtype=F64))
        bn.weight[0], bn.weight[-1] = bn.weight[0].abs(), -bn.weight[-1].abs()   # mixed sign
        bn.bias.copy_(0.3 * torch.randn(Co, generator=g, dtype=F64))
        if track:
            bn.running_mean.copy_(torch.randn(Co, generator=g, dtype=F64))
            bn.running_var.copy_(torch.rand(Co, generator=g, dtype=F64) + 0.5)
    return bn


@pytest.mark.parametrize("momentum,track,steps", [(0.1, True, 1), (None, True, 2), (0.1, False, 1)])
@pytest.mark.parametrize("B,Co,N,k", [(2, 5, 7, 3), (1, 3, 1, 2)])
def test_finalize_equals_batchnorm2d(B, Co, N, k, momentum, track, steps):
    g = torch.Generator().manual_seed(B + Co + N)
    bn = _module(Co, g, momentum, track).train()
    for _ in range(steps):
        y = torch.randn(B, Co, N, k, generator=g, dtype=F64) * 1.5 + 0.7
        rm, rv = (bn.running_mean.clone(), bn.running_var.clone()) if track else (None, None)
        nbt = int(bn.num_batches_tracked) if track else None
        z = bn(y)
        r = R.finalize(_block_sums(y), B * N * k, bn.weight, bn.bias, rm, rv, -1.0 if momentum is None else momentum,
                       bn.eps, nbt)
        e = _edges(y)
        assert _rel(r.mean, e.mean(0)) < TOL and _rel(r.var, e.var(0, unbiased=False)) < TOL
        assert _rel(r.invstd, (e.var(0, unbiased=False) + bn.eps).rsqrt()) < TOL
        zz = r.scale.view(1, Co, 1, 1) * y + r.shift.view(1, Co, 1, 1)
        assert _rel(zz, z.detach()) < TOL
        if track:
            assert _rel(r.rm, bn.running_mean) < TOL and _rel(r.rv, bn.running_var) < TOL
            assert r.nbt == int(bn.num_batches_tracked)
        else:
            assert r.rm is None and r.rv is None and r.nbt is None


def test_finalize_count_one():
    """One sample per channel: nn.BatchNorm2d refuses it in training mode; the
    native batch_norm still normalises (var = 0, output = beta) and the engine's
    documented rule keeps the biased value for the running variance."""
    g = torch.Generator().manual_seed(3)
    Co, eps = 4, 1e-5
    y = torch.randn(1, Co, 1, 1, generator=g, dtype=F64)
    gamma, beta = torch.randn(Co, generator=g, dtype=F64), torch.randn(Co, generator=g, dtype=F64)
    rm, rv = torch.randn(Co, generator=g, dtype=F64), torch.rand(Co, generator=g, dtype=F64) + 0.5
    z = torch.batch_norm(y, gamma, beta, None, None, True, 0.1, eps, False)
    r = R.finalize(_block_sums(y), 1, gamma, beta, rm, rv, 0.1, eps, 0)
    # the given sum y^2 is the ROUNDED square: the exact var is its rounding error (or 0 after the clamp)
    assert float(r.var.abs().max()) < 2.0 ** -50 and _rel(r.invstd, torch.full((Co,), eps ** -0.5, dtype=F64)) < 2.0 ** -50 / eps
    assert float((r.scale * y.view(Co) + r.shift - z.view(Co)).abs().max()) < 1e-9   # a ~ 316: y a cancels to beta
    assert _rel(r.rm, 0.9 * rm + 0.1 * y.view(Co)) < TOL and _rel(r.rv, 0.9 * rv) < TOL and r.nbt == 1


@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("B,Co,N,k", [(2, 5, 7, 3), (1, 3, 2, 4), (3, 6, 5, 1)])
def test_dz_and_bwd_consts_equal_autograd(B, Co, N, k, train):
    g = torch.Generator().manual_seed(B * N + k)
    eps = 2.0 ** -17                                  # an fp32 value: eval_affine's (float)eps changes nothing
    bn = _module(Co, g, eps=eps)
    bn = bn.train() if train else bn.eval()
    y = (torch.randn(B, Co, N, k, generator=g, dtype=F64) * 1.5 + 0.7).requires_grad_(True)
    gout = torch.randn(B, Co, N, generator=g, dtype=F64)
    rm, rv = bn.running_mean.clone(), bn.running_var.clone()
    out, arg = torch.nn.functional.leaky_relu(bn(y), 0.2).max(dim=-1)
    out.backward(gout)
    M, count = B * N, B * N * k
    with torch.no_grad():
        if train:
            st = R.finalize(_block_sums(y), count, bn.weight, bn.bias, None, None, 0.1, eps, None)
        else:
            st = R.eval_affine(bn.weight, bn.bias, rm, rv, eps)
            st.mean = rm
        pm = lambda t: t.permute(0, 2, 1).reshape(M, Co)                       # (B, Co, N) -> point-major
        ysel = pm(torch.gather(y.detach(), 3, arg.unsqueeze(-1)).squeeze(-1))
        zs = st.scale * ysel + st.shift
        assert _rel(torch.where(zs > 0, zs, 0.2 * zs), pm(out.detach())) < TOL
        d, _, _ = R.dz(pm(gout), ysel, st.scale, st.shift, 0.2, f32=False)
        nrows = 3
        part, _, _ = R.dz_partials(d, ysel, st.mean, st.invstd, R.row_blocks(M, nrows), nrows)
        c = R.bwd_consts(part, count, st.scale, st.mean, st.invstd, 0, eval=not train)
        if not train:
            assert float(c.c0.abs().max()) == 0.0 and float(c.c1.abs().max()) == 0.0
        sel = torch.zeros(B, Co, N, k, dtype=F64).scatter_(3, arg.unsqueeze(-1), 1.0)
        v = lambda t: t.view(1, Co, 1, 1)
        dzf = (st.scale * d).view(B, N, Co).permute(0, 2, 1).unsqueeze(-1)
        dy = dzf * sel + v(c.c0) + v(c.c1) * y.detach()
    assert _rel(dy, y.grad) < TOL
    assert _rel(c.dgamma, bn.weight.grad) < TOL and _rel(c.dbeta, bn.bias.grad) < TOL


def test_bwd_consts_accumulates_and_reads_the_device_count():
    c = R.make_bwdfin_case("random", 5, 7, seed=1, f64=True)
    a = R.bwd_consts(c.partials, c.count, c.scale, c.mean, c.invstd, 0)
    b = R.bwd_consts(R.with_count(c.partials, c.count), -1.0, c.scale, c.mean, c.invstd, 1, c.prev, co=5)
    assert torch.equal(a.c0, b.c0) and torch.equal(a.c1, b.c1)
    assert torch.equal(b.dgamma, a.dgamma + c.prev[0].double()) and torch.equal(b.dbeta, a.dbeta + c.prev[1].double())


def test_fl32_is_one_rounding_of_the_exact_sum():
    """fl32(TwoSum) against exact rational arithmetic, on random data and on
    planted midpoints where the fp64 sum rounds the other way."""
    from fractions import Fraction
    g = torch.Generator().manual_seed(0)
    a, y, b = (torch.randn(4000, generator=g) for _ in range(3))
    # a y = 1 + 2^-11 + 2^-24 is exactly the midpoint of two fp32 neighbours and b = +-2^-60 vanishes in the
    # fp64 sum: rounding that sum to nearest-even goes the wrong way for one sign of b
    y[:8] = 1.0 + 2.0 ** -12
    a[:8] = torch.tensor([1.0, 1.0, 1.0, 1.0, -1.0, -1.0, -1.0, -1.0]) * (1.0 + 2.0 ** -12)
    b[:8] = torch.tensor([2.0 ** -60, -2.0 ** -60, 2.0 ** -80, -2.0 ** -80] * 2)
    s, e = R.affine(y, a, b)
    got = R.fl32(s, e)
    for i in range(a.numel()):
        q = Fraction(float(a[i])) * Fraction(float(y[i])) + Fraction(float(b[i]))
        f = torch.tensor(float(s[i])).float()
        cands = [float(f), float(torch.nextafter(f, torch.tensor(float("inf")))),
                 float(torch.nextafter(f, torch.tensor(float("-inf"))))]
        best = min(abs(Fraction(c) - q) for c in cands)
        near = [c for c in cands if abs(Fraction(c) - q) == best]
        assert float(got[i]) in near, i
        if len(near) == 1:
            assert float(got[i]) == near[0]
    assert bool((got[:8] != s[:8].float().double()).any())


@pytest.mark.parametrize("count", [1, 2, 4])
@pytest.mark.parametrize("Co,nrows", [(1, 1), (5, 65), (130, 1024)])
def test_finalize_lattice_outputs_fit_fp32(Co, nrows, count):
    for f64, nbt in itertools.product((False, True), (None, 0, 1, 3)):
        c = R.make_finalize_case("lattice", Co, nrows, count, seed=1, f64=f64)
        r = R.finalize(c.partials, c.count, c.gamma, c.beta, c.rm, c.rv, c.momentum if nbt is None else -1.0, c.eps, nbt)
        assert R.fits_f32(r.scale, r.shift, r.mean, r.invstd, r.rm, r.rv)
        cc = R.clamp_channel(Co)
        assert float(r.var[cc]) == 0.0 and float(r.invstd[cc]) == 2.0
        if Co > 3:
            assert set(r.invstd[:cc].tolist()) == {1.0, 0.5, 0.25}


def test_random_finalize_case_clamps_and_spans_r():
    c = R.make_finalize_case("random", 5, 64, 0, seed=2)
    r = R.finalize(c.partials, c.count, c.gamma, c.beta, c.rm, c.rv, 0.1, c.eps, 0)
    assert float(r.var[4]) == 0.0 and abs(float(r.invstd[4]) - c.eps ** -0.5) < 1e-9
    ratio = (r.mean.abs() * r.invstd)[:4]
    assert float(ratio[0]) < 0.5 and 3 < float(ratio[1]) < 5 and 50 < float(ratio[2]) < 80


def test_edge_lattice_is_exact_and_has_zeros():
    for M, nrows, Co, _ in R.DZ_GRID:
        c = R.make_edge_case("lattice", M, Co, seed=3)
        d, pos, zero = R.dz(c.dY, c.ysel, c.scale, c.shift, c.slope)
        assert bool(zero.any(0).all()) and not bool((zero & pos).any())
        assert bool((d[zero] == c.dY.double()[zero] * c.slope).all())          # the slope branch at z == 0
        _, _, mag = R.dz_partials(d, c.ysel, c.mean, c.invstd, R.row_blocks(M, nrows), nrows)
        R.assert_dz_exact(mag)
        assert set(c.arg.view(-1).tolist()) <= set(range(64)) and (M * Co < 64 or int(c.arg.max()) == 63)
    for B, N, Co in R.CM_GRID:
        c = R.make_edge_case("lattice", B * N, Co, seed=4)
        d, _, _ = R.dz(c.dY, c.ysel, c.scale, c.shift, c.slope)
        blocks, nrows = R.cm_blocks(B, N)
        R.assert_dz_exact(R.dz_partials(d, c.ysel, c.mean, c.invstd, blocks, nrows)[2])


def test_bwdfin_lattice_outputs_fit_fp32():
    for (Co, nrows), f64 in itertools.product(R.FIN_GRID, (False, True)):
        c = R.make_bwdfin_case("lattice", Co, nrows, seed=5, f64=f64)
        r = R.bwd_consts(c.partials, c.count, c.scale, c.mean, c.invstd, 1, c.prev)
        assert R.fits_f32(r.dgamma, r.dbeta, r.c0, r.c1)


def test_row_blocks_and_grids_cover_the_edges():
    # rows per block 1, 64, 33, 44, 63, 34; ragged last blocks; blocks entirely past M
    assert [-(-M // nr) for M, nr in R.DZ_ROWS] == [1, 1, 64, 33, 44, 63, 34]
    assert any(M % -(-M // nr) for M, nr in R.DZ_ROWS)
    assert any(int(R.row_blocks(M, nr).max()) + 1 < nr for M, nr in R.DZ_ROWS)
    assert {co for _, _, co, _ in R.DZ_GRID} == set(R.DZ_COS) and {p for *_, p in R.DZ_GRID} == {0, 3, 64}
    for M, nr in R.DZ_ROWS:
        assert {co for m, n, co, _ in R.DZ_GRID if (m, n) == (M, nr)} == set(R.DZ_COS)
    assert {b for b, _, _ in R.CM_GRID} == set(R.CM_BS) and {n for _, n, _ in R.CM_GRID} == set(R.CM_NS)
    assert {co for *_, co in R.CM_GRID} == set(R.DZ_COS)
    blocks, nrows = R.cm_blocks(3, 130)
    assert nrows == 9 and blocks.tolist()[128:132] == [2, 2, 3, 3]
    assert [R.compact_slabs(r) for r in R.COMPACT_ROWS] == [0, 8, 8, 9]
    assert [r - 128 * (r // 128) for r in R.COMPACT_ROWS[1:]] == [1, 127, 0]
    # the apply grid: which kernel the host must pick, from the documented alignment rule
    for M, Co, ldo, twin, oo, oy, ot, v4 in R.APPLY_GRID:
        assert v4 == (Co % 4 == 0 and ldo % 4 == 0 and oo % 4 == 0 and oy % 4 == 0 and (not twin or ot % 4 == 0))
    for M, Co, ldo, _ in R.APPLY_STRIDE_GRID:
        per = 4 if Co % 4 == 0 else 1
        assert 8192 * 256 < M * Co // per < 1.1 * 8192 * 256      # some threads take a second element, most do not
