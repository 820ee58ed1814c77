"""The edge-MLP oracle (tests/_edgemlp_ref.py) checked on the CPU: its chain of
restatements, without the bf16 roundings, equals fp64 autograd of the reference
op sequence (oracle.reference.graph_feature -> conv1 -> conv2 -> max,
reference models/layers.py:45-52); every lattice case the GPU file runs meets
its exactness conditions; the geometry grids cover what they claim; the Python
reverse-graph builder equals a brute-force enumeration."""
import itertools

import pytest
import torch
import torch.nn.functional as F

import _edgemlp_ref as R
from oracle import reference as O


def _chain(B, N, k, C, C2, seed, slope=0.2, eps=1e-5):
    """(autograd gradients, restatement-chain gradients) of the stage, fp64"""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    x = rn(B, C, N).requires_grad_(True)
    w1, w2 = (0.5 * rn(R.C1, 2 * C)).requires_grad_(True), (0.2 * rn(C2, R.C1)).requires_grad_(True)
    g1, b1, g2, b2 = [t.requires_grad_(True) for t in (rn(R.C1), 0.1 * rn(R.C1), rn(C2), 0.1 * rn(C2))]
    idx = R.make_idx(g, B, N, k).long().view(B, N, k)
    gout = rn(B, C2, N)
    e = O.graph_feature(x, idx=idx)
    z1 = F.batch_norm(F.conv2d(e, w1.view(R.C1, 2 * C, 1, 1)), None, None, g1, b1, True, 0.1, eps)
    z2 = F.batch_norm(F.conv2d(F.leaky_relu(z1, slope), w2.view(C2, R.C1, 1, 1)), None, None, g2, b2, True, 0.1, eps)
    out = F.leaky_relu(z2, slope).max(dim=-1)[0]
    out.backward(gout)
    want = {"out": out.detach(), "x": x.grad, "w1": w1.grad, "g1": g1.grad, "b1": b1.grad, "w2": w2.grad,
            "g2": g2.grad, "b2": b2.grad}
    # the same through the restatements
    with torch.no_grad():
        M, E = B * N, B * N * k
        X = x.permute(0, 2, 1).reshape(M, C)
        PQ = torch.cat([X @ w1[:, :C].t(), X @ w1[:, C:].t()], 1)
        c = R.Case()
        c.kind, c.B, c.N, c.k, c.C2, c.M, c.E, c.slope = "chain", B, N, k, C2, M, E, slope
        c.PQg = torch.cat([PQ, torch.full((1, 2 * R.C1), float("nan"), dtype=torch.float64)])
        c.idxg = idx.view(M, k).int()
        i, j = R.edge_ij(c.idxg, B, N, k)
        y = PQ[:, :R.C1][j] + PQ[:, R.C1:][i]
        mean1, var1 = y.mean(0), y.var(0, unbiased=False)
        c.mean1, c.invstd1 = mean1, (var1 + eps).rsqrt()
        c.a1 = g1 * c.invstd1
        c.b1 = b1 - c.a1 * mean1
        c.W2, c.dir2 = w2.detach(), torch.sign(g2)
        r = R.Ref(c, rounding=False)
        mean2 = r.part2[:, 0].sum(0) / E
        var2 = r.part2[:, 1].sum(0) / E - mean2 ** 2
        is2 = (var2 + eps).rsqrt()
        a2 = g2 * is2
        zs = a2 * r.ysel + (b2 - a2 * mean2)
        got = {"out": torch.where(zs > 0, zs, slope * zs).view(B, N, C2).permute(0, 2, 1)}
        dz = gout.permute(0, 2, 1).reshape(M, C2) * R.lrelu_grad(zs > 0, slope)
        got["b2"] = dz.sum(0)
        got["g2"] = (dz * (r.ysel - mean2) * is2).sum(0)
        k1 = -a2 * got["g2"] * is2 / E
        r.backward(r.arg, dz, -a2 * got["b2"] / E - k1 * mean2, k1, a2)
        got["w2"] = r.dW2
        got["b1"], got["g1"] = r.bwd.part[:, 0].sum(0), r.bwd.part[:, 1].sum(0)
        s = R.Case()
        s.kind, s.B, s.N, s.k, s.C, s.M, s.E = "chain", B, N, k, R.C1, M, E
        s.PQg, s.g, s.a = c.PQg, r.bwd.g, c.a1
        s.c1 = -c.a1 * got["g1"] * c.invstd1 / E
        s.c0 = -c.a1 * got["b1"] / E - s.c1 * mean1
        s.sumP = PQ[:, :R.C1][j].view(M, k, R.C1).sum(1)
        s.rowptr, s.edges = R.graph_reverse(c.idxg, B, N, k)
        dPQ, _, _ = R.scatter_ref(s)
        dP, dQ = dPQ[:, :R.C1], dPQ[:, R.C1:]
        got["x"] = (dP @ w1[:, :C] + dQ @ w1[:, C:]).view(B, N, C).permute(0, 2, 1)
        got["w1"] = torch.cat([dP.t() @ X, dQ.t() @ X], 1)
    return want, got


@pytest.mark.parametrize("B,N,k,C,C2", [(1, 5, 3, 3, 64), (2, 9, 17, 3, 128), (3, 20, 4, 6, 128)])
def test_restatement_chain_equals_fp64_autograd(B, N, k, C, C2):
    want, got = _chain(B, N, k, C, C2, seed=B + N)
    for name in want:
        err = float((got[name] - want[name]).abs().max() / want[name].abs().max().clamp_min(1e-300))
        assert err < 1e-12, (name, err)


def test_first_slot_on_ties():
    c = R.make_case("lattice", 1, 4, 17, 64, 0)
    r = R.Ref(c)
    v = r.v
    for p, ch in itertools.product(range(c.M), (0, 5, 63)):
        col = v[p, :, ch].tolist()
        assert int(r.arg[p, ch]) == col.index(max(col))
    assert bool(((v == r.best.unsqueeze(1)).sum(1) > 1).any()), "lattice data should tie"


LATTICE = sorted({(B, N, k, C2, pad) for B, N, k, C2, _, pad in R.FWD_GRID} |
                 {(B, N, k, 128, pad) for B, N, k, pad in R.BWD_GRID} |
                 {(B, N, k, C2, 0) for B, N, k, C2 in R.GEMM_GRID} | {(2, 130, 17, 128, 0), (2, 130, 64, 128, 0)})


@pytest.mark.parametrize("B,N,k,C2,pad", LATTICE)
def test_lattice_cases_meet_their_exactness_conditions(B, N, k, C2, pad):
    c = R.make_case("lattice", B, N, k, C2, seed=1, pad=pad)
    R.assert_exact(c, R.Ref(c))


def test_lattice_plants_duplicates_zeros_and_self_edges():
    c = R.make_case("lattice", 2, 17, 33, 128, seed=1)
    idx = c.idxg[:c.M].long()
    n = torch.arange(c.M) % c.N
    assert bool((idx[:, 0] == n).any())
    assert bool((idx[:, 32] == idx[:, 0]).any()) and bool((idx[:, 16] == idx[:, 1]).any())
    r = R.Ref(c)
    assert bool((r.z1 == 0).any())
    arg = c.argg[:c.M].long()
    assert bool((arg[:, 0] == 0).all()) and bool((arg[:, 1] == c.k - 1).all())
    assert all(len(set(row.tolist())) == 4 for row in arg[:, 4:8])


def test_scatter_and_h1bwd_lattice_cases_are_exact():
    for gb, C, B, N, k, graph, pad, off in R.SCATTER_GRID:
        c = R.make_scatter_case("lattice", B, N, k, C, seed=2, graph=graph, pad=pad)
        R.assert_scatter_exact(c)
        if graph == "degrees":
            deg = (c.rowptr[1:] - c.rowptr[:-1]).view(B, N)
            assert deg[:, 1:9].tolist() == [c.want_deg] * B and bool((deg[:, 0] == 0).all())
    for B, N, k, C in R.H1BWD_GRID:
        c = R.make_h1bwd_case("lattice", B, N, k, C, seed=3)
        R.h1bwd_f32_ref(c, max(1, min(2048, -(-c.E // (256 // (C // 4) * 8)))))


@pytest.mark.parametrize("name", ["FWD_GRID", "BWD_GRID"])
def test_grids_pair_every_value_with_two_of_every_other_axis(name):
    grid = getattr(R, name)
    Ns = R.FWD_NS if name == "FWD_GRID" else R.BWD_NS
    axes = {"B": R.BS, "N": Ns, "k": R.KS, "pad": (0, 4)}
    if name == "FWD_GRID":
        axes.update({"C2": (64, 128), "h1": (False, True)})
    names = R.AXES if name == "FWD_GRID" else ("B", "N", "k", "pad")
    col = {a: names.index(a) for a in axes}
    for a, b in itertools.permutations(axes, 2):
        for va in axes[a]:
            seen = {case[col[b]] for case in grid if case[col[a]] == va}
            assert len(seen) >= min(2, len(axes[b])), (a, va, b, seen)
    # one B < 8 case whose tile count rep = 8 // B does not divide
    ppb = 8 if name == "FWD_GRID" else 64
    assert any(B < 8 and -(-N // ppb) % (8 // B) for B, N, *_ in grid)
    # rep = 8, 4, 2, padding blocks (rep * B < 8), the B >= 8 form, a second round of clouds
    assert {1, 2, 3, 5, 8, 9} <= {case[0] for case in grid}


def test_gemm_grid_covers_the_tile_edges():
    Es = {B * N * k for B, N, k, _ in R.GEMM_GRID}
    assert {7, 64, 127, 128, 129, 272} <= Es
    assert {1, 7, 40, 64} == {k for _, _, k, _ in R.GEMM_GRID}
    assert {64, 128} == {C2 for *_, C2 in R.GEMM_GRID}
    # a cloud boundary strictly inside a 128-row tile
    assert any(B == 3 and (N * k) % 128 for B, N, k, _ in R.GEMM_GRID)


@pytest.mark.parametrize("B,N,k", [(1, 1, 1), (2, 7, 3), (3, 20, 64)])
def test_graph_reverse_equals_brute_force(B, N, k):
    g = torch.Generator().manual_seed(N)
    idx = R.make_idx(g, B, N, k)
    rowptr, edges = R.graph_reverse(idx, B, N, k)
    flat = idx.view(-1).tolist()
    lists = [[] for _ in range(B * N)]
    for i in range(B * N):
        for s in range(k):
            lists[(i // N) * N + flat[i * k + s]].append((i << 6) | s)
    assert rowptr.tolist() == [0] + list(itertools.accumulate(len(l) for l in lists))
    assert edges.tolist() == [e for l in lists for e in sorted(l)]
