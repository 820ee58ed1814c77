"""a1 parity for EVERY selection kernel the kNN dispatcher can choose
(csrc/knn.hip dispatch_k / launch_knn): knn_kernel<NSTEP, KB, QG> for NSTEP in
{1, 3, 8, 16, 32} x KB in {16, 20, 32, 40, 64} with one query group per wave,
plus the four two-group forms at NSTEP 32, KB <= 40 — 29 instantiations, each
compared bit for bit with the CPU oracle on generic features, on a clustered
cloud built to overflow the per-lane lists (the exact fix-up pass) and on a
cloud with duplicated points.

The table's self-check is a CPU test: a change of the tiers that leaves an
instantiation without a case fails without a GPU."""
import numpy as np
import pytest
import torch

import oracle
from _shapes import KNN_CHANNELS
from conftest import assert_knn_equivalent
from dgx import synth

NSTEPS = (1, 3, 8, 16, 32)
KBS = (16, 20, 32, 40, 64)

# (B, C, N, k, (NSTEP, KB, QG)): C at a tier's edge or ragged, k at a list
# size's edge, N ragged unless noted. QG 2 needs NSTEP 32, KB <= 40 AND a grid
# of at least 512 workgroups at 32 queries each (not knn_small): B = 16 at
# N ~ 1000 is the smallest such batch; every other entry stays below it.
CASES = [
    # ---- NSTEP 1 (C <= 4): the values-only admission pre-pass runs here
    (2, 4, 77, 16, (1, 16, 1)),
    (2, 3, 77, 1, (1, 16, 1)),            # k = 1
    (2, 3, 300, 17, (1, 20, 1)),
    # FIX_MAXN: the largest cloud of the fused kernel, the fix-up's tie bitmap at full size
    (1, 3, 12288, 20, (1, 20, 1)),
    (2, 2, 200, 21, (1, 32, 1)),
    (1, 4, 333, 32, (1, 32, 1)),
    (2, 1, 150, 33, (1, 40, 1)),
    (1, 3, 520, 40, (1, 40, 1)),
    (2, 4, 130, 41, (1, 64, 1)),
    (1, 3, 64, 64, (1, 64, 1)),           # k = N
    # ---- NSTEP 3 (5 <= C <= 12)
    (2, 5, 129, 16, (3, 16, 1)),
    (1, 12, 100, 1, (3, 16, 1)),          # k = 1
    (2, 12, 200, 17, (3, 20, 1)),
    (2, 9, 333, 20, (3, 20, 1)),
    (1, 12, 96, 21, (3, 32, 1)),
    (2, 5, 257, 32, (3, 32, 1)),
    (2, 12, 150, 33, (3, 40, 1)),
    (2, 9, 300, 40, (3, 40, 1)),
    (2, 12, 77, 41, (3, 64, 1)),
    (2, 5, 100, 64, (3, 64, 1)),
    (1, 9, 50, 50, (3, 64, 1)),           # k = N
    # ---- NSTEP 8 (13 <= C <= 32)
    (2, 13, 129, 16, (8, 16, 1)),
    (1, 32, 77, 1, (8, 16, 1)),           # k = 1
    (1, 17, 300, 17, (8, 20, 1)),
    (2, 32, 200, 20, (8, 20, 1)),
    (2, 13, 257, 21, (8, 32, 1)),
    (2, 32, 333, 32, (8, 32, 1)),
    (2, 24, 150, 33, (8, 40, 1)),
    (1, 32, 520, 40, (8, 40, 1)),
    (1, 13, 40, 40, (8, 40, 1)),          # k = N
    (2, 13, 100, 41, (8, 64, 1)),
    (2, 32, 130, 64, (8, 64, 1)),
    # ---- NSTEP 16 (33 <= C <= 64)
    # The unit past the end of the operand ring. At NSTEP 16 a tile is SPT = 2
    # units of SW = 8 MFMA steps; with KB <= 20 the ring holds RING = 4 units
    # and a loop trip runs UB = max(RING, SPT) = 4 units = 2 tiles. A wave
    # serves the tiles h, h + 2, ... of its half h: ntl = ceil((N/16 - h) / 2)
    # of them. nunits = 2 ntl is no multiple of UB exactly when ntl is odd, and
    # the last trip then runs one whole tile past the half's end (it re-reads
    # the last tile; its candidates must all fail j < N). N % 16 == 0 keeps the
    # cloud's real last tile full, so only that phantom tile takes the padded
    # form. N = 16 * 38 = 608: ntl = 19 for both halves, 19 workgroups;
    # N = 16 * 6 = 96: ntl = 3 for both. (From KB 32 on RING = 2 and UB = SPT,
    # and at NSTEP 32 SPT = UB = 4: nunits is always a multiple of UB there.)
    (2, 33, 608, 16, (16, 16, 1)),
    (1, 64, 77, 1, (16, 16, 1)),          # k = 1
    (1, 64, 96, 20, (16, 20, 1)),
    (2, 64, 200, 17, (16, 20, 1)),
    (2, 40, 257, 21, (16, 32, 1)),
    (1, 64, 300, 32, (16, 32, 1)),
    (2, 33, 150, 33, (16, 40, 1)),
    (2, 64, 333, 40, (16, 40, 1)),
    (2, 64, 130, 41, (16, 64, 1)),
    (1, 33, 200, 64, (16, 64, 1)),
    (1, 33, 48, 48, (16, 64, 1)),         # k = N
    # ---- NSTEP 32 (65 <= C <= 128), small grids: one query group per wave
    (2, 65, 129, 16, (32, 16, 1)),
    (1, 128, 77, 1, (32, 16, 1)),         # k = 1
    (1, 68, 257, 17, (32, 20, 1)),
    (2, 128, 200, 20, (32, 20, 1)),
    (2, 128, 150, 21, (32, 32, 1)),
    (1, 100, 333, 32, (32, 32, 1)),
    (2, 68, 200, 33, (32, 40, 1)),
    (2, 128, 520, 40, (32, 40, 1)),
    (1, 65, 33, 33, (32, 40, 1)),         # k = N
    (2, 65, 100, 41, (32, 64, 1)),
    (1, 128, 300, 64, (32, 64, 1)),
    # ---- NSTEP 32, two query groups per wave (B * ceil(N / 32) >= 512)
    (16, 65, 1000, 16, (32, 16, 2)),
    (16, 128, 1000, 17, (32, 20, 2)),
    (16, 68, 1001, 32, (32, 32, 2)),
    (16, 128, 1024, 40, (32, 40, 2)),     # block 4 at cfg3 / cfg4: C 128, k 40, N % 32 == 0
]

EXPECTED = {(ns, kb, 1) for ns in NSTEPS for kb in KBS} | {(32, kb, 2) for kb in (16, 20, 32, 40)}


def _knn_small(B, N):
    """csrc/knn.hip knn_small restated: fewer than 512 workgroups at 32 queries
    each keep one query group per wave whatever the kernel name says."""
    return B * ((N + 31) // 32) < 512


def _taken(B, C, N, k):
    """(NSTEP, KB, QG) of the kernel the library launches: the name's tiers, and
    the query groups from dgx_knn_query_groups — the dispatcher's own rule
    (launch_knn runs the same function), which the restatement must match."""
    from dgx import _native as nat
    L = nat.lib()
    name = L.dgx_knn_kernel_name(C, k, N).decode()
    assert name.startswith("knn_kernel<") and name.endswith(">"), name
    ns, kb, qg = (int(v) for v in name[len("knn_kernel<"):-1].split(","))
    launched = L.dgx_knn_query_groups(B, C, k, N)
    assert launched == (1 if _knn_small(B, N) else qg), (B, C, N, k)
    return ns, kb, launched


def test_case_table_reaches_every_instantiation():
    """Not a GPU test: every entry selects the kernel it names, and the table
    as a whole selects all 29 the dispatcher can launch — no more, no fewer."""
    taken = set()
    for B, C, N, k, want in CASES:
        assert _taken(B, C, N, k) == want, (B, C, N, k)
        taken.add(want)
    assert taken == EXPECTED and len(EXPECTED) == 29
    for ns in NSTEPS:   # k = 1 and k = N once per channel tier
        assert any(w[0] == ns and k == 1 for _, _, _, k, w in CASES), ns
        assert any(w[0] == ns and k == N for _, _, N, k, w in CASES), ns
    ns16 = [(N, w) for _, _, N, _, w in CASES if w[0] == 16 and w[1] <= 20 and N % 16 == 0]
    assert any(((N // 16 + 1) // 2) % 2 == 1 and ((N // 16) // 2) % 2 == 1 for N, _ in ns16)   # odd ntl, both halves
    assert any(N % 32 for _, _, N, _, _ in CASES) and (1, 3, 12288, 20, (1, 20, 1)) in CASES


def _data(kind, B, C, N, k):
    seed = 9000 + 131 * C + 7 * N + k
    if kind == "relu_normal":
        return synth.relu_normal(seed, (B, N, C))
    if kind == "lane_clustered":
        # test_knn_gpu's cloud: a tight cluster on a quarter of the indices, built
        # to crowd a query's neighbours into few of its per-lane lists so that
        # they overflow and the row is redone exactly (knn_fix_row). Whether a
        # row overflows depends on N and k, and nothing here counts flagged rows:
        # where none is, the cloud is one more kind of adversarial data.
        from test_knn_gpu import _lane_clustered
        return np.concatenate([_lane_clustered(N, C, seed + 17 * b) for b in range(B)], 0)
    if kind == "duplicates":       # an eighth of the points twice: exact ties, some at the k-th value
        # A candidate's list is chosen by its tile's parity and its index mod 4
        # (knn_row), so a copy 32 m points further on lands in the SAME per-lane
        # list as its original (the order of equal values inside a list), while
        # other distances put the pair in different lists (the canonical merge).
        pts = synth.uniform(seed, (B, N, C)).astype(np.float32) - np.float32(0.5)
        n16 = N // 16
        far = (N // 2) // 32 * 32
        if n16 >= 1 and far >= 2 * n16 and far + n16 <= N - n16:
            pts[:, far:far + n16] = pts[:, :n16]                      # a sixteenth 32 m further on: same list
            pts[:, N - n16:] = pts[:, n16:2 * n16]                    # another sixteenth at the cloud's end
        else:                                                         # (clouds of fewer than 64 points)
            pts[:, N // 2:N // 2 + N // 8] = pts[:, :N // 8]
        return pts
    raise ValueError(kind)


def _id(c):
    B, C, N, k, (ns, kb, qg) = c
    return f"ns{ns}kb{kb}qg{qg}-B{B}C{C}N{N}k{k}"


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["relu_normal", "lane_clustered", "duplicates"])
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_knn_instantiation_vs_oracle(cuda, case, kind):
    """Selected values bit-equal, indices equal (both are canonical: value
    descending, index ascending), int32 and int64 outputs equal."""
    from dgx.ops import knn_raw
    B, C, N, k, want = case
    pts = _data(kind, B, C, N, k)
    cheap = B * N * N * C <= 10 ** 8   # all but FIX_MAXN and the two-group batches
    for layout in (("bcn", "perm") if cheap else ("bcn",)):
        f = torch.from_numpy(pts).permute(0, 2, 1)
        if layout == "bcn":
            f = f.contiguous()
        x = f.to(cuda)
        ref_idx, ref_vals = oracle.knn(f, k, return_values=True)
        idx, vals = knn_raw(x, k, return_values=True)
        i32 = knn_raw(x, k, out_dtype=torch.int32)
        got_v, got_i = vals.cpu().numpy(), idx.cpu().numpy()
        np.testing.assert_array_equal(got_v.view(np.uint32), ref_vals.view(np.uint32), err_msg=layout)
        np.testing.assert_array_equal(got_i, ref_idx, err_msg=layout)
        assert i32.dtype == torch.int32 and torch.equal(idx.to(torch.int32), i32), layout


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["bcn", "perm"])
@pytest.mark.parametrize("C", KNN_CHANNELS)
def test_knn_matches_reference_every_channel_tier(golden, cuda, C, layout):
    """The device against the reference itself (knn_channels.npz) at every
    channel width: selected values bit-exact, indices up to the reference's
    arbitrary choice inside a tie group at the k-th value."""
    from dgx.ops import knn_raw
    g = golden("knn_channels.npz")
    key = f"c{C}_{layout}"
    t = torch.from_numpy(g[key + "_x"]).to(cuda).permute(0, 2, 1)
    x = t if layout == "perm" else t.contiguous()
    idx, vals = knn_raw(x, g[key + "_idx"].shape[-1], return_values=True)
    assert_knn_equivalent(idx.cpu().numpy(), vals.cpu().numpy(), g[key + "_idx"], g[key + "_val"])
