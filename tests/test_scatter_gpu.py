"""The EdgeConv backward scatter (dgx_edge_bwd_scatter_f32 / _packed_f32; the
autograd of dgcnn.py:84-98's gather + max through BN, the reverse of
get_graph_feature's index at dgcnn.py:33-36). Each point pulls the selected
dz of its in-edges from the cloud's LDS slices, so:

* against an fp64 restatement of the same scatter (every term summed in fp64)
  the result is within fp32 rounding (2e-6 of the output scale), with packed
  dz|slot words or dz + slot bytes, including at hubs, where hundreds of
  sources select one target, and at channels not a multiple of 8 and N needing
  several point parts or narrow slices;
* it sums in a fixed order: two launches are bitwise equal;
* every output mode (fp32, bf16, the split bf16 planes) at every slice
  geometry stays within its rounding of the fp64 result;
* the largest cloud runs, one more point is refused before any launch, and the
  training forward names that limit."""

import ctypes

import pytest
import torch

from dgx import _native as nat
from dgx import bn as bn_
from dgx import edgeconv as E
from dgx import schedule

pytestmark = pytest.mark.gpu


def _rel(a, b):
    return ((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30)).item()


def _setup(cuda, B, N, k, Co, hubs=False, seed=0, packed=False):
    g = torch.Generator(device="cpu").manual_seed(seed + N + Co)
    M = B * N
    L = nat.lib()
    PQ = torch.randn(M, 2 * Co, generator=g).to(cuda)
    if hubs:   # three in four neighbours are one of 4 hub points: in-degrees in the thousands
        idx = torch.where(torch.rand(B, N, k, generator=g) < 0.75, torch.randint(0, 4, (B, N, k), generator=g),
                          torch.randint(0, N, (B, N, k), generator=g)).to(torch.int32).to(cuda)
    else:
        idx = torch.randint(0, N, (B, N, k), generator=g, dtype=torch.int32).to(cuda)
    gamma = torch.randn(Co, generator=g).to(cuda)
    stream = nat.stream_of(PQ)
    ysel, arg, sumP, part, prow = E.edge_select(PQ, idx, B, N, k, Co, gamma, stream)
    bn = torch.nn.BatchNorm2d(Co).to(cuda).train()
    st = bn_.batch_stats(part, prow, float(M * k), bn, gamma, torch.zeros_like(gamma), stream)
    dY = torch.randn(M, Co, generator=g).to(cuda)
    nblk = max(1, min(1024, (M + 63) // 64))
    dz = torch.empty(M, Co, device=cuda)
    partials = torch.empty(nblk, 2, Co, device=cuda)
    bn_args = (M, Co, nat.f32(st.scale), nat.f32(st.shift), nat.f32(st.mean), nat.f32(st.invstd), 0.2, nat.f32(dz),
               nat.f32(partials), nblk, stream)
    if packed:
        nat.check(L.dgx_edge_bwd_dz_packed_f32(nat.f32(dY), Co, nat.f32(ysel), nat.u8(arg), *bn_args), "dz")
    else:
        nat.check(L.dgx_edge_bwd_dz_f32(nat.f32(dY), Co, nat.f32(ysel), *bn_args), "dz")
    (rowptr, edges), = schedule.reverse_graphs([idx])
    c = bn_.backward_consts(partials, nblk, float(M * k), st, stream)
    return dict(L=L, B=B, N=N, k=k, Co=Co, M=M, PQ=PQ, idx=idx, arg=arg, sumP=sumP, st=st, dz=dz, partials=partials,
                nblk=nblk, rowptr=rowptr, edges=edges, c0=c[2], c1=c[3], stream=stream)


def _pull(S, packed, mode=0):
    """The pull scatter with out_bf16 = ``mode``: fp32 (M, 2Co), bf16 (M, 2Co), or
    (modes 2 / 3) the bf16 planes (3, M, 2Co), zero where the mode writes none."""
    L, st = S["L"], S["st"]
    dev = S["PQ"].device
    if mode == 0:
        out = torch.empty(S["M"], 2 * S["Co"], device=dev)
    elif mode == 1:
        out = torch.empty(S["M"], 2 * S["Co"], device=dev, dtype=torch.bfloat16)
    else:
        out = torch.zeros(3, S["M"], 2 * S["Co"], device=dev, dtype=torch.bfloat16)
    common = (S["B"], S["N"], S["k"], S["Co"], nat.f32(st.scale), nat.f32(S["c0"]), nat.f32(S["c1"]),
              nat.ptr(out, nat.F32, nat.BF16), mode, S["stream"])
    if packed:
        nat.check(L.dgx_edge_bwd_scatter_packed_f32(nat.f32(S["PQ"]), 2 * S["Co"], nat.i32(S["rowptr"]),
                                                    nat.i32(S["edges"]), nat.f32(S["dz"]), nat.f32(S["sumP"]),
                                                    *common), "scatter")
    else:
        nat.check(L.dgx_edge_bwd_scatter_f32(nat.f32(S["PQ"]), 2 * S["Co"], nat.i32(S["rowptr"]), nat.i32(S["edges"]),
                                             nat.f32(S["dz"]), nat.u8(S["arg"]), nat.f32(S["sumP"]), *common),
                  "scatter")
    return out


def _ref64(S, packed):
    """dP_j = a sum_{(i,s): idx[i][s] = j, arg[i][c] = s} dz_i[c] + sum_{idx[i][s] = j} (c0 + c1 (P_j + Q_i)),
    dQ_i = a dz_i + k c0 + c1 (k Q_i + sum_s P_idx[i][s]), every term in fp64."""
    B, N, k, Co, M = S["B"], S["N"], S["k"], S["Co"], S["M"]
    PQ = S["PQ"].double()
    P, Q = PQ[:, :Co], PQ[:, Co:]
    dz = S["dz"]
    if packed:
        dz = (dz.view(torch.int32) & ~63).view(torch.float32)
    dz = dz.double()
    a, c0, c1 = S["st"].scale.double(), S["c0"].double(), S["c1"].double()
    gidx = (S["idx"].long() + (torch.arange(B, device=PQ.device) * N).view(B, 1, 1)).view(M, k)
    jsel = torch.gather(gidx, 1, S["arg"].long())                     # (M, Co): the selected target per channel
    sd = torch.zeros(M, Co, dtype=torch.float64, device=PQ.device).scatter_add_(0, jsel, dz)
    deg = torch.bincount(gidx.flatten(), minlength=M).double().unsqueeze(1)
    sq = torch.zeros(M, Co, dtype=torch.float64, device=PQ.device).index_add_(0, gidx.flatten(),
                                                                               Q.repeat_interleave(k, 0))
    dP = a * sd + c0 * deg + c1 * (deg * P + sq)
    dQ = a * dz + k * c0 + c1 * (k * Q + P[gidx].sum(1))
    return torch.cat([dP, dQ], 1)


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("B,N,k,Co,hubs", [(32, 1024, 20, 64, False), (4, 777, 11, 20, False),
                                           (8, 1024, 20, 256, True), (2, 2048, 40, 64, False),
                                           (1, 12000, 16, 8, False)])
def test_pull_matches_fp64(cuda, B, N, k, Co, hubs, packed):
    S = _setup(cuda, B, N, k, Co, hubs=hubs, packed=packed)
    ref = _ref64(S, packed)
    pull = _pull(S, packed)
    pull2 = _pull(S, packed)
    torch.cuda.synchronize()
    e_pull = _rel(pull, ref)
    print(f"B{B} N{N} k{k} Co{Co} hubs={hubs} packed={packed}: pull {e_pull:.2e}")
    assert torch.equal(pull, pull2)                  # a fixed summation order: bitwise repeatable
    assert e_pull < 2e-6


@pytest.mark.parametrize("mode", [2, 3])
@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("B,N,k,Co", [(8, 1024, 20, 64), (4, 777, 11, 20)])
def test_pull_split_planes_output(cuda, packed, B, N, k, Co, mode):
    """out_bf16 = 2 / 3 (the fp32 mode's split class): the pull scatter writes dPQ
    as its (hi, lo) bf16 planes, lo at + B*N*2Co (mode 3: hi again at + 2 B*N*2Co)
    — bitwise the fp32 output split by dgx_split_bf16's rounding (hi = bf16(v),
    lo = bf16(v - hi))."""
    S = _setup(cuda, B, N, k, Co, packed=packed, seed=5)
    L, st = S["L"], S["st"]
    ref = _pull(S, packed)
    planes = torch.zeros(3, S["M"], 2 * Co, device=cuda, dtype=torch.bfloat16)
    common = (B, N, k, Co, nat.f32(st.scale), nat.f32(S["c0"]), nat.f32(S["c1"]), nat.ptr(planes, nat.BF16), mode,
              S["stream"])
    if packed:
        nat.check(L.dgx_edge_bwd_scatter_packed_f32(nat.f32(S["PQ"]), 2 * Co, nat.i32(S["rowptr"]), nat.i32(S["edges"]),
                                                    nat.f32(S["dz"]), nat.f32(S["sumP"]), *common), "scatter split")
    else:
        nat.check(L.dgx_edge_bwd_scatter_f32(nat.f32(S["PQ"]), 2 * Co, nat.i32(S["rowptr"]), nat.i32(S["edges"]),
                                             nat.f32(S["dz"]), nat.u8(S["arg"]), nat.f32(S["sumP"]), *common),
                  "scatter split")
    torch.cuda.synchronize()
    hi = ref.to(torch.bfloat16)
    lo = (ref - hi.float()).to(torch.bfloat16)
    assert torch.equal(planes[0], hi) and torch.equal(planes[1], lo)
    assert torch.equal(planes[2], hi if mode == 3 else torch.zeros_like(hi))


# ---- the pull scatter's output modes at every slice geometry -------------------------------------------------------
BW_LDS_BYTES = 72 * 1024   # csrc/edgeconv.hip: the Q | dz | slot slices of two workgroups per CU


def _scatter_cs(N, packed, B=1, Co=8):
    """launch_scatter's slice width, from the launcher's own rules
    (dgx_edge_bwd_scatter_geometry): 9 bytes per (point, channel) with slot bytes,
    8 with packed dz|slot words, halved from 8 channels until the slice fits."""
    cs = ctypes.c_int(-1)
    nat.check(nat.lib().dgx_edge_bwd_scatter_geometry(B, N, Co, int(packed), ctypes.byref(cs), None, None, None),
              "scatter geometry")
    return cs.value


# one ragged N per geometry (the same for both dz forms): 8 / 4 / 2 / 1 channels
# per slice within BW_LDS_BYTES, then one-channel slices beyond it (the 160 KiB mode)
SCATTER_GEOMETRIES = [(1000, 8, False), (2003, 4, False), (4001, 2, False), (7001, 1, False), (12001, 1, True)]


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("N,cs,big", SCATTER_GEOMETRIES)
def test_pull_output_modes_vs_fp64(cuda, N, cs, big, packed):
    """Every out_bf16 mode of the pull scatter against the fp64 restatement:
    fp32 within 2e-6 of the output scale; bf16 within its rounding, 2^-8 |ref|,
    on top of that; the split planes hi + lo within 2^-15 |ref| on top of it
    (lo = bf16(v - hi) leaves 2^-16 |v|); mode 3's third plane is the first."""
    B, k, Co = 1, 8, 8
    assert _scatter_cs(N, packed) == cs and ((8 if packed else 9) * N * cs > BW_LDS_BYTES) == big
    S = _setup(cuda, B, N, k, Co, packed=packed, seed=9)
    ref = _ref64(S, packed)
    out = [_pull(S, packed, mode) for mode in range(4)]
    torch.cuda.synchronize()
    scale = float(ref.abs().max())
    fp32_err = 2e-6 * scale
    e0 = float((out[0].double() - ref).abs().max())
    e1 = (out[1].double() - ref).abs() - 2.0 ** -8 * ref.abs()
    print(f"N{N} cs{cs} packed={packed}: fp32 {e0 / scale:.2e}, bf16 excess {float(e1.max()) / scale:.2e}")
    assert e0 < fp32_err
    assert bool((e1 <= fp32_err).all())
    for mode in (2, 3):
        hi, lo, third = out[mode]
        e = (hi.double() + lo.double() - ref).abs() - 2.0 ** -15 * ref.abs()
        print(f"  mode {mode}: split excess {float(e.max()) / scale:.2e}")
        assert bool((e <= fp32_err).all())
        assert torch.equal(third, hi if mode == 3 else torch.zeros_like(hi))


@pytest.mark.parametrize("packed", [False, True])
def test_pull_largest_cloud_and_one_more(cuda, packed):
    """dgx_edge_bwd_scatter_max_n: the largest cloud runs and matches fp64; one
    more point is refused by the entry's shape check, before any launch (the
    output buffer is untouched)."""
    B, k, Co = 1, 8, 8
    L = nat.lib()
    nmax = L.dgx_edge_bwd_scatter_max_n(B, Co, int(packed))
    assert 17000 < nmax < 21000                       # about 17900 with slot bytes, 20000 packed
    assert L.dgx_edge_bwd_scatter_fits(B, nmax, Co, int(packed)) == 1
    assert L.dgx_edge_bwd_scatter_fits(B, nmax + 1, Co, int(packed)) == 0
    S = _setup(cuda, B, nmax, k, Co, packed=packed, seed=13)
    ref = _ref64(S, packed)
    got = _pull(S, packed)
    torch.cuda.synchronize()
    assert _rel(got, ref) < 2e-6
    S = _setup(cuda, B, nmax + 1, k, Co, packed=packed, seed=13)
    out = torch.full((S["M"], 2 * Co), float("nan"), device=cuda)
    st = S["st"]
    common = (B, nmax + 1, k, Co, nat.f32(st.scale), nat.f32(S["c0"]), nat.f32(S["c1"]), nat.f32(out), 0, S["stream"])
    if packed:
        rc = L.dgx_edge_bwd_scatter_packed_f32(nat.f32(S["PQ"]), 2 * Co, nat.i32(S["rowptr"]), nat.i32(S["edges"]),
                                               nat.f32(S["dz"]), nat.f32(S["sumP"]), *common)
    else:
        rc = L.dgx_edge_bwd_scatter_f32(nat.f32(S["PQ"]), 2 * Co, nat.i32(S["rowptr"]), nat.i32(S["edges"]),
                                        nat.f32(S["dz"]), nat.u8(S["arg"]), nat.f32(S["sumP"]), *common)
    torch.cuda.synchronize()
    assert rc == -2 and L.dgx_strerror(rc) == b"unsupported shape"
    assert bool(torch.isnan(out).all())


@pytest.mark.parametrize("mode,packed", [("fp32", False), ("bf16", True)])
def test_training_forward_names_the_backward_limit(cuda, mode, packed):
    """A cloud the backward scatter cannot take is refused when the training
    forward is entered, with the limit in the message; the same cloud runs
    forward-only."""
    from dgx import precision
    from dgx.edgeconv import edgeconv_stack
    B, C, Co, k = 1, 3, 8, 8
    nmax = nat.lib().dgx_edge_bwd_scatter_max_n(B, Co, int(packed))
    blk = torch.nn.Sequential(torch.nn.Conv2d(2 * C, Co, 1, bias=False), torch.nn.BatchNorm2d(Co),
                              torch.nn.LeakyReLU(0.2)).to(cuda).train()
    x = torch.randn(B, C, nmax + 1, generator=torch.Generator().manual_seed(1)).to(cuda)
    precision.set(mode)
    try:
        with pytest.raises(RuntimeError, match=f"at most N = {nmax} points"):
            edgeconv_stack(x.clone().requires_grad_(True), k, [blk], True)
        with torch.no_grad():
            y = edgeconv_stack(x, k, [blk], True)
        ok = edgeconv_stack(x[:, :, :nmax].contiguous().requires_grad_(True), k, [blk], True)
        ok.sum().backward()
    finally:
        precision.set("fp32")
    torch.cuda.synchronize()
    assert tuple(y.shape) == (B * (nmax + 1), Co) and bool(torch.isfinite(y).all())
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in blk.parameters())
