"""dgx.loader on the device (csrc/loader.hip) against the host path (dgx.cpu)
at every edge of the kernel's geometry: integer results and the exactly
rounded draws are equal bit for bit, the points equal the fp32 numpy
restatement fed the device's own exported draws, and the libm-dependent draws
lie within derived bounds of an fp64 evaluation of the same integer words.
Containment of bad ids, the epoch's tail, overrun, guard words, HIP-graph
replay and the datasets' policies."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 4


def _dataset(n, P, C=3, seed=0):
    g = torch.Generator().manual_seed(seed)
    points = torch.rand(n, P, C, generator=g) * 2 - 1
    seg = torch.randint(0, 50, (n, P), generator=g, dtype=torch.int32) + 12
    label = ((torch.arange(n) * 5 + 3) % 16).to(torch.int32)
    return points, seg, label


def _pair(cuda, data, **kw):
    from dgx.loader import DeviceLoader
    kw = dict(dict(seed=77, _guard=GUARD, _debug=True), **kw)
    return DeviceLoader(*data, device=cuda, **kw), DeviceLoader(*data, device="cpu", **kw)


def _check_batch(dev, host, points, libm=True, zeros=()):
    """One batch of the device loader ``dev`` (its ``last`` outputs) against
    the same batch of the host loader ``host``; the clouds ``zeros`` are
    invalid ones, written as zeros."""
    from dgx import cpu
    d, h = dev.last, host.last
    assert d.intact() and h.intact()
    aug = dev.augment != "none"
    B = d.data.shape[0]
    N = dev.num_points
    for name in ("seg", "label", "onehot", "perm"):
        x, y = getattr(d, name), getattr(h, name)
        assert (x is None) == (y is None), name
        if x is not None:
            assert torch.equal(x.cpu(), y), name
    dq, hq = d.params.cpu().numpy(), h.params.numpy()
    # order, switches, scale, shift, item id and epoch: every operation exactly rounded, so equal bit for bit
    assert np.array_equal(dq[:, :10].view(np.int32), hq[:, :10].view(np.int32))
    assert np.array_equal(dq[:, 13:].view(np.int32), hq[:, 13:].view(np.int32))
    perm = d.perm.cpu().numpy()
    noise = d.noise.cpu().numpy() if aug else None
    out = d.data.cpu().numpy()
    for b in range(B):
        if b in zeros:
            assert not (out[b].any() or perm[b].any() or dq[b].any() or (aug and noise[b].any()))
            continue
        item, epoch = (int(v) for v in dq[b, 13:15].view(np.int32))
        assert np.array_equal(np.sort(perm[b]), np.arange(N))
        pc = points[item].numpy()[perm[b]]
        if aug:
            # the fp32 numpy restatement fed the device's own exported draws
            pc = cpu.batch_apply(pc, dq[b], noise[b])
        assert np.array_equal(out[b].view(np.int32), np.ascontiguousarray(pc.T).view(np.int32)), (b, item)
        if aug and libm:
            # fp64 evaluation from the same integer words. z = R t with R = sqrtf(-2 logf(u1)) <= 5.77 (u1 >=
            # 2^-24) and t = cospif / sinpif(2u), the argument exact. One ulp is a relative error of at most 2^-23.
            #   R: logf within 1 ulp, halved by the root, sqrtf within 1 ulp: 1.5 ulp, 5.8 * 1.5 * 2^-23 = 1.04e-6
            #   t: within 2 ulp of a value <= 1, 2 * 2^-24 = 1.2e-7, times R: 6.9e-7
            #   the product's rounding: half an ulp of a value < 8, 2^-22 = 2.4e-7          |dz| <= 2.0e-6
            #   theta = fl(2 pi) * z: 2 pi * 2.0e-6 = 1.24e-5, fl(2 pi)'s 2.8e-8 relative error on |theta| <=
            #   36.5 = 1.0e-6, the product's rounding 2^-19 / 2 = 1.9e-6: 1.5e-5 < atol 2e-5.
            #   cosf / sinf within 2 ulp of a value <= 1: 2 * 2^-24 < atol 2^-22 against fp64 of the exported theta.
            #   noise = clamp(0.01f * z): 0.01 * 2.0e-6 = 2.0e-8, 0.01f's 2.2e-8 relative error on 0.02 = 5e-10,
            #   the rounding 2^-29 / 2 = 9e-10: 2.2e-8 < atol 3e-8.
            theta64, noise64 = cpu.batch_draws64(item, epoch, dev.seed, N)
            assert abs(float(dq[b, 10]) - theta64) <= 2e-5, (b, float(dq[b, 10]), theta64)
            t = np.float64(dq[b, 10])
            assert abs(float(dq[b, 11]) - np.cos(t)) <= 2.0 ** -22 and abs(float(dq[b, 12]) - np.sin(t)) <= 2.0 ** -22
            assert np.abs(noise[b].astype(np.float64) - noise64).max() <= 3e-8
            assert np.abs(noise[b]).max() <= np.float32(0.02)


def _run_both(dev, host, points, epoch=0, libm=True):
    dev.set_epoch(epoch)
    host.set_epoch(epoch)
    sizes = []
    for got, want in zip(dev, host):
        assert len(got) == len(want)
        sizes.append(got[0].shape[0])
        assert got[0].is_contiguous() and got[0].dtype == torch.float32
        _check_batch(dev, host, points, libm)
    assert dev.state() == host.state()
    return sizes


# N: 1, 2, 3 (sorts over 1, 2, 4 words), 64 / 65 (a wave and one lane), 1023 / 1024 / 1025 (the workgroup's 512
# lanes twice, with a ragged tail; the sort over 1024 and 2048 words), 4096 (the LDS limit). 7 items in batches of
# 3: launches of B = 3, 3 and 1. P = N + 3 > N. C = 3 takes the shuffle and all three augmentations, C = 9 the
# shuffle alone (and the generic channel loop).
@pytest.mark.parametrize("C", [3, 9])
@pytest.mark.parametrize("N", [1, 2, 3, 64, 65, 1023, 1024, 1025, 4096])
def test_edges_against_the_host_path(cuda, N, C):
    data = _dataset(7, N + 3, C, seed=N)
    kw = dict(batch_size=3, num_points=N, shuffle=True, shuffle_points=True, seg_start_index=12, num_categories=16)
    if C == 3:
        kw.update(augment="random3", _force=(N % 6, 7))    # all three on, in an order that varies with N
    dev, host = _pair(cuda, data, **kw)
    assert _run_both(dev, host, data[0], epoch=N % 5) == [3, 3, 1]


@pytest.mark.parametrize("N", [1, 65, 1025])
def test_random3_unforced_and_without_shuffle(cuda, N):
    """The drawn order and switches (no override), with and without the point
    shuffle, without seg / one-hot outputs."""
    points, seg, label = _dataset(9, N + 1, seed=100 + N)
    for shuffle_points in (False, True):
        dev, host = _pair(cuda, (points, None, label), batch_size=4, num_points=N, shuffle=False,
                          shuffle_points=shuffle_points, augment="random3")
        assert _run_both(dev, host, points, epoch=2) == [4, 4, 1]
        if not shuffle_points:
            assert torch.equal(dev.last.perm.cpu()[0], torch.arange(N, dtype=torch.int32))


@pytest.mark.parametrize("order,switches", [(0, 1), (0, 2), (0, 4), (0, 0)] + [(o, 7) for o in range(6)]
                         + [(3, 5), (4, 6)])
def test_forced_augmentations(cuda, order, switches):
    """Each augmentation alone, none, each of the six orders with all three
    on, and two pairs, through the test-only flags override."""
    from dgx import cpu
    N = 130
    data = _dataset(4, N, seed=order * 8 + switches)
    dev, host = _pair(cuda, data, batch_size=4, shuffle=False, shuffle_points=False, augment="random3",
                      _force=(order, switches))
    assert _run_both(dev, host, data[0]) == [4]
    q = dev.last.params.cpu().numpy()
    assert (q[:, 0] == order).all() and (q[:, 1:4] == [(switches >> a) & 1 for a in range(3)]).all()
    out = dev.last.data.cpu().permute(0, 2, 1).numpy()
    src = data[0].numpy()
    if switches == 0:
        assert np.array_equal(out, src)
    if switches == 1:
        assert np.array_equal(out, src * q[:, None, 4:7] + q[:, None, 7:10])
    if switches == 2:
        assert np.array_equal(out, src + dev.last.noise.cpu().numpy())
    if switches == 4:
        c, s = q[:, None, 11], q[:, None, 12]
        assert np.array_equal(out[..., 1], src[..., 1])
        assert np.array_equal(out[..., 0], src[..., 0] * c + src[..., 2] * s)
        assert np.array_equal(out[..., 2], -(src[..., 0] * s) + src[..., 2] * c)
        assert np.allclose((out ** 2).sum(-1), (src ** 2).sum(-1), atol=1e-5)      # a rotation
    if switches == 7 and order in (0, 5):      # the orders differ: T J R against R J T on the same draws
        other = cpu.batch_apply(src[0], np.concatenate([[5 - order], q[0, 1:]]).astype(np.float32),
                                dev.last.noise.cpu().numpy()[0])
        assert not np.array_equal(out[0], other)


def test_translate_policy_and_draw_independence(cuda):
    """augment="translate" (ModelNet40 train) is ``pc * scale + shift``; a
    cloud's result does not depend on the batch size or its place in the
    batch."""
    points, seg, label = _dataset(6, 70, seed=5)
    dev, host = _pair(cuda, (points, None, label), batch_size=2, num_points=64, shuffle=True, shuffle_points=True,
                      augment="translate")
    assert _run_both(dev, host, points, epoch=1, libm=False) == [2, 2, 2]
    dev3, _ = _pair(cuda, (points, None, label), batch_size=3, num_points=64, shuffle=True, shuffle_points=True,
                    augment="translate")
    dev.set_epoch(1)
    dev3.set_epoch(1)
    a, b = [d.clone() for d, _, _ in dev], [d.clone() for d, _, _ in dev3]
    assert torch.equal(torch.cat(a), torch.cat(b))


def test_shuffle_limit_and_long_clouds(cuda):
    """N = 4097 with the shuffle is refused (by the class and by the C ABI);
    N = 5000 without it works and uses no LDS."""
    import ctypes
    from dgx import _native as nat
    from dgx.loader import DeviceLoader
    points, seg, label = _dataset(3, 5003, seed=6)
    with pytest.raises(ValueError, match="4096"):
        DeviceLoader(points, seg, label, batch_size=2, num_points=4097, shuffle_points=True, device=cuda)
    dev, host = _pair(cuda, (points, seg, label), batch_size=2, num_points=5000, shuffle=True, shuffle_points=False,
                      augment="random3")
    assert _run_both(dev, host, points) == [2, 1]
    L = nat.lib()
    assert L.dgx_batch_max_points() == 4096
    o = dev.last
    args = lambda n, flags: (
        nat.f32(dev.points), nat.i32(dev.seg), nat.i32(dev.label), 3, 5003, 3, nat.i32(dev.order), dev.n_epoch,
        nat.ptr(dev._state), 1, n, 0, 0, ctypes.c_uint64(1), flags, nat.f32(o.data), nat.ptr(o.seg), nat.ptr(o.label),
        None, None, None, None, None)
    before = dev.state()
    assert L.dgx_batch_assemble(*args(4097, 1)) == -2            # DGX_EUNSUPPORTED
    assert L.dgx_batch_assemble(*args(5004, 0)) == -1            # N > P
    assert L.dgx_batch_assemble(*args(5000, 1 << 10)) == -1      # unknown flag bits
    assert dev.state() == before and o.intact()                  # refused before any device work


def test_tail_batch_and_cursor(cuda):
    """Five items in batches of two: three batches, the last of one cloud, and
    the cursor reaches 5."""
    data = _dataset(5, 40, seed=7)
    dev, host = _pair(cuda, data, batch_size=2, shuffle=True, shuffle_points=True, augment="random3",
                      num_categories=16)
    assert len(dev) == 3
    assert _run_both(dev, host, data[0]) == [2, 2, 1]
    assert dev.state() == {"cursor": 5, "epoch": 0, "invalid": 0, "overrun": 0, "batches": 3}


def test_bad_ids_and_labels_are_contained(cuda):
    """Item ids outside [0, n) in ``order`` and labels outside [0, ncat) are
    counted in ``invalid`` and never used as an address: those clouds are
    zeros, the others as on the host, and every guard word stays."""
    points, seg, label = _dataset(8, 33, seed=8)
    label[2] = 16
    label[5] = -1
    dev, host = _pair(cuda, (points, seg, label), batch_size=4, shuffle=False, shuffle_points=True,
                      augment="random3", num_categories=16)
    bad = {0: 8, 3: -1, 6: 2 ** 31 - 1, 7: -2 ** 31}
    zero = []
    for ld in (dev, host):
        ld.set_epoch(0)
        for slot, v in bad.items():
            ld.order[slot] = v
    for at, ((data, onehot, sg, lab), _) in enumerate(zip(dev, host)):
        _check_batch(dev, host, points, zeros=[b for b in range(4) if 4 * at + b in (0, 2, 3, 5, 6, 7)])
        zero += [not bool(data[b].any() or onehot[b].any() or sg[b].any() or lab[b].any()) for b in range(4)]
    assert zero == [True, False, True, True, False, True, True, True]
    want = {"cursor": 8, "epoch": 0, "invalid": 6, "overrun": 0, "batches": 2}
    assert dev.state(check=False) == want and host.state(check=False) == want
    with pytest.raises(ValueError, match="invalid=6"):
        dev.state()


def test_overrun_leaves_the_outputs(cuda):
    """A fixed-size launch past the epoch's end counts ``overrun``, writes
    nothing and leaves the cursor; one that straddles the end writes only the
    clouds that exist."""
    data = _dataset(5, 20, seed=9)
    dev, host = _pair(cuda, data, batch_size=3, shuffle=True, shuffle_points=True, augment="random3",
                      num_categories=16)
    for ld in (dev, host):
        ld.set_epoch(0)
        ld.next_into()                                           # slots 0..2
        o = ld._fixed
        for t in ld._tuple(o):
            t.fill_(7)
        ld.next_into()                                           # slots 3, 4 and one past the end
        assert bool((o.data[2] == 7).all() and (o.seg[2] == 7).all() and (o.onehot[2] == 7).all() and o.label[2] == 7)
        assert not bool((o.data[:2] == 7).any() or (o.seg[:2] == 7).any() or (o.onehot[:2] == 7).any())
        assert o.intact()
        assert ld.state(check=False) == {"cursor": 5, "epoch": 0, "invalid": 0, "overrun": 1, "batches": 2}
    d, h = dev._fixed, host._fixed
    assert torch.equal(d.seg.cpu(), h.seg) and torch.equal(d.label.cpu(), h.label) and torch.equal(d.perm.cpu(), h.perm)
    for ld in (dev, host):
        for t in ld._tuple(ld._fixed):
            t.fill_(7)
        assert all(bool((t == 7).all()) for t in ld.next_into())
        assert ld._fixed.intact()
        assert ld.state(check=False) == {"cursor": 5, "epoch": 0, "invalid": 0, "overrun": 4, "batches": 3}
    with pytest.raises(ValueError, match="overrun=4"):
        dev.state()


def test_graph_replay_equals_eager(cuda):
    """``next_into`` captured once and replayed three times gives the three
    eager batches of an identically seeded loader, bit for bit; the cursor
    reaches 3 B on the device; a ``set_epoch`` between replays is followed."""
    from dgx.loader import DeviceLoader
    B, N = 4, 257
    points, seg, label = _dataset(16, N + 2, seed=10)
    kw = dict(batch_size=B, num_points=N, shuffle=True, shuffle_points=True, augment="random3", num_categories=16,
              seed=3, device=cuda)
    cap, eager = DeviceLoader(points, seg, label, **kw), DeviceLoader(points, seg, label, **kw)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fixed = cap.next_into()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        again = cap.next_into()
    assert all(x is y or x.data_ptr() == y.data_ptr() for x, y in zip(fixed, again))
    cap.set_epoch(0)
    eager.set_epoch(0)
    it = iter(eager)
    for _ in range(3):
        graph.replay()
        want = next(it)
        assert all(torch.equal(x, y) for x, y in zip(fixed, want))
    assert cap.state()["cursor"] == 3 * B and cap.state()["batches"] == 4
    cap.set_epoch(1)
    eager.set_epoch(1)
    graph.replay()
    want = next(iter(eager))
    assert all(torch.equal(x, y) for x, y in zip(fixed, want))
    assert cap.state()["cursor"] == B and cap.state()["epoch"] == 1
    eager.set_epoch(0)
    assert not torch.equal(next(iter(eager))[0], fixed[0])       # the epochs differ


def test_shapenet_augmented_batch_feeds_the_model(cuda, monkeypatch):
    """``data.device_loader`` on the synthetic ShapeNetPart_Augmented split
    yields what the partseg loop builds by hand, and a small DGCNN runs on the
    batch as it is."""
    import types
    import warnings
    import data
    from models.dgcnn import DGCNN
    monkeypatch.setenv("DGX_SYNTHETIC_DATA", "1")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ds = data.ShapeNetPart_Augmented("trainval")
    ld = data.device_loader(ds, 4, device=cuda)
    assert ld.augment == "random3" and ld.n_items == len(ds)
    ld.set_epoch(0)
    cloud, onehot, seg, label = next(iter(ld))
    assert cloud.shape == (4, 3, 2048) and cloud.dtype == torch.float32 and cloud.is_contiguous()
    assert onehot.shape == (4, 16) and onehot.dtype == torch.float32
    assert seg.shape == (4, 2048) and seg.dtype == torch.int64 and label.shape == (4,)
    assert torch.equal(onehot.argmax(dim=1), label) and torch.equal(onehot.sum(dim=1), torch.ones(4, device=cuda))
    ids = list(ld.sampler)[:4]
    assert label.tolist() == [i % 16 for i in ids]
    assert bool((seg >= 0).all()) and bool((seg < 50).all())
    torch.manual_seed(0)
    y = DGCNN(types.SimpleNamespace(emb_dim=64, k=10)).to(cuda).train()(cloud)
    assert y.shape == (4, 64, 2048) and bool(torch.isfinite(y).all())
    assert ld.state()["cursor"] == 4
