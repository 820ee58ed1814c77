"""dgx.loader on the host (dgx.cpu's restatement of csrc/loader.hip): the
Philox words against known answers, the distribution of the draws, the
translate arithmetic, the epoch order and its independence of the batch size."""
import numpy as np
import pytest
import torch
from torch.utils.data.distributed import DistributedSampler


def _dataset(n, P, C=3, seed=0):
    g = torch.Generator().manual_seed(seed)
    points = torch.rand(n, P, C, generator=g) * 2 - 1
    seg = torch.randint(0, 50, (n, P), generator=g, dtype=torch.int32)
    label = (torch.arange(n) % 16).to(torch.int32)
    return points, seg, label


@pytest.mark.parametrize("ctr,key,want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(ctr, key, want):
    """Philox4x32-10; the first and third are Random123's published vectors."""
    from dgx import cpu
    assert " ".join(f"{int(w):08x}" for w in cpu.philox4x32(*ctr, *key)) == want
    # broadcast over an array of counters: the same words at every place
    many = cpu.philox4x32(np.full(5, ctr[0]), ctr[1], ctr[2], ctr[3], *key)
    assert all((w == int(x, 16)).all() and w.dtype == np.uint32 for w, x in zip(many, want.split()))


def test_draws_over_4096_items():
    """A fixed seed (deterministic): all six orders occur, each switch is on
    within 4 sigma of half the items (sigma = sqrt(4096) / 2 = 32), and every
    draw lies in its interval."""
    from dgx import cpu
    from dgx.loader import DeviceLoader
    n, P = 4096, 5
    points, seg, label = _dataset(n, P)
    ld = DeviceLoader(points, seg, label, batch_size=n, shuffle=False, shuffle_points=True, augment="random3",
                      seed=20240521, _debug=True)
    ld.set_epoch(3)
    batches = list(ld)
    assert len(batches) == 1 and ld.state()["cursor"] == n
    o = ld.last
    params, perm, noise = o.params.numpy(), o.perm.numpy(), o.noise.numpy()
    assert np.array_equal(params[:, 13].view(np.int32), np.arange(n)) and (params[:, 14].view(np.int32) == 3).all()
    assert sorted(set(params[:, 0].tolist())) == [0, 1, 2, 3, 4, 5]
    for a in range(3):
        assert set(params[:, 1 + a].tolist()) == {0.0, 1.0}
        assert abs(int(params[:, 1 + a].sum()) - n // 2) <= 128, a
    scale, shift = params[:, 4:7], params[:, 7:10]
    assert (scale >= np.float32(2) / np.float32(3)).all() and (scale < 1.5).all()
    assert (shift >= np.float32(-0.2)).all() and (shift < 0.2).all()
    assert scale.max() - scale.min() > 0.8 and shift.max() - shift.min() > 0.39      # the intervals are used
    assert (np.abs(noise) <= np.float32(0.02)).all() and np.abs(noise).max() == np.float32(0.02)
    assert abs(float(noise.mean())) < 1e-3 and 0.008 < float(noise.std()) < 0.01      # sigma 0.01, clipped at 2
    assert np.array_equal(np.sort(perm, axis=1), np.tile(np.arange(P, dtype=np.int32), (n, 1)))
    assert len({tuple(r) for r in perm.tolist()}) > 100                               # of the 120 permutations
    # theta is normal with sigma 2 pi, not uniform on a circle
    theta = params[:, 10].astype(np.float64)
    assert 0.95 < theta.std() / (2 * np.pi) < 1.05 and np.abs(theta).max() > 3 * 2 * np.pi
    assert np.allclose(params[:, 11], np.cos(theta), atol=1e-7) and np.allclose(params[:, 12], np.sin(theta), atol=1e-7)
    assert cpu.BATCH_ORDERS == ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))


def test_translate_is_the_reference_expression():
    """augment="translate": the output is ``pc * scale + shift`` in float32
    numpy (data.translate_pointcloud's expression) of the shuffled cloud with
    the exported params, bit for bit; the dataset is unchanged."""
    from dgx.loader import DeviceLoader
    n, P, N = 6, 40, 33
    points, seg, label = _dataset(n, P, seed=1)
    kept = points.clone()
    ld = DeviceLoader(points, seg, label, batch_size=4, num_points=N, shuffle=True, shuffle_points=True,
                      augment="translate", seed=5, _debug=True)
    ld.set_epoch(0)
    ids = list(ld.sampler)
    at = 0
    for data, lab, sg in ld:
        o = ld.last
        for b in range(data.shape[0]):
            item, perm, q = ids[at], o.perm[b].numpy(), o.params[b].numpy()
            at += 1
            assert int(q[13:14].view(np.int32)[0]) == item and q[1:4].tolist() == [1.0, 0.0, 0.0]
            assert sorted(perm.tolist()) == list(range(N))
            pc = points[item].numpy()[perm]
            want = (pc * q[4:7] + q[7:10]).astype(np.float32)
            assert np.array_equal(data[b].numpy(), want.T)
            assert np.array_equal(sg[b].numpy(), seg[item].numpy()[perm].astype(np.int64))
            assert int(lab[b]) == int(label[item])
        assert data.is_contiguous() and data.dtype == torch.float32 and sg.dtype == torch.int64
    assert at == n and torch.equal(points, kept)


@pytest.mark.parametrize("drop_last", [False, True])
@pytest.mark.parametrize("shuffle", [True, False])
def test_epoch_order_is_the_distributed_samplers(shuffle, drop_last):
    from dgx.loader import DeviceLoader
    n = 7
    points, _, label = _dataset(n, 4)
    label = torch.arange(n, dtype=torch.int32)          # the label names the item
    for rank in (0, 1):
        ld = DeviceLoader(points, label=label, batch_size=2, shuffle=shuffle, shuffle_points=False, seed=11,
                          num_replicas=2, rank=rank, drop_last=drop_last)
        ref = DistributedSampler(range(n), num_replicas=2, rank=rank, shuffle=shuffle, seed=11, drop_last=drop_last)
        for epoch in (0, 1, 5):
            ld.set_epoch(epoch)
            ref.set_epoch(epoch)
            want = list(ref)
            assert len(want) == (3 if drop_last else 4) and len(ld) == 2
            got = torch.cat([lab for _, lab, _ in ld]).tolist()
            assert got == want
            assert ld.order[:ld.n_epoch].tolist() == want
            assert ld.state() == {"cursor": len(want), "epoch": epoch, "invalid": 0, "overrun": 0,
                                  "batches": 2 * (1 + (0, 1, 5).index(epoch))}


def test_epoch_is_independent_of_the_batch_size():
    """The same seed and epoch with batches of 2 and of 3 over 6 items give the
    same concatenated epoch: a cloud's draws depend on (seed, epoch, item)."""
    from dgx.loader import DeviceLoader
    points, seg, label = _dataset(6, 20, seed=2)

    def epoch(bs, e, seed=9):
        ld = DeviceLoader(points, seg, label, batch_size=bs, num_points=17, shuffle=True, shuffle_points=True,
                          augment="random3", num_categories=16, seed=seed)
        ld.set_epoch(e)
        parts = list(ld)
        assert [p[0].shape[0] for p in parts] == [bs] * (6 // bs)
        return [torch.cat([p[i] for p in parts]) for i in range(4)]

    a, b = epoch(2, 4), epoch(3, 4)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert a[0].shape == (6, 3, 17) and a[1].shape == (6, 16) and a[2].shape == (6, 17) and a[3].shape == (6,)
    assert torch.equal(a[1].argmax(dim=1), a[3]) and torch.equal(a[1].sum(dim=1), torch.ones(6))
    assert not torch.equal(a[0], epoch(2, 5)[0]) and not torch.equal(a[0], epoch(2, 4, seed=10)[0])


def test_tail_overrun_and_bad_ids_on_the_host():
    """Five items in batches of two: three batches, the last of one cloud, the
    cursor at 5; a further fixed-size launch counts ``overrun`` and writes
    nothing; ids and labels outside their range are counted and zeroed."""
    from dgx.loader import DeviceLoader
    points, seg, label = _dataset(5, 8, seed=3)
    label[3] = 16
    ld = DeviceLoader(points, seg, label, batch_size=2, shuffle=False, num_categories=16)
    ld.set_epoch(0)
    ld.order[1] = 5
    sizes, zero = [], []
    for data, onehot, sg, lab in ld:
        sizes.append(data.shape[0])
        zero += [not bool(data[b].any() or onehot[b].any() or sg[b].any()) for b in range(data.shape[0])]
    assert sizes == [2, 2, 1] and zero == [False, True, False, True, False]
    assert ld.state(check=False) == {"cursor": 5, "epoch": 0, "invalid": 2, "overrun": 0, "batches": 3}
    with pytest.raises(ValueError, match="invalid=2"):
        ld.state()
    for t in ld.next_into():
        t.fill_(7)
    assert all(bool((t == 7).all()) for t in ld.next_into())
    assert ld.state(check=False)["overrun"] == 4 and ld.state(check=False)["cursor"] == 5


def test_limits_and_arguments():
    from dgx.loader import DeviceLoader, MAX_SHUFFLE_POINTS
    points = torch.zeros(2, 4100, 3)
    with pytest.raises(ValueError, match="4096"):
        DeviceLoader(points, batch_size=1, num_points=MAX_SHUFFLE_POINTS + 1, shuffle_points=True)
    DeviceLoader(points, batch_size=1, num_points=MAX_SHUFFLE_POINTS + 1, shuffle_points=False)
    with pytest.raises(ValueError, match="3 channels"):
        DeviceLoader(torch.zeros(2, 8, 9), batch_size=1, augment="translate")
    with pytest.raises(ValueError, match="augment"):
        DeviceLoader(points, batch_size=1, augment="rotate")
    with pytest.raises(ValueError, match="one-hot"):
        DeviceLoader(points, batch_size=1, num_points=8, num_categories=16)


def test_datasets_raw_and_policy(monkeypatch):
    """``raw()`` returns the stored items ``__getitem__`` starts from, and
    ``data.device_loader`` picks each class / partition's own policy."""
    import warnings
    import data
    monkeypatch.setenv("DGX_SYNTHETIC_DATA", "1")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sets = {"mn_train": data.ModelNet40(1024, "train"), "mn_test": data.ModelNet40(1024, "test"),
                "sp_trainval": data.ShapeNetPart(2048, "trainval"), "sp_test": data.ShapeNetPart(512, "test", "chair"),
                "aug_train": data.ShapeNetPart_Augmented("trainval"), "aug_test": data.ShapeNetPart_Augmented("test"),
                "s3_train": data.S3DIS(4096, "train"), "s3_test": data.S3DIS(2048, "test")}
    for name in ("mn_test", "sp_test", "aug_test", "s3_test"):      # partitions whose items are the stored ones
        ds = sets[name]
        pts, label, seg = ds.raw([2, 9])
        item = ds[9]
        n = np.asarray(item[0]).shape[0]
        assert pts.dtype == np.float32 and np.array_equal(pts[1][:n], np.asarray(item[0])), name
        if seg is not None:
            assert np.array_equal(seg[1][:n], np.asarray(item[-1])), name
        if label is not None:
            assert int(label[1]) == int(np.asarray(item[1]).reshape(-1)[0]), name
    want = {"mn_train": (True, True, "translate", 1024, 0, 3), "mn_test": (False, False, "none", 1024, 0, 3),
            "sp_trainval": (True, True, "none", 2048, 16, 3), "sp_test": (False, False, "none", 512, 16, 3),
            "aug_train": (True, False, "random3", 2048, 16, 3), "aug_test": (False, False, "none", 2048, 16, 3),
            "s3_train": (True, True, "none", 4096, 0, 9), "s3_test": (False, False, "none", 2048, 0, 9)}
    for name, ds in sets.items():
        ld = data.device_loader(ds, 2, items=slice(0, 3), device="cpu")
        assert (ld.shuffle, ld.shuffle_points, ld.augment, ld.num_points, ld.num_categories, ld.C) == want[name], name
        first = next(iter(ld))
        assert first[0].shape == (2, ld.C, ld.num_points) and len(first) == (4 if ld.num_categories else 3)
    assert data.device_loader(sets["sp_test"], 2, items=[0], device="cpu").seg_start_index == 12
