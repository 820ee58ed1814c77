"""CPU checks of the boundary: libdgx.so loads and exports every symbol that
include/dgx.h declares; the Python mirror binds them; no silent CPU path."""
import ctypes
import os
import re
import types

import pytest
import torch

from conftest import REPO


def _declared():
    with open(os.path.join(REPO, "include", "dgx.h")) as f:
        src = f.read()
    return sorted(set(re.findall(r"\b(dgx_[A-Za-z0-9_]+)\s*\(", src)))


def test_header_symbols_exported():
    from dgx import _native
    lib = ctypes.CDLL(_native.LIB_PATH)
    declared = _declared()
    assert len(declared) >= 15
    for name in declared:
        assert hasattr(lib, name), name
    # the Python binding declares a signature for every exported symbol
    assert sorted(_native.exported_symbols()) == declared


def test_version_and_errors():
    from dgx import _native
    L = _native.lib()
    assert L.dgx_version().decode().startswith("dgx")
    assert L.dgx_strerror(-1).decode() == "invalid argument"
    # argument validation happens before any device work
    assert L.dgx_knn_f32(None, 0, 0, 0, 1, 3, 8, 2, 0, None, None, None, 0, None) == -1
    # |x|^2 (B*N floats) + operand image per cloud: 32-point tiles x 64 lanes x NS = ceil(C/2) (rounded
    # to 2, 4, 8, ...) MFMA steps + 32 norms per tile (C=64: 32 tiles x 64 x 32 + 32 x 32)
    assert L.dgx_knn_workspace_bytes(2, 64, 1024) == 2 * 1024 * 4 + 2 * (32 * 64 * 32 + 32 * 32) * 4
    # |x|^2 (B*N floats) + operand image (64 tiles x 64 lanes x 16 floats + 64 x 16 norms per cloud at C=64)
    assert L.dgx_knn_workspace_bytes(2, 64, 1024) == 2 * 1024 * 4 + 2 * (64 * 64 * 16 + 64 * 16) * 4
    assert L.dgx_knn_image_bytes(2, 3, 1000) == 2 * (63 * 64 * 1 + 63 * 16) * 4


def test_host_tensors_take_the_cpu_path_without_libdgx(monkeypatch):
    """Host tensors are served by dgx.cpu and never reach the
    HIP library: with libdgx.so made unloadable the drop-in still runs on the
    CPU, while the device-only entry points keep rejecting host tensors."""
    from dgx import _native as nat
    from models.dgcnn import DGCNN, knn, get_graph_feature

    def no_lib():
        raise ImportError("libdgx.so unavailable (test)")
    monkeypatch.setattr(nat, "lib", no_lib)
    x = torch.rand(2, 3, 32)
    assert knn(x, 4).shape == (2, 32, 4)
    assert get_graph_feature(x, k=4).shape == (2, 6, 32, 4)
    assert DGCNN(types.SimpleNamespace(emb_dim=64, k=4))(x).shape == (2, 64, 32)
    with pytest.raises(RuntimeError, match="ROCm device"):
        nat.require_device(x)


def test_state_dict_keys_match_reference():
    import json
    from conftest import GOLDEN
    from models.dgcnn import DGCNN
    from models.layers import PositionEmbedding
    with open(os.path.join(GOLDEN, "hashes.json")) as f:
        keys = json.load(f)["state_dict_keys"]
    assert list(DGCNN(types.SimpleNamespace(emb_dim=1024, k=20)).state_dict().keys()) == keys["DGCNN"]
    assert list(PositionEmbedding(types.SimpleNamespace(k=20)).state_dict().keys()) == keys["PositionEmbedding"]


def test_host_op_library_loads():
    """libdgx_torch.so (the C++ schedule + autograd layer over libdgx.so) loads
    and registers the torch.ops.dgx_host ops every device path runs; host
    tensors never take them."""
    from dgx import host
    from models.dgcnn import DGCNN
    host.load()
    want = {
        "dgcnn": "dgx_host::dgcnn(Tensor x, Tensor[] params, Tensor?[] bufs, float[] bn_f, int[] bn_i, str[] groups",
        "chain_forward": "dgx_host::chain_forward(Tensor x, int k, Tensor[] weights",
        "chain_backward": "dgx_host::chain_backward(Tensor dxcat, Tensor xcat, Tensor xcat16, Tensor[] saved",
        "pointconv_forward": "dgx_host::pointconv_forward(Tensor X, Tensor X16, int B, int N",
        "pointconv_backward": "dgx_host::pointconv_backward(Tensor dout, Tensor[] saved",
        "edge_mlp2_forward": "dgx_host::edge_mlp2_forward(Tensor x, Tensor idx, int k, Tensor w1",
        "edge_mlp2_backward": "dgx_host::edge_mlp2_backward(Tensor dout, Tensor[] saved, Tensor w1, Tensor w2",
        "knn": "dgx_host::knn(Tensor x, int k, int order, ScalarType ids, bool values, bool generic, Tensor? xx, "
               "Tensor? image) -> Tensor[]",
        "knn_image_buffers": "dgx_host::knn_image_buffers(int B, int C, int N, Device device) -> (Tensor, Tensor)",
        "knn_timing": "dgx_host::knn_timing(bool on) -> float[]",
        "reverse_graphs": "dgx_host::reverse_graphs(Tensor[] idxs) -> Tensor[]",
        "graph_feature": "dgx_host::graph_feature(Tensor x, Tensor idx, int mode) -> Tensor",
        "graph_feature_backward": "dgx_host::graph_feature_backward(Tensor dout, Tensor idx, int C, int mode) "
                                  "-> Tensor",
        "gemm_xwt": "dgx_host::gemm_xwt(Tensor x, Tensor w, Tensor(a!)? out, bool stats, bool out_bf16",
        "gemm_xw": "dgx_host::gemm_xw(Tensor x, Tensor w, Tensor(a!)? out, bool accumulate)",
        "gemm_atb": "dgx_host::gemm_atb(Tensor a, Tensor b, Tensor(c!) out, int split_rows, bool lds, int slab_cap_mb)",
        "gemm32": "dgx_host::gemm32(Tensor a, Tensor b, Tensor(c!)? out, bool accumulate, Tensor? addend)",
        "gemm_edge_dz_ok": "dgx_host::gemm_edge_dz_ok(Tensor dpq16, int cin) -> bool",
        "weight_prep": "dgx_host::weight_prep(Tensor[] weights, int[] rows, int[] cols, bool[] stacked, bool[] split",
        "weight_prep_one": "dgx_host::weight_prep_one(Tensor w, int rows, int cols, bool stacked)",
    }
    for name, head in want.items():
        assert str(getattr(torch.ops.dgx_host, name).default._schema).startswith(head), name
    assert torch.ops.dgx_host.knn_timing(False) == []
    assert not host.applies(DGCNN(types.SimpleNamespace(emb_dim=64, k=4)).train(), torch.rand(2, 3, 32))


def test_schedule_layout_named_once(monkeypatch):
    """The saved-state field names and the opts bits of dgx.schedule are the
    C++ schedule's own tables (dgx_host::layout()), and ``opts()`` puts each
    A/B switch of dgx.edgeconv at the bit of its name, read at call time."""
    from dgx import edgeconv as E, gemm as G, host, schedule as S
    host.load()
    chain, pc, bits, emlp = (tuple(names) for names in torch.ops.dgx_host.layout())
    assert (chain, pc, bits, emlp) == (S.CHAIN_FIELDS, S.PC_FIELDS, S.OPT_BITS, S.EMLP_FIELDS)
    assert E.opts is S.opts
    monkeypatch.setattr(G, "SLAB_CAP_MB", 0)
    for on in bits:
        for name in bits:
            monkeypatch.setattr(E, name, name == on)
        assert S.opts() == 1 << bits.index(on), on
    for name in bits:
        monkeypatch.setattr(E, name, False)
    assert S.opts() == 0 and S.opts(split=True) == 1 << bits.index("SPLIT32")
    monkeypatch.setattr(G, "SLAB_CAP_MB", 8)
    assert S.opts() == 8 << 8


@pytest.mark.parametrize("fn,bk", [("dgx_gemm_slabs", 32), ("dgx_gemm_lds_slabs", 64), ("dgx_gemm_f32_slabs", 16)])
def test_split_k_slab_counts(fn, bk):
    """The slabs a split-K launch writes — what the launcher's grid, the slab
    allocation and dgx_slab_reduce_f32's S all take from one function per GEMM
    family: ceil(K / kchunk), kchunk = ceil(K / splits) rounded up to the
    kernel's K-step; fewer than ``splits`` when K is short; 1 for K = 0."""
    from dgx import _native
    count = getattr(_native.lib(), fn)
    for splits in (1, 2, 3, 7, 17, 128, 512):
        assert count(0, splits) == 1
        for K in (1, bk - 1, bk, bk + 1, 100, 2047, 2048, 4099, 32768):
            chunk = -(-K // splits)
            kchunk = -(-chunk // bk) * bk
            assert count(K, splits) == -(-K // kchunk), (K, splits)
    assert count(100, 0) == 1 and count(-5, 3) == 1
    # a short K: 7 splits asked, one 64-deep K-step per slab, so fewer slabs written
    assert _native.lib().dgx_gemm_lds_slabs(100, 7) == 2


def test_weight_prep_layout_matches_schedule():
    """gemm.prep_layout (plain Python: dynamo and torch.export trace through
    it) restates the layout of the C++ schedule's weight-prep buffer; the
    host-only dgx_host::weight_prep_layout reports the C++ one."""
    from dgx import gemm as G, host
    host.load()
    T, F = True, False

    def both(shapes):
        total, lay = G.prep_layout(shapes)
        ctotal, nt_off, nt_shape, tn_off, tn_shape = torch.ops.dgx_host.weight_prep_layout(
            *(list(f) for f in zip(*shapes)))
        assert ctotal == total
        for j, (o1, s1, o2, s2) in enumerate(lay):
            assert (nt_off[j], tuple(nt_shape[2 * j:2 * j + 2])) == (o1, s1)
            assert (tn_off[j], tuple(tn_shape[2 * j:2 * j + 2])) == (o2, s2)
            assert o1 % 8 == 0 and o2 % 8 == 0
        return total, [(o1, o2) for (o1, _, o2, _) in lay], [s1 for (_, s1, _, _) in lay]

    total, offs, nt = both([(64, 64, T, T), (128, 64, T, T), (256, 128, T, T), (1024, 512, F, F)])   # DGCNN
    assert total == 1318912
    assert offs == [(0, 16384), (24576, 57344), (73728, 204800), (270336, 794624)]
    assert nt == [(128, 128), (256, 128), (512, 256), (1024, 512)]
    total, offs, _ = both([(40, 24, F, F), (5, 3, T, T)])   # unaligned sizes: padded to 8 elements
    assert (total, offs) == (2016, [(0, 960), (1920, 1984)])


def test_knn_shape_routing():
    """Shapes outside the fused kNN kernel route to the generic path (any C,
    k up to 8192, any N) instead of failing; its workspace query is exported."""
    from dgx import _native, ops
    assert ops.fast_shape(128, 64, 12288) and not ops.fast_shape(129, 20, 1024)
    assert not ops.fast_shape(3, 65, 1024) and not ops.fast_shape(3, 20, 12289)
    L = _native.lib()
    # |x|^2 (B*N, 16-byte rounded) + one chunk of dot rows (min(N, 2^24 / N rounded to 64) x N)
    assert L.dgx_knn_generic_workspace_bytes(2, 256, 1000) == (2000 + 1000 * 1000) * 4


def test_knn_limits_exported():
    """The kernels state their own shape limits (host queries of libdgx.so: no
    device needed): the fused kernel's C <= 128, k <= 64, N <= 12288, which
    ``ops.fast_shape`` and the C++ dispatch both ask for, and the generic
    kernel's k <= 8192."""
    from dgx import _native, ops
    L = _native.lib()
    assert L.dgx_knn_fast_shape(128, 64, 12288) == 1 and L.dgx_knn_fast_shape(129, 20, 1024) == 0
    assert L.dgx_knn_fast_shape(3, 65, 1024) == 0 and L.dgx_knn_fast_shape(3, 20, 12289) == 0
    for shape in ((1, 1, 1), (3, 20, 2048), (128, 64, 12288), (129, 64, 12288), (128, 65, 12288), (128, 64, 12289)):
        assert ops.fast_shape(*shape) is bool(L.dgx_knn_fast_shape(*shape)), shape
    assert L.dgx_knn_generic_max_k() == 8192
