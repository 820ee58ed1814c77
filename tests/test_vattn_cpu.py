"""Host path of models.attention / models.transformer against the reference's
own results (tests/golden/make_vattn_goldens.py): output 1e-5, gradients 2e-4
(rel_err), state_dict keys equal; and the fp64 restatement tests/_vattn_ref.py,
the GPU tests' oracle, pinned to the same fixtures."""
import json
import os
import types

import numpy as np
import pytest
import torch

import _vattn_ref as VR
from conftest import GOLDEN, load_golden, rel_err

OUT_TOL, GRAD_TOL = 1e-5, 2e-4


def _t(a, grad=False):
    return torch.from_numpy(np.asarray(a).copy()).requires_grad_(grad)


def _load_state(module, z, prefix="w_"):
    module.load_state_dict({k: _t(z[prefix + k]) for k in module.state_dict().keys()})


def _keys():
    with open(os.path.join(GOLDEN, "vattn_keys.json")) as f:
        return json.load(f)


def _args(**kw):
    return types.SimpleNamespace(**kw)


def _check_grads(z, module, leaves, zero=()):
    """``zero``: name endings of parameters whose gradient is exactly 0 in real
    arithmetic (a bias added just before a training-mode BatchNorm): there the
    reference's values and ours are both rounding noise, which has no relative
    error; both must vanish at GRAD_TOL of the largest parameter gradient."""
    scale = max(float(np.abs(z["grad_" + n]).max()) for n, _ in module.named_parameters())
    for name, p in module.named_parameters():
        if name.endswith(tuple(zero)) and zero:
            assert float(np.abs(z["grad_" + name]).max()) <= GRAD_TOL * scale, name
            assert float(p.grad.abs().max()) <= GRAD_TOL * scale, name
            continue
        assert rel_err(p.grad.numpy(), z["grad_" + name]) <= GRAD_TOL, name
    for name, t in leaves.items():
        assert rel_err(t.grad.numpy(), z["gin_" + name]) <= GRAD_TOL, name


def test_state_dict_keys_match_reference():
    from models.attention import MultiHeadedAttention, MultiHeadVectorAttention, VectorAttention
    from models.transformer import Transformer
    keys = _keys()
    assert list(VectorAttention(_args(emb_dim=32, d_qkv=64, k=10)).state_dict()) == keys["VectorAttention"]
    assert (list(MultiHeadVectorAttention(_args(emb_dim=32, k=10, n_heads=2)).state_dict())
            == keys["MultiHeadVectorAttention"])
    assert list(MultiHeadedAttention(4, 32).state_dict()) == keys["MultiHeadedAttention"]
    targs = _args(emb_dim=16, d_qkv=16, ff_dims=32, n_blocks=1, dropout=0.0, k=10, n_heads=4)
    assert list(Transformer(targs).state_dict()) == keys["Transformer"]


@pytest.mark.parametrize("which", ["VectorAttention", "MultiHeadVectorAttention"])
def test_vector_attention_host_matches_reference(which):
    import models.attention as MA
    z = load_golden("vattn_small.npz" if which == "VectorAttention" else "mhvattn_small.npz")
    args = _args(emb_dim=32, d_qkv=64, k=10, n_heads=2)
    m = getattr(MA, which)(args).train()
    _load_state(m, z)
    leaves = {n: _t(z["in_" + n], True) for n in ("query", "key", "value", "canonical")}
    y = m(leaves["query"], leaves["key"], leaves["value"], leaves["canonical"])
    assert rel_err(y.detach().numpy(), z["out"]) <= OUT_TOL
    y.backward(_t(z["g"]))
    _check_grads(z, m, leaves)


def test_multi_headed_attention_host_matches_reference():
    from models.attention import MultiHeadedAttention
    z = load_golden("mhattn_small.npz")
    m = MultiHeadedAttention(4, 32, dropout=0.0).train()
    _load_state(m, z)
    leaves = {n: _t(z["in_" + n], True) for n in ("query", "key", "value")}
    y = m(leaves["query"], leaves["key"], leaves["value"])
    assert rel_err(y.detach().numpy(), z["out"]) <= OUT_TOL
    y.backward(_t(z["g"]))
    _check_grads(z, m, leaves)


def test_transformer_host_matches_reference():
    from models.transformer import Transformer
    z = load_golden("vtransformer_small.npz")
    m = Transformer(_args(emb_dim=16, d_qkv=16, ff_dims=32, n_blocks=1, dropout=0.0, k=10, n_heads=4)).train()
    _load_state(m, z)
    leaves = {n: _t(z["in_" + n], True) for n in ("src", "tgt")}
    y0, y1 = m(leaves["src"], leaves["tgt"], _t(z["in_pointcloud"]))
    assert rel_err(y0.detach().numpy(), z["out0"]) <= OUT_TOL
    assert rel_err(y1.detach().numpy(), z["out1"]) <= OUT_TOL
    torch.autograd.backward([y0, y1], [_t(z["g0"]), _t(z["g1"])])
    # every sublayer's last bias (and the feed-forward BatchNorm's shift, which w_2 turns into one) is a
    # per-channel constant added to the residual stream right before the next BatchNorm
    _check_grads(z, m, leaves, zero=("to_out.bias", "w_2.bias", "feed_forward.norm.bias"))
    for k, v in m.state_dict().items():   # BatchNorm running statistics after the step
        if v.is_floating_point():
            assert rel_err(v.numpy(), z["after_" + k]) <= OUT_TOL, k
        else:
            assert int(v) == int(z["after_" + k]), k


def test_batch_local_gathers_each_clouds_own_rows():
    """batch_local=True (engine extension): each cloud's own D / V rows and its
    transposed (N, 3) positions, against the fp64 restatement; the clouds are
    then independent of one another."""
    from dgx import cpu
    from models.attention import VectorAttention
    torch.manual_seed(3)
    m = VectorAttention(_args(emb_dim=8, d_qkv=16, k=4), batch_local=True)
    x, pts = torch.randn(2, 24, 8), torch.rand(2, 3, 24)
    y = m(x, x, x, pts)
    want = VR.module(m.state_dict(), x, x, x, pts, cpu.knn(pts, 4), batch_local=True)
    assert rel_err(y.detach().numpy(), want.detach().numpy()) <= OUT_TOL
    assert torch.equal(m(x[1:], x[1:], x[1:], pts[1:]), y[1:])


def test_features_of_later_clouds_do_not_reach_the_output():
    """The reference's local-id gather: clouds b >= 1 use their own graph and
    centre row but cloud 0's D / V rows, so changing their features changes nothing."""
    from models.attention import VectorAttention
    torch.manual_seed(4)
    m = VectorAttention(_args(emb_dim=8, d_qkv=16, k=4))
    x, pts = torch.randn(3, 20, 8), torch.rand(3, 3, 20)
    x2 = x.clone()
    x2[1:] = torch.randn(2, 20, 8)
    assert torch.equal(m(x, x, x, pts), m(x2, x2, x2, pts))


def test_restatement_pinned_to_reference():
    """tests/_vattn_ref.py in fp64 on the VectorAttention fixture: output and
    gradients as the reference's fp32 run (its own distance from fp64 is 4-6e-7
    on the output, 1-2e-5 on parameter gradients)."""
    from dgx import cpu
    z = load_golden("vattn_small.npz")
    state = {k[2:]: _t(z[k]).double().requires_grad_(True) for k in z.files if k.startswith("w_")}
    ins = {n: _t(z["in_" + n]).double().requires_grad_(n != "canonical") for n in ("query", "key", "value", "canonical")}
    idx = cpu.knn(_t(z["in_canonical"]), 10)
    y = VR.module(state, ins["query"], ins["key"], ins["value"], ins["canonical"], idx)
    assert rel_err(y.detach().numpy(), z["out"]) <= OUT_TOL
    y.backward(_t(z["g"]).double())
    for name, p in state.items():
        assert rel_err(p.grad.numpy(), z["grad_" + name]) <= GRAD_TOL, name
    for n in ("query", "key", "value"):
        assert rel_err(ins[n].grad.numpy(), z["gin_" + n]) <= GRAD_TOL, n
    # the bf16-rounded yardstick moves the output by about 1e-3, not more
    yb = VR.module(state, ins["query"], ins["key"], ins["value"], ins["canonical"], idx, bf16=True)
    e = rel_err(yb.detach().numpy(), y.detach().numpy())
    assert 1e-5 < e < 1e-2, e


def test_fused_shape_limits_exported():
    """The kernel states its own shape limits (host queries of libdgx.so)."""
    from dgx import vattn
    assert vattn.fused_shape(64, 256, 64, 1) and vattn.fused_shape(64, 256, 64, 64)
    assert not vattn.fused_shape(64, 256, 64, 65) and not vattn.fused_shape(64, 256, 64, 0)
    assert not vattn.fused_shape(32, 128, 64, 20) and not vattn.fused_shape(64, 256, 32, 20)
    assert vattn.fwd_points() >= 1


def test_host_op_registered():
    from dgx import host
    host.load()
    head = "dgx_host::vattn_forward(Tensor D, Tensor V, Tensor pos, Tensor idx, int gather_stride, Tensor[] weights"
    assert str(torch.ops.dgx_host.vattn_forward.default._schema).startswith(head)
