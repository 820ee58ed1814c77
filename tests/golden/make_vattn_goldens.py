"""Generate the vector-attention fixtures from the REFERENCE itself (build
container only), as make_goldens.py does for the other modules.

It imports the reference's models.attention / models.transformer (read-only;
nothing is written there; they need einops) and records on the host, fp32:

  vattn_small.npz        VectorAttention (emb 32, d_qkv 64, k 10, clouds
                         (2, 3, 128), key != query): inputs, initial weights,
                         output, and for a fixed g every parameter and input
                         gradient (query, key, value, canonical)
  mhvattn_small.npz      MultiHeadVectorAttention (n_heads 2), the same
  vtransformer_small.npz Transformer (emb 16, d_qkv 16, ff 32, n_blocks 1,
                         dropout 0, k 10, training): inputs, initial state,
                         both outputs, gradients of parameters and src / tgt for
                         fixed g, and the state (BN running statistics) after
  mhattn_small.npz       MultiHeadedAttention (h 4, d_model 32, dropout 0) on
                         (2, 40, 32) query / key / value: the same
  vattn_keys.json        the state_dict key lists of the four

Arrays are named ``in_*``, ``w_<state key>``, ``out*``, ``g*`` (the fixed
output gradients), ``grad_<parameter name>``, ``gin_*`` and ``after_<key>``.

  python tests/golden/make_vattn_goldens.py
"""
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"


def _cloud(B, N, gen):
    return torch.rand(B, 3, N, generator=gen) * 2 - 1


def _save(name, out):
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < (1 << 20), (path, size)
    print(path, size, "bytes")


def _attention_case(cls, args, seed, name):
    gen = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    m = cls(args).train()
    B, N = 2, 128
    ins = {"query": torch.randn(B, N, args.emb_dim, generator=gen), "key": torch.randn(B, N, args.emb_dim, generator=gen),
           "value": torch.randn(B, N, args.emb_dim, generator=gen), "canonical": _cloud(B, N, gen)}
    g = torch.randn(B, N, args.emb_dim, generator=gen)
    out = {f"in_{k}": v.numpy().copy() for k, v in ins.items()}
    out.update({f"w_{k}": v.detach().numpy().copy() for k, v in m.state_dict().items()})
    leaves = {k: v.clone().requires_grad_(True) for k, v in ins.items()}
    y = m(leaves["query"], leaves["key"], leaves["value"], leaves["canonical"])
    y.backward(g)
    out["out"], out["g"] = y.detach().numpy(), g.numpy()
    out.update({f"grad_{k}": p.grad.numpy() for k, p in m.named_parameters()})
    out.update({f"gin_{k}": v.grad.numpy() for k, v in leaves.items()})
    _save(name, out)
    return list(m.state_dict().keys())


def _transformer_case(Transformer, seed, name):
    args = types.SimpleNamespace(emb_dim=16, d_qkv=16, ff_dims=32, n_blocks=1, dropout=0.0, k=10, n_heads=4)
    gen = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    m = Transformer(args).train()
    B, N = 2, 128
    ins = {"src": torch.randn(B, 16, N, generator=gen), "tgt": torch.randn(B, 16, N, generator=gen),
           "pointcloud": _cloud(B, N, gen)}
    g0, g1 = torch.randn(B, 16, N, generator=gen), torch.randn(B, 16, N, generator=gen)
    out = {f"in_{k}": v.numpy().copy() for k, v in ins.items()}
    out.update({f"w_{k}": v.detach().numpy().copy() for k, v in m.state_dict().items()})
    src, tgt = ins["src"].clone().requires_grad_(True), ins["tgt"].clone().requires_grad_(True)
    y0, y1 = m(src, tgt, ins["pointcloud"])
    torch.autograd.backward([y0, y1], [g0, g1])
    out.update({"out0": y0.detach().numpy(), "out1": y1.detach().numpy(), "g0": g0.numpy(), "g1": g1.numpy(),
                "gin_src": src.grad.numpy(), "gin_tgt": tgt.grad.numpy()})
    out.update({f"grad_{k}": p.grad.numpy() for k, p in m.named_parameters()})
    out.update({f"after_{k}": v.detach().numpy().copy() for k, v in m.state_dict().items()})
    _save(name, out)
    return list(m.state_dict().keys())


def _mha_case(MultiHeadedAttention, seed, name):
    gen = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    m = MultiHeadedAttention(4, 32, dropout=0.0).train()
    ins = {k: torch.randn(2, 40, 32, generator=gen) for k in ("query", "key", "value")}
    g = torch.randn(2, 40, 32, generator=gen)
    out = {f"in_{k}": v.numpy().copy() for k, v in ins.items()}
    out.update({f"w_{k}": v.detach().numpy().copy() for k, v in m.state_dict().items()})
    leaves = {k: v.clone().requires_grad_(True) for k, v in ins.items()}
    y = m(leaves["query"], leaves["key"], leaves["value"])
    y.backward(g)
    out["out"], out["g"] = y.detach().numpy(), g.numpy()
    out.update({f"grad_{k}": p.grad.numpy() for k, p in m.named_parameters()})
    out.update({f"gin_{k}": v.grad.numpy() for k, v in leaves.items()})
    _save(name, out)
    return list(m.state_dict().keys())


def main():
    sys.path.insert(0, REF)   # `models` below is the reference's
    from models.attention import MultiHeadedAttention, MultiHeadVectorAttention, VectorAttention
    from models.transformer import Transformer
    keys = {
        "VectorAttention": _attention_case(
            VectorAttention, types.SimpleNamespace(emb_dim=32, d_qkv=64, k=10), 11, "vattn_small.npz"),
        "MultiHeadVectorAttention": _attention_case(
            MultiHeadVectorAttention, types.SimpleNamespace(emb_dim=32, k=10, n_heads=2), 12, "mhvattn_small.npz"),
        "Transformer": _transformer_case(Transformer, 13, "vtransformer_small.npz"),
        "MultiHeadedAttention": _mha_case(MultiHeadedAttention, 14, "mhattn_small.npz"),
    }
    with open(os.path.join(HERE, "vattn_keys.json"), "w") as f:
        json.dump(keys, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
