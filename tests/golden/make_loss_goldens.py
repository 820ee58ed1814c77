"""Generate tests/golden/loss_small.npz from the REFERENCE itself (build
container only), as make_goldens.py does for the other modules.

It imports the reference's loss.cross_entropy (loss.py:4-21; read-only, nothing
is written there) and records, for (M, C) = (37, 50), (5, 2), (64, 13) and
smoothing True / False: seeded fp32 logits, int64 labels, the reference's loss
and its autograd gradient on the host. Labels cover class 0 and class C - 1.

  python tests/golden/make_loss_goldens.py
"""
import importlib.util
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
SHAPES = [(37, 50), (5, 2), (64, 13)]


def main():
    spec = importlib.util.spec_from_file_location("reference_loss", os.path.join(REF, "loss.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    out = {"shapes": np.asarray(SHAPES, np.int64)}
    for M, C in SHAPES:
        g = torch.Generator().manual_seed(1000 * M + C)
        logits = torch.randn(M, C, generator=g) * 2.0
        labels = torch.randint(0, C, (M,), generator=g)
        labels[0], labels[-1] = 0, C - 1
        tag = f"m{M}_c{C}"
        out[f"{tag}_logits"] = logits.numpy()
        out[f"{tag}_labels"] = labels.numpy()
        for smoothing in (True, False):
            x = logits.clone().requires_grad_(True)
            loss = ref.cross_entropy(x, labels.view(-1, 1), smoothing=smoothing)
            loss.backward()
            kind = "smooth" if smoothing else "plain"
            out[f"{tag}_{kind}_loss"] = loss.detach().numpy()
            out[f"{tag}_{kind}_grad"] = x.grad.numpy()
    path = os.path.join(HERE, "loss_small.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
