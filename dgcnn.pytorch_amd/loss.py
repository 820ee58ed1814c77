"""Drop-in for the reference's ``loss`` module (loss.py:4-21), which
main_partseg_dist.py imports (main_partseg_dist.py:30): the label-smoothed cross
entropy of (M, n_class) logits, run by the engine's loss head
(dgx.loss.smoothed_cross_entropy: one forward and one backward kernel on the
device, torch's own expression on host tensors)."""
from dgx.loss import smoothed_cross_entropy


def cross_entropy(pred, gold, smoothing=True):
    """Cross entropy of ``pred`` (M, n_class) against the labels ``gold`` (any
    shape with M elements); with ``smoothing`` the target puts 1 - 0.2 on the
    labelled class and 0.2 / (n_class - 1) on every other."""
    return smoothed_cross_entropy(pred, gold.contiguous().view(-1), smoothing=smoothing)
