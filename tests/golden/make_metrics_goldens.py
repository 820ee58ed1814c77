"""Generate tests/golden/seg_metrics.npz from the REFERENCE itself (build
container only), as make_loss_goldens.py does for the loss.

It imports the reference's main_partseg_dist (read-only; its module level only
defines things) and records, for seeded labels, what its epoch end computes:
calculate_shape_IoU (:63-84) and sklearn's accuracy_score /
balanced_accuracy_score on the flattened epoch (:277-283). plyfile, h5py and
cv2, which the module imports and this never calls, are stubbed when absent.
Only recorded numbers are stored; the tests import neither sklearn nor the
reference.

Two sets, labels as int16:
  all_*   41 shapes x 129 points over all 16 categories. Predictions are right
          for about 80 % of the points, the wrong ones drawn from all 50
          classes (so they land outside the shape's part range). Shape 0 is
          perfect; shape 16 (a motorbike, 6 parts) lacks two parts in both pred
          and seg (U == 0 -> IoU 1); class 49 (table) never occurs in seg but
          does in pred (balanced accuracy drops it).
  one_*   9 chairs x 129 points for the class_choice branch: labels shifted
          to start at 0, parts = range(seg_num[label[0]]).

  python tests/golden/make_metrics_goldens.py <path of the reference checkout>
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
N_POINTS = 129


def load_reference(ref):
    for name in ("plyfile", "h5py", "cv2"):
        try:
            __import__(name)
        except ImportError:
            stub = types.ModuleType(name)
            stub.PlyData = stub.PlyElement = None
            sys.modules[name] = stub
    sys.path.insert(0, ref)
    import main_partseg_dist
    return main_partseg_dist


def make_set(ref, rng, cats, shift):
    seg_num, index_start = ref.seg_num, ref.index_start
    B = len(cats)
    seg = np.empty((B, N_POINTS), np.int64)
    for b, c in enumerate(cats):
        seg[b] = (0 if shift else index_start[c]) + rng.integers(0, seg_num[c], N_POINTS)
    return seg


def noisy(rng, seg, n_class):
    wrong = rng.random(seg.shape) < 0.2
    return np.where(wrong, rng.integers(0, n_class, seg.shape), seg)


def scores(seg, pred):
    from sklearn import metrics
    return (metrics.accuracy_score(seg.reshape(-1), pred.reshape(-1)),
            metrics.balanced_accuracy_score(seg.reshape(-1), pred.reshape(-1)))


def main():
    ref = load_reference(sys.argv[1])
    rng = np.random.default_rng(20240607)
    out = {"part_start": np.asarray(ref.index_start, np.int32), "part_count": np.asarray(ref.seg_num, np.int32)}

    # every category, 41 shapes; shape 16 a motorbike (category 10)
    cats = np.concatenate([np.arange(16), rng.integers(0, 16, 25)])
    cats[16] = 10
    cats[cats == 15] = 14          # tables become skateboards below: class 49 ...
    cats[15] = 15                  # ... is left to one table
    seg = make_set(ref, rng, cats, shift=False)
    seg[15][seg[15] == 49] = 48    # ... which never shows its last part
    pred = noisy(rng, seg, 50)
    pred[0] = seg[0]                                       # a perfect shape
    for part in (33, 35):                                  # motorbike parts 3 and 5: in neither pred nor seg
        seg[16][seg[16] == part] = 30
    pred[16] = np.where(np.isin(pred[16], (33, 35)), 31, pred[16])
    pred[2][:3] = 49                                       # class 49 in pred only
    assert not (seg == 49).any() and (pred == 49).any() and set(cats) == set(range(16))
    label = cats.reshape(-1, 1)
    ious = ref.calculate_shape_IoU(pred, seg, label, None)
    assert ious[0] == 1.0
    acc, avg = scores(seg, pred)
    out.update(all_pred=pred.astype(np.int16), all_seg=seg.astype(np.int16), all_label=cats.astype(np.int16),
               all_shape_ious=np.asarray(ious, np.float64), all_acc=np.float64(acc), all_avg_acc=np.float64(avg))

    # class_choice = 'chair' (category 4, 4 parts), labels start at 0
    cats = np.full(9, 4)
    seg = make_set(ref, rng, cats, shift=True)
    pred = noisy(rng, seg, ref.seg_num[4])
    label = cats.reshape(-1, 1)
    ious = ref.calculate_shape_IoU(pred, seg, label, "chair")
    acc, avg = scores(seg, pred)
    out.update(one_pred=pred.astype(np.int16), one_seg=seg.astype(np.int16), one_label=cats.astype(np.int16),
               one_shape_ious=np.asarray(ious, np.float64), one_acc=np.float64(acc), one_avg_acc=np.float64(avg))

    path = os.path.join(HERE, "seg_metrics.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
