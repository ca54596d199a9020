"""Generator of tests/golden/g12_metrics.npz: the reference's own ``calculate_metrics`` (xrays/train_xrays_example.py:260-295)
on seeded inputs, stored as plain arrays -- inputs and the three outputs, no reference source text.

    python tests/golden/make_g12_metrics.py --reference <checkout of the reference> [--out tests/golden/g12_metrics.npz]

Needs the reference checkout, CPU torch and sklearn.  The logits lie on the grid of multiples of 1/8 in [-6, 6]: 97 values for
300 rows, so every class is full of ties, and float32 sigmoid is injective and increasing on the grid (asserted below), so the
reference -- which ranks float32 sigmoids -- and a ranking of the logits themselves see the same order and the same ties, and
``sigmoid(x) > 0.5`` is ``x > 0``.  Class 4 has no positive (the reference leaves it out of mAP and gives it F1 = 0) and
class 5 scores every positive below zero (F1 = 0: left out of the reference's macro F1)."""
import argparse
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="directory of the reference checkout")
    ap.add_argument("--out", default=os.path.join(HERE, "g12_metrics.npz"))
    args = ap.parse_args()
    sys.path.insert(0, args.reference)              # the example imports the reference package beside it
    spec = importlib.util.spec_from_file_location("ref_xrays", os.path.join(args.reference, "xrays", "train_xrays_example.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)

    grid = np.arange(-48, 49, dtype=np.float32) / 8
    sig = torch.sigmoid(torch.from_numpy(grid)).numpy()
    assert sig.dtype == np.float32 and np.all(np.diff(sig) > 0), "float32 sigmoid is not injective on the grid"
    assert np.array_equal(sig > 0.5, grid > 0)

    g = np.random.default_rng(12)
    n, c = 300, 6
    labels = (g.random((n, c)) < 0.25).astype(np.float32)
    logits = grid[np.clip(np.round(g.standard_normal((n, c)) * 14 + 8 * (labels - 0.3)).astype(np.int64) + 48, 0, 96)]
    labels[:, 4] = 0.0
    logits[:, 5] = np.where(labels[:, 5] > 0, -np.abs(logits[:, 5]) - 0.125, logits[:, 5])
    assert np.isin(logits, grid).all()
    map_score, macro_f1, f1_scores = ref.calculate_metrics(torch.from_numpy(logits), torch.from_numpy(labels))
    np.savez(args.out, logits=logits, labels=labels.astype(np.uint8), map=np.float64(map_score), macro_f1=np.float64(macro_f1),
             f1=np.asarray(f1_scores, dtype=np.float64))
    print(f"{args.out}: {n} x {c}, map {map_score:.6f} macro_f1 {macro_f1:.6f} f1 {np.round(f1_scores, 4)}")


if __name__ == "__main__":
    main()
