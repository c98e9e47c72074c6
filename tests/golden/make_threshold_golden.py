"""Writes tests/golden/g11_thresholds.npz: the fixture of tests/test_thresholds_host.py -- what the reference's own five
binary-relevance functions (utils/metrics.py:29-109) return on seeded inputs for a grid of thresholds.

    levels [10] fp32, grid [7] fp32 (tests/threshold_cases.py: LEVELS, GRID7), shapes [6, 2]
    per shape i:  idx_i  uint8 [n, C]   the probabilities as indices into levels (many equal a threshold exactly)
                  y_i    uint8          np.packbits of the 0 / 1 targets [n, C]
                  ref_i  fp64 [7, 5]    per threshold: ACC, HA, ebF1, miF1, maF1 as the reference returns them (its float32
                                        values, NaN where it gives NaN), with y_hat = (p >= theta) as float32:
                                        subset_accuracy(y, y_hat, axis=1), 1 - hamming_loss(y, y_hat, axis=1),
                                        example_f1_score(y, y_hat, axis=1), f1_score(y, y_hat, 'micro' | 'macro', axis=0)
Every shape has a label that is never positive and never predicted and an all-empty row; there is no NaN probability (the
reference leaves NaN in its thresholded matrix, and its results for them mean nothing).  Data only.

Run from the repository root where the reference is mounted: CHROMEGCN_REFERENCE=<its root> python
tests/golden/make_threshold_golden.py (the reference's module imports scikit-learn, scipy and pandas)."""
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ref = os.environ.get("CHROMEGCN_REFERENCE")
    if not ref:
        raise SystemExit("set CHROMEGCN_REFERENCE to the root of the reference")
    sys.path.insert(0, ref)
    import threshold_cases as tc
    from utils import metrics as ref_metrics       # the reference

    out = {"levels": tc.LEVELS, "grid": tc.GRID7, "shapes": np.array(tc.GOLDEN_SHAPES, dtype=np.int64)}
    for i, (n, C) in enumerate(tc.GOLDEN_SHAPES):
        idx, y = tc.level_case(n, C, 1000 * n + C)
        p = tc.LEVELS[idx]
        res = np.zeros((tc.GRID7.size, 5), dtype=np.float64)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")        # means of empty arrays, 0 / 0: the NaN the fixture records
            for t, theta in enumerate(tc.GRID7):
                y_hat = (p >= theta).astype(np.float32)
                res[t] = [ref_metrics.subset_accuracy(y, y_hat, axis=1), 1 - ref_metrics.hamming_loss(y, y_hat, axis=1),
                          ref_metrics.example_f1_score(y, y_hat, axis=1), ref_metrics.f1_score(y, y_hat, "micro", axis=0),
                          ref_metrics.f1_score(y, y_hat, "macro", axis=0)]
        out["idx_%d" % i] = idx
        out["y_%d" % i] = np.packbits(y.astype(np.uint8))
        out["ref_%d" % i] = res
        print("%5d x %-4d" % (n, C), np.array2string(res[3], precision=6), "NaN:", int(np.isnan(res).sum()))
    path = os.path.join(ROOT, "tests", "golden", "g11_thresholds.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
