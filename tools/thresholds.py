"""Thresholded multi-label metrics (ACC, HA, ebF1, miF1, maF1 and per-label precision / recall / F1) from saved predictions,
on the GPU: what scripts/analyze_results.py:63-66 tabulates for its threshold grid through utils/metrics.py:29-109.

--preds / --targets: [n, C] arrays saved with torch.save (.pt) or numpy (.npy), as for tools/curves.py.
--grid: comma-separated thresholds shared by all labels, or "reference": the 27 values of scripts/analyze_results.py:63.
--cutoffs roc: instead of a grid, one threshold per label -- chromegcn_amd.curves.optimal_cutoffs of the same predictions
    (labels without both classes have no cutoff: they get +inf and are never predicted).
Written to --out, one .npz: thresholds [T, C] float32; the int64 counts pos, tp, pp, exact, rows, tpsum
(chromegcn_amd.thresholds.ThresholdCounts); ACC, HA, ebF1, miF1, maF1 [T]; precision, recall, f1 [T, C] float64; and
best_f1_thresholds [C] float32 (per label the grid value with the largest F1)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from chromegcn_amd import curves, thresholds  # noqa: E402
from tools.curves import load_matrix  # noqa: E402

REFERENCE_GRID = [0.01, 0.02, 0.03, 0.04, 0.05, 0.06, 0.07, 0.08, 0.09, 0.10, 0.15, 0.20, 0.25, 0.30, 0.35, 0.40, 0.45, 0.50,
                  0.55, 0.60, 0.65, 0.70, 0.75, 0.8, 0.85, 0.9, 0.95]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--preds", required=True)
    ap.add_argument("--targets", required=True)
    which = ap.add_mutually_exclusive_group(required=True)
    which.add_argument("--grid", default=None, help='comma-separated thresholds, or "reference"')
    which.add_argument("--cutoffs", default=None, choices=["roc"])
    ap.add_argument("--gpu-id", type=int, default=0)
    ap.add_argument("--out", required=True)
    opt = ap.parse_args(argv)
    preds, targets = load_matrix(opt.preds), load_matrix(opt.targets)
    if preds.shape != targets.shape:
        raise SystemExit("predictions %s and targets %s differ in shape" % (tuple(preds.shape), tuple(targets.shape)))
    if opt.grid is not None:
        grid = REFERENCE_GRID if opt.grid == "reference" else [float(v) for v in opt.grid.split(",")]
    if not torch.cuda.is_available():
        raise SystemExit("tools/thresholds.py needs a GPU (the HIP path has no CPU fallback)")
    dev = torch.device("cuda", opt.gpu_id)
    torch.cuda.set_device(dev)
    p, t = preds.to(dev), targets.to(dev)
    if opt.cutoffs:
        cut = curves.optimal_cutoffs(p, t)
        grid = torch.where(torch.isnan(cut), torch.full_like(cut, float("inf")), cut)[None]
    counts = thresholds.threshold_counts(p, t, grid)
    host = thresholds._host(counts)
    out = {"thresholds": host.thresholds}
    out.update({k: getattr(host, k) for k in ("pos", "tp", "pp", "exact", "rows", "tpsum")})
    m = thresholds.metrics_from_counts(host)
    out.update(m)
    out["best_f1_thresholds"] = thresholds.best_thresholds(host)
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    np.savez(opt.out, **out)
    at = int(np.nanargmax(m["miF1"])) if not np.isnan(m["miF1"]).all() else 0
    print(json.dumps({"n": int(preds.shape[0]), "C": int(preds.shape[1]), "T": int(host.thresholds.shape[0]),
                      "best_miF1": float(m["miF1"][at]), "at_row": at, "out": opt.out}))


if __name__ == "__main__":
    main()
