"""ROC curves, precision-recall curves and optimal cutoffs of every label from saved predictions (what
scripts/analyze_results.py:387 draws through utils/evals.py:28-84), on the GPU.  It plots nothing.

--preds / --targets: [n, C] arrays saved with torch.save (.pt: the reference's epochs/best_test_preds_metrics.pt and
best_test_targets_metrics.pt) or numpy (.npy).  Written to --out, one .npz:
    roc_offsets [C + 1] int64; roc_tps, roc_fps int32; roc_thresholds float32; roc_fpr, roc_tpr float64
        label c's ROC points are [roc_offsets[c], roc_offsets[c + 1]), the origin (threshold inf) first
    pr_offsets, pr_tps, pr_fps, pr_thresholds, pr_precision, pr_recall: the same for the precision-recall curves, in
        descending order of threshold and without scikit-learn's terminal (1, 0) point
    cutoffs [C] float32: the threshold where tpr = 1 - fpr is closest (NaN for a single-class label)
    auroc, aupr, recall_at_fdr, average_precision [C] float32
--groups: a JSON file {"tfbs": [label indices], "hm": [...], "dnase": [...]}: group_names and group_meanAUC / group_meanAUPR /
group_meanFDR (one value per group, means over the group's labels with a defined value) are added."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from chromegcn_amd import curves, metrics  # noqa: E402


def load_matrix(path):
    """[n, C] float32 tensor from a .pt (a tensor or array saved with torch.save) or .npy file"""
    if path.endswith(".npy"):
        a = torch.from_numpy(np.load(path, allow_pickle=False))
    else:
        a = torch.as_tensor(torch.load(path, map_location="cpu", weights_only=False))
    if a.dim() != 2:
        raise SystemExit("%s: expected a matrix [n, C], found shape %s" % (path, tuple(a.shape)))
    return a.float()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--preds", required=True)
    ap.add_argument("--targets", required=True)
    ap.add_argument("--groups", default=None, help="JSON: group name -> list of label indices")
    ap.add_argument("--keep-intermediate", action="store_true", help="roc_curve(drop_intermediate=False)")
    ap.add_argument("--gpu-id", type=int, default=0)
    ap.add_argument("--out", required=True)
    opt = ap.parse_args(argv)
    preds, targets = load_matrix(opt.preds), load_matrix(opt.targets)
    if preds.shape != targets.shape:
        raise SystemExit("predictions %s and targets %s differ in shape" % (tuple(preds.shape), tuple(targets.shape)))
    groups = None
    if opt.groups:
        with open(opt.groups) as f:
            groups = json.load(f)
        for g, idx in groups.items():
            if any(not 0 <= int(i) < preds.shape[1] for i in idx):
                raise SystemExit("group %s names a label outside 0 .. %d" % (g, preds.shape[1] - 1))
    if not torch.cuda.is_available():
        raise SystemExit("tools/curves.py needs a GPU (the HIP path has no CPU fallback)")
    dev = torch.device("cuda", opt.gpu_id)
    torch.cuda.set_device(dev)
    p, t = preds.to(dev), targets.to(dev)
    roc = curves.roc_curves(p, t, drop_intermediate=not opt.keep_intermediate)
    pr = curves.pr_curves(p, t)
    cut = curves.cutoffs_of(roc) if not opt.keep_intermediate else curves.optimal_cutoffs(p, t)
    per_label = {k: v.cpu().numpy() for k, v in metrics.multilabel_metrics(p, t).items()}
    out = {"cutoffs": cut.cpu().numpy(), **per_label}
    for tag, obj, derived in (("roc", roc, ("fpr", "tpr")), ("pr", pr, ("precision", "recall"))):
        for name in ("offsets", "tps", "fps", "thresholds") + derived:
            out["%s_%s" % (tag, name)] = getattr(obj, name).cpu().numpy()
    if groups is not None:
        means = metrics.group_means(per_label, groups)
        out["group_names"] = np.array(list(groups))
        for name in ("meanAUC", "meanAUPR", "meanFDR"):
            out["group_" + name] = np.array([means["%s_%s" % (g, name)] for g in groups], dtype=np.float64)
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    np.savez(opt.out, **out)
    print(json.dumps({"n": int(preds.shape[0]), "C": int(preds.shape[1]), "roc_points": int(roc.tps.numel()),
                      "pr_points": int(pr.tps.numel()), "out": opt.out}))


if __name__ == "__main__":
    main()
