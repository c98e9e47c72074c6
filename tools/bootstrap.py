"""Block-bootstrap confidence intervals of the multi-label metrics from saved predictions, on the GPU
(chromegcn_amd/bootstrap.py); with a second prediction set, the paired comparison of the two models under the same
replicates.  It plots nothing.

--preds / --preds-b / --targets: [n, C] matrices as tools/analyze_results.py reads them (.pt, .npy, or .npz[::array]), the
    chromosomes one after the other.  --preds-b is the second model: differences are preds - preds-b.
--lengths: JSON, {"chr3": 12345, ...} or [["chr3", 12345], ...] in the order of the rows: the chromosomes become strata.
--groups: JSON {"tfbs": [label indices], "hm": [...], "dnase": [...]}.
Written to --out, one .npz -- per metric m of auroc, aupr, recall_at_fdr, average_precision: m [C] (the point estimate),
m_ci_low, m_ci_high, m_se, m_n_valid [C]; scalar_names and scalar_point / _ci_low / _ci_high / _se / _n_valid, one value per
name (meanAUC, meanAUPR, meanFDR, mAP and the group means).  With --preds-b the same arrays describe the DIFFERENCE, m_a and
m_b hold both models' point estimates, and m_p / scalar_p the two-sided p-values.  --keep-replicates adds m_replicates
[n_boot, C] and scalar_replicates [n_boot, names]."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from chromegcn_amd import bootstrap as B  # noqa: E402
from analyze_results import load_lengths, load_matrix  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--preds", required=True)
    ap.add_argument("--preds-b", default=None)
    ap.add_argument("--targets", required=True)
    ap.add_argument("--lengths", default=None)
    ap.add_argument("--groups", default=None)
    ap.add_argument("--n-boot", type=int, default=1000)
    ap.add_argument("--block", type=int, default=50)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--level", type=float, default=0.95)
    ap.add_argument("--fdr-cutoff", type=float, default=0.5)
    ap.add_argument("--keep-replicates", action="store_true")
    ap.add_argument("--gpu-id", type=int, default=0)
    ap.add_argument("--out", required=True)
    opt = ap.parse_args(argv)
    pa, tg = load_matrix(opt.preds), load_matrix(opt.targets)
    pb = load_matrix(opt.preds_b) if opt.preds_b else None
    if pa.shape != tg.shape or (pb is not None and pb.shape != tg.shape):
        raise SystemExit("predictions and targets differ in shape")
    lengths = None
    if opt.lengths:
        _, lengths = load_lengths(opt.lengths)
        if sum(lengths) != tg.shape[0]:
            raise SystemExit("the lengths sum to %d but there are %d rows" % (sum(lengths), tg.shape[0]))
    groups = None
    if opt.groups:
        with open(opt.groups) as f:
            groups = json.load(f)
    if not torch.cuda.is_available():
        raise SystemExit("tools/bootstrap.py needs a GPU (the HIP path has no CPU fallback)")
    dev = torch.device("cuda", opt.gpu_id)
    torch.cuda.set_device(dev)
    kw = dict(n_boot=opt.n_boot, seed=opt.seed, block=opt.block, lengths=lengths, level=opt.level, label_groups=groups,
              fdr_cutoff=opt.fdr_cutoff, keep_replicates=opt.keep_replicates)
    if pb is None:
        res = B.bootstrap_metrics(pa.to(dev), tg.to(dev), **kw)
        centre, fields = res.point, ("ci_low", "ci_high", "se", "n_valid")
    else:
        res = B.bootstrap_compare(pa.to(dev), pb.to(dev), tg.to(dev), **kw)
        centre, fields = res.diff, ("ci_low", "ci_high", "se", "n_valid", "p")
    out = {}
    for m in B.METRICS:
        out[m] = centre[m]
        for f in fields:
            out["%s_%s" % (m, f)] = getattr(res, f)[m]
        if pb is not None:
            out[m + "_a"], out[m + "_b"] = res.a[m], res.b[m]
        if opt.keep_replicates:
            out[m + "_replicates"] = res.replicates[m]
    names = list(res.scalars)
    out["scalar_names"] = np.array(names)
    for f in (("point",) if pb is None else ("diff", "a", "b")) + fields:
        out["scalar_" + f] = np.array([res.scalars[k][f] for k in names])
    if opt.keep_replicates:
        out["scalar_replicates"] = np.stack([res.scalar_replicates[k] for k in names], 1)
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    np.savez(opt.out, **out)
    key = "point" if pb is None else "diff"
    print(json.dumps({"n": int(tg.shape[0]), "C": int(tg.shape[1]), "n_boot": opt.n_boot, "block": opt.block, "out": opt.out,
                      "scalars": {k: {f: res.scalars[k][f] for f in (key, "ci_low", "ci_high") + (("p",) if pb is not None else ())}
                                  for k in names}}))


if __name__ == "__main__":
    main()
