"""Two models compared label by label (scripts/analyze_results.py:69,97-168): the numbers behind the paper's figure of
per-label improvement of the GCN over the CNN against the label's average Hi-C degree -- the difference per label, the paired
t-test, the regression of the difference on the degree, and how many labels of every group improved.  Host only: the inputs
are [C] arrays of per-label metrics (chromegcn_amd.metrics) and of weights (LabelStats.average_degree)."""
from __future__ import annotations

from typing import Dict

import numpy as np


def compare_labels(metric_a, metric_b, weights=None, label_groups=None) -> Dict[str, object]:
    """metric_a, metric_b: [C] per-label values of one metric for model a (the baseline; the reference's CNN) and model b (its
    GCN).  Labels with a NaN in either array -- and, with `weights`, labels with a NaN weight -- are dropped first; the
    result lists them.  Returns
      kept, dropped     int64 index arrays (ascending)
      diff              b - a on the kept labels (analyze_results.py:99)
      t, p              scipy.stats.ttest_rel(a, b) on the kept labels (:69,111), NaN with fewer than two
    with weights ([C], e.g. the labels' average degree):
      order             the kept labels in stable ascending order of weight (:103); weights_sorted, diff_sorted in that order
      slope, intercept, r, p_regress, stderr    scipy.stats.linregress(weights, diff) (:164), NaN with fewer than two labels or
                        when every weight is the same
    with label_groups (a mapping group name -> label indices, as metrics.group_means takes):
      groups            {name: {"improved": labels with diff >= 0, "worse": labels with diff < 0}} over the group's kept labels
                        (:116-136)."""
    from scipy import stats
    a = np.asarray(metric_a, dtype=np.float64).ravel()
    b = np.asarray(metric_b, dtype=np.float64).ravel()
    if a.shape != b.shape:
        raise ValueError("compare_labels: the two metric arrays must have the same length, got %d and %d" % (a.size, b.size))
    ok = ~(np.isnan(a) | np.isnan(b))
    w = None
    if weights is not None:
        w = np.asarray(weights, dtype=np.float64).ravel()
        if w.shape != a.shape:
            raise ValueError("compare_labels: weights must have one entry per label")
        ok &= ~np.isnan(w)
    kept = np.flatnonzero(ok).astype(np.int64)
    ak, bk = a[kept], b[kept]
    diff = bk - ak
    out: Dict[str, object] = {"kept": kept, "dropped": np.flatnonzero(~ok).astype(np.int64), "diff": diff,
                              "t": float("nan"), "p": float("nan")}
    if kept.size >= 2:
        res = stats.ttest_rel(ak, bk)
        out["t"], out["p"] = float(res[0]), float(res[1])
    if w is not None:
        wk = w[kept]
        order = np.argsort(wk, kind="stable")
        out.update(order=kept[order], weights_sorted=wk[order], diff_sorted=diff[order])
        reg = dict.fromkeys(("slope", "intercept", "r", "p_regress", "stderr"), float("nan"))
        if kept.size >= 2 and np.ptp(wk) > 0:
            lr = stats.linregress(wk, diff)
            reg = {"slope": float(lr[0]), "intercept": float(lr[1]), "r": float(lr[2]), "p_regress": float(lr[3]),
                   "stderr": float(lr[4])}
        out.update(reg)
    if label_groups is not None:
        d_full = np.full(a.shape, np.nan)
        d_full[kept] = diff
        groups = {}
        for name, idx in label_groups.items():
            d = d_full[np.asarray(list(idx), dtype=np.int64)]
            d = d[~np.isnan(d)]
            groups[name] = {"improved": int((d >= 0).sum()), "worse": int((d < 0).sum())}
        out["groups"] = groups
    return out
