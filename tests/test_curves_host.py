"""The numpy restatements of chromegcn_amd.curves -- the specification the device arrays are held to -- against scikit-learn's
own roc_curve / precision_recall_curve on every case of tests/curves_cases.py, by exact equality; the cutoff rule against a
direct float64 evaluation; and the label-group means of metrics.compute_metrics through their host helper.  No GPU needed."""
import inspect
import warnings

import numpy as np
import pytest
from sklearn.metrics import precision_recall_curve, roc_curve

import curves_cases as cc
from chromegcn_amd import curves, metrics


def same(a, b):
    """equal element for element, NaN positions too, and the same dtype"""
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def _labels(preds, targets):
    for c in range(preds.shape[1]):
        yield c, targets[:, c].astype(np.int64), preds[:, c]


CASES = cc.all_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatements_equal_sklearn_bit_for_bit(name):
    preds, targets = CASES[name]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")     # sklearn warns about single-class labels; they are cases here
        for c, y, s in _labels(preds, targets):
            for drop in (True, False):
                want = roc_curve(y, s, drop_intermediate=drop)
                got = curves.roc_curve_host(y, s, drop_intermediate=drop)
                assert all(same(g, w) for g, w in zip(got, want)), (name, c, drop)
            want = precision_recall_curve(y, s)
            got = curves.pr_curve_host(y, s)
            assert all(same(g, w) for g, w in zip(got, want)), (name, c)


def test_the_cases_hold_what_they_are_named_for():
    preds, targets, names = cc.runs_case()
    for c, (first, last) in enumerate(cc.RUNS.values()):
        s, _ = cc.mc.sorted_view(preds[:, c], targets[:, c])
        ends = cc.mc.run_ends_of(s)
        assert last in ends and not ((ends >= first) & (ends < last)).any() and first - 1 in ends, names[c]
    first, last = cc.RUNS["covers_middle_chunk"]
    assert first < cc.CHUNK and last >= 2 * cc.CHUNK and last - first + 1 == 5000
    preds, targets, names = cc.corner_case()
    for c, name in enumerate(names):
        fps, tps, thr = curves.roc_points_host(targets[:, c], preds[:, c], True)
        pos = (fps + tps - 1)[1:]           # sorted positions of the kept points (the origin aside)
        if name.startswith("last_corner_"):
            x = int(name.rsplit("_", 1)[1])
            assert x in pos and not ((pos > 3000) & (pos < x)).any(), name
        if name.startswith("first_corner_"):
            x = int(name.rsplit("_", 1)[1])
            assert x in pos and not ((pos > x) & (pos < 9000)).any() and 9000 in pos, name
        if name == "collinear":
            lo, hi = cc.COLLINEAR
            assert lo - 1 in pos and hi in pos and not ((pos >= lo) & (pos < hi)).any()
            assert (lo - 1) // cc.CHUNK == 0 and hi // cc.CHUNK == 2
        if name == "two_points":
            assert fps.size == 3
        if name == "three_points_collinear":
            assert fps.size == 3 and curves.roc_points_host(targets[:, c], preds[:, c], False)[0].size == 4
        if name == "three_points_bent":
            assert fps.size == 4
    preds, targets, names = cc.degenerate_case()
    t = dict(zip(names, targets.T))
    assert t["all_positive"].all() and not t["all_negative"].any() and t["one_positive"].sum() == 1
    assert t["one_negative"].sum() == cc.DEGENERATE_N - 1
    for name in ("saturated_half", "saturated_rare"):
        s = preds[:, names.index(name)]
        assert (s == 1.0).sum() > cc.CHUNK and (s == 0.0).sum() > cc.CHUNK
    assert [cc.mc.pack_rows(C) for C in cc.WIDTHS] == [128, 64]
    assert -(-cc.MANY_N // cc.CHUNK) == 65


def _cutoff_direct(y, s):
    """the rule evaluated point by point in float64 from sklearn's own curve counts"""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        fpr, tpr, thr = roc_curve(y, s)
    P, N = int((y > 0).sum()), int((y <= 0).sum())
    if P == 0 or N == 0:
        return np.float32(np.nan), None
    best, at, vals = None, None, []
    for j in range(thr.size):
        v = abs(np.float64(tpr[j]) - (np.float64(1.0) - np.float64(fpr[j])))
        vals.append(v)
        if best is None or v < best:
            best, at = v, j
    return np.float32(thr[at]), np.array(vals)


@pytest.mark.parametrize("name", sorted(cc.small_cases()) + ["edge_n1_C3_q1", "edge_n65_C3_q16", "edge_n4097_C3_q3"])
def test_cutoff_restatement_equals_the_rule(name):
    preds, targets = CASES[name]
    for c, y, s in _labels(preds, targets):
        want, _ = _cutoff_direct(y, s)
        got = curves.optimal_cutoff_host(y, s)
        assert got.dtype == np.float32 and same(got, want), (name, c)


def test_cutoff_tie_goes_to_the_earliest_point():
    preds, targets, names = cc.corner_case()
    c = names.index("tie")
    y, s = targets[:, c].astype(np.int64), preds[:, c]
    want, vals = _cutoff_direct(y, s)
    low = np.flatnonzero(vals == vals.min())
    assert low.size == 2 and vals[low[0]].tobytes() == vals[low[1]].tobytes() and vals.min() == 0.25   # a tie, bit for bit
    srt, _ = cc.mc.sorted_view(s, targets[:, c])
    assert want == srt[3 * cc.TIE_M - 1] and want > srt[5 * cc.TIE_M - 1]     # the point before the run, not the run's
    assert curves.optimal_cutoff_host(y, s) == want
    one_class = curves.optimal_cutoff_host(np.ones(5), np.linspace(0.1, 0.9, 5, dtype=np.float32))
    assert np.isnan(one_class) and np.isnan(curves.optimal_cutoff_host(np.zeros(5), np.linspace(0.1, 0.9, 5, dtype=np.float32)))


def test_group_means_are_means_over_the_defined_labels():
    rng = np.random.RandomState(3)
    C = 12
    per_label = {k: rng.rand(C) for k in ("auroc", "aupr", "recall_at_fdr", "average_precision")}
    per_label["auroc"][[1, 4, 5]] = np.nan
    per_label["recall_at_fdr"][4] = np.nan
    groups = {"tfbs": [0, 1, 2, 3], "hm": [4, 5], "dnase": [6, 7, 8, 9, 10, 11]}
    out = metrics.group_means(per_label, groups)
    assert sorted(out) == sorted("%s_%s" % (g, m) for g in groups for m in ("meanAUC", "meanAUPR", "meanFDR"))
    for g, idx in groups.items():
        for key, name in (("auroc", "meanAUC"), ("aupr", "meanAUPR"), ("recall_at_fdr", "meanFDR")):
            v = per_label[key][idx]
            v = v[~np.isnan(v)]
            if v.size:
                assert out["%s_%s" % (g, name)] == float(np.mean(v)), (g, name)
            else:
                assert np.isnan(out["%s_%s" % (g, name)]), (g, name)
    assert np.isnan(out["hm_meanAUC"]) and not np.isnan(out["hm_meanAUPR"])      # a group with every label undefined
    assert out["tfbs_meanAUC"] == float(np.mean(per_label["auroc"][[0, 2, 3]]))
    assert metrics.group_means(per_label, {}) == {}


def test_label_groups_is_a_keyword_that_defaults_to_none():
    sig = inspect.signature(metrics.compute_metrics)
    assert sig.parameters["label_groups"].default is None
    assert list(sig.parameters)[:9] == ["all_predictions", "all_targets", "loss", "args", "elapsed", "data_dict", "cell_type",
                                        "device", "verbose"]


def test_device_entry_points_refuse_cpu_tensors():
    import torch
    p, t = torch.rand(8, 2), torch.zeros(8, 2)
    for fn in (curves.roc_curves, curves.pr_curves, curves.optimal_cutoffs):
        with pytest.raises(RuntimeError, match="must be on the GPU"):
            fn(p, t)
