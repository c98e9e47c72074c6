"""The numpy restatement of the thresholded metrics (chromegcn_amd.thresholds: threshold_counts_host, metrics_from_counts,
best_thresholds) without a GPU: against what the reference's own functions returned (tests/golden/g11_thresholds.npz,
written by tests/golden/make_threshold_golden.py), against an independent brute-force loop, and on hand-made counts."""
import os

import numpy as np
import pytest
import torch

import threshold_cases as tc
from chromegcn_amd import thresholds as th

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g11_thresholds.npz")
FIELDS = ("pos", "tp", "pp", "exact", "rows", "tpsum")


def golden_cases():
    g = np.load(GOLDEN)
    assert np.array_equal(g["levels"], tc.LEVELS) and np.array_equal(g["grid"], tc.GRID7)
    assert [tuple(s) for s in g["shapes"]] == tc.GOLDEN_SHAPES
    for i, (n, C) in enumerate(tc.GOLDEN_SHAPES):
        p = g["levels"][g["idx_%d" % i]]
        y = np.unpackbits(g["y_%d" % i])[:n * C].reshape(n, C).astype(np.float32)
        yield (n, C), p, y, g["grid"], g["ref_%d" % i]


def test_metrics_match_the_reference_on_the_fixture():
    """Within 1e-6 absolute, NaN where and only where the reference gives NaN.  The reference computes in float32 (counts
    cast to float32, a handful of float32 operations, a float32 pairwise mean over at most 1000 values: about 10 roundings of
    6e-8 on values in [0, 1]); ours is exact integer counts, then float64."""
    worst = 0.0
    for shape, p, y, grid, ref in golden_cases():
        assert p.shape == shape and not np.isnan(p).any()
        assert (y[shape[0] // 2] == 0).all() and (p[shape[0] // 2] == 0).all()            # the all-empty row
        assert (y[:, -1] == 0).all() and (p[:, -1] < grid.min()).all()                    # the dead label
        m = th.threshold_metrics_host(p, y, grid)
        for j, key in enumerate(th.METRIC_KEYS):
            got, want = m[key], ref[:, j]
            assert got.shape == (grid.size,) and got.dtype == np.float64
            assert np.array_equal(np.isnan(got), np.isnan(want)), (shape, key, got, want)
            ok = ~np.isnan(want)
            if ok.any():
                worst = max(worst, float(np.abs(got[ok] - want[ok]).max()))
            assert np.all(np.abs(got[ok] - want[ok]) <= 1e-6), (shape, key, got, want)
    print("worst difference to the reference: %.3g" % worst)


def test_ties_are_predicted_on_the_fixture():
    """p == theta counts as predicted: with > instead of >= the counts differ at every threshold that is a level"""
    (_, p, y, grid, _), = [c for c in golden_cases() if c[0] == (257, 103)]
    c = th.threshold_counts_host(p, y, grid)
    for t, theta in enumerate(grid[:-1]):
        assert (p == theta).sum() > 1000
        assert c.pp[t].sum() == (p >= theta).sum() > (p > theta).sum()
    assert c.pp[-1].sum() == 0                                                            # 1.5: nothing is predicted


@pytest.mark.parametrize("name", ["small", "infinities", "nan", "square_matrix"])
def test_counts_equal_a_brute_force_loop(name):
    if name == "small":
        (p, y), thr = tc.quantised(40, 9), tc.GRID7
    else:
        p, y, thr = tc.special_case(name)
        if np.ndim(thr) == 1:                      # a shared grid: a corner of the case is enough for the loop
            p, y = p[:48, :11], y[:48, :11]
    got = th.threshold_counts_host(p, y, thr)
    want = tc.brute_force_counts(p, y, th.threshold_matrix(thr, p.shape[1]))
    for f, w in zip(FIELDS, want):
        g = getattr(got, f)
        assert g.dtype == np.int64 and g.shape == w.shape and np.array_equal(g, w), (name, f)
    assert got.n == p.shape[0] and got.C == p.shape[1]
    assert got.rows.sum(axis=1).tolist() == [p.shape[0]] * got.tp.shape[0]                # every row is in one bin


def test_the_three_threshold_forms():
    p, y = tc.quantised(64, 7)
    one = th.threshold_counts_host(p, y, 0.5)
    assert one.thresholds.shape == (1, 7) and one.thresholds.dtype == np.float32 and (one.thresholds == 0.5).all()
    grid = th.threshold_counts_host(p, y, [0.3, 0.5])
    as_tensor = th.threshold_counts_host(p, y, torch.tensor([0.3, 0.5], dtype=torch.float64))
    full = th.threshold_counts_host(p, y, np.repeat(np.array([[0.3], [0.5]]), 7, axis=1))
    for f in FIELDS:
        assert np.array_equal(getattr(grid, f), getattr(as_tensor, f)) and np.array_equal(getattr(grid, f), getattr(full, f))
        assert np.array_equal(np.atleast_1d(getattr(grid, f))[-1] if f != "pos" else grid.pos,
                              np.atleast_1d(getattr(one, f))[0] if f != "pos" else one.pos)
    assert th.threshold_counts_host(p, y, 0.1).thresholds[0, 0] == np.float32(0.1)       # rounded to float32 on the way in
    per_label = tc.per_label_matrix(7, 7)
    a, b = th.threshold_counts_host(p, y, per_label), th.threshold_counts_host(p, y, per_label.T.copy())
    assert not np.array_equal(a.pp, b.pp)                                                 # [t][c] is not [c][t]
    with pytest.raises(ValueError):
        th.threshold_counts_host(p, y, np.zeros((2, 6)))
    with pytest.raises(ValueError):
        th.threshold_counts_host(p, y, [])


@pytest.mark.parametrize("bad", [float("nan"), [0.5, float("nan")], np.array([[0.5] * 6 + [np.nan]])])
def test_a_nan_threshold_raises(bad):
    p, y = tc.quantised(64, 7)
    with pytest.raises(ValueError, match="NaN"):
        th.threshold_counts_host(p, y, bad)
    with pytest.raises(ValueError, match="NaN"):
        th.threshold_matrix(bad, 7)


def test_metrics_from_hand_made_counts():
    # n = 4, C = 2, one threshold; rows (Y | P): (11|11) (10|00) (00|00) (01|11)
    c = th.ThresholdCounts(pos=np.array([2, 2]), tp=np.array([[1, 2]]), pp=np.array([[2, 2]]), exact=np.array([2]),
                           rows=np.array([[1, 1, 0, 1, 1]]), tpsum=np.array([[0, 0, 0, 1, 2]]), n=4, C=2,
                           thresholds=np.array([[0.5, 0.5]], dtype=np.float32))
    m = th.metrics_from_counts(c)
    assert m["ACC"][0] == 0.5 and m["HA"][0] == 1 - 2 / 8
    assert m["miF1"][0] == 6 / 8 and m["maF1"][0] == (2 / 4 + 4 / 4) / 2
    assert m["ebF1"][0] == (0 / 1 + 2 * 1 / 3 + 2 * 2 / 4) / 3                            # the empty row is left out
    assert m["precision"].tolist() == [[0.5, 1.0]] and m["recall"].tolist() == [[0.5, 1.0]]
    empty = th.ThresholdCounts(pos=np.array([0]), tp=np.array([[0]]), pp=np.array([[0]]), exact=np.array([3]),
                               rows=np.array([[3, 0, 0]]), tpsum=np.array([[0, 0, 0]]), n=3, C=1,
                               thresholds=np.array([[0.5]], dtype=np.float32))
    m = th.metrics_from_counts(empty)
    assert m["ACC"][0] == 1.0 and m["HA"][0] == 1.0
    assert all(np.isnan(m[k][0]) for k in ("ebF1", "miF1", "maF1")) and np.isnan(m["f1"]).all()


def test_best_thresholds_on_a_hand_made_table():
    # four grid rows, four labels (10, 10, 0, 0 positives).  f1 = 2 tp / (pp + pos)
    #   label 0: a single best row (row 2)        label 1: rows 1 and 3 tie -- the first wins
    #   label 2: never positive, never predicted: undefined on every row       label 3: defined on the last row only
    pos = np.array([10, 10, 0, 0])
    tp = np.array([[10, 4, 0, 0], [8, 6, 0, 0], [9, 5, 0, 0], [2, 6, 0, 0]])
    pp = np.array([[40, 10, 0, 0], [14, 10, 0, 0], [10, 12, 0, 0], [2, 10, 0, 3]])
    grid = np.array([0.1, 0.3, 0.5, 0.7], dtype=np.float32)
    z = np.zeros((4, 9), dtype=np.int64)
    c = th.ThresholdCounts(pos, tp, pp, np.zeros(4, dtype=np.int64), z, z, 50, 4, th.threshold_matrix(grid, 4))
    best = th.best_thresholds(c)
    assert best.dtype == np.float32 and best.shape == (4,)
    assert best[0] == np.float32(0.5) and best[1] == np.float32(0.3) and np.isnan(best[2])
    assert best[3] == np.float32(0.7)              # the only row where it is defined (0 / 3)
    f1 = th.metrics_from_counts(c)["f1"]
    assert np.isnan(f1[:, 2]).all() and np.isnan(f1[:3, 3]).all() and f1[3, 3] == 0.0
    with pytest.raises(ValueError):
        th.best_thresholds(c, criterion="precision")
    # per-label thresholds: the chosen entry is the label's own column
    thr = np.arange(16, dtype=np.float32).reshape(4, 4) / 16
    best = th.best_thresholds(c._replace(thresholds=thr))
    assert best[0] == thr[2, 0] and best[1] == thr[1, 1]
