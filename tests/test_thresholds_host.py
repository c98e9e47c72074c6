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


# ---- the launch plan restated in threshold_cases.plan: its invariants, and what the GPU cases chosen with it reach -----------
# (tests/test_gpu_thresholds.py pins plan()["groups"] to the library for every (C, T))
ALL_CT = [(C, T) for C in range(1, tc.THR_MAX_C + 1) for T in range(1, tc.THR_MAX_T + 1)]


def test_plan_invariants_over_every_label_and_threshold_count():
    assert len(ALL_CT) == 65536
    for C, T in ALL_CT:
        q = tc.plan(300, C, T)
        assert 1 <= q["waves"] <= 8 and q["teams"] == 8 // q["waves"] and q["block"] <= 512, (C, T)
        assert q["tile_rows"] >= 1, (C, T)
        assert q["tile_rows"] * C <= 64 * q["waves"] * q["teams"] * q["NLD"], (C, T)     # a tile fits the registers in flight
        assert q["hist_bytes"] + q["tile_rows"] * C * 8 <= 65536, (C, T)                 # ... and the LDS beside the histograms
        assert 64 * q["CH"] >= C and (q["TT"], q["NLD"]) == tc.INSTANCES[q["CH"]], (C, T)
        assert q["TW"] == q["waves"] * q["TT"] and (q["groups"] - 1) * q["TW"] < T <= q["groups"] * q["TW"], (C, T)
        assert 0 <= q["spare"] < q["waves"] and 1 <= q["last_nt"] <= q["TT"], (C, T)
        assert (q["groups"] - 1) * q["TW"] + (q["waves"] - q["spare"] - 1) * q["TT"] + q["last_nt"] == T, (C, T)
    for n in (1, 127, 128, 129, 65536, 65537, tc.HALVES_N - 1, tc.HALVES_N, 1 << 40):
        q = tc.plan(n, 7, 3)
        assert 128 <= q["rows_per_wg"] <= 65535 and (q["grid_x"] - 1) * q["rows_per_wg"] < n <= q["grid_x"] * q["rows_per_wg"]


def test_the_plan_space_has_25_team_shapes_and_four_odd_blocks():
    space = tc.plan_space()
    assert len(space) == 25 and {ch for ch, _ in space} == set(tc.INSTANCES)
    assert {w for ch, w in space if ch == 1} == set(range(1, 9))
    assert {tc.plan(1, C, T)["block"] for C, T in ALL_CT} == {320, 384, 448, 512}


def test_the_sweep_reaches_every_team_shape_spare_waves_and_full_and_single_last_waves():
    plans = [tc.plan(tc.SWEEP_N, C, T) for C in tc.SWEEP_C for T in range(1, tc.THR_MAX_T + 1)]
    assert {(q["CH"], q["waves"]) for q in plans} == tc.plan_space()
    assert {q["block"] for q in plans} == {320, 384, 448, 512}
    for CH, (TT, _) in tc.INSTANCES.items():
        mine = [q for q in plans if q["CH"] == CH]
        assert any(q["spare"] >= 1 for q in mine), CH
        assert any(q["last_nt"] == 1 for q in mine) and any(q["last_nt"] == TT for q in mine), CH
        assert any(q["groups"] > 1 and q["last_nt"] < TT for q in mine), CH       # a short wave read at blockIdx.y > 0
    for C, most in tc.SWEEP_C.items():
        assert {tc.plan(tc.SWEEP_N, C, T)["waves"] for T in range(1, tc.THR_MAX_T + 1)} == set(range(1, most + 1)), C
    assert all(q["grid_x"] == 3 for q in plans)                                    # more than one workgroup, the last short


def test_the_chosen_cases_are_on_the_paths_they_name():
    for C, CH in tc.CHUNK_EDGE_C.items():
        assert tc.plan(300, C, 7)["CH"] == CH
    assert sorted(tc.TILE_PLANS) == sorted(tc.INSTANCES)
    limits = set()
    for CH, (C, T, tile_by) in tc.TILE_PLANS.items():
        q = tc.plan(1, C, T)
        assert q["CH"] == CH and q["tile_by"] == tile_by
        limits.add(tile_by)
        ns = tc.tile_edge_rows(C, T)
        assert [g for _, g in ns] == [1, 1, 1, 3, 3, 3]
        for n, g in ns:
            qn = tc.plan(n, C, T)
            tail = n - (g - 1) * qn["rows_per_wg"]
            assert qn["grid_x"] == g and 0 < tail <= qn["rows_per_wg"] and tail > q["tile_rows"] - 2
        assert [(n - ns[1][0]) for n, _ in ns[:3]] == [-1, 0, 1] and ns[1][0] % q["tile_rows"] == 0
    assert limits == {"lds", "registers"}
    assert {tc.plan(1, C, T)["waves"] for C, T, _ in tc.TILE_PLANS.values()} >= {1, 2, 4, 5}
    q = tc.plan(tc.HALVES_N, 1, tc.HALVES_T)
    assert (q["rows_per_wg"], q["grid_x"], q["teams"], q["groups"]) == (65535, 513, 1, 1)
    assert tc.HALVES_N - 512 * 65535 == 1 and tc.HALVES_GRID.size == tc.HALVES_T and tc.HALVES_GRID[0] == -np.inf


def test_single_label_shortcut_equals_the_restatement():
    n = 100000
    idx, y = tc.halves_case(n)
    assert (y[:65535] == 1).all() and 0 < y[65535:].sum() < n - 65535
    got = tc.single_label_counts(idx, y, tc.HALVES_GRID)
    want = th.threshold_counts_host(tc.LEVELS[idx].reshape(n, 1), y, tc.HALVES_GRID)
    for f, g in zip(FIELDS, got):
        w = getattr(want, f)
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), f
    assert got[2][0, 0] == n and got[1][0, 0] == got[0][0]                          # -inf: every row is predicted
    small = tc.brute_force_counts(tc.LEVELS[idx[:300]].reshape(300, 1), y[:300], tc.HALVES_GRID.reshape(-1, 1))
    for f, g, w in zip(FIELDS, tc.single_label_counts(idx[:300], y[:300], tc.HALVES_GRID), small):
        assert np.array_equal(g, w), f


def test_special_at_rebuilds_the_special_cases():
    p, y, thr = tc.special_at("nan", 200, 449)
    assert p.shape == (200, 449) and np.isnan(p[17]).all() and np.isnan(p[100]).all() and (y[100] == 0).all()
    assert 0.03 < np.isnan(p).mean() < 0.08 and thr is tc.GRID7
    p, y, thr = tc.special_at("infinities", 130, 257)
    assert (p[3] == np.inf).all() and (p[5, ::2] == -np.inf).all() and np.signbit(p[0, 0]) and p[0, 0] == 0
    p, y, thr = tc.special_at("all_ones", 150, 1024)
    c = th.threshold_counts_host(p, y, thr)
    assert (c.rows[:-1, 2048] == 150).all() and (c.tpsum[:-1, 2048] == 150 * 1024).all() and c.rows[-1, 1024] == 150
