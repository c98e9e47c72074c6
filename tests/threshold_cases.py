"""Inputs for tests/test_thresholds_host.py and tests/test_gpu_thresholds.py (and tests/golden/make_threshold_golden.py):
probabilities drawn from a short list of float32 LEVELS, so that many of them equal a threshold exactly, and the special
values of the threshold rule.  Builders only: nothing here touches the GPU.  The arrays are shared between tests
(lru_cache): do not write to them."""
import functools

import numpy as np

# every grid value but 1.5 is a level: p == theta on a large share of the elements
LEVELS = np.array([0.0, 0.01, 0.05, 0.2, 0.3, 0.5, 0.7, 0.9, 0.95, 1.0], dtype=np.float32)
LEVEL_P = np.array([0.55, 0.05, 0.05, 0.05, 0.05, 0.05, 0.05, 0.05, 0.05, 0.05])
GRID7 = np.array([0.01, 0.05, 0.3, 0.5, 0.7, 0.95, 1.5], dtype=np.float32)        # at 1.5 nothing is predicted
# scripts/analyze_results.py:63: the reference's 27-value grid
GRID27 = np.array([0.01, 0.02, 0.03, 0.04, 0.05, 0.06, 0.07, 0.08, 0.09, 0.10, 0.15, 0.20, 0.25, 0.30, 0.35, 0.40, 0.45,
                   0.50, 0.55, 0.60, 0.65, 0.70, 0.75, 0.8, 0.85, 0.9, 0.95], dtype=np.float32)
GOLDEN_SHAPES = [(1, 1), (7, 3), (64, 64), (65, 65), (257, 103), (1000, 129)]


def level_case(n, C, seed):
    """(level index uint8 [n, C], targets float32 [n, C]): targets lean to the high levels; row n // 2 is all empty (no
    target, probability 0) and label C - 1 is never positive and has probability 0 (never predicted above threshold 0)"""
    rng = np.random.RandomState(seed)
    idx = rng.choice(LEVELS.size, size=(n, C), p=LEVEL_P).astype(np.uint8)
    y = (rng.rand(n, C) < 0.03 + 0.8 * LEVELS[idx]).astype(np.float32)
    idx[n // 2, :] = 0
    y[n // 2, :] = 0.0
    idx[:, C - 1] = 0
    y[:, C - 1] = 0.0
    return idx, y


@functools.lru_cache(maxsize=None)
def quantised(n, C, seed=None):
    """(probs, targets) float32 [n, C] of level_case"""
    idx, y = level_case(n, C, 1000 * n + C if seed is None else seed)
    return np.ascontiguousarray(LEVELS[idx]), np.ascontiguousarray(y)


def brute_force_counts(probs, targets, thr):
    """(pos, tp, pp, exact, rows, tpsum) as int64 arrays by a loop over thresholds, rows and labels: independent of numpy's
    reductions and of np.bincount.  thr: float32 [T, C]."""
    n, C = probs.shape
    T = thr.shape[0]
    pos = np.zeros(C, dtype=np.int64)
    tp, pp = np.zeros((T, C), dtype=np.int64), np.zeros((T, C), dtype=np.int64)
    exact = np.zeros(T, dtype=np.int64)
    rows, tpsum = np.zeros((T, 2 * C + 1), dtype=np.int64), np.zeros((T, 2 * C + 1), dtype=np.int64)
    for i in range(n):
        for c in range(C):
            pos[c] += 1 if targets[i, c] > 0.5 else 0
    for t in range(T):
        for i in range(n):
            k = both = 0
            same = True
            for c in range(C):
                y = bool(targets[i, c] > 0.5)
                p = bool(np.float32(probs[i, c]) >= np.float32(thr[t, c]))      # False for a NaN probability
                k += int(y) + int(p)
                both += int(y and p)
                same = same and (y == p)
                pp[t, c] += int(p)
                tp[t, c] += int(y and p)
            exact[t] += int(same)
            rows[t, k] += 1
            tpsum[t, k] += both
    return pos, tp, pp, exact, rows, tpsum


# ---- the GPU cases: name -> (probs, targets, thresholds as threshold_counts takes them) ------------------------------------
EDGE_N = [1, 63, 64, 65, 1000]
EDGE_C = [1, 63, 64, 65, 103, 128, 129]


def per_label_matrix(T, C):
    """[T, C] float32 of levels, threshold (t, c) = LEVELS[(2 t + 3 c + t c) % 10]: rows differ by label and the matrix is not
    symmetric -- reading it as [c][t] changes the decisions"""
    t, c = np.meshgrid(np.arange(T), np.arange(C), indexing="ij")
    return np.ascontiguousarray(LEVELS[(2 * t + 3 * c + t * c) % LEVELS.size])


@functools.lru_cache(maxsize=None)
def special_case(name):
    rng = np.random.RandomState(sum(map(ord, name)))
    if name == "infinities":          # theta = +inf, -inf, 0 against -0.0, +-inf and ordinary probabilities
        p, y = (a.copy() for a in quantised(130, 70))
        p[::7, ::3] = -0.0
        p[3, :] = np.inf
        p[5, ::2] = -np.inf
        return p, y, np.array([np.inf, -np.inf, 0.0, 0.5], dtype=np.float32)
    if name == "nan":                 # NaN probabilities scattered, and a whole NaN row with and without targets
        p, y = (a.copy() for a in quantised(200, 103))
        p[rng.rand(*p.shape) < 0.05] = np.nan
        p[17, :] = np.nan
        p[100, :] = np.nan            # row 100 = n // 2 has no target: a NaN row that is exact
        return p, y, GRID7
    if name == "all_ones":            # every target 1 and everything predicted: the k = 2C bin; at 1.5 nothing is
        return np.ones((150, 65), dtype=np.float32), np.ones((150, 65), dtype=np.float32), GRID7
    if name == "all_zero":            # the k = 0 bin only
        return np.zeros((150, 65), dtype=np.float32), np.zeros((150, 65), dtype=np.float32), GRID7[1:]
    if name == "soft_targets":        # targets 0.0 / 0.9999 instead of 0 / 1
        p, y = quantised(300, 103)
        return p, (y * np.float32(0.9999)).astype(np.float32), GRID7
    if name == "per_label":
        p, y = quantised(500, 37)
        return p, y, per_label_matrix(9, 37)
    if name == "square_matrix":       # T == C: a transposed read would still be in bounds
        p, y = quantised(200, 5)
        return p, y, per_label_matrix(5, 5)
    raise KeyError(name)


SPECIAL = ["infinities", "nan", "all_ones", "all_zero", "soft_targets", "per_label", "square_matrix"]
# (n, C, T): many workgroups and the project's grid | the T limits | the routes of large C (several passes)
SHAPES = {"grid27": (70001, 103, 27), "t64": (2000, 103, 64), "t1": (2000, 103, 1), "c1024": (3000, 1024, 64),
          "c600": (3000, 600, 40)}


def grid_of(T):
    """T float32 thresholds: the 27-value grid, then levels and values between them"""
    extra = np.linspace(0.005, 0.995, 199, dtype=np.float64).astype(np.float32)
    return np.concatenate([GRID27, LEVELS, extra])[:T] if T > 1 else np.array([0.5], dtype=np.float32)


@functools.lru_cache(maxsize=None)
def shape_case(name):
    n, C, T = SHAPES[name]
    p, y = quantised(n, C)
    return p, y, grid_of(T)
