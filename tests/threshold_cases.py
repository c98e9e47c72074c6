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
def special_at(name, n, C):
    """the construction of special_case(name) at another shape: the wide instances of the kernel (WIDE_SPECIAL)"""
    rng = np.random.RandomState(sum(map(ord, name)))
    if name == "infinities":          # theta = +inf, -inf, 0 against -0.0, +-inf and ordinary probabilities
        p, y = (a.copy() for a in quantised(n, C))
        p[::7, ::3] = -0.0
        p[3, :] = np.inf
        p[5, ::2] = -np.inf
        return p, y, np.array([np.inf, -np.inf, 0.0, 0.5], dtype=np.float32)
    if name == "nan":                 # NaN probabilities scattered, and a whole NaN row with and without targets
        p, y = (a.copy() for a in quantised(n, C))
        p[rng.rand(*p.shape) < 0.05] = np.nan
        p[17, :] = np.nan
        p[n // 2, :] = np.nan         # row n // 2 has no target: a NaN row that is exact
        return p, y, GRID7
    if name == "all_ones":            # every target 1 and everything predicted: the k = 2C bin; at 1.5 nothing is
        return np.ones((n, C), dtype=np.float32), np.ones((n, C), dtype=np.float32), GRID7
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def special_case(name):
    if name == "infinities":
        return special_at(name, 130, 70)
    if name == "nan":
        return special_at(name, 200, 103)
    if name == "all_ones":
        return special_at(name, 150, 65)
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


# ---- the launch plan of csrc/cgcn_threshold.hip, restated --------------------------------------------------------------------
# tests/test_gpu_thresholds.py pins plan()["groups"] to cgcn_debug_threshold_route for every (C, T): groups as a function of T
# gives TW (= waves * TT), and C gives the instance -- so a retuned threshold_plan fails that pin, not the coverage claims.
THR_MAX_C, THR_MAX_T, THR_MAX_WAVES = 1024, 64, 8
THR_MAX_ROWS, THR_MIN_ROWS, THR_GRID_X = 65535, 128, 512
THR_LDS_BYTES, THR_TILE_MIN_BYTES = 65536, 8192
INSTANCES = {1: (8, 8), 2: (8, 8), 3: (8, 8), 4: (8, 8), 8: (4, 8), 16: (2, 16)}       # CH -> (TT, NLD)


@functools.lru_cache(maxsize=None)
def _team_plan(C, T):
    assert 1 <= C <= THR_MAX_C and 1 <= T <= THR_MAX_T
    ch = (C + 63) // 64
    CH = ch if ch <= 4 else 8 if ch <= 8 else 16
    TT, NLD = INSTANCES[CH]
    per_t = 2 * (2 * C + 1) * 4                                  # rows and tpsum, uint32 [2C + 1] each
    fit = (THR_LDS_BYTES - THR_TILE_MIN_BYTES) // per_t
    waves = min((T + TT - 1) // TT, THR_MAX_WAVES, fit // TT)
    teams = THR_MAX_WAVES // waves
    TW = waves * TT
    groups = (T + TW - 1) // TW
    hist_bytes = min(TW, T) * per_t
    in_flight = 64 * waves * teams * NLD // C                    # rows the threads can hold in registers
    room = (THR_LDS_BYTES - hist_bytes) // (8 * C)               # rows the LDS has left beside the histograms
    last = T - (groups - 1) * TW                                 # thresholds of the last group
    live = (last + TT - 1) // TT
    return dict(CH=CH, TT=TT, NLD=NLD, waves=waves, teams=teams, TW=TW, groups=groups, tile_rows=min(in_flight, room),
                tile_by="lds" if room < in_flight else "registers", hist_bytes=hist_bytes, block=64 * waves * teams,
                spare=waves - live, last_nt=last - (live - 1) * TT)


def plan(n, C, T):
    """threshold_plan(n, C, T) as a dict: the kernel instance (CH, TT, NLD), waves per team, teams, thresholds per workgroup TW,
    groups (grid y), tile_rows and which of the two limits set them (tile_by), rows_per_wg, grid_x; and of the LAST group:
    spare = waves with no threshold, last_nt = thresholds of the last wave that has one.  (A copy: change it freely.)"""
    assert n >= 1
    rows = min(max((n + THR_GRID_X - 1) // THR_GRID_X, THR_MIN_ROWS), THR_MAX_ROWS)
    return dict(_team_plan(C, T), rows_per_wg=rows, grid_x=(n + rows - 1) // rows)


def plan_space():
    """every (CH, waves) pair that some 1 <= C <= 1024, 1 <= T <= 64 is launched with"""
    return {(q["CH"], q["waves"]) for q in (_team_plan(C, T) for C in range(1, THR_MAX_C + 1) for T in range(1, THR_MAX_T + 1))}


# ---- cases chosen by plan ----------------------------------------------------------------------------------------------------
# every instance at the edges of its label chunks (n = 300, GRID7): C -> CH
CHUNK_EDGE_C = {192: 3, 193: 4, 255: 4, 256: 4, 257: 8, 320: 8, 448: 8, 449: 8, 511: 8, 512: 8, 513: 16, 1023: 16, 1024: 16}
WIDE_SPECIAL = [("nan", 200, 257), ("nan", 200, 449), ("infinities", 130, 257), ("infinities", 130, 449),
                ("all_ones", 150, 1024)]
# one call per T = 1 .. 64 on n = 300 with per_label_matrix(64, C)[:T]: tests/test_thresholds_host.py holds the union of
# these plans to every (CH, waves) pair of plan_space(), a spare wave in every instance and last_nt = 1 and = TT in every
# instance.  (5 is one group at every T, so 60 brings the spare waves of CH = 1 -- 7 waves per team, T = 57 is a second
# group of one threshold; 600 stops at 2 waves per team, so 513 brings the 3 waves of CH = 16.)
SWEEP_N = 300
SWEEP_C = {5: 8, 60: 7, 65: 6, 103: 4, 129: 3, 200: 2, 257: 3, 300: 2, 513: 3, 600: 2}      # C -> the most waves per team it reaches
# one (C, T) per instance for the tile edges: the team shapes differ, and the tile is set by the LDS room in some and by the
# registers in flight in the others
TILE_PLANS = {1: (40, 40, "registers"), 2: (103, 27, "lds"), 3: (150, 7, "registers"), 4: (200, 16, "lds"),
              8: (300, 5, "registers"), 16: (600, 3, "lds")}         # CH -> (C, T, what sets tile_rows)
MIN_ROWS_SHAPES = [(103, 7), (300, 9)]          # (C, T) for n = 127, 128, 129


def sweep_case(C):
    p, y = quantised(SWEEP_N, C)
    return p, y, per_label_matrix(THR_MAX_T, C)


def tile_edge_rows(C, T):
    """[(n, workgroups)]: tile_rows * k - 1, tile_rows * k, tile_rows * k + 1 rows (the largest k that keeps them in one
    workgroup) as a single workgroup, and as the rows of the last of three workgroups"""
    q = plan(1, C, T)
    k = (THR_MIN_ROWS - 1) // q["tile_rows"]
    assert k >= 1
    tail = [q["tile_rows"] * k + d for d in (-1, 0, 1)]
    return [(m, 1) for m in tail] + [(2 * THR_MIN_ROWS + m, 3) for m in tail]


# ---- the 16-bit halves at their bound: C = 1 ---------------------------------------------------------------------------------
HALVES_N, HALVES_T = THR_GRID_X * THR_MAX_ROWS + 1, 33
HALVES_GRID = np.concatenate([np.array([-np.inf], dtype=np.float32), grid_of(HALVES_T - 1)])     # -inf: every row predicted


def halves_case(n):
    """(level index uint8 [n], targets float32 [n, 1]) of one label: rows 0 .. 65534 (the first workgroup of HALVES_N rows)
    are all positive, the rest at random.  The same first rows whatever n is."""
    rng = np.random.RandomState(65535)
    idx = rng.randint(0, LEVELS.size, size=n, dtype=np.uint8)
    y = rng.randint(0, 2, size=n, dtype=np.uint8).astype(np.float32)
    y[:THR_MAX_ROWS] = 1.0
    return idx, y.reshape(n, 1)


def single_label_counts(idx, targets, thr):
    """(pos, tp, pp, exact, rows, tpsum) at C = 1 from the joint histogram of (level, target) alone: a row is in bin
    k = [predicted] + [positive], and tpsum is non-zero in bin 2 only.  thr: float32 [T]."""
    y = (targets.reshape(-1) > np.float32(0.5)).astype(np.int64)
    joint = np.bincount(2 * idx.astype(np.int64) + y, minlength=2 * LEVELS.size).reshape(LEVELS.size, 2)
    T = thr.size
    tp, pp = np.zeros((T, 1), dtype=np.int64), np.zeros((T, 1), dtype=np.int64)
    exact, rows, tpsum = np.zeros(T, dtype=np.int64), np.zeros((T, 3), dtype=np.int64), np.zeros((T, 3), dtype=np.int64)
    for t in range(T):
        m = LEVELS >= thr[t]
        pp[t, 0], tp[t, 0] = joint[m].sum(), joint[m, 1].sum()
        rows[t] = joint[~m, 0].sum(), joint[~m, 1].sum() + joint[m, 0].sum(), joint[m, 1].sum()
        tpsum[t, 2] = rows[t, 2]
        exact[t] = rows[t, 0] + rows[t, 2]
    return joint[:, 1].sum(keepdims=True).astype(np.int64), tp, pp, exact, rows, tpsum
