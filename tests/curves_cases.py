"""Inputs for tests/test_curves_host.py and tests/test_gpu_curves.py: labels built BY RANK, so that the sorted position of
every element, every run of tied scores and every curve point is known from the construction -- run ends and ROC corners at
stated positions around the 4096-element chunks of chromegcn_amd/csrc/cgcn_metrics.hip.  Builders only: nothing here
touches the GPU.  The arrays are shared between tests (lru_cache): do not write to them.

A "sorted position" is an index into one label's list after a stable descending sort by score; a label is described by
the level of every sorted position (equal level = tied score) and the target at it, then its rows are shuffled."""
import functools

import numpy as np

import metrics_cases as mc

CHUNK = mc.CHUNK


def label(level, target, rng):
    """(scores, targets) float32 [n], rows shuffled: sorted position i has score number level[i] (non-decreasing; level k
    of m maps to the float32 (m - k) / (m + 1), strictly descending in k) and target target[i]"""
    level = np.asarray(level, dtype=np.int64)
    assert level[0] == 0 and ((np.diff(level) == 0) | (np.diff(level) == 1)).all()
    m = int(level[-1]) + 1
    values = ((m - np.arange(m, dtype=np.float64)) / (m + 1)).astype(np.float32)
    assert (np.diff(values) < 0).all() and values[-1] > 0
    perm = rng.permutation(level.size)
    return values[level][perm], np.asarray(target, dtype=np.float32)[perm]


def levels_with_runs(n, runs):
    """level of every sorted position of a list of n elements whose only ties are the runs [first, last] (inclusive) given"""
    step = np.ones(n, dtype=np.int64)
    step[0] = 0
    for first, last in runs:
        assert 0 <= first < last < n
        step[first + 1:last + 1] = 0
    return np.cumsum(step)


def quantised(n, C, q, rng):
    """(preds, targets) [n, C]: scores (k + 0.5) / q, k uniform in 0 .. q - 1 (exact in float32 for q <= 2^20), targets that
    lean to the high scores"""
    k = rng.randint(0, q, size=(n, C))
    preds = ((k + 0.5) / q).astype(np.float32)
    targets = (rng.rand(n, C) < 0.15 + 0.6 * preds).astype(np.float32)
    return np.ascontiguousarray(preds), np.ascontiguousarray(targets)


# ---- chunk edges ---------------------------------------------------------------------------------------------------------
EDGE_N = [1, 2, 63, 64, 65, 4095, 4096, 4097, 8209]
EDGE_C = [1, 3]
EDGE_LEVELS = [1, 3, 16, 1 << 20]


@functools.lru_cache(maxsize=None)
def edge_case(n, C, q):
    return quantised(n, C, q, np.random.RandomState(7 * n + 3 * C + q % 1000))


# ---- runs against chunk boundaries ---------------------------------------------------------------------------------------
RUNS_N = 3 * CHUNK
RUNS = {"ends_4095": (4088, 4095), "ends_4096": (4088, 4096), "spans_4090_4100": (4090, 4100),
        "covers_middle_chunk": (3800, 8799)}   # 5000 equal scores: chunk 1 holds no run end


@functools.lru_cache(maxsize=None)
def runs_case():
    """(preds, targets, names) [3 * 4096, 4]: one label per entry of RUNS, distinct scores but for the stated run"""
    rng = np.random.RandomState(40950)
    n = RUNS_N
    cols = [label(levels_with_runs(n, [run]), rng.rand(n) < 0.3, rng) for run in RUNS.values()]
    return mc._stack(cols) + (list(RUNS),)


# ---- the corner rule across chunks ---------------------------------------------------------------------------------------
CORNER_N = 3 * CHUNK
CORNER_AT = [4095, 4096, 4097]
COLLINEAR = (4000, 8300)       # all negatives: the kept neighbours are positions 3999 and 8300, two chunks apart
TIE_M = CORNER_N // 8          # the tie label: n = 8 m


def tie_label_sorted(m):
    """(level, target) of 8 m elements by sorted position: 2 m positives, m negatives, then ONE run of m positives and m
    negatives, m positives, 2 m negatives; distinct scores outside the run.  P = N = 4 m.  The point before the run is
    (fpr, tpr) = (1/4, 1/2), the run's point (1/2, 3/4): |tpr - (1 - fpr)| is 1/4 at both, bit for bit, and larger at
    every other point -- the cutoff is the earlier one's threshold."""
    t = np.concatenate([np.ones(2 * m), np.zeros(m), np.tile([1.0, 0.0], m), np.ones(m), np.zeros(2 * m)])
    return levels_with_runs(8 * m, [(3 * m, 5 * m - 1)]), t


@functools.lru_cache(maxsize=None)
def corner_case():
    """(preds, targets, names) [3 * 4096, 12], distinct scores unless stated (every element is a curve point):
      last_corner_x    negatives on [3000, x], a positive at x + 1: x is the stretch's last kept corner   (x = 4095, 4096, 4097)
      first_corner_x   negatives on [x + 1, 9000], a positive at x: x is the stretch's first kept corner
      collinear        negatives on COLLINEAR, positives at both sides
      two_points / three_points_collinear / three_points_bent   2 / 3 score levels: where the rule switches on
      tie              tie_label_sorted
      sawtooth         P N N N repeated over all three chunks"""
    rng = np.random.RandomState(81920)
    n = CORNER_N
    distinct = np.arange(n)
    cols, names = [], []

    def stretch(first, last):
        t = (rng.rand(n) < 0.5).astype(np.float32)
        t[first:last + 1] = 0.0
        t[first - 1] = 1.0
        t[last + 1] = 1.0
        return t
    for x in CORNER_AT:
        cols.append(label(distinct, stretch(3000, x), rng))
        names.append("last_corner_%d" % x)
    for x in CORNER_AT:
        cols.append(label(distinct, stretch(x + 1, 9000), rng))
        names.append("first_corner_%d" % x)
    cols.append(label(distinct, stretch(*COLLINEAR), rng))
    names.append("collinear")
    cols.append(label(np.repeat([0, 1], [5000, n - 5000]), rng.rand(n) < 0.4, rng))
    names.append("two_points")
    third = np.tile(np.repeat([1.0, 0.0], [1024, CHUNK - 1024]), 3)      # the same counts in each of three runs: collinear
    cols.append(label(np.repeat([0, 1, 2], CHUNK), third, rng))
    names.append("three_points_collinear")
    cols.append(label(np.repeat([0, 1, 2], [100, 5000, n - 5100]), rng.rand(n) < 0.4, rng))
    names.append("three_points_bent")
    cols.append(label(*tie_label_sorted(TIE_M), rng))
    names.append("tie")
    small = np.tile(np.repeat([1.0, 0.0], [1, 3]), n // 4)               # P N N N repeated: the middle negative of each group is dropped
    cols.append(label(distinct, small, rng))
    names.append("sawtooth")
    return mc._stack(cols) + (names,)


# ---- degenerate labels ---------------------------------------------------------------------------------------------------
DEGENERATE_N = 9000
SATURATED_RUN = CHUNK + 104


@functools.lru_cache(maxsize=None)
def degenerate_case():
    """(preds, targets, names) [9000, 6]: all positive, all negative, one positive, one negative (distinct scores), and two
    labels with runs of exactly 1.0f and exactly 0.0f longer than a chunk around ordinary values"""
    rng = np.random.RandomState(90001)
    n = DEGENERATE_N
    distinct = np.arange(n)
    one_p, one_n = np.zeros(n), np.ones(n)
    one_p[int(rng.randint(0, n))] = 1.0
    one_n[int(rng.randint(0, n))] = 0.0
    cols = [label(distinct, np.ones(n), rng), label(distinct, np.zeros(n), rng), label(distinct, one_p, rng),
            label(distinct, one_n, rng)]
    L = SATURATED_RUN
    for rate in (0.5, 0.05):
        s = np.concatenate([np.ones(L), rng.rand(n - 2 * L) * 0.98 + 0.01, np.zeros(L)]).astype(np.float32)
        perm = rng.permutation(n)
        cols.append((s[perm], (rng.rand(n) < rate * (0.5 + s)).astype(np.float32)[perm]))
    return mc._stack(cols) + (["all_positive", "all_negative", "one_positive", "one_negative", "saturated_half",
                               "saturated_rare"],)


# ---- widths and many chunks ----------------------------------------------------------------------------------------------
WIDTH_N = 5000
WIDTHS = [33, 103]             # rows per block of the flat pack: 128 and 64 (metrics_cases.pack_rows)


@functools.lru_cache(maxsize=None)
def width_case(C):
    return quantised(WIDTH_N, C, 1000, np.random.RandomState(5000 + C))


MANY_N = 64 * CHUNK + 5        # 65 chunks: the second step of the per-label prefix kernels


@functools.lru_cache(maxsize=None)
def many_chunk_case():
    """(preds, targets) [64 * 4096 + 5, 2]: distinct random scores, and scores quantised to 4096 levels"""
    rng = np.random.RandomState(262149)
    n = MANY_N
    s0 = ((rng.permutation(n) + 0.5) / n).astype(np.float32)
    assert np.unique(s0).size == n
    s1 = ((rng.randint(0, 4096, size=n) + 0.5) / 4096).astype(np.float32)
    t = np.stack([rng.rand(n) < 0.1 + 0.5 * s0, rng.rand(n) < 0.05 + 0.3 * s1], axis=1).astype(np.float32)
    return np.ascontiguousarray(np.stack([s0, s1], axis=1)), np.ascontiguousarray(t)


# ---- every case by name --------------------------------------------------------------------------------------------------
def small_cases():
    """{name: (preds, targets)} of every case but the chunk-edge grid and the many-chunk one"""
    out = {"runs": runs_case()[:2], "corner": corner_case()[:2], "degenerate": degenerate_case()[:2],
           "saturated": mc.saturated_case()}
    for C in WIDTHS:
        out["width_%d" % C] = width_case(C)
    return out


def all_cases():
    """{name: (preds, targets)}: every case of this module"""
    out = {"edge_n%d_C%d_q%d" % (n, C, q): edge_case(n, C, q) for n in EDGE_N for C in EDGE_C for q in EDGE_LEVELS}
    out.update(small_cases())
    out["many_chunks"] = many_chunk_case()
    return out
