"""Inputs for tests/test_metrics_cases_host.py and tests/test_gpu_metrics.py: rankings built so that a stated branch of
chromegcn_amd/csrc/cgcn_metrics.hip runs -- more than 64 chunks of 4096 elements per label (the second and third step of
k_metrics_prefix, the lane-strided loop of k_metrics_final, T >= 64 in k_rs_scan), runs of tied scores that end at stated sorted
positions, precision that equals a cutoff exactly, degenerate labels, saturated probabilities -- and the rows-per-block rule of
the flat pack as a function of C.  Builders only: nothing here touches the GPU.

A "sorted position" is an index into one label's list after a stable descending sort by score; a "run end" is the position
of the last element of a run of equal scores (one curve point of scikit-learn's distinct-threshold curves)."""
import functools

import numpy as np

CHUNK = 4096       # METRIC_CHUNK
GROUP = 64         # chunk records per step of k_metrics_prefix (one wave)


# ---- the flat pack's rows per block --------------------------------------------------------------------------------------
def pack_rows(C):
    """Rows per block R that cgcn_multilabel_metrics_nonneg picks for C labels: from R = 128, halved while R > 4 and
    C (R + 1) 4 bytes exceed 48 KB of LDS; 0 when even R = 4 does not fit (the 32 x 32 tile pack runs instead)."""
    R = 128
    while R > 4 and C * (R + 1) * 4 > 48 * 1024:
        R //= 2
    return R if C * (R + 1) * 4 <= 48 * 1024 else 0


# C -> the R it is meant to hit: both sides of every switch, and the product's C = 256
PACK_CASES = {95: 128, 96: 64, 189: 64, 190: 32, 256: 32, 372: 32, 373: 16, 722: 16, 723: 8, 1365: 8, 1366: 4, 2457: 4, 2458: 0}
PACK_N = 301                               # 301 = 2 * 128 + 45 = 75 * 4 + 1: the last block is partial for every R
PACK_TWO_TILES = [(4099, 256), (4099, 373)]   # two sort tiles
BAD_CASES = {256: 32, 2600: 0}             # `bad` word: R = 32 and the tile pack


def oracle_columns(C):
    """the columns the oracle is run on where C is wide"""
    return sorted({c for c in (0, 1, 2, C // 2, C - 2, C - 1) if 0 <= c < C})


# ---- single labels -------------------------------------------------------------------------------------------------------
def distinct_scores(n):
    """n distinct float32 scores in (0, 1), descending"""
    s = np.linspace(0.99, 0.01, n).astype(np.float32)
    assert (np.diff(s) < 0).all()
    return s


def levels(k):
    """k strictly descending float32 levels in (0, 1)"""
    return distinct_scores(k)


def _random_runs(total, rng, longest=7):
    """run lengths in 1 .. longest that add up to `total`"""
    out = []
    while total > 0:
        r = min(total, int(rng.randint(1, longest + 1)))
        out.append(r)
        total -= r
    return out


def runs_from_ends(ends):
    """run lengths of a list whose run ends are the sorted positions `ends` (the last one is n - 1)"""
    e = np.asarray(ends, dtype=np.int64)
    assert (np.diff(e) > 0).all() and e[0] >= 0
    return np.diff(np.concatenate([[-1], e])).tolist()


def staircase(run_lengths, rng, positive_rate=0.3):
    """(scores, targets, run_ends): level k (strictly descending float32) repeated run_lengths[k] times, random 0 / 1
    targets, rows shuffled; run_ends are the sorted positions of the run ends."""
    runs = np.asarray(run_lengths, dtype=np.int64)
    assert (runs > 0).all()
    scores = np.repeat(levels(runs.size), runs)
    targets = (rng.rand(scores.size) < positive_rate).astype(np.float32)
    perm = rng.permutation(scores.size)
    return scores[perm], targets[perm], np.cumsum(runs) - 1


def alternating(depth, n, negative_first=False):
    """(scores, targets) in rank order: P N P N ... for the first `depth` elements (depth even), then only negatives;
    distinct scores.  tp = fp at every even depth <= `depth`, the deepest of them holds every positive.
    As P N the point before it (odd depth, precision above 1/2) holds every positive too, so recall at FDR 1/2 is 1 whether
    or not the exact point qualifies; negative_first (N P N P ...) leaves the even depths as the ONLY points with
    precision >= 1/2, so the answer hangs on the comparison at equality."""
    assert depth % 2 == 0 and 0 < depth <= n
    t = np.zeros(n, dtype=np.float32)
    t[(1 if negative_first else 0):depth:2] = 1.0
    return distinct_scores(n), t


def three_to_one(depth, n, negative_first=False):
    """(scores, targets) in rank order: P P P N repeated for the first `depth` elements (depth a multiple of 4), then only
    negatives; distinct scores.  tp = 3 fp, precision exactly 3/4, at every depth 4 k <= `depth`.  negative_first (N P P P):
    the depths 4 k are the only points with precision >= 3/4 (see `alternating`)."""
    assert depth % 4 == 0 and 0 < depth <= n
    t = np.zeros(n, dtype=np.float32)
    t[:depth] = np.tile(np.array([0, 1, 1, 1] if negative_first else [1, 1, 1, 0], dtype=np.float32), depth // 4)
    return distinct_scores(n), t


def sorted_view(scores, targets):
    """(scores, targets) after a stable descending sort by score, -0 folded onto +0"""
    order = np.argsort(-(scores.astype(np.float64) + 0.0), kind="stable")
    return scores[order], targets[order]


def run_ends_of(sorted_scores):
    s = sorted_scores.astype(np.float64)
    return np.flatnonzero(np.concatenate([s[1:] != s[:-1], [True]]))


def _shuffled(rng, scores, targets):
    perm = rng.permutation(scores.size)
    return scores[perm], targets[perm]


def _stack(cols):
    preds = np.stack([c[0] for c in cols], axis=1).astype(np.float32)
    targets = np.stack([c[1] for c in cols], axis=1).astype(np.float32)
    return np.ascontiguousarray(preds), np.ascontiguousarray(targets)


# ---- whole inputs --------------------------------------------------------------------------------------------------------
MANY_N = 129 * CHUNK + 100                 # 130 chunks: three prefix groups, T = 130
MANY_LONG_RUN = (63 * CHUNK + 50, 128 * CHUNK + 50)   # [first, past-the-last) sorted position of column b's long run
MANY_C_ENDS = [63, 64, 65, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, GROUP * CHUNK - 1, GROUP * CHUNK, GROUP * CHUNK + 1,
               65 * CHUNK - 1, 66 * CHUNK - 1, MANY_N - 1]     # ... and a run that is exactly chunk 65
MANY_ALT_DEPTH = 2 * (GROUP * CHUNK + 10)  # the deepest tp = fp point: sorted position MANY_ALT_DEPTH - 1, in chunk 128
MANY_E_TOP, MANY_E_BOTTOM = 10, 1000       # column e: positives at the top / at the very bottom


@functools.lru_cache(maxsize=None)
def many_chunk_case():
    """dict(preds, targets [n, 6] float32, b_ends, c_ends): n = 129 * 4096 + 100.  Columns: a distinct random scores;
    b a staircase whose long run leaves chunks 64 .. 127 -- a whole prefix group -- without a run end; c run ends around
    lanes 63 / 64, wave-step groups, chunk and group boundaries; d alternating, deepest tp = fp point in chunk 128;
    e qualifying FDR points in chunk 0 only; f one run.  The arrays are shared: do not write to them."""
    rng = np.random.RandomState(1290100)
    n = MANY_N
    a_s = ((rng.permutation(n) + 0.5) / n).astype(np.float32)
    a = (a_s, (rng.rand(n) < 0.1 + 0.5 * a_s).astype(np.float32))
    lo, hi = MANY_LONG_RUN
    b = staircase(_random_runs(lo, rng) + [hi - lo] + _random_runs(n - hi, rng), rng)
    c = staircase(runs_from_ends(MANY_C_ENDS), rng, positive_rate=0.4)
    d = _shuffled(rng, *alternating(MANY_ALT_DEPTH, n))
    e_t = np.zeros(n, dtype=np.float32)
    e_t[:MANY_E_TOP] = 1.0
    e_t[n - MANY_E_BOTTOM:] = 1.0
    e = _shuffled(rng, distinct_scores(n), e_t)
    f = (np.full(n, 0.5, dtype=np.float32), (rng.rand(n) < 0.25).astype(np.float32))
    preds, targets = _stack([a, b, c, d, e, f])
    return {"preds": preds, "targets": targets, "b_ends": b[2], "c_ends": c[2]}


TWO_N = GROUP * CHUNK + 1                  # 65 chunks: the smallest n that enters the second prefix step
TWO_NEGATIVE_RANK = 5


@functools.lru_cache(maxsize=None)
def two_group_case():
    """dict(preds, targets [n, 6] float32, positive_rank): n = 64 * 4096 + 1.  Columns: all positive, all negative, one
    positive (at sorted position positive_rank), one negative (at sorted position 5), scores rounded to one decimal,
    distinct random scores.  The arrays are shared: do not write to them."""
    rng = np.random.RandomState(2620145)
    n = TWO_N
    rnd = lambda: ((rng.permutation(n) + 0.5) / n).astype(np.float32)   # noqa: E731
    positive_rank = int(rng.randint(0, n))
    one_p = np.zeros(n, dtype=np.float32)
    one_p[positive_rank] = 1.0
    one_n = np.ones(n, dtype=np.float32)
    one_n[TWO_NEGATIVE_RANK] = 0.0
    s4 = rnd()
    s5 = rnd()
    cols = [(rnd(), np.ones(n, dtype=np.float32)),
            (rnd(), np.zeros(n, dtype=np.float32)),
            _shuffled(rng, distinct_scores(n), one_p),
            _shuffled(rng, distinct_scores(n), one_n),
            (np.round(s4, 1), (rng.rand(n) < 0.05 + 0.4 * s4).astype(np.float32)),
            (s5, (rng.rand(n) < 0.02 + 0.3 * s5).astype(np.float32))]
    preds, targets = _stack(cols)
    return {"preds": preds, "targets": targets, "positive_rank": positive_rank}


SUBNORMAL = np.float32(1e-44)              # a subnormal float32 (7 * 2^-149)


def saturated_case(n=9000):
    """(preds, targets) [n, 5] float32: what a trained model's sigmoid emits.  Runs of exactly 1.0, of exactly 0.0 and of
    +0.0 / -0.0 mixed, each longer than one chunk; a band of subnormal probabilities (multiples of 1e-44, heavily tied);
    ordinary values between them; positive rates of about 0.5, 0.1, 0.3, 0.02 and 0.65.  Rows are shuffled."""
    assert n >= 9000
    rng = np.random.RandomState(9000 + n)
    L = CHUNK + 104                        # 4200: a run longer than one chunk
    ordinary = lambda k: (rng.rand(k) * 0.98 + 0.01).astype(np.float32)   # noqa: E731
    subnormal = lambda k, top: (SUBNORMAL * rng.randint(1, top + 1, size=k).astype(np.float32)).astype(np.float32)  # noqa: E731
    signed_zero = lambda k: np.where(rng.rand(k) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)   # noqa: E731
    one, zero = (lambda k: np.ones(k, dtype=np.float32)), (lambda k: np.zeros(k, dtype=np.float32))
    rest = n - 2 * L
    cols_s = [np.concatenate([one(L), ordinary(rest - 200), subnormal(200, 40), zero(L)]),
              np.concatenate([one(100), ordinary(n - L - 500), subnormal(400, 20), signed_zero(L)]),
              np.concatenate([one(n - L - 50), signed_zero(L + 50)]),
              np.concatenate([one(30), ordinary(n - 60), zero(30)]),
              np.concatenate([ordinary(n - L - 800), subnormal(L + 800, 50)])]
    cols = []
    for s, rate in zip(cols_s, (0.5, 0.1, 0.3, 0.02, 0.7)):
        assert s.size == n and s.dtype == np.float32
        # positives lean to the high scores, so that the curves are not flat
        t = (rng.rand(n) < np.clip(rate * (0.8 + 0.4 * s.astype(np.float64)), 0.0, 1.0)).astype(np.float32)
        cols.append(_shuffled(rng, s, t))
    return _stack(cols)


CUTOFFS = [0.0, 0.25, 0.5, 0.75, 1.0, 0.1, 0.05]
CUTOFF_N = 9000
# column -> (depth, negative_first); every depth lies past the first chunk
CUTOFF_ALT = {0: (5000, False), 2: (8190, True)}        # `alternating`
# `three_to_one`: depths d at which 3 d / 4 times the correctly rounded 1 / d is below 3/4 in float64 (the CPU tier checks it), so
# that a predicate taken from a product with the reciprocal instead of the quotient misses the deepest point -- which the
# negative_first label cannot make up for with the point before it
CUTOFF_3TO1 = {1: (5528, False), 3: (8180, True)}
CUTOFF_ALL_NEGATIVE = 4
CUTOFF_TOP_POSITIVES = (7, 7)              # (column, number of positives on top, the next element a negative)


@functools.lru_cache(maxsize=None)
def cutoff_case():
    """(preds, targets) [9000, 8] float32 for the fdr_cutoff sweep: two `alternating` and two `three_to_one` labels (one of each
    with the negative first) whose depths lie past the first chunk, an all-negative label, distinct random scores, scores rounded to two decimals,
    and a label with exactly 7 positives on top.  Rows are shuffled.  The arrays are shared: do not write to them."""
    rng = np.random.RandomState(90008)
    n = CUTOFF_N
    cols = [None] * 8
    for c, (depth, negative_first) in CUTOFF_ALT.items():
        cols[c] = _shuffled(rng, *alternating(depth, n, negative_first))
    for c, (depth, negative_first) in CUTOFF_3TO1.items():
        cols[c] = _shuffled(rng, *three_to_one(depth, n, negative_first))
    cols[CUTOFF_ALL_NEGATIVE] = ((rng.rand(n) * 0.9 + 0.05).astype(np.float32), np.zeros(n, dtype=np.float32))
    s5 = ((rng.permutation(n) + 0.5) / n).astype(np.float32)
    cols[5] = (s5, (rng.rand(n) < 0.05 + 0.8 * s5).astype(np.float32))
    s6 = ((rng.permutation(n) + 0.5) / n).astype(np.float32)
    cols[6] = (np.round(s6, 2), (rng.rand(n) < 0.1 + 0.6 * s6).astype(np.float32))
    col, top = CUTOFF_TOP_POSITIVES
    t7 = (rng.rand(n) < 0.3).astype(np.float32)
    t7[:top] = 1.0
    t7[top] = 0.0
    cols[col] = _shuffled(rng, distinct_scores(n), t7)
    return _stack(cols)
