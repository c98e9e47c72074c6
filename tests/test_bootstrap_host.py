"""The host side of chromegcn_amd/bootstrap.py (no GPU): the known answers of both rules, the properties of the weight
rule, the weighted restatement against resampled rows and against scikit-learn's sample_weight, and the statistics."""
import numpy as np
import pytest

import bootstrap_cases as K
from chromegcn_amd import bootstrap as B


# ---- known answers ----
def test_known_answers_of_the_weighted_metric_rule():
    for w, ints, s_ap, s_pr in K.KNOWN_SUMS:
        got = B.weighted_sums_host(K.KNOWN_SCORES, K.KNOWN_TARGETS, w, 0.5)
        assert tuple(int(got[k][0, 0]) for k in ("A", "P", "TOT", "F")) == ints, w
        np.testing.assert_allclose([got["S_ap"][0, 0], got["S_pr"][0, 0]], [s_ap, s_pr], rtol=4 * 2.0 ** -52, atol=0)
    both = B.weighted_sums_host(K.KNOWN_SCORES, K.KNOWN_TARGETS, [w for w, _, _, _ in K.KNOWN_SUMS])   # as one [R, n] call
    assert both["A"][:, 0].tolist() == [11, 14, 0, 0] and both["F"].dtype == np.int64 and both["S_pr"].dtype == np.float64


def test_known_answers_of_the_weight_rule():
    for (n, reps, seed, block, lengths), rows in K.KNOWN_WEIGHTS:
        got = B.bootstrap_weights_host(n, reps, seed=seed, block=block, lengths=lengths)
        assert got.dtype == np.int64 and got.tolist() == rows
    # both halves of the seed and of the replicate index matter
    n, reps, seed, block, _ = K.KNOWN_WEIGHTS[2][0]
    base = B.bootstrap_weights_host(n, [reps[1]], seed, block)
    assert not np.array_equal(base, B.bootstrap_weights_host(n, [reps[0]], seed, block))
    assert not np.array_equal(base, B.bootstrap_weights_host(n, [reps[1]], seed & 0xFFFFFFFF, block))


def test_metrics_from_sums_and_its_degenerate_labels():
    sums = B.weighted_sums_host(K.KNOWN_SCORES, K.KNOWN_TARGETS, [w for w, _, _, _ in K.KNOWN_SUMS])
    m = B.metrics_from_sums(sums)
    np.testing.assert_allclose(m["auroc"][:2, 0], [11 / 24, 14 / 24], rtol=1e-15)
    np.testing.assert_allclose(m["average_precision"][:2, 0], [(1 / 2 + 6 / 5 + 4 / 7) / 4, (4 / 3 + 3 / 7) / 3], rtol=1e-15)
    np.testing.assert_allclose(m["aupr"][:3, 0], [(3 / 2 + 11 / 5 + 15 / 14) / 8, (10 / 3 + 16 / 21) / 6, 1.0], rtol=1e-15)
    np.testing.assert_allclose(m["recall_at_fdr"][:3, 0], [1.0, 2 / 3, 1.0], rtol=1e-15)
    assert np.isnan(m["auroc"][2, 0])                       # only positives carry weight
    assert all(np.isnan(m[k][3, 0]) for k in B.METRICS)     # TOT = 0
    none = B.metrics_from_sums(B.weighted_sums_host([.3, .2, .1], [0, 0, 0], [1, 2, 1]))   # P = 0 < TOT
    assert np.isnan(none["auroc"][0, 0])
    assert (none["average_precision"][0, 0], none["aupr"][0, 0], none["recall_at_fdr"][0, 0]) == (0.0, 0.5, 0.0)


# ---- the weight rule ----
SETTINGS = [(200, 1, None), (200, 7, None), (300, 25, [100, 200]), (50, 80, [20, 0, 30]), (7, 3, [3, 4])]


@pytest.mark.parametrize("n,block,lengths", SETTINGS)
def test_stratum_totals_and_circular_runs(n, block, lengths):
    seed, R = (5 << 32) | 11, 6
    W = B.bootstrap_weights_host(n, R, seed, block, lengths)
    offsets = np.concatenate([[0], np.cumsum(lengths if lengths is not None else [n])])
    g0 = 0
    for off, end in zip(offsets[:-1], offsets[1:]):
        ns = int(end - off)
        if ns == 0:
            continue
        L = min(block, ns)
        k = -(-ns // L)
        assert (W[:, off:end].sum(1) == k * L).all()
        # every draw is a circular run of L rows inside its stratum: rebuilding the weights from the starts gives W
        for b in range(R):
            starts = B.draw(np.arange(g0, g0 + k), seed, b, B.STREAM_BOOTSTRAP, ns)
            assert ((0 <= starts) & (starts < ns)).all()
            w = np.zeros(ns, np.int64)
            for st in starts:
                for q in range(L):
                    w[(st + q) % ns] += 1
            np.testing.assert_array_equal(w, W[b, off:end])
        g0 += k


def test_a_replicate_is_the_same_alone_in_a_batch_and_by_index():
    n, seed, block, lengths = 120, 9, 7, [50, 70]
    batch = B.bootstrap_weights_host(n, 10, seed, block, lengths)
    for b in (0, 3, 9):
        np.testing.assert_array_equal(B.bootstrap_weights_host(n, [b], seed, block, lengths)[0], batch[b])
    np.testing.assert_array_equal(B.bootstrap_weights_host(n, np.array([9, 2, 2]), seed, block, lengths), batch[[9, 2, 2]])
    np.testing.assert_array_equal(B.bootstrap_weights_host(n, 4, seed, block, lengths), batch[:4])


@pytest.mark.parametrize("n,block,lengths", [(200, 1, None), (200, 7, None), (300, 25, [100, 200])])
def test_coverage_every_row_has_its_expected_weight(n, block, lengths):
    W = B.bootstrap_weights_host(n, 2000, (5 << 32) | 11, block, lengths)
    mean = W.mean(0)
    at = 0
    for ns in (lengths or [n]):
        L = min(block, ns)
        ratio = mean[at:at + ns] / (-(-ns // L) * L / ns)
        print("n=%d block=%d stratum of %d: mean weight / expected in [%.3f, %.3f]" % (n, block, ns, ratio.min(), ratio.max()))
        assert ratio.min() >= 0.85 and ratio.max() <= 1.15
        at += ns


def test_refusals_of_the_host_rules():
    with pytest.raises(ValueError, match="block"):
        B.bootstrap_weights_host(10, 2, block=0)
    with pytest.raises(ValueError, match="lengths"):
        B.bootstrap_weights_host(10, 2, lengths=[3, 4])
    with pytest.raises(ValueError, match="negative"):
        B.weighted_sums_host([.1, .2], [0, 1], [1, -1])
    with pytest.raises(ValueError, match="2\\^31"):
        B.weighted_sums_host([.1, .2], [0, 1], [2 ** 30, 2 ** 30])
    with pytest.raises(ValueError, match="NaN"):
        B.weighted_sums_host([.1, np.nan], [0, 1], [1, 1])
    for q in (0.0, 1.0, -0.1, float("nan")):
        with pytest.raises(ValueError, match="fdr_cutoff"):
            B.weighted_sums_host([.1, .2], [0, 1], [1, 1], q)
    with pytest.raises(ValueError):
        B.weighted_sums_host([.1, .2], [0, 1], [1, 1, 1])
    with pytest.raises(ValueError, match="integers"):
        B.weighted_sums_host([.1, .2], [0, 1], [1.0, 1.0])


# ---- the restatement ----
def _inputs(n, seed):
    rng = np.random.default_rng(seed)
    t = (rng.random(n) < 0.35).astype(np.float32)
    s = np.round(1.0 / (1.0 + np.exp(-(rng.normal(size=n) + 0.8 * t))), 2).astype(np.float32)   # two decimals: heavy ties
    return s, t


def _weight_sets(n):
    """20 replicates each: blocks 1, 7 and 25, and strata with an empty stratum"""
    sets = [B.bootstrap_weights_host(n, 20, 3, block) for block in (1, 7, 25)]
    a = n // 3
    sets.append(B.bootstrap_weights_host(n, 20, 4, 7, [a, 0, n - a]))
    return sets


SIZES = [1, 2, 65, 300, 1000, 4097]


@pytest.mark.parametrize("n", SIZES)
def test_weights_equal_resampled_rows(n):
    s, t = _inputs(n, n)
    for q in (0.5, 0.3):
        for W in _weight_sets(n):
            got = B.weighted_sums_host(s, t, W, q)
            for r in range(0, W.shape[0], 5):
                rows = np.repeat(np.arange(n), W[r])
                want = B.weighted_sums_host(s[rows], t[rows], np.ones(rows.size, np.int64), q)
                for k in ("A", "P", "TOT", "F"):
                    assert got[k][r, 0] == want[k][0, 0], (k, r)
                for k in ("S_ap", "S_pr"):
                    np.testing.assert_allclose(got[k][r, 0], want[k][0, 0], rtol=K.sum_rtol(rows.size), atol=0)


@pytest.mark.parametrize("n", SIZES)
def test_restatement_against_scikit_learn_sample_weight(n):
    import sklearn.metrics as skm
    s, t = _inputs(n, 100 + n)
    worst = 0.0
    for W in _weight_sets(n):
        m = B.metrics_from_sums(B.weighted_sums_host(s, t, W))
        for r in range(W.shape[0]):
            ss, tt, ww = s.astype(np.float64), t, W[r].astype(np.float64)
            if tt[ww > 0].min() == tt[ww > 0].max():   # one class carries all the weight
                assert np.isnan(m["auroc"][r, 0])
                continue
            want = {"auroc": skm.roc_auc_score(tt, ss, sample_weight=ww),
                    "average_precision": skm.average_precision_score(tt, ss, sample_weight=ww),
                    "aupr": skm.auc(*skm.precision_recall_curve(tt, ss, sample_weight=ww)[1::-1])}
            for k, v in want.items():
                worst = max(worst, abs(m[k][r, 0] - v))
                assert abs(m[k][r, 0] - v) <= 1e-12, (k, r, m[k][r, 0], v)
    print("n=%d: worst |restatement - scikit-learn| = %.3g" % (n, worst))


# ---- the statistics ----
def test_summary_against_hand_computed_quantiles():
    rep = np.array([[1.0, 10.0], [2.0, np.nan], [3.0, 30.0], [4.0, np.nan], [5.0, 20.0]])
    out = B.bootstrap_summary([3.0, 20.0], rep, level=0.5)
    # column 0: quantiles 0.25 / 0.75 of 1..5 (linear: position q (n - 1)) are 2 and 4; column 1 keeps 10, 30, 20 -> 15 and 25
    assert out["ci_low"].tolist() == [2.0, 15.0] and out["ci_high"].tolist() == [4.0, 25.0]
    assert out["n_valid"].tolist() == [5, 3] and out["point"].tolist() == [3.0, 20.0]
    np.testing.assert_allclose(out["se"], [np.sqrt(2.5), 10.0], rtol=1e-15)
    out = B.bootstrap_summary(0.5, np.array([0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 1.0, 1.1]), level=0.8)
    np.testing.assert_allclose([out["ci_low"], out["ci_high"]], [0.2, 1.0], rtol=1e-15)
    none = B.bootstrap_summary([np.nan], np.full((4, 1), np.nan))
    assert none["n_valid"].tolist() == [0] and np.isnan(none["ci_low"][0]) and np.isnan(none["se"][0])
    one = B.bootstrap_summary([1.0], np.array([[np.nan], [2.0]]))
    assert one["n_valid"].tolist() == [1] and one["ci_low"][0] == one["ci_high"][0] == 2.0 and np.isnan(one["se"][0])
    with pytest.raises(ValueError):
        B.bootstrap_summary([1.0], np.zeros((3, 2)))
    with pytest.raises(ValueError):
        B.bootstrap_summary([1.0], np.zeros((3, 1)), level=1.0)


def test_the_p_value_formula_on_a_literal():
    d = np.array([[0.2, 0.0, -1.0, np.nan], [0.1, 0.0, -2.0, np.nan], [-0.3, 0.0, -3.0, np.nan], [0.4, 0.0, np.nan, np.nan]])
    # column 0: B = 4, one <= 0, three >= 0 -> 2 * min(2 / 5, 4 / 5); column 1: all zero -> 1; column 2: B = 3, none >= 0
    # -> 2 * min(4 / 4, 1 / 4); column 3: no defined difference -> 1
    np.testing.assert_allclose(B.paired_p(d), [0.8, 1.0, 0.5, 1.0], rtol=1e-15)


def test_scalars_follow_compute_metrics_rule():
    m = {"auroc": np.array([[0.5, np.nan, 0.7], [np.nan, np.nan, np.nan]]), "aupr": np.array([[0.1, 0.2, 0.3], [0.3, 0.5, 0.4]]),
         "recall_at_fdr": np.array([[0.0, 1.0, np.nan], [0.5, 0.5, 0.5]]),
         "average_precision": np.array([[0.2, 0.4, 0.6], [0.1, np.nan, 0.3]])}
    s = B.scalar_metrics(m, {"tf": [0, 1], "hm": [2]})
    np.testing.assert_allclose(s["meanAUC"], [0.6, np.nan], rtol=1e-15)
    np.testing.assert_allclose(s["meanAUPR"], [0.2, 0.4], rtol=1e-15)
    np.testing.assert_allclose(s["meanFDR"], [0.5, 0.5], rtol=1e-15)
    np.testing.assert_allclose(s["mAP"], [0.4, np.nan], rtol=1e-15)   # the plain mean: a NaN label makes it NaN
    np.testing.assert_allclose(s["tf_meanAUC"], [0.5, np.nan], rtol=1e-15)
    np.testing.assert_allclose(s["hm_meanFDR"], [np.nan, 0.5], rtol=1e-15)
    assert set(s) == {"meanAUC", "meanAUPR", "meanFDR", "mAP"} | {"%s_%s" % (g, k) for g in ("tf", "hm")
                                                                   for k in ("meanAUC", "meanAUPR", "meanFDR")}


def test_names_are_exported():
    import chromegcn_amd as C
    for name in ("bootstrap_weights_host", "bootstrap_weights", "weighted_sums_host", "weighted_sums", "metrics_from_sums",
                 "weighted_metrics", "bootstrap_metrics", "bootstrap_compare", "bootstrap_summary", "BootstrapResult",
                 "BootstrapComparison"):
        assert hasattr(C, name) and name in C.__all__, name
