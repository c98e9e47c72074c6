"""csrc/cgcn_bootstrap.hip against the host restatement of chromegcn_amd/bootstrap.py: the weights of the rule bit for
bit, A / P / TOT / F equal, S_ap / S_pr within (n + 4) 2^-52 and bit-equal from run to run, on every case of
tests/bootstrap_cases.py; then the layers above: the point estimate against multilabel_metrics, bootstrap_metrics and
bootstrap_compare end to end, the refusals, and compute_metrics' unchanged default."""
import numpy as np
import pytest
import torch

import bootstrap_cases as K
from chromegcn_amd import bootstrap as B
from chromegcn_amd import metrics as M

pytestmark = pytest.mark.gpu
DEV = "cuda"
INTS, FLOATS = ("A", "P", "TOT", "F"), ("S_ap", "S_pr")


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.array(a)).to(DEV).to(dtype)


def check_sums(got, want, n):
    for k in INTS:
        assert got[k].dtype == np.int64
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    for k in FLOATS:
        assert got[k].dtype == np.float64
        with np.errstate(divide="ignore", invalid="ignore"):
            rel = np.nanmax(np.abs(got[k] - want[k]) / np.abs(want[k]), initial=0.0)
        print("%s: worst relative difference %.3g (allowed %.3g)" % (k, rel, K.sum_rtol(n)))
        np.testing.assert_allclose(got[k], want[k], rtol=K.sum_rtol(n), atol=0, err_msg=k)


# ---- equality with the restatement ----
@pytest.mark.parametrize("name", K.NAMES)
def test_sums_equal_the_restatement(name):
    n, C, R, _, _ = K.CASES[name]
    s, t = K.scores_targets(name)
    W = K.weights(name)
    got = B.weighted_sums(dev(s), dev(t), dev(W, torch.int32))
    assert all(got[k].shape == (R, C) for k in B.SUMS)
    check_sums(got, K.host_sums(name), n)
    again = B.weighted_sums(dev(s), dev(t), np.asarray(W))      # a host array of weights; a second device run
    for k in B.SUMS:
        assert got[k].tobytes() == again[k].tobytes(), k        # bit-equal between two device runs


@pytest.mark.parametrize("name", [k for k in K.NAMES if K.rule_args(k) is not None])
def test_weights_of_the_rule_are_bit_equal(name):
    n = K.CASES[name][0]
    reps, seed, block, lengths = K.rule_args(name)
    got = B.bootstrap_weights(n, reps, seed, block, lengths, device=DEV)
    assert got.dtype == torch.uint8 and got.is_cuda
    np.testing.assert_array_equal(got.cpu().numpy().astype(np.int64), K.weights(name))


def test_known_answers_on_the_device():
    s, t = dev(np.array(K.KNOWN_SCORES)[:, None]), dev(np.array(K.KNOWN_TARGETS)[:, None])
    got = B.weighted_sums(s, t, np.array([w for w, _, _, _ in K.KNOWN_SUMS]))
    for r, (_, ints, s_ap, s_pr) in enumerate(K.KNOWN_SUMS):
        assert tuple(int(got[k][r, 0]) for k in INTS) == ints
        np.testing.assert_allclose([got["S_ap"][r, 0], got["S_pr"][r, 0]], [s_ap, s_pr], rtol=K.sum_rtol(7), atol=0)
    for (n, reps, seed, block, lengths), rows in K.KNOWN_WEIGHTS:
        assert B.bootstrap_weights(n, reps, seed, block, lengths, device=DEV).tolist() == rows


def test_a_device_replicate_is_the_same_alone_in_a_batch_and_by_index():
    n, seed, block, lengths = 333, K.HIGH_SEED, 7, [100, 0, 233]
    want = B.bootstrap_weights_host(n, 70, seed, block, lengths)
    batch = B.bootstrap_weights(n, 70, seed, block, lengths, device=DEV).cpu().numpy()
    np.testing.assert_array_equal(batch, want)
    np.testing.assert_array_equal(B.bootstrap_weights(n, [69], seed, block, lengths, device=DEV).cpu().numpy(), want[69:])
    np.testing.assert_array_equal(B.bootstrap_weights(n, [5, 6, 7, 64, 2], seed, block, lengths, device=DEV).cpu().numpy(),
                                  want[[5, 6, 7, 64, 2]])


def test_device_weights_of_every_integer_dtype():
    """what bootstrap_weights returns (uint8) goes straight back in; so do bool, int8, int16 and int64 tensors"""
    name = "n300"
    n = K.CASES[name][0]
    s, t = K.scores_targets(name)
    reps, seed, block, lengths = K.rule_args(name)
    w8 = B.bootstrap_weights(n, reps, seed, block, lengths, device=DEV)
    assert w8.dtype == torch.uint8
    check_sums(B.weighted_sums(dev(s), dev(t), w8), K.host_sums(name), n)
    m = B.weighted_metrics(dev(s), dev(t), w8)
    want = B.metrics_from_sums(K.host_sums(name))
    for k in B.METRICS:
        np.testing.assert_allclose(m[k], want[k], rtol=K.sum_rtol(n), atol=0, equal_nan=True, err_msg=k)
    W = np.minimum(np.asarray(K.weights(name)), 1)[:5]          # 0 / 1 rows: every dtype holds them
    ref = B.weighted_sums_host(s, t, W)
    for dtype in (torch.bool, torch.int8, torch.uint8, torch.int16, torch.int64):
        check_sums(B.weighted_sums(dev(s), dev(t), dev(W, dtype)), ref, n)
    with pytest.raises(ValueError, match="negative"):
        B.weighted_sums(dev(s), dev(t), dev(W, torch.int8) - 1)
    with pytest.raises(ValueError, match="above 255"):
        B.weighted_sums(dev(s), dev(t), dev(W, torch.int16) * 300)


@pytest.mark.parametrize("q", [0.1, 0.3, 0.75])
def test_other_cutoffs(q):
    name = "n300_explicit"
    s, t = K.scores_targets(name)
    got = B.weighted_sums(dev(s), dev(t), np.asarray(K.weights(name)), q)
    check_sums(got, K.host_sums(name, q), K.CASES[name][0])


# ---- the point estimate ----
@pytest.mark.parametrize("name", ["n2", "n65_explicit", "n300", "n4097", "n5000"])
def test_unit_weights_equal_multilabel_metrics(name):
    n, C = K.CASES[name][:2]
    s, t = K.scores_targets(name)
    got = B.weighted_metrics(dev(s), dev(t), np.ones((1, n), np.int64))
    want = M.multilabel_metrics(dev(s), dev(t))
    for k in B.METRICS:
        w = want[k].cpu().numpy().astype(np.float64)
        assert got[k].shape == (1, C) and got[k].dtype == np.float64
        np.testing.assert_array_equal(np.isnan(got[k][0]), np.isnan(w), err_msg=k)
        np.testing.assert_allclose(got[k][0], w, rtol=3e-6, atol=3e-7, equal_nan=True, err_msg=k)
    if C >= 3:   # no positive | only positives | a single positive
        assert np.isnan(got["auroc"][0, :2]).all() and not np.isnan(got["auroc"][0, 2])
        assert (got["average_precision"][0, 0], got["aupr"][0, 0], got["recall_at_fdr"][0, 0]) == (0.0, 0.5, 0.0)
        assert (got["average_precision"][0, 1], got["aupr"][0, 1], got["recall_at_fdr"][0, 1]) == (1.0, 1.0, 1.0)


def test_zero_one_rows_leave_a_chromosome_out():
    name = "n300"
    s, t = K.scores_targets(name)
    W = np.ones((2, 300), np.int64)
    W[0, :100] = 0
    W[1, 100:] = 0
    got = B.weighted_metrics(dev(s), dev(t), W)
    for r, rows in enumerate((slice(100, 300), slice(0, 100))):
        want = B.metrics_from_sums(B.weighted_sums_host(s[rows], t[rows], np.ones(s[rows].shape[0], np.int64)))
        for k in B.METRICS:
            np.testing.assert_allclose(got[k][r], want[k][0], rtol=K.sum_rtol(300), atol=0, equal_nan=True, err_msg=k)


# ---- end to end ----
def _model(seed, n=700, C=6):
    rng = np.random.default_rng(seed)
    t = (rng.random((n, C)) < 0.25).astype(np.float32)
    t[:, 0] = 0   # a label without positives: NaN AUROC in every replicate
    a = (1.0 / (1.0 + np.exp(-(rng.normal(size=(n, C)) + 1.2 * t)))).astype(np.float32)
    b = (1.0 / (1.0 + np.exp(-(rng.normal(size=(n, C)) + 0.9 * t)))).astype(np.float32)
    return a, b, t


E2E = dict(n_boot=150, seed=(3 << 32) | 5, block=20, lengths=[300, 400], level=0.9, label_groups={"g": [1, 2], "h": [0, 5]})


def test_bootstrap_metrics_equals_the_summary_of_the_restatements_replicates():
    a, _, t = _model(1)
    res = B.bootstrap_metrics(dev(a), dev(t), keep_replicates=True, batch=64, **E2E)
    one = B.bootstrap_metrics(dev(a), dev(t), keep_replicates=True, batch=150, **E2E)   # batches of 64 against one batch
    W = B.bootstrap_weights_host(700, 150, E2E["seed"], 20, [300, 400])
    want = B.metrics_from_sums(B.weighted_sums_host(a, t, W))
    point = B.metrics_from_sums(B.weighted_sums_host(a, t, np.ones((1, 700), np.int64)))
    tol = dict(rtol=K.sum_rtol(700), atol=0, equal_nan=True)
    atol = dict(rtol=0, atol=2 * K.sum_rtol(700), equal_nan=True)
    for k in B.METRICS:
        assert res.replicates[k].tobytes() == one.replicates[k].tobytes()
        np.testing.assert_allclose(res.replicates[k], want[k], err_msg=k, **tol)
        np.testing.assert_allclose(res.point[k], point[k][0], err_msg=k, **tol)
        s = B.bootstrap_summary(res.point[k], res.replicates[k], 0.9)
        for f in ("ci_low", "ci_high", "se", "n_valid"):
            np.testing.assert_array_equal(getattr(res, f)[k], s[f], err_msg=k + " " + f)
            np.testing.assert_array_equal(getattr(one, f)[k], s[f], err_msg=k + " " + f)
        # against the restatement's own summary: a quantile interpolates two replicates and every metric is at most 1, so
        # the replicates' tolerance holds as an absolute one (twice, for the interpolation's own rounding)
        sw = B.bootstrap_summary(point[k][0], want[k], 0.9)
        np.testing.assert_allclose(res.ci_low[k], sw["ci_low"], err_msg=k, **atol)
        np.testing.assert_allclose(res.ci_high[k], sw["ci_high"], err_msg=k, **atol)
        np.testing.assert_array_equal(res.n_valid[k], sw["n_valid"])
    assert res.n_valid["auroc"][0] == 0 and np.isnan(res.ci_low["auroc"][0]) and res.n_valid["aupr"][0] == 150
    sc = B.scalar_metrics(want, E2E["label_groups"])
    assert set(res.scalars) == set(sc) == {"meanAUC", "meanAUPR", "meanFDR", "mAP", "g_meanAUC", "g_meanAUPR", "g_meanFDR",
                                           "h_meanAUC", "h_meanAUPR", "h_meanFDR"}
    for name, v in sc.items():
        sw = B.bootstrap_summary(B.scalar_metrics(point, E2E["label_groups"])[name][0], v, 0.9)
        for f in ("point", "ci_low", "ci_high", "se"):
            np.testing.assert_allclose(res.scalars[name][f], sw[f], err_msg=name + " " + f, **atol)   # means of values <= 1
    assert B.bootstrap_metrics(dev(a), dev(t), **E2E).replicates is None


def test_bootstrap_compare():
    a, b, t = _model(2)
    same = B.bootstrap_compare(dev(a), dev(a), dev(t), **E2E)
    for k in B.METRICS:
        assert not np.nan_to_num(same.diff[k]).any() and not np.nan_to_num(same.ci_low[k]).any()
        assert (same.p[k] == 1.0).all()
    assert all(v["p"] == 1.0 and (v["diff"] == 0.0 or np.isnan(v["diff"])) for v in same.scalars.values())
    cmp_ = B.bootstrap_compare(dev(a), dev(b), dev(t), keep_replicates=True, batch=64, **E2E)
    ra = B.bootstrap_metrics(dev(a), dev(t), keep_replicates=True, **E2E)
    rb = B.bootstrap_metrics(dev(b), dev(t), keep_replicates=True, **E2E)
    for k in B.METRICS:
        d = ra.replicates[k] - rb.replicates[k]
        np.testing.assert_array_equal(cmp_.replicates[k], d, err_msg=k)
        np.testing.assert_array_equal(cmp_.diff[k], ra.point[k] - rb.point[k], err_msg=k)
        s = B.bootstrap_summary(cmp_.diff[k], d, 0.9)
        np.testing.assert_array_equal(cmp_.ci_low[k], s["ci_low"])
        np.testing.assert_array_equal(cmp_.ci_high[k], s["ci_high"])
        np.testing.assert_array_equal(cmp_.p[k], B.paired_p(d))
    for name, v in cmp_.scalars.items():
        d = ra.scalar_replicates[name] - rb.scalar_replicates[name]
        np.testing.assert_array_equal(cmp_.scalar_replicates[name], d)
        assert v["p"] == float(B.paired_p(d)) and v["diff"] == v["a"] - v["b"]
    assert cmp_.scalars["meanAUC"]["diff"] > 0 and cmp_.scalars["meanAUC"]["p"] < 0.05   # a is the better model by construction


# ---- refusals ----
def test_refusals_before_any_launch():
    s, t = torch.rand(50, 3), (torch.rand(50, 3) < 0.3).float()
    w = np.ones((2, 50), np.int64)
    with pytest.raises(RuntimeError, match="GPU"):
        B.weighted_sums(s, t, w)
    with pytest.raises(RuntimeError, match="GPU"):
        B.bootstrap_metrics(s, t, n_boot=4)
    with pytest.raises(RuntimeError, match="GPU"):
        B.bootstrap_compare(s.to(DEV), s, t.to(DEV), n_boot=4)
    with pytest.raises(RuntimeError, match="GPU"):
        B.bootstrap_weights(10, 2, device="cpu")
    s, t = s.to(DEV), t.to(DEV)
    with pytest.raises(ValueError, match=r"\[n, C\]"):
        B.weighted_sums(s, t[:, :2], w)
    with pytest.raises(ValueError, match=r"\[n, C\]"):
        B.bootstrap_compare(s, s[:, :2], t, n_boot=4)
    with pytest.raises(ValueError, match=r"\[R, n\]"):
        B.weighted_sums(s, t, w[:, :49])
    with pytest.raises(ValueError, match="block"):
        B.bootstrap_metrics(s, t, n_boot=4, block=0)
    with pytest.raises(ValueError, match="lengths"):
        B.bootstrap_metrics(s, t, n_boot=4, lengths=[20, 20])
    for q in (0.0, 1.0, 1.5):
        with pytest.raises(ValueError, match="fdr_cutoff"):
            B.weighted_sums(s, t, w, q)
        with pytest.raises(ValueError, match="fdr_cutoff"):
            B.bootstrap_metrics(s, t, n_boot=4, fdr_cutoff=q)
    for bad, what in ((256, "above 255"), (-1, "negative"), (2 ** 30, "2\\^31|above 255")):
        w2 = w.copy()
        w2[1, 7] = w2[1, 8] = bad
        with pytest.raises(ValueError, match=what):
            B.weighted_sums(s, t, w2)                                    # a host array: refused on the host
        with pytest.raises(ValueError, match=what):
            B.weighted_sums(s, t, torch.from_numpy(w2).to(DEV))          # a device tensor: the kernel's flag word
    with pytest.raises(ValueError, match="integers"):
        B.weighted_sums(s, t, torch.ones(2, 50, device=DEV))


def test_a_nan_score_is_a_value_error_through_the_bad_word():
    s, t = torch.rand(300, 4, device=DEV), (torch.rand(300, 4, device=DEV) < 0.3).float()
    s[177, 2] = float("nan")
    with pytest.raises(ValueError, match="NaN"):
        B.weighted_sums(s, t, np.ones((3, 300), np.int64))
    with pytest.raises(ValueError, match="NaN"):
        B.bootstrap_metrics(s, t, n_boot=8)


def test_blocks_as_long_as_the_stratum_and_half_of_it():
    got = B.bootstrap_weights(300, 64, 1, 300, device=DEV)   # one draw covers the whole stratum
    assert (got == 1).all()
    got = B.bootstrap_weights(300, 64, 1, 150, device=DEV)   # two draws of half of it
    assert int(got.max()) <= 2 and (got.sum(1) == 300).all()
    np.testing.assert_array_equal(got.cpu().numpy(), B.bootstrap_weights_host(300, 64, 1, 150))


# ---- defaults ----
def test_compute_metrics_without_bootstrap_is_unchanged_and_with_it_gains_intervals():
    a, _, t = _model(3)
    base = M.compute_metrics(a, t, 0.25, device=DEV)
    assert sorted(base) == sorted(["mAP", "meanAUC", "medianAUC", "allAUC", "allFDR", "meanAUPR", "medianAUPR", "allAUPR",
                                   "meanFDR", "medianFDR", "loss", "time"])
    again = M.compute_metrics(a, t, 0.25, device=DEV, bootstrap=None)
    for k, v in base.items():
        np.testing.assert_array_equal(again[k], v, err_msg=k)
    boot = M.compute_metrics(a, t, 0.25, device=DEV, bootstrap=dict(n_boot=100, block=10, seed=4))
    assert sorted(set(boot) - set(base)) == ["mAP_ci", "meanAUC_ci", "meanAUPR_ci", "meanFDR_ci"]
    for k, v in base.items():
        np.testing.assert_array_equal(boot[k], v, err_msg=k)
    res = B.bootstrap_metrics(dev(a), dev(t), n_boot=100, block=10, seed=4)
    for k in ("meanAUC", "meanAUPR", "meanFDR", "mAP"):
        lo, hi = boot[k + "_ci"]
        assert (lo, hi) == (res.scalars[k]["ci_low"], res.scalars[k]["ci_high"])
        assert lo <= hi
    per = M.per_chromosome_metrics(a, t, [300, 400], names=["chrA", "chrB"], device=DEV, bootstrap=dict(n_boot=64, block=10))
    assert all("meanAUC_ci" in per[c] for c in ("chrA", "chrB"))
    assert "meanAUC_ci" not in M.per_chromosome_metrics(a, t, [300, 400], device=DEV)["0"]


# ---- the command lines ----
def _tool(name):
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", name + ".py")
    spec = importlib.util.spec_from_file_location(name + "_tool", path)
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def _saved(tmp_path):
    import json
    a, b, t = _model(4)
    np.save(tmp_path / "a.npy", a)
    np.save(tmp_path / "b.npy", b)
    np.save(tmp_path / "t.npy", t)
    (tmp_path / "lengths.json").write_text(json.dumps([["chr8", 300], ["chr21", 400]]))
    (tmp_path / "groups.json").write_text(json.dumps(E2E["label_groups"]))
    common = ["--targets", str(tmp_path / "t.npy"), "--lengths", str(tmp_path / "lengths.json"), "--groups", str(tmp_path / "groups.json")]
    return a, b, t, common


def test_bootstrap_tool_writes_what_the_library_returns(tmp_path):
    a, b, t, common = _saved(tmp_path)
    tool = _tool("bootstrap")
    kw = dict(n_boot=100, seed=3, block=20, lengths=[300, 400], label_groups=E2E["label_groups"])
    args = common + ["--n-boot", "100", "--seed", "3", "--block", "20"]
    tool.main(["--preds", str(tmp_path / "a.npy"), "--out", str(tmp_path / "o" / "one.npz"), "--keep-replicates"] + args)
    z = np.load(tmp_path / "o" / "one.npz")
    res = B.bootstrap_metrics(dev(a), dev(t), keep_replicates=True, **kw)
    names = list(res.scalars)
    assert z["scalar_names"].tolist() == names
    for m in B.METRICS:
        for key, want in ((m, res.point[m]), (m + "_ci_low", res.ci_low[m]), (m + "_ci_high", res.ci_high[m]), (m + "_se", res.se[m]),
                          (m + "_n_valid", res.n_valid[m]), (m + "_replicates", res.replicates[m])):
            np.testing.assert_array_equal(z[key], want, err_msg=key)
    for f in ("point", "ci_low", "ci_high", "se", "n_valid"):
        np.testing.assert_array_equal(z["scalar_" + f], np.array([res.scalars[k][f] for k in names]), err_msg=f)
    assert z["scalar_replicates"].shape == (100, len(names))
    tool.main(["--preds", str(tmp_path / "a.npy"), "--preds-b", str(tmp_path / "b.npy"), "--out", str(tmp_path / "o" / "cmp.npz")] + args)
    z = np.load(tmp_path / "o" / "cmp.npz")
    cmp_ = B.bootstrap_compare(dev(a), dev(b), dev(t), **kw)
    for m in B.METRICS:
        for key, want in ((m, cmp_.diff[m]), (m + "_a", cmp_.a[m]), (m + "_b", cmp_.b[m]), (m + "_ci_low", cmp_.ci_low[m]),
                          (m + "_ci_high", cmp_.ci_high[m]), (m + "_p", cmp_.p[m])):
            np.testing.assert_array_equal(z[key], want, err_msg=key)
    for f in ("diff", "a", "b", "ci_low", "ci_high", "p"):
        np.testing.assert_array_equal(z["scalar_" + f], np.array([cmp_.scalars[k][f] for k in names]), err_msg=f)
    assert "auroc_replicates" not in z.files


def test_analyze_results_bootstrap_columns(tmp_path):
    import csv
    import pickle
    import scipy.sparse as sp
    a, b, t, common = _saved(tmp_path)
    graphs = {}
    for c, k in (("chr8", 300), ("chr21", 400)):
        g = sp.random(k, k, density=0.02, random_state=k, format="csr")
        graphs[c] = ((g + g.T) > 0).astype(np.float64).tocsr()
    with open(tmp_path / "graphs.pkl", "wb") as f:
        pickle.dump(graphs, f)
    base = ["--preds-a", str(tmp_path / "a.npy"), "--preds-b", str(tmp_path / "b.npy"), "--graphs", str(tmp_path / "graphs.pkl")] + common
    tool = _tool("analyze_results")
    tool.main(base + ["--out", str(tmp_path / "plain.npz"), "--csv", str(tmp_path / "plain.csv")])
    tool.main(base + ["--bootstrap", "100", "--bootstrap-block", "20", "--out", str(tmp_path / "boot.npz"), "--csv", str(tmp_path / "boot.csv")])
    plain, boot = np.load(tmp_path / "plain.npz"), np.load(tmp_path / "boot.npz")
    metrics3 = ("auroc", "aupr", "recall_at_fdr")
    assert sorted(set(boot.files) - set(plain.files)) == sorted(m + s for m in metrics3 for s in ("_diff_ci_low", "_diff_ci_high", "_diff_p"))
    for k in plain.files:                                      # without the switch, and beside it, nothing changes
        np.testing.assert_array_equal(boot[k], plain[k], err_msg=k)
    cmp_ = B.bootstrap_compare(dev(b), dev(a), dev(t), n_boot=100, block=20, lengths=[300, 400], label_groups=E2E["label_groups"])
    for m in metrics3:                                         # the tool's difference is b - a
        np.testing.assert_array_equal(boot[m + "_diff_ci_low"], cmp_.ci_low[m])
        np.testing.assert_array_equal(boot[m + "_diff_ci_high"], cmp_.ci_high[m])
        np.testing.assert_array_equal(boot[m + "_diff_p"], cmp_.p[m])
    rows_p = list(csv.reader(open(tmp_path / "plain.csv")))
    rows_b = list(csv.reader(open(tmp_path / "boot.csv")))
    assert rows_p[0] == ["label", "windows", "average_degree"] + ["%s_%s" % (m, k) for m in metrics3 for k in ("a", "b", "diff")]
    assert rows_b[0] == ["label", "windows", "average_degree"] + ["%s_%s" % (m, k) for m in metrics3
                                                                  for k in ("a", "b", "diff", "diff_lo", "diff_hi", "p")]
    assert len(rows_b) == len(rows_p) == 1 + t.shape[1]
    at = rows_b[0].index("aupr_diff_lo")
    assert [float(r[at]) for r in rows_b[1:]] == cmp_.ci_low["aupr"].tolist()


def test_train_bootstrap_prints_the_test_intervals_with_the_chromosomes_as_strata(capsys):
    import types
    import chromegcn_amd as C
    from chromegcn_amd import runner, synth
    data = {"train": {}, "valid": {}, "test": {}}
    graphs = {"train": {}, "valid": {}, "test": {}}
    for i, (c, sp_) in enumerate([("chr2", "train"), ("chr3", "valid"), ("chr1", "test"), ("chr8", "test")]):
        n = 300 + 40 * i
        data[sp_][c] = synth.chrom_features(n, 128, 9, i, positive_rate=0.3)
        graphs[sp_][c] = synth.contact_graph(n, 6 * n, i)
    torch.manual_seed(0)
    model = C.ChromeGCN(128, 128, 9, 0.0, True, 2).to(DEV)
    optim = torch.optim.SGD(model.parameters(), lr=0.25, momentum=0.9, weight_decay=1e-6)
    opt = types.SimpleNamespace(epochs=2, adj_type="hic", model_name=None, lr_decay2=0, load_gcn=False, test_only=False,
                                bootstrap=100, bootstrap_block=25)
    hist = runner.run_model(None, model, data["train"], data["valid"], data["test"], None, optim, None, opt, None, graphs=graphs)
    assert not any(k.endswith("_ci") for k in hist[0]["test"])          # the last epoch only
    last = hist[-1]["test"]
    assert sorted(k for k in last if k.endswith("_ci")) == ["mAP_ci", "meanAUC_ci", "meanAUPR_ci", "meanFDR_ci"]
    # the same call by hand: the last epoch's test predictions, the two test chromosomes (380 and 420 rows) as strata
    stage = runner._stage_for(model, optim, opt, "test")
    p, tg, _ = stage.run_split("test", list(data["test"]), to_cpu=False)
    res = B.bootstrap_metrics(p.float(), tg.float(), n_boot=100, block=25, lengths=[380, 420])
    for k in ("mAP", "meanAUC", "meanAUPR", "meanFDR"):
        assert last[k + "_ci"] == (res.scalars[k]["ci_low"], res.scalars[k]["ci_high"]), k
    line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("test, 100 bootstrap replicates in blocks of 25")]
    assert len(line) == 1 and all(k in line[0] for k in ("mAP", "meanAUC", "meanAUPR", "meanFDR"))
    from chromegcn_amd import train
    o = train.parse(["-synthetic", "-bootstrap", "500", "-bootstrap_block", "40"])
    assert (o.bootstrap, o.bootstrap_block) == (500, 40) and train.parse(["-synthetic"]).bootstrap == 0
