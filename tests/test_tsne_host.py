"""The numpy restatements of chromegcn_amd.tsne against scikit-learn's own functions (sklearn/manifold/_t_sne.py), and the
single-label selection of chromegcn_amd.embed against the reference's loop.  No GPU needed: these pin what the GPU tests
(tests/test_gpu_tsne.py) compare the kernels with."""
import numpy as np
import pytest
import torch
from scipy.spatial.distance import squareform

from chromegcn_amd import embed, tsne


def _points(n, d=16, seed=0):
    return np.random.RandomState(seed).standard_normal((n, d)).astype(np.float32)


@pytest.fixture(scope="module")
def fixture(golden):
    return golden("g8_tsne.npz")


@pytest.fixture(scope="module")
def fixture_P(fixture):
    return tsne.joint_probabilities_host(tsne.sqdist_host(fixture["X"]).astype(np.float32), 30.0)


@pytest.mark.parametrize("n", [7, 65, 384])
@pytest.mark.parametrize("perplexity", [2, 5, 30])
def test_joint_probabilities_match_sklearn(n, perplexity):
    from sklearn.manifold import _t_sne
    if perplexity >= n:
        with pytest.raises(ValueError, match="less than n_samples"):
            tsne._check_perplexity(perplexity, n)
        return
    D = tsne.sqdist_host(_points(n, seed=n)).astype(np.float32)
    ref = squareform(_t_sne._joint_probabilities(D, perplexity, 0))
    P, info = tsne.joint_probabilities_host(D, perplexity, return_info=True)
    off = ~np.eye(n, dtype=bool)
    np.testing.assert_allclose(P[off], ref[off], rtol=1e-12, atol=0)
    assert np.all(np.diag(P) == 0) and np.array_equal(P, P.T)
    assert abs(P.sum() - 1.0) <= 1e-12 + n * n * tsne.EPS                  # the clamp at eps adds at most that
    assert info["beta"].shape == info["margin"].shape == (n,) and np.all(info["margin"] >= 0)


@pytest.mark.parametrize("exaggeration", [1.0, 12.0])
def test_kl_gradient_matches_sklearn(fixture, fixture_P, exaggeration):
    from sklearn.manifold import _t_sne
    n = len(fixture_P)
    for Y in (fixture["Y0"].astype(np.float64), np.random.RandomState(3).standard_normal((n, 2))):
        kl_ref, g_ref = _t_sne._kl_divergence(Y.ravel().copy(), squareform(fixture_P * exaggeration), 1, n, 2)
        kl, g, Z = tsne.kl_gradient_host(fixture_P, Y, exaggeration)
        np.testing.assert_allclose(kl, kl_ref, rtol=1e-12)
        # 1e-12 of the gradient's scale, max |g|, as the GPU tests state their bound: a component that cancels (one of the
        # 768 here is 3e-8 of the largest, a sum of terms 1e5 times its size) differs by 1e-11 of ITSELF between any two
        # float64 summation orders, scikit-learn's np.dot and a row sum among them
        assert np.abs(g - g_ref.reshape(n, 2)).max() <= 1e-12 * np.abs(g_ref).max()
        assert Z > 0
        # the row blocks of the restatement are an implementation detail
        kl_b, g_b, _ = tsne.kl_gradient_host(fixture_P, Y, exaggeration, block=100)
        np.testing.assert_allclose(kl_b, kl, rtol=1e-13)
        np.testing.assert_allclose(g_b, g, rtol=0, atol=1e-13 * np.abs(g).max())


def test_ten_iterations_match_sklearns_gradient_descent(fixture, fixture_P):
    from sklearn.manifold import _t_sne
    n = len(fixture_P)
    Y0 = fixture["Y0"].astype(np.float64)
    lr = max(n / 12.0 / 4.0, 50.0)
    p, err, it = _t_sne._gradient_descent(_t_sne._kl_divergence, Y0.ravel().copy(), it=0, max_iter=10, n_iter_check=50,
                                          momentum=0.5, learning_rate=lr, n_iter_without_progress=250,
                                          args=[squareform(fixture_P * 12.0), 1, n, 2])
    Y, info = tsne.tsne_embed_host(fixture_P, Y0, max_iter=10, dtype="float64")
    assert info["n_iter"] == it == 9 and info["learning_rate"] == lr
    assert np.abs(Y - p.reshape(n, 2)).max() <= 1e-12 * np.ptp(Y)
    np.testing.assert_allclose(info["kl_divergence"], err, rtol=1e-12)


def test_schedule_switches_stage_and_stops_like_sklearn(fixture_P):
    """the control flow alone, on a recorded sequence of errors: exploration to 250 with momentum 0.5 and exaggeration, then
    momentum 0.8; a check every 50 iterations; stop when no new best for more than the patience"""
    calls = []

    def stage(it, stop, momentum, patience, exaggeration):
        calls.append((it, stop, momentum, patience, exaggeration))
        seen = []
        errors = iter([5.0, 4.0, 3.0, 3.5, 3.6, 3.7, 3.8, 3.9, 4.0, 4.1, 4.2, 4.3, 4.4, 4.5, 4.6, 4.7])
        err, i = tsne._descent_loop(lambda want: (next(errors), 1.0) if want else None, it, stop, patience, 1e-7, seen)
        calls.append(seen)
        return err, i
    err, it = tsne._run_schedule(stage, 1000, 100, 12.0)
    assert calls[0] == (0, 250, 0.5, 250, 12.0) and [c[0] for c in calls[1]] == [50, 100, 150, 200, 250]
    assert calls[2] == (250, 1000, 0.8, 100, 1.0)
    # best at iteration index 399 (the third check of the stage); 549 - 399 = 150 > 100 stops at the check of 550
    assert [c[0] for c in calls[3]] == [300, 350, 400, 450, 500, 550] and it == 549 and err == 3.7


def test_fixture_records_what_the_generator_states(fixture):
    kls = [float(fixture[k]) for k in ("kl_sklearn", "kl_host_float32", "kl_host_float64", "kl_host_mixed")]
    assert float(fixture["kl_bound"]) == pytest.approx(kls[0] + 3.0 * (max(kls) - min(kls)), rel=1e-12)
    assert fixture["X"].shape == (384, 128) and fixture["X"].dtype == np.float32
    assert fixture["Y0"].shape == (384, 2) and fixture["Y0"].dtype == np.float32
    assert str(fixture["sklearn_version"]) and len(np.unique(fixture["labels"])) == 6


def test_three_dtype_forms_agree_over_ten_iterations(fixture, fixture_P):
    """ten iterations only (a long run belongs to the generator): the fp32 forms follow the float64 form while the
    trajectories are still comparable"""
    Y64, i64 = tsne.tsne_embed_host(fixture_P, fixture["Y0"], max_iter=10, dtype="float64")
    Y32, i32 = tsne.tsne_embed_host(fixture_P, fixture["Y0"], max_iter=10, dtype="float32")
    Ymx, imx = tsne.tsne_embed_host(fixture_P, fixture["Y0"], max_iter=10, dtype="mixed")
    assert Y32.dtype == Ymx.dtype == np.float32 and Y64.dtype == np.float64
    assert np.abs(Y32 - Y64).max() <= 1e-4 * np.ptp(Y64) and np.abs(Ymx - Y64).max() <= 1e-4 * np.ptp(Y64)
    np.testing.assert_allclose([i32["kl_divergence"], imx["kl_divergence"]], i64["kl_divergence"], rtol=1e-5)


def _targets(seed, n, C, counts):
    """[n, C] targets: counts[c] windows whose only label is c, the rest with no or two labels, shuffled"""
    rng = np.random.RandomState(seed)
    t = np.zeros((n, C), np.float32)
    rows = rng.permutation(n)
    k = 0
    for c, m in enumerate(counts):
        t[rows[k:k + m], c] = 1.0
        k += m
    rest = rows[k:]
    two = rest[::2]
    t[two, rng.randint(0, C, len(two))] = 1.0
    t[two, (np.argmax(t[two], 1) + 1 + rng.randint(0, C - 1, len(two))) % C] = 1.0
    return t


def test_single_label_selection_matches_the_reference_loop():
    C, min_count = 6, 20
    # two chromosomes; label 1 ends just below min_count over both, label 2 exactly at it, label 4 has none
    t1 = _targets(1, 150, C, [25, 9, 12, 30, 0, 3])
    t2 = _targets(2, 131, C, [11, 10, 8, 22, 0, 40])
    both = np.concatenate([t1, t2])
    per_row = (both != 0).sum(1)
    assert set(np.unique(per_row)) == {0, 1, 2}
    single_counts = [(both[per_row == 1].argmax(1) == c).sum() for c in range(C)]
    assert single_counts == [36, 19, 20, 52, 0, 43]
    for labels in (None, [5, 0, 2, 1], [4]):
        rows_ref, lab_ref = embed.select_single_label_host([t1, t2], labels, min_count)
        # the reference's loop, word for word (scripts/visualize.py:162-170)
        targs = np.where(per_row == 1, both.argmax(1), -1)
        want = []
        for i in (range(C) if labels is None else sorted(labels)):
            nz = np.flatnonzero(targs == i)
            if len(nz) > min_count - 1:
                want += list(nz)
        assert list(rows_ref) == want and list(lab_ref) == list(targs[want])
        pos = torch.from_numpy(both != 0)
        rows, lab = embed._selection(pos.to(torch.int32).argmax(1), pos.sum(1) == 1, C, labels, min_count)
        assert rows.dtype == lab.dtype == torch.int64
        assert rows.tolist() == list(rows_ref) and lab.tolist() == list(lab_ref)
    kept = embed.select_single_label_host([t1, t2], None, min_count)[1]
    assert sorted(set(kept.tolist())) == [0, 2, 3, 5]                       # 19 is out, 20 is in
    with pytest.raises(ValueError, match="outside"):
        embed._selection(pos.to(torch.int32).argmax(1), pos.sum(1) == 1, C, [6], min_count)


def test_cpu_tensors_and_bad_perplexity_raise():
    z = torch.zeros(8, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tsne.tsne_embed(z, perplexity=2.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tsne.TsneAffinities(z)
    with pytest.raises(ValueError, match="dtype"):
        tsne.tsne_embed_host(np.zeros((2, 2)), np.zeros((2, 2)), dtype="bf16")
