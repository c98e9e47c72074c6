"""The numpy / scipy restatement of the Hi-C norm vectors (chromegcn_amd/hicnorm.py) against the definitions, no GPU: the
contact matrix against a dense double loop, VC / SQRTVC against dense sums, Knight-Ruiz against its own residual, the
product cap, the sparse-row ladder, and the string norms of build_hic_graph_host."""
import numpy as np
import pytest
import scipy.sparse as sp

from chromegcn_amd import HicNormError, build_hic_graph_host, contact_matrix_host, hic, hic_norm_vector_host, hicnorm, kr_balance_host

import hicnorm_cases as HC

SMALL = [n for n in HC.CASES if HC.CASES[n]()["n_bins"] <= 65]


@pytest.mark.parametrize("name", SMALL)
def test_contact_matrix_against_the_dense_double_loop(name):
    c, a = HC.case(name), HC.host_matrix(name)
    want = HC.dense(c)
    assert a.dtype == np.float64 and a.shape == want.shape and a.has_sorted_indices
    assert np.array_equal(a.toarray(), want)                       # integer counts: exact in any order
    assert np.array_equal(a.toarray(), a.toarray().T)
    assert a.nnz == np.count_nonzero(want)                         # counts are >= 1: no stored zero, no duplicate left
    for kind, ref in (("VC", want.sum(1)), ("SQRTVC", np.sqrt(want.sum(1)))):
        v, _ = hic_norm_vector_host(c["pos1"], c["pos2"], c["count"], kind, c["res"], c["n_bins"])
        assert np.array_equal(np.flatnonzero(np.isnan(v)), c["empty"]), (name, kind)
        keep = ~np.isnan(v)
        assert np.array_equal(v[keep], ref[keep]), (name, kind)


def test_fractional_counts_are_added_in_record_order():
    c = HC.case("n257_frac")
    a = HC.host_matrix("n257_frac").toarray()
    assert np.array_equal(a, HC.dense(c))                          # the double loop adds in record order too


def test_n_bins_defaults_to_the_largest_bin_and_a_smaller_one_raises():
    c = HC.case("n65")
    top = int(max(c["pos1"].max(), c["pos2"].max())) // c["res"] + 1
    assert contact_matrix_host(c["pos1"], c["pos2"], c["count"], c["res"]).shape == (top, top)
    assert contact_matrix_host(c["pos1"], c["pos2"], c["count"], c["res"], top + 7).shape == (top + 7, top + 7)
    with pytest.raises(ValueError, match="n_bins"):
        contact_matrix_host(c["pos1"], c["pos2"], c["count"], c["res"], top - 1)
    assert contact_matrix_host([], [], [], 1000).shape == (0, 0)


@pytest.mark.parametrize("bad", [-1.0, float("nan"), float("inf")])
def test_a_negative_or_non_finite_count_raises(bad):
    with pytest.raises(ValueError, match="finite and non-negative"):
        contact_matrix_host([0, 1000], [1000, 2000], [1.0, bad], 1000)
    with pytest.raises(ValueError, match="finite and non-negative"):
        hic_norm_vector_host([0, 1000], [1000, 2000], [1.0, bad], "KR", 1000)


@pytest.mark.parametrize("tol", [1e-6, 1e-10])
@pytest.mark.parametrize("name", HC.KR_CASES)
def test_kr_meets_its_residual(name, tol):
    a = HC.host_matrix(name)
    x, info = HC.host_kr(name, tol)
    c = HC.case(name)
    assert info["converged"] and info["residual"] <= tol and info["mvp"] < 200, (name, info)
    assert np.array_equal(np.flatnonzero(np.isnan(x)), c["empty"])
    assert np.all(x[~np.isnan(x)] > 0)
    worst, k_row = HC.kr_residual(a, x)
    assert worst <= tol + (k_row + 2) * 2.0 ** -52, (name, worst)
    assert info["kept"] == c["n_bins"] - c["empty"].size and info["excluded"] == 0 and info["host_syncs"] == 0


@pytest.mark.parametrize("tol", [1e-6, 1e-10])
@pytest.mark.parametrize("name", HC.KR_CASES + ("n70001_tiny",))
def test_clips_entry_agrees_with_an_independent_count(name, tol):
    """info["clips"] against the listing written out once more (HC.kr_clip_count); the scaled cases take the upper clip, the
    wide ones the lower one, no other case takes either; and no run comes within 1e-6 of a branch it did not take, so the
    device's roundings cannot send it down another one"""
    x, info = HC.host_kr(name, tol)
    clips, margin, mvp = HC.kr_clip_count(HC.host_matrix(name), tol)
    print("%s tol %g: clips %s, margin %.3g, %d products" % (name, tol, clips, margin, mvp))
    assert info["clips"] == clips and info["mvp"] == mvp and info["converged"]
    assert (clips[1] >= 1) == (name in HC.UPPER_CLIP) and (clips[0] >= 1) == (name in HC.LOWER_CLIP)
    if name.endswith("_tiny"):
        assert clips[1] >= 5
    assert margin > 1e-6


@pytest.mark.parametrize("name", ["n63_leafy", "n257", "fullrow", "n257_tiny", "n65_wide", "n257_wide"])
def test_the_step_restatement_in_the_drivers_order_is_the_listing(name):
    """HC.kr_step_host, which tests/test_gpu_hicnorm.py holds every operation of cgcn_hicnorm_kr_step to, run in
    _kr_run_device's order with scipy's product: the listing's x within a few roundings, its products and its clips"""
    mrn = 3 if name == "n63_leafy" else 1
    xh, ih = kr_balance_host(HC.host_matrix(name), tol=1e-10, min_row_nnz=mrn, kr_retry=False)
    x, mvp, clips = HC.kr_run_by_steps(HC.host_matrix(name), 1e-10, min_row_nnz=mrn)
    assert np.array_equal(np.isnan(x), np.isnan(xh)) and (mvp, clips) == (ih["mvp"], ih["clips"])
    keep = ~np.isnan(xh)
    assert np.abs(x[keep] / xh[keep] - 1.0).max() <= 1e-13


@pytest.mark.parametrize("name", HC.KR_LARGE)
def test_large_cases_need_a_second_trip_of_the_vector_step(name):
    """70 001 bins are 274 workgroups of 256: more partials than the 256 threads that fold them; 262 401 bins are 1026: more
    than the 1024 workgroups of the vector step's grid.  The host balances each in well under 100 products."""
    c = HC.case(name)
    blocks = -(-c["n_bins"] // 256)
    assert blocks > 256 and (blocks > 1024) == (name == "n262401")
    for tol in (1e-6, 1e-10):
        x, info = HC.host_kr(name, tol)
        worst, k_row = HC.kr_residual(HC.host_matrix(name), x)
        assert info["converged"] and info["mvp"] < 100 and worst <= tol + (k_row + 2) * 2.0 ** -52, (name, tol, info)
        assert np.array_equal(np.flatnonzero(np.isnan(x)), c["empty"])


def test_one_and_two_bins():
    x, info = kr_balance_host(sp.csr_matrix(np.array([[4.0]])))
    assert info["converged"] and x[0] == pytest.approx(0.5, abs=1e-6)   # |4 x^2 - 1| <= tol
    v, _ = hic_norm_vector_host([0], [10], [4.0], "KR", 1000)
    assert v[0] == pytest.approx(2.0, abs=1e-5)                    # count / (nv nv) = 1
    x, info = kr_balance_host(sp.csr_matrix(np.array([[2.0, 1.0], [1.0, 3.0]])))
    assert info["converged"] and np.abs(x * (np.array([[2.0, 1.0], [1.0, 3.0]]) @ x) - 1).max() <= 1e-6
    x, info = kr_balance_host(sp.csr_matrix((2, 2)))               # nothing in contact: nothing kept
    assert info["converged"] and info["kept"] == 0 and np.isnan(x).all()


def test_a_balanced_matrix_needs_no_inner_iteration():
    a = sp.csr_matrix(np.array([[0.5, 0.25, 0.25], [0.25, 0.5, 0.25], [0.25, 0.25, 0.5]]))
    x, info = kr_balance_host(a)
    assert np.array_equal(x, np.ones(3)) and info["converged"] and info["outer"] == 0 and info["mvp"] == 1


def test_the_product_cap_returns_unconverged():
    x, info = kr_balance_host(HC.host_matrix("n257"), max_mvp=5, kr_retry=False)
    assert info["converged"] is False and np.isfinite(info["residual"]) and info["mvp"] == 5
    assert info["residual"] > 1e-6


def test_the_ladder_moves_on_after_a_capped_run():
    a = HC.host_matrix("n257")
    _, nnz = hicnorm._row_stats_host(a)
    srt = np.sort(nnz[nnz > 0])
    x, info = kr_balance_host(a, max_mvp=5, kr_retry=True)
    want, last = [1], 1
    for q in hicnorm.LADDER:
        last = max(int(srt[int(q * srt.size)]), last + 1)
        want.append(last)
    assert info["ladder"] == want and info["min_row_nnz"] == want[-1] and not info["converged"]
    assert np.array_equal(np.isnan(x), ~(nnz >= want[-1]))
    # a run that converges at the second value stops there: the first one is capped by hand
    calls = []
    run = hicnorm._kr_run_host

    def capped_once(A, tol, max_mvp):
        calls.append(A.shape[0])
        return run(A, tol, 3 if len(calls) == 1 else max_mvp)

    hicnorm._kr_run_host = capped_once
    try:
        x, info = kr_balance_host(a, kr_retry=True)
    finally:
        hicnorm._kr_run_host = run
    assert info["converged"] and info["ladder"] == want[:2] and info["min_row_nnz"] == want[1] and len(calls) == 2
    assert info["excluded"] == int((nnz > 0).sum() - (nnz >= want[1]).sum())


def test_min_row_nnz_excludes_rows_and_balances_the_rest():
    a = HC.host_matrix("n63_leafy")
    _, nnz = hicnorm._row_stats_host(a)
    x, info = kr_balance_host(a, min_row_nnz=3, kr_retry=False)
    assert np.array_equal(np.flatnonzero(np.isnan(x)), [60, 61, 62]) and np.array_equal(np.isnan(x), nnz < 3)
    assert info["excluded"] == 3 and info["kept"] == 60
    assert info["converged"] and HC.kr_residual(a, x)[0] <= 1e-6 + 70 * 2.0 ** -52


def _rank_gap(c, ws, nv, k):
    v = np.sort(hic.survivor_values(c["pos1"], c["pos2"], c["count"], nv, c["res"], ws)[3])[::-1]
    assert v.size > k
    return (v[k - 1] - v[k]) / v[k - 1]


def test_string_norms_of_the_host_builder_and_scale_invariance():
    c, ws = HC.graph_case()
    k = HC.GRAPH_EDGES // 2
    for kind in ("KR", "VC", "SQRTVC"):
        nv, info = hic_norm_vector_host(c["pos1"], c["pos2"], c["count"], kind, c["res"], c["n_bins"])
        assert info.get("converged", True)
        # the values at rank K and K + 1 are apart: a vector that differs in the last bits selects the same records
        assert _rank_gap(c, ws, nv, k) > 1e-6, kind
        by_name = build_hic_graph_host(c["pos1"], c["pos2"], c["count"], kind, c["res"], ws, HC.GRAPH_EDGES)
        for vec in (nv, 7.5 * nv):
            a = build_hic_graph_host(c["pos1"], c["pos2"], c["count"], vec, c["res"], ws, HC.GRAPH_EDGES)
            assert np.array_equal(a.indptr, by_name.indptr) and np.array_equal(a.indices, by_name.indices), kind
        assert by_name.nnz > 0
    with pytest.raises(HicNormError) as e:
        build_hic_graph_host(c["pos1"], c["pos2"], c["count"], "KR", c["res"], ws, HC.GRAPH_EDGES, norm_args=dict(max_mvp=5))
    assert e.value.info["converged"] is False
    with pytest.raises(ValueError, match="none of"):
        build_hic_graph_host(c["pos1"], c["pos2"], c["count"], "kr", c["res"], ws, HC.GRAPH_EDGES)
