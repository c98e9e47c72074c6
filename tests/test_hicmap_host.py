"""The front end that the Hi-C map analyses share (chromegcn_amd/hicmap.py, hicnorm.clean_norm; no GPU): the norm vector as a
balanced value reads it, bin validity, the CSR of a graph and its edge rows, the band of a matrix, and resolve_host against the
sequence of calls it replaces."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from chromegcn_amd import hicdist, hicmap, hicnorm

import loops_cases as LC


def same(a, b):
    """equal arrays, NaNs aligned; None equals None alone"""
    if a is None or b is None:
        return a is None and b is None
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def test_clean_norm_and_valid_bins():
    norm = np.array([2.0, np.nan, 0.0, -3.0, np.inf, 0.5])
    got = hicnorm.clean_norm(norm, 8)
    assert np.array_equal(got, [2.0, np.inf, np.inf, -3.0, np.inf, 0.5, np.inf, np.inf])       # beyond its length: +inf
    assert np.array_equal(hicnorm.clean_norm(norm, 3), [2.0, np.inf, np.inf]) and hicnorm.clean_norm(norm, 0).size == 0
    assert np.isnan(norm[1]) and norm[2] == 0.0                                                 # the argument is not written
    vc = np.array([1.0, 1.0, 1.0, 1.0, 1.0, 0.0, 4.0, 0.0])
    assert np.array_equal(hicmap.valid_bins(vc, None), vc > 0)
    assert np.array_equal(hicmap.valid_bins(vc, norm), [True, False, False, True, False, False, False, False])
    assert np.array_equal(hicmap.valid_bins(vc[:, None], norm), hicmap.valid_bins(vc, norm))    # a column of row sums


def test_csr_of_and_edge_rows():
    g = sp.csr_matrix(np.array([[1, 1, 0, 0], [0, 0, 0, 0], [1, 0, 1, 1], [0, 0, 1, 0]], dtype=np.float64))
    want = (g.indptr.astype(np.int64), g.indices.astype(np.int64), int(g.nnz))

    class Graph:
        rowptr, col = torch.from_numpy(g.indptr.copy()), torch.from_numpy(np.concatenate([g.indices, [9, 9]]))

    for given in (g, g.tocoo(), (g.indptr, g.indices), [g.indptr, np.concatenate([g.indices, [9]]), 99], Graph()):
        rowptr, col, nnz = hicmap.csr_of(given)
        assert rowptr.dtype == col.dtype == np.int64 and nnz == want[2]
        assert np.array_equal(rowptr, want[0]) and np.array_equal(col, want[1])                 # col is cut at nnz
    row, col, nnz = hicmap.edge_rows(g, 4, "x")
    assert np.array_equal(row, g.tocoo().row) and np.array_equal(col, g.tocoo().col) and nnz == g.nnz
    with pytest.raises(ValueError, match="the graph has 4 windows but x has 3"):
        hicmap.edge_rows(g, 3, "x")


def test_band_host():
    A = LC.sparse_integer_map(40, 12, 3)
    dense = A.toarray()
    for width in (1, 5, 13, 64, 70):
        band = hicmap.band_host(A, width)
        assert band.shape == (40, width)
        for i in range(40):
            for d in range(width):
                assert band[i, d] == (dense[i, i + d] if i + d < 40 else 0.0)


def records_40():
    """40 bins of 1 kb, integer counts within 12 bins of the diagonal, bin 17 empty"""
    p1, p2, c = LC.records_of(LC.sparse_integer_map(40, 12, 3, density=0.4))
    k = (p1 // LC.RES != 17) & (p2 // LC.RES != 17)
    return p1[k], p2[k], c[k]


@pytest.mark.parametrize("expected", [None, "auto", "vector"])
@pytest.mark.parametrize("norm", [None, "VC", "short"])
def test_resolve_host_is_the_sequence_it_replaces(norm, expected):
    p1, p2, c = records_40()
    res, n = LC.RES, 40
    norm = LC.noisy_norm(30, 5)[:25] if norm == "short" else norm
    expected = np.random.default_rng(1).uniform(0.5, 2.0, 33) if expected == "vector" else expected
    A = hicnorm.contact_matrix_host(p1, p2, c, res, n)
    assert A.shape == (n, n) and A[17].nnz == 0
    nv = norm
    if isinstance(norm, str):
        nv, info = hicnorm.hic_norm_vector_host(p1, p2, c, norm, res, n)
        hicnorm._require_converged(info)
    ex = expected
    if isinstance(expected, str):
        ex = hicdist.expected_from_sums(*hicdist.distance_sums_device_order_host(p1, p2, c, nv, res, n), min_count=50)
    got_A, got_vc, got_nv, got_ex = hicmap.resolve_host(p1, p2, c, norm, res, n, None, expected, dict(min_count=50))
    assert (got_A != A).nnz == 0 and np.array_equal(got_A.indptr, A.indptr) and np.array_equal(got_A.indices, A.indices)
    assert np.array_equal(got_vc, np.asarray(A.sum(axis=1)).ravel()) and got_vc[17] == 0
    assert same(got_nv, nv) and same(got_ex, ex)
    assert (got_nv is None) == (norm is None) and (got_ex is None) == (expected is None)
    if isinstance(expected, str):
        assert got_ex.shape == (n,) and np.isfinite(got_ex).any()


def test_resolve_host_errors_and_its_two_halves():
    p1, p2, c = records_40()
    with pytest.raises(ValueError, match="expected='nonsense' is neither a vector nor 'auto'"):
        hicmap.resolve_host(p1, p2, c, None, LC.RES, 40, expected="nonsense")
    A, vc = hicmap.matrix_host(p1, p2, c, LC.RES)                              # n_bins left to the records
    assert A.shape[0] == vc.size == int(max(p1.max(), p2.max())) // LC.RES + 1
    nv, ex = hicmap.vectors_host(p1, p2, c, A.shape[0], "VC", LC.RES, expected="auto")
    whole = hicmap.resolve_host(p1, p2, c, "VC", LC.RES, expected="auto")
    assert (whole[0] != A).nnz == 0 and same(whole[1], vc) and same(whole[2], nv) and same(whole[3], ex)
