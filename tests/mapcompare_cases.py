"""Inputs of the map-comparison tests (tests/test_mapcompare_host.py, tests/test_gpu_mapcompare.py): sparse integer maps,
holes, noisy norm vectors, and planted maps with domains."""
import numpy as np
import scipy.sparse as sp

RES = 1000


def sparse_integer_map(n, reach, seed, density=0.3, top=40):
    """a symmetric CSR [n, n] of sparse integer counts within `reach` bins of the diagonal, some of them large"""
    rng = np.random.default_rng(seed)
    m = max(int(density * n * (reach + 1)), 1)
    i = rng.integers(0, n, m)
    j = np.minimum(i + rng.integers(0, reach + 1, m), n - 1)
    v = rng.integers(1, top, m).astype(np.float64)
    up = sp.coo_matrix((v, (i, j)), shape=(n, n)).tocsr()
    up.sum_duplicates()
    return sp.csr_matrix(up + sp.triu(up, 1).T)


def with_holes(A, bins):
    """the symmetric matrix without the rows and columns of `bins`"""
    A = sp.lil_matrix(A)
    for b in bins:
        A[b, :] = 0
        A[:, b] = 0
    A = sp.csr_matrix(A)
    A.eliminate_zeros()
    return A


def records_of(A, res=RES):
    """(pos1, pos2, count) at res with one record per upper-triangle entry of a symmetric matrix"""
    coo = sp.triu(sp.csr_matrix(A)).tocoo()
    return (coo.row * res).astype(np.int32), (coo.col * res).astype(np.int32), coo.data.astype(np.float64)


def noisy_norm(n, seed):
    """a norm vector of n entries around 1 with a NaN, a 0, an inf and a negative entry in it (where n allows)"""
    rng = np.random.default_rng(seed)
    v = rng.uniform(0.5, 2.0, n)
    for at, bad in zip((1, 3, 4, 6), (np.nan, 0.0, np.inf, -1.25)):
        if at < n:
            v[at] = bad
    return v


def planted_intensity(n, period, depth, factor=3.0):
    """the mean counts of a map with the distance decay depth / (1 + d), times `factor` inside domains of `period` bins"""
    i = np.arange(n)
    d = np.abs(i[:, None] - i[None, :])
    lam = depth / (1.0 + d)
    return np.where((i[:, None] // period) == (i[None, :] // period), factor * lam, lam)


def planted_draw(n, period, depth, seed, reach=None):
    """(pos1, pos2, count) of one Poisson draw of planted_intensity, upper triangle, up to `reach` bins from the diagonal"""
    rng = np.random.default_rng(seed)
    c = np.triu(rng.poisson(planted_intensity(n, period, depth))).astype(np.float64)
    if reach is not None:
        c = np.triu(c) - np.triu(c, reach + 1)
    return records_of(sp.csr_matrix(c + np.triu(c, 1).T))
