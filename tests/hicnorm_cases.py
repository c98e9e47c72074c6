"""Seeded, small Hi-C-like record sets for the norm-vector tests (tests/test_hicnorm_host.py, tests/test_gpu_hicnorm.py):
contacts whose density decays with distance, a log-normal bias per bin, Poisson counts; with and without diagonal records, a
share of duplicated records, a share of records with pos1 > pos2, some bins left empty.  Host references are computed once
per case and shared (functools.lru_cache); nobody writes to them."""
import functools

import numpy as np

from chromegcn_amd import hicnorm

RES = 1000


def hic_like(n_bins, n_pairs, seed, diagonal=True, dup_share=0.15, swap_share=0.3, n_empty=0, fractional=False, jitter=True):
    """dict(pos1, pos2, count, res, n_bins, empty): every bin that is not empty is in contact with the next such bin (and with
    itself when `diagonal`), so no kept row is isolated"""
    rng = np.random.default_rng(seed)
    alive = np.sort(rng.choice(n_bins, n_bins - n_empty, replace=False))
    na = alive.size
    bias = rng.lognormal(0.0, 0.5, na)
    a = rng.integers(0, na, n_pairs)
    d = np.floor(np.exp(rng.uniform(0.0, np.log(na + 1.0), n_pairs))).astype(np.int64) - 1   # log-uniform distance
    b = a + d
    ok = b < na
    a, b = a[ok], b[ok]
    chain = np.arange(na - 1)
    a, b = np.concatenate([a, chain]), np.concatenate([b, chain + 1])
    if diagonal:
        a, b = np.concatenate([a, np.arange(na)]), np.concatenate([b, np.arange(na)])
    else:
        a, b = a[a != b], b[a != b]
    key = np.unique(a * na + b)
    a, b = key // na, key % na
    if dup_share:
        again = rng.integers(0, a.size, int(dup_share * a.size))
        a, b = np.concatenate([a, a[again]]), np.concatenate([b, b[again]])
    count = 1.0 + rng.poisson(20.0 * bias[a] * bias[b] / (1.0 + (b - a)))
    if fractional:
        count = count * rng.uniform(0.5, 1.5, count.size)
    order = rng.permutation(a.size)
    a, b, count = a[order], b[order], count[order]
    p1, p2 = alive[a] * RES, alive[b] * RES
    if jitter:
        p1, p2 = p1 + rng.integers(0, RES, p1.size), p2 + rng.integers(0, RES, p2.size)
    swap = rng.random(p1.size) < swap_share
    p1, p2 = np.where(swap, p2, p1), np.where(swap, p1, p2)
    return dict(pos1=p1.astype(np.int32), pos2=p2.astype(np.int32), count=count.astype(np.float64), res=RES, n_bins=n_bins,
                empty=np.setdiff1d(np.arange(n_bins), alive))


def full_row(n_bins=300, hub=7, merged=600, seed=11):
    """one bin in contact with all n_bins (a row longer than a workgroup), one entry merged from `merged` duplicate records"""
    c = hic_like(n_bins, 4000, seed)
    rng = np.random.default_rng(seed + 1)
    others = np.arange(n_bins)
    p1 = np.concatenate([c["pos1"], np.full(n_bins, hub * RES), np.full(merged, 3 * RES + 1)])
    p2 = np.concatenate([c["pos2"], others * RES + 5, np.full(merged, 9 * RES + 2)])
    cnt = np.concatenate([c["count"], 1.0 + rng.poisson(3.0, n_bins), 1.0 + rng.poisson(2.0, merged)])
    order = rng.permutation(p1.size)
    return dict(pos1=p1[order].astype(np.int32), pos2=p2[order].astype(np.int32), count=cnt[order].astype(np.float64), res=RES,
                n_bins=n_bins, empty=np.zeros(0, np.int64))


def leafy(n_bins=63, leaves=3, seed=13):
    """the last `leaves` bins touch only themselves and one other bin: rows of two entries, which min_row_nnz = 3 leaves out"""
    c = hic_like(n_bins - leaves, 80, seed)
    leaf = np.arange(n_bins - leaves, n_bins)
    p1 = np.concatenate([c["pos1"], leaf * RES, leaf * RES + 3])
    p2 = np.concatenate([c["pos2"], leaf * RES + 1, (leaf - 20) * RES])
    cnt = np.concatenate([c["count"], np.full(leaves, 6.0), np.full(leaves, 2.0)])
    return dict(pos1=p1.astype(np.int32), pos2=p2.astype(np.int32), count=cnt, res=RES, n_bins=n_bins, empty=np.zeros(0, np.int64))


CASES = {
    "n1": lambda: dict(pos1=np.array([10], np.int32), pos2=np.array([900], np.int32), count=np.array([5.0]), res=RES, n_bins=1,
                       empty=np.zeros(0, np.int64)),
    "n2": lambda: hic_like(2, 6, 2),
    "n63": lambda: hic_like(63, 400, 3, n_empty=4),
    "n63_leafy": leafy,
    "n64": lambda: hic_like(64, 2000, 4),
    "n65": lambda: hic_like(65, 3000, 5, n_empty=3),
    "n65_nodiag": lambda: hic_like(65, 3000, 6, diagonal=False),
    "n257": lambda: hic_like(257, 8000, 7, n_empty=9),
    "n257_frac": lambda: hic_like(257, 8000, 8, n_empty=5, fractional=True, dup_share=0.5),
    "n1000": lambda: hic_like(1000, 30000, 9, n_empty=20),
    "fullrow": full_row,
}
KR_CASES = tuple(CASES)   # every generator case is balanced


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def host_matrix(name):
    c = case(name)
    return hicnorm.contact_matrix_host(c["pos1"], c["pos2"], c["count"], c["res"], c["n_bins"])


@functools.lru_cache(maxsize=None)
def host_kr(name, tol, min_row_nnz=1):
    """(x, info) of the host restatement"""
    return hicnorm.kr_balance_host(host_matrix(name), tol=tol, max_mvp=1000, min_row_nnz=min_row_nnz, kr_retry=False)


def dense(c):
    """A by the definition, one record after the other"""
    n, res = c["n_bins"], c["res"]
    a = np.zeros((n, n))
    for p, q, v in zip(c["pos1"].tolist(), c["pos2"].tolist(), c["count"].tolist()):
        i, j = p // res, q // res
        a[i, j] += v
        if i != j:
            a[j, i] += v
    return a


def kr_residual(A, x):
    """(max_i |x_i (A_S x)_i - 1| over the kept rows S = where x is a number, the longest kept row)"""
    keep = ~np.isnan(x)
    idx = np.flatnonzero(keep)
    As = A[idx][:, idx].tocsr()
    xs = x[idx]
    k_row = int(np.diff(As.indptr).max()) if idx.size else 0
    return (float(np.abs(xs * (As @ xs) - 1.0).max()) if idx.size else 0.0), k_row


def graph_case(seed=21, n_bins=120, n_pairs=2500):
    """records for the graph builder (no two records of one ordered pair, positions on the grid) and a window set"""
    c = hic_like(n_bins, n_pairs, seed, dup_share=0.0, n_empty=6, jitter=False)
    rng = np.random.default_rng(seed + 100)
    ws = np.sort(rng.choice(n_bins, 90, replace=False)).astype(np.int32) * RES
    return c, ws


GRAPH_EDGES = 800   # hic_edges of the end-to-end case: K = 400 records
