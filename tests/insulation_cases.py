"""Seeded record sets for the insulation tests (tests/test_insulation_host.py, tests/test_gpu_insulation.py): the Hi-C-like sets
of hicnorm_cases for the diamond sums, and contact maps with PLANTED domains for everything behind the sums.  References are
computed once per case and shared (functools.lru_cache); nobody writes to them."""
import functools

import numpy as np
import scipy.sparse as sp

from chromegcn_amd import hicnorm, insulation

from hicnorm_cases import GRAPH_EDGES, RES, case, dense, full_row, graph_case, hic_like  # noqa: F401

EPS = 2.0 ** -53
SUM_WINDOWS = (1, 2, 5, 63, 64, 65, 300)     # lane trips either side of 64; the largest exceeds every n of the sums cases
# Recovery of the planted starts: windows of 10 and 25 bins on raw counts with span = w (a 5-bin window is for the sums only:
# with empty bins next to a boundary it misses a planted start).  On seeds 1-5 every planted start has strength >= 1.54 and the
# strongest other minimum 0.52, so min_strength = 1.0 returns exactly the planted starts.
RECOVERY_WINDOWS = (10, 25)
RECOVERY_STRENGTH = 1.0
SEEDS = (1, 2, 3, 4, 5)


def planted(n_bins, starts, seed, reach=60, inside=40.0, leak=0.25, n_empty=0, frac=False):
    """(pos1, pos2, count, empty bins): Poisson counts that fall with distance, `leak` times weaker across a planted start"""
    rng = np.random.default_rng(seed)
    dom = np.searchsorted(np.asarray(starts), np.arange(n_bins), side="right")
    a, b = np.triu_indices(n_bins)
    k = (b - a) <= reach
    a, b = a[k], b[k]
    c = rng.poisson(inside / (1.0 + (b - a)) * np.where(dom[a] == dom[b], 1.0, leak)).astype(np.float64)
    empty = rng.choice(n_bins, n_empty, replace=False) if n_empty else np.zeros(0, int)
    k = (c > 0) & ~np.isin(a, empty) & ~np.isin(b, empty)
    a, b, c = a[k], b[k], c[k]
    if frac:
        c = c * rng.uniform(0.5, 1.5, c.size)
    o = rng.permutation(a.size)
    a, b, c = a[o], b[o], c[o]
    sw = rng.random(a.size) < 0.3
    return np.where(sw, b, a) * RES, np.where(sw, a, b) * RES, c, empty


PLANTED = {
    "n257": dict(n_bins=257, starts=(64, 128, 192)),
    "n400": dict(n_bins=400, starts=(57, 130, 171, 260, 333)),
    "n400_empty": dict(n_bins=400, starts=(57, 130, 171, 260, 333), n_empty=6),
    "n400_frac": dict(n_bins=400, starts=(57, 130, 171, 260, 333), frac=True),
    "n1000": dict(n_bins=1000, starts=(90, 200, 260, 400, 555, 640, 700, 850, 930)),
}
INTEGER_PLANTED = ("n257", "n400", "n400_empty", "n1000")


@functools.lru_cache(maxsize=None)
def planted_case(name, seed=1):
    """dict(pos1, pos2, count, res, n_bins, starts, empty) of one planted case"""
    kw = PLANTED[name]
    p1, p2, c, empty = planted(seed=seed, **kw)
    return dict(pos1=p1.astype(np.int32), pos2=p2.astype(np.int32), count=c, res=RES, n_bins=kw["n_bins"],
                starts=np.asarray(kw["starts"], dtype=np.int64), empty=empty)


@functools.lru_cache(maxsize=None)
def planted_host(name, seed=1):
    """insulation_host of a planted case on raw counts at RECOVERY_WINDOWS with span = w and min_strength = RECOVERY_STRENGTH"""
    c = planted_case(name, seed)
    return insulation.insulation_host(c["pos1"], c["pos2"], c["count"], None, RES, [w * RES for w in RECOVERY_WINDOWS],
                                      n_bins=c["n_bins"], min_strength=RECOVERY_STRENGTH)


def noisy_norm(n, seed, inf=False):
    """a norm vector with NaN and 0 bins, one bin short of n (the last bin reads as +inf); inf: one +inf entry as well"""
    rng = np.random.default_rng(seed)
    v = rng.lognormal(0.0, 0.4, max(n - 1, 1))
    if n > 4:
        v[rng.choice(v.size, 2, replace=False)] = np.nan
        v[rng.choice(v.size, 2, replace=False)] = 0.0
    if inf:
        good = np.flatnonzero(np.isfinite(v) & (v != 0.0))
        v[good[good.size // 2]] = np.inf
    return v


def balanced(A, norm):
    """B of rule 1 as a CSR with A's pattern (sorted columns)"""
    A = sp.csr_matrix(A, dtype=np.float64)
    A.sort_indices()
    if norm is None:
        return A
    nv = hicnorm.clean_norm(norm, A.shape[0])
    row = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        return sp.csr_matrix((A.data / (nv[row] * nv[A.indices]), A.indices, A.indptr), shape=A.shape)


def term_counts(A, norm, windows):
    """K int64 [W, n]: the non-zero terms inside each diamond (the diamond sums of B's pattern: exact small integers)"""
    B = balanced(A, norm)
    pattern = sp.csr_matrix(((B.data != 0).astype(np.float64), B.indices, B.indptr), shape=B.shape)
    return insulation.diamond_sums_host(pattern, None, windows).astype(np.int64)


def assert_sums_close(got, ref, K, exact):
    """the same zero pattern; bit-equal when `exact`, else within 2 max(K - 1, 0) 2^-53 relative"""
    assert got.shape == ref.shape
    assert np.array_equal(got == 0, ref == 0)
    if exact:
        assert np.array_equal(got, ref)
    else:
        err = np.abs(got - ref)
        bound = 2.0 * np.maximum(K - 1, 0) * EPS * np.abs(ref)
        assert np.all(err <= bound), float(np.max(err / np.maximum(np.abs(ref), 1e-300) / EPS))


def loop_sums(a, norm, windows):
    """rule 2 as the literal double loop over the dense matrix: (S, K) with K the non-zero terms of each sum"""
    n = a.shape[0]
    if norm is not None:
        nv = hicnorm.clean_norm(norm, n)
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            a = a / (nv[:, None] * nv[None, :])
    rows = a.tolist()
    S, K = np.zeros((len(windows), n)), np.zeros((len(windows), n), np.int64)
    for k, w in enumerate(windows):
        for i in range(n):
            s, cnt = 0.0, 0
            hi = min(i + w, n)
            for r in range(max(i - w, 0), i):
                for v in rows[r][i:hi]:
                    if v != 0.0:
                        s += v
                        cnt += 1
            S[k, i], K[k, i] = s, cnt
    return S, K
