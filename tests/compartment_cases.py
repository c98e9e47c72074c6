"""Seeded contact maps with PLANTED A/B compartments for the compartment tests (tests/test_compartments_host.py,
tests/test_gpu_compartments.py), and the bounds both tiers assert.  References are computed once per case and shared
(functools.lru_cache); nobody writes to them.

The generator: comp is +-1 in runs of max(4, n // 10) bins, alternating, with every run flipped with probability 0.3 (both signs
are kept present); counts are Poisson(2000 / (1 + d) * (1.6 within a compartment, 0.6 across) + 0.5) on the upper triangle;
chosen bins are emptied to make holes.  The seeds below are fixed so that lambda_2 / lambda_1 <= 0.5 on every case and, on the
three-vector cases, every tested vector has a gap of at least 0.2 lambda_j to both neighbours: the host tier re-checks both."""
import functools

import numpy as np

from chromegcn_amd import compartments as CP

RES = 100000
EPS = 2.0 ** -53
TOL = 1e-10

# name: (n bins, seed, emptied bins)
PLANTED = {
    "n17_a": (17, 1, ()), "n17_b": (17, 7, ()),
    "n40_a": (40, 1, ()), "n40_b": (40, 3, ()),
    "n65_a": (65, 1, (30,)), "n65_b": (65, 2, (7,)),
    "n130_a": (130, 1, (3, 64, 100)), "n130_b": (130, 2, (0, 65, 129)),
    "n257_a": (257, 1, (128,)), "n257_b": (257, 3, (200,)),
    "n600_a": (600, 1, ()), "n600_b": (600, 3, ()),
}
THREE_VECTORS = ("n17_b", "n40_b", "n257_b", "n600_b")
GPU_PLANTED = ("n17_a", "n65_b", "n130_a", "n257_a", "n600_b")


def planted_comp(n, rng):
    run = max(4, n // 10)
    runs = -(-n // run)
    sign = np.where(np.arange(runs) % 2 == 0, 1, -1) * np.where(rng.random(runs) < 0.3, -1, 1)
    if runs > 1 and abs(int(sign.sum())) == runs:
        sign[runs // 2] = -sign[runs // 2]
    return np.repeat(sign, run)[:n].astype(np.int64)


def planted(n, seed, holes=(), frac=False):
    """dict(pos1, pos2, count, res, n_bins, comp int64 [n] (+-1), holes)"""
    rng = np.random.default_rng(seed)
    comp = planted_comp(n, rng)
    a, b = np.triu_indices(n)
    c = rng.poisson(2000.0 / (1.0 + (b - a)) * np.where(comp[a] == comp[b], 1.6, 0.6) + 0.5).astype(np.float64)
    k = (c > 0) & ~np.isin(a, holes) & ~np.isin(b, holes)
    a, b, c = a[k], b[k], c[k]
    if frac:
        c = c * rng.uniform(0.5, 1.5, c.size)
    sw = rng.random(a.size) < 0.3
    return dict(pos1=(np.where(sw, b, a) * RES).astype(np.int32), pos2=(np.where(sw, a, b) * RES).astype(np.int32), count=c, res=RES,
                n_bins=n, comp=comp, holes=np.asarray(holes, dtype=np.int64))


@functools.lru_cache(maxsize=None)
def planted_case(name):
    n, seed, holes = PLANTED[name]
    return planted(n, seed, holes)


@functools.lru_cache(maxsize=None)
def planted_host(name, n_eigs=1):
    """compartments_host of a planted case on raw counts, oriented by the planted calls"""
    c = planted_case(name)
    return CP.compartments_host(c["pos1"], c["pos2"], c["count"], None, RES, n_bins=c["n_bins"], n_eigs=n_eigs,
                                orient=c["comp"].astype(np.float64), tol=TOL)


# ----------------------------------------------------------------------------------------------
# the kernel cases: m kept bins exactly, with and without holes, with and without a norm vector
# ----------------------------------------------------------------------------------------------
KERNEL_M = (1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 130, 257)
LARGE_M = 1500


def _holes(m, with_holes, with_norm=False):
    """the emptied bins of a kernel case with m kept bins: none, or one near each end (one only below 5 bins); with_norm =
    "short": five, the last of them the map's last bin"""
    if not with_holes:
        return ()
    if with_norm == "short":
        return (2, 20, 40, 50, m + 4)
    return (1,) if m < 5 else (2, m - 1)       # bins of the n = m + len(holes) map


@functools.lru_cache(maxsize=None)
def kernel_case(m, with_holes, with_norm):
    """a planted map that keeps exactly m bins: dict(planted's, norm: None or float64 [n], keep).  With a norm and holes, the
    second hole is a NaN of the vector over a bin that HAS contacts, and the counts are fractional.  with_norm = "short" (with
    holes, m >= 51): the holes behind the first are a NaN, a 0 and a +inf of the vector and a last bin beyond its end, all
    over bins that have contacts."""
    holes = _holes(m, with_holes, with_norm)
    n = m + len(holes)
    by_norm = holes[1:] if with_norm else ()
    c = planted(n, 100 + m, tuple(h for h in holes if h not in by_norm), frac=bool(with_norm))
    norm = None
    if with_norm:
        norm = np.random.default_rng(7 + m).lognormal(0.0, 0.4, n)
        norm[list(by_norm)] = np.nan
    if with_norm == "short":
        norm[holes[2]], norm[holes[3]] = 0.0, np.inf
        norm = norm[:n - 1].copy()
    keep = np.setdiff1d(np.arange(n), holes).astype(np.int32)
    assert keep.size == m
    return dict(c, norm=norm, keep=keep)


KERNEL_CASES = [(m, h, v) for m in KERNEL_M for h in (False, True) for v in (False, True)] + [(LARGE_M, False, False),
                                                                                             (LARGE_M, True, True),
                                                                                             (65, True, "short")]


def case_id(c):
    return "m%d%s%s" % (c[0], "_holes" if c[1] else "", "_shortnorm" if c[2] == "short" else "_norm" if c[2] else "")


# ----------------------------------------------------------------------------------------------
# bounds
# ----------------------------------------------------------------------------------------------
def reordered_sum_bound(abs_terms, axis=-1):
    """(K - 1) 2^-53 sum|terms| per sum, K the non-zero terms: the first-order bound of one summation order of K terms"""
    abs_terms = np.asarray(abs_terms)
    K = np.count_nonzero(abs_terms, axis=axis)
    return np.maximum(K - 1, 0) * EPS * abs_terms.sum(axis=axis)


def eigh_desc(C):
    """(eigenvalues descending, vectors as columns) of the symmetric C"""
    w, V = np.linalg.eigh(C)
    return w[::-1], V[:, ::-1]


def vector_bounds(lam, m, tol, n_vectors):
    """The host tier's bound per vector j < n_vectors: 2 tol lambda_j / gap_j + 64 m 2^-53, gap_j the distance of lambda_j to
    its nearest other eigenvalue (Davis-Kahan for the residual stop r <= tol lambda: sin(angle) <= r / gap, and
    |v - u|_2 <= sqrt(2) sin(angle) at a small angle, rounded up to 2), plus the bounds of the vectors found before it, whose
    errors the deflation passes on.  lam: every eigenvalue, descending."""
    own = []
    for j in range(n_vectors):
        gap = min(abs(lam[j] - lam[k]) for k in (j - 1, j + 1) if 0 <= k < lam.size)
        own.append(2.0 * tol * lam[j] / gap + 64.0 * m * EPS)
    return [sum(own[:j + 1]) for j in range(n_vectors)]


def gaps(lam, j):
    """the distances of lambda_j to its two neighbours, as shares of lambda_j"""
    return [abs(lam[j] - lam[k]) / lam[j] for k in (j - 1, j + 1) if 0 <= k < lam.size]


def aligned(u, v):
    """u with the sign that makes u . v positive"""
    return u if float(u @ v) >= 0 else -u
