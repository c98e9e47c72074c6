"""Shared inputs and references of the pile-up tests (tests/test_pileup_host.py, tests/test_gpu_pileup.py): the literal Python
loop over centres, cells and slices that states pileup.py's rules 2 to 4, seeded centre lists with every kind of skipped
centre, and the integer maps, noisy norm and planted maps of loops_cases.  References are computed once per case and shared
(functools.lru_cache); nobody writes to them."""
import functools

import numpy as np

from chromegcn_amd import pileup

import loops_cases as LC  # noqa: F401
from loops_cases import RES, noisy_norm, planted, records_of, sparse_integer_map  # noqa: F401

W_ALL = (1, 2, 5, 10)
M_ALL = (0, 1, 255, 256, 257, 1025)        # either side of one slice, and five slices
G_ALL = (1, 3, 64)                         # 3: group 1 stays empty


def rule_for(n, w, value="oe", extra=25, **kw):
    """a rule at RES with the default min_dist = 3 w and max_dist = 3 w + extra"""
    return pileup.pileup_rule(RES, n, value=value, w=w, max_distance_bp=(3 * w + extra) * RES, **kw)


def smallest_n(w, min_dist=None):
    """the smallest map with one legal centre: (w, w + min_dist)"""
    return 2 * w + 1 + (3 * w if min_dist is None else min_dist)


def centres(n, r, M, G, seed, legal=0.7):
    """(ci, cj, group) int64 [M]: `legal` of them drawn inside the limits (where the map has room), the rest anywhere within
    two bins outside them; three in ten with the larger bin first; groups interleaved at random over -1 .. G (both ends are
    skipped), group 1 left empty when G == 3"""
    rng = np.random.default_rng(seed)
    i = rng.integers(-2, n + 2, M)
    d = rng.integers(max(r.min_dist - 2, 0), r.max_dist + 3, M)
    room = n - 1 - 2 * r.w - r.min_dist          # i runs over w .. w + room
    if room >= 0:
        li = r.w + rng.integers(0, room + 1, M)
        ld = r.min_dist + rng.integers(0, np.minimum(r.max_dist, n - 1 - r.w - li) - r.min_dist + 1)
        ok = rng.random(M) < legal
        i, d = np.where(ok, li, i), np.where(ok, ld, d)
    j = i + d
    sw = rng.random(M) < 0.3
    g = rng.integers(-1, G + 1, M)
    g = np.where(rng.random(M) < 0.8, np.clip(g, 0, G - 1), g)
    if G == 3:
        g = np.where(g == 1, 2, g)
    return np.where(sw, j, i).astype(np.int64), np.where(sw, i, j).astype(np.int64), g.astype(np.int64)


def literal_sums(vb, ci, cj, group, G, r):
    """rules 2 to 4 as the literal loop: (P [G, S, S], N, kept, skipped) from a value band"""
    vb = np.asarray(vb, dtype=np.float64)
    n, w, S = vb.shape[0], r.w, r.S
    group = [0] * len(ci) if group is None else group
    lists, skipped = [[] for _ in range(G)], dict.fromkeys(pileup.REASONS, 0)
    for a, b, g in zip(ci, cj, group):
        i, j, g = int(min(a, b)), int(max(a, b)), int(g)
        if not 0 <= g < G:
            skipped["group"] += 1
        elif i - w < 0 or j + w > n - 1:
            skipped["edge"] += 1
        elif j - i < r.min_dist:
            skipped["near"] += 1
        elif j - i > r.max_dist:
            skipped["far"] += 1
        else:
            lists[g].append((i, j))
    P, N = np.zeros((G, S, S)), np.zeros((G, S, S), np.int64)
    for g in range(G):
        for s in range(0, len(lists[g]), pileup.SLICE):
            part = [[0.0] * S for _ in range(S)]
            for i, j in lists[g][s:s + pileup.SLICE]:
                for da in range(-w, w + 1):
                    for db in range(-w, w + 1):
                        v = float(vb[i + da, (j + db) - (i + da)])
                        if v == v:
                            part[da + w][db + w] = part[da + w][db + w] + v
                            N[g, da + w, db + w] += 1
            for x in range(S):
                for y in range(S):
                    P[g, x, y] = float(P[g, x, y]) + part[x][y]
    return P, N, np.array([len(x) for x in lists], dtype=np.int64), skipped


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def assert_same_pileup(got: pileup.Pileup, want: pileup.Pileup):
    assert same_bits(got.sum, want.sum) and np.array_equal(got.count, want.count)
    assert np.array_equal(got.kept, want.kept) and got.skipped == want.skipped
    assert same_bits(got.mean, want.mean)


@functools.lru_cache(maxsize=None)
def integer_map(n, seed=0, density=0.5):
    """(the symmetric CSR of sparse integer counts, its records) with contacts at every distance"""
    A = sparse_integer_map(n, n, 100 + n + seed, density=density)
    return A, records_of(A)


def integer_reference(A, ci, cj, g, G, r):
    """(P, N) int64 [G, S, S] of value = "observed" without a vector on an integer map, by np.add.at"""
    dense = np.asarray(A.todense()).astype(np.int64)
    n, w, S = dense.shape[0], r.w, r.S
    valid = dense.sum(axis=1) > 0
    want, cnt = np.zeros((G, S, S), np.int64), np.zeros((G, S, S), np.int64)
    i, j = np.minimum(ci, cj), np.maximum(ci, cj)
    k = (g >= 0) & (g < G) & (i >= w) & (j <= n - 1 - w) & (j - i >= r.min_dist) & (j - i <= r.max_dist)
    for da in range(-w, w + 1):
        for db in range(-w, w + 1):
            a, b = i[k] + da, j[k] + db
            ok = valid[a] & valid[b]
            np.add.at(want[:, da + w, db + w], g[k][ok], dense[a, b][ok])
            np.add.at(cnt[:, da + w, db + w], g[k][ok], 1)
    return want, cnt


@functools.lru_cache(maxsize=None)
def planted_scores(seed):
    """(scores of the pile-up around the six plants, scores around the same centres shifted by 3 w = 9 bins) of a planted map of
    loops_cases: n = 200, w = 3, VC norm, expected = "auto", value = "oe\""""
    c = planted(seed)
    kw = dict(norm="VC", resolution_bp=c["res"], expected="auto", n_bins=c["n_bins"], w=LC.P_PW[1],
              max_distance_bp=LC.P_D * LC.P_RES)
    pi, pj = c["plants"][:, 0], c["plants"][:, 1]
    plants = pileup.pileup_host(c["pos1"], c["pos2"], c["count"], (pi, pj), **kw)
    control = pileup.pileup_host(c["pos1"], c["pos2"], c["count"], pileup.shifted_centres(pi, pj, 3 * LC.P_PW[1]), **kw)
    return plants, control
