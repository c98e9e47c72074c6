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


def scaled(make, factor):
    """the case with every count multiplied by `factor`: at 1e-6 the first Newton steps overshoot and KR clips them from above"""
    c = make()
    return dict(c, count=c["count"] * factor)


def wide(make, span, seed):
    """the case with every count multiplied by 10^u, u uniform in (-span, span): rows whose sums are orders of magnitude
    apart, on which the first Newton steps undershoot and KR clips them from below"""
    c = make()
    return dict(c, count=c["count"] * 10.0 ** np.random.default_rng(seed).uniform(-span, span, c["count"].size))


# balanced only (their counts are no integers, their sizes too large for the dense double loop): KR's upper clip, and more
# than 65 536 and than 262 144 bins -- 257 and 1026 partials of a vector step, a second trip of its fold and of its grid
TINY_CASES = {
    "n257_tiny": lambda: scaled(CASES["n257"], 1e-6),
    "n1000_tiny": lambda: scaled(CASES["n1000"], 1e-6),
    "n65_wide": lambda: wide(CASES["n65"], 3, 2),      # the lower clip once, the upper never
    "n257_wide": lambda: wide(CASES["n257"], 5, 2),    # each clip twice
}
LARGE_CASES = {
    "n70001": lambda: hic_like(70001, 420000, 77, dup_share=0.05, n_empty=37),
    "n262401": lambda: hic_like(262401, 1500000, 77, dup_share=0.05, n_empty=113),
    "n70001_tiny": lambda: scaled(LARGE_CASES["n70001"], 1e-6),
}
KR_CASES = tuple(CASES) + tuple(TINY_CASES)   # every generator case is balanced
KR_LARGE = tuple(LARGE_CASES)
UPPER_CLIP = ("n257_tiny", "n1000_tiny", "n70001_tiny", "n257_wide")   # the cases whose runs clip a step from above,
LOWER_CLIP = ("n65_wide", "n257_wide")                                 # ... from below


@functools.lru_cache(maxsize=None)
def case(name):
    return {**CASES, **TINY_CASES, **LARGE_CASES}[name]()


@functools.lru_cache(maxsize=None)
def host_matrix(name):
    c = case(name)
    return hicnorm.contact_matrix_host(c["pos1"], c["pos2"], c["count"], c["res"], c["n_bins"])


@functools.lru_cache(maxsize=None)
def host_kr(name, tol, min_row_nnz=1):
    """(x, info) of the host restatement"""
    return hicnorm.kr_balance_host(host_matrix(name), tol=tol, max_mvp=1000, min_row_nnz=min_row_nnz, kr_retry=False)


def kr_clip_count(A, tol, max_mvp=1000):
    """The listing of chromegcn_amd/hicnorm.py's docstring written out once more on the rows of A that are not empty, to
    count what its run does not report: ((lower clips, upper clips), margin, products).  margin = the smallest relative
    distance, over every inner iteration, of min(ynew) from delta and of max(ynew) from Delta: roundings of 1e-15 cannot
    change a branch of a run whose margin is far above them."""
    keep = np.flatnonzero(np.asarray(A.sum(axis=1)).ravel() > 0)
    A = A[keep][:, keep].tocsr()
    n, mvp, clips, margin = A.shape[0], 1, [0, 0], np.inf
    x = np.ones(n)
    v = x * (A @ x)
    rk = 1.0 - v
    rho1 = rout = rold = float(rk @ rk)
    eta, rho2, Z, p = 0.1, 0.0, None, None
    while rout > tol * tol and mvp < max_mvp:
        k, y = 0, np.ones(n)
        innertol = max(eta * eta * rout, tol * tol)
        while rho1 > innertol and mvp < max_mvp:
            k += 1
            if k == 1:
                Z = rk / v
                p = Z.copy()
                rho1 = float(rk @ Z)
            else:
                p = Z + (rho1 / rho2) * p
            w = x * (A @ (x * p)) + v * p
            mvp += 1
            alpha = rho1 / float(p @ w)
            ap = alpha * p
            ynew = y + ap
            margin = min(margin, abs(ynew.min() - 0.1) / 0.1, abs(ynew.max() - 3.0) / 3.0)
            if ynew.min() <= 0.1:
                y = y + ((0.1 - y[ap < 0]) / ap[ap < 0]).min() * ap
                clips[0] += 1
                break
            if ynew.max() >= 3.0:
                y = y + ((3.0 - y[ynew > 3.0]) / ap[ynew > 3.0]).min() * ap
                clips[1] += 1
                break
            y, rk, rho2 = ynew, rk - alpha * w, rho1
            Z = rk / v
            rho1 = float(rk @ Z)
        x = x * y
        v = x * (A @ x)
        mvp += 1
        rk = 1.0 - v
        rho1 = rout = float(rk @ rk)
        eta_o, eta = eta, 0.9 * rout / rold
        rold = rout
        if 0.9 * eta_o * eta_o > 0.1:
            eta = max(eta, 0.9 * eta_o * eta_o)
        eta = max(min(eta, 0.1), 0.5 * tol / np.sqrt(rout) if rout > 0 else 0.1)
    return tuple(clips), float(margin), mvp


# ----------------------------------------------------------------------------------------------
# one operation of cgcn_hicnorm_kr_step on the host: the state as a dict of float64 vectors and the 32-double record
# (hicnorm.py: 0 rho1, 1 rho2, 2 p.w, 3 min ynew, 4 max ynew, 5 gamma of the lower bound, 6 gamma of the upper bound,
# 7 rho1 of the accepted step, 8 rout, 9 alpha, 10 kept rows, 11 non-empty rows)
# ----------------------------------------------------------------------------------------------
KR_VECTORS = ("m", "x", "v", "p", "w", "y0", "y1", "rk0", "rk1", "z0", "z1")     # the order of the state's vectors
OP_MASK, OP_RES, OP_FIRST, OP_DIR, OP_W, OP_Y, OP_CLIP = range(7)
KR_STEPS = ((OP_MASK, 2), (OP_RES, 0), (OP_RES, 1), (OP_FIRST, 0), (OP_DIR, 0), (OP_W, 0), (OP_W, 1), (OP_Y, 0), (OP_CLIP, 0),
            (OP_CLIP, 1))


def kr_step_host(op, flag, c, vec, rec, vc=None, row_nnz=None):
    """(vectors written: {name: (value, magnitude of its terms)}, record slots written: {slot: (value, sum of the magnitudes
    of its terms or None for a value that is exact, a minimum or a maximum)}) of one step from the state (vec, rec) at
    parity c, in float64 numpy after _kr_run_host's listing.  Nothing is changed in place."""
    y, y2, rk, rk2, z, z2 = "y%d" % c, "y%d" % (c ^ 1), "rk%d" % c, "rk%d" % (c ^ 1), "z%d" % c, "z%d" % (c ^ 1)
    keep = vec["m"] != 0.0
    one = np.ones_like(vec["m"])
    with np.errstate(all="ignore"):
        if op == OP_MASK:
            full = vc > 0.0
            kept = full & (row_nnz >= flag)
            return ({"m": (kept.astype(np.float64), 0 * one), "x": (one, 0 * one), y: (one, 0 * one)},
                    {10: (float(kept.sum()), None), 11: (float(full.sum()), None)})
        if op == OP_RES:
            x = vec["x"] * vec[y] if flag else vec["x"]
            v = x * vec["w"]
            r = np.where(keep, 1.0 - v, 0.0)
            s = float(np.sum(r * r))
            out = {"v": (v, np.abs(v)), rk: (r, 1.0 + np.abs(v)), y: (one, 0 * one)}
            if flag:
                out["x"] = (x, np.abs(x))
            return out, {0: (s, s), 8: (s, s)}
        if op == OP_FIRST:
            zz = np.where(keep, vec[rk] / vec["v"], 0.0)
            return {z: (zz, 0 * one), "p": (zz, 0 * one)}, {0: (float(np.sum(vec[rk] * zz)), float(np.sum(np.abs(vec[rk] * zz))))}
        if op == OP_DIR:
            beta = rec[7] / rec[0]
            return {"p": (vec[z] + beta * vec["p"], np.abs(vec[z]) + np.abs(beta * vec["p"]))}, {}
        if op == OP_W:
            w = vec["x"] * vec["w"] + vec["v"] * vec["p"]
            s = float(np.sum(vec["p"] * w))
            rho1 = rec[7] if flag else rec[0]
            slots = {2: (s, float(np.sum(np.abs(vec["p"] * w)))), 9: (rho1 / s, None)}
            if flag:
                slots.update({1: (rec[0], None), 0: (rec[7], None)})
            return {"w": (w, np.abs(vec["x"] * vec["w"]) + np.abs(vec["v"] * vec["p"]))}, slots
        if op == OP_Y:
            alpha = rec[9]
            ap = alpha * vec["p"]
            yn = vec[y] + ap
            r = vec[rk] - alpha * vec["w"]
            zz = np.where(keep, r / vec["v"], 0.0)
            lo, up = keep & (ap < 0.0), keep & (yn > 3.0)
            slots = {3: (np.min(yn[keep], initial=np.inf), None), 4: (np.max(yn[keep], initial=-np.inf), None),
                     5: (np.min((0.1 - vec[y][lo]) / ap[lo], initial=np.inf), None),
                     6: (np.min((3.0 - vec[y][up]) / ap[up], initial=np.inf), None),
                     7: (float(np.sum(r * zz)), float(np.sum(np.abs(r * zz))))}
            return {y2: (yn, np.abs(vec[y]) + np.abs(ap)), rk2: (r, np.abs(vec[rk]) + np.abs(alpha * vec["w"])),
                    z2: (zz, (np.abs(vec[rk]) + np.abs(alpha * vec["w"])) / np.abs(vec["v"]))}, slots
        gamma = rec[6] if flag else rec[5]
        step = gamma * (rec[9] * vec["p"])
        return {y: (vec[y] + step, np.abs(vec[y]) + np.abs(step))}, {}


def apply_kr_step(out, slots, vec, rec):
    """the state after a step: kr_step_host's values put in place (copies)"""
    vec, rec = dict(vec), rec.copy()
    for k, (val, _) in out.items():
        vec[k] = val
    for k, (val, _) in slots.items():
        rec[k] = val
    return vec, rec


def kr_run_by_steps(A, tol, max_mvp=1000, min_row_nnz=1):
    """_kr_run_device's loop with kr_step_host as the step and scipy as the product: (x with NaN outside the kept set, products,
    (lower clips, upper clips)).  It ties the per-step restatement to the listing without a device."""
    import math
    vc, nnz = hicnorm._row_stats_host(A)
    state = [{k: np.zeros(A.shape[0]) for k in KR_VECTORS}, np.zeros(32)]

    def step(op, flag, c):
        state[:] = apply_kr_step(*kr_step_host(op, flag, c, state[0], state[1], vc, nnz), state[0], state[1])

    def product(pv):
        vec = dict(state[0])
        vec["w"] = vec["m"] * (A @ (vec["m"] * vec["x"] * (1.0 if pv is None else vec[pv])))
        state[0] = vec

    c, mvp, clips = 0, 1, [0, 0]
    step(OP_MASK, min_row_nnz, c)
    product(None)
    step(OP_RES, 0, c)
    rho1 = rout = rold = state[1][8]
    eta, rt = 0.1, tol * tol
    while rout > rt and mvp < max_mvp:
        k = 0
        innertol = max(eta * eta * rout, rt)
        while rho1 > innertol and mvp < max_mvp:
            k += 1
            step(OP_FIRST if k == 1 else OP_DIR, 0, c)
            product("p")
            mvp += 1
            step(OP_W, k > 1, c)
            step(OP_Y, 0, c)
            if state[1][3] <= 0.1 or state[1][4] >= 3.0:
                upper = not state[1][3] <= 0.1
                step(OP_CLIP, upper, c)
                clips[upper] += 1
                break
            c ^= 1
            rho1 = state[1][7]
        product("y%d" % c)
        mvp += 1
        step(OP_RES, 1, c)
        rout = rho1 = state[1][8]
        eta_o, eta = eta, 0.9 * rout / rold
        rold = rout
        if 0.9 * eta_o * eta_o > 0.1:
            eta = max(eta, 0.9 * eta_o * eta_o)
        eta = max(min(eta, 0.1), 0.5 * tol / math.sqrt(rout) if rout > 0 else 0.1)
    return np.where(state[0]["m"] != 0.0, state[0]["x"], np.nan), mvp, tuple(clips)


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
