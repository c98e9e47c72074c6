"""Inputs shared by tests/test_bootstrap_host.py and tests/test_gpu_bootstrap.py: the known answers of the rules in
chromegcn_amd/bootstrap.py, and the (scores, targets, weights) cases the device is held to the restatement on.  A case's
restatement is computed once (functools.lru_cache) and never modified."""
import functools

import numpy as np

from chromegcn_amd import bootstrap as B

# ---- known answers of the weighted-metric rule (q = 0.5) ----
KNOWN_SCORES = [.9, .9, .7, .7, .7, .2, .1]
KNOWN_TARGETS = [1, 0, 1, 1, 0, 0, 1]
KNOWN_SUMS = [   # weights, (A, P, TOT, F), S_ap, S_pr
    ([1] * 7, (11, 4, 7, 4), 1 / 2 + 6 / 5 + 4 / 7, 3 / 2 + 11 / 5 + 15 / 14),
    ([0, 0, 2, 0, 1, 3, 1], (14, 3, 7, 2), 4 / 3 + 3 / 7, 10 / 3 + 16 / 21),
    ([2, 0, 0, 0, 0, 0, 0], (0, 2, 2, 2), 2.0, 4.0),
    ([0] * 7, (0, 0, 0, 0), 0.0, 0.0),
]
# ---- known answers of the weight rule ----
HIGH_SEED = (0xDEADBEEF << 32) | 12345
KNOWN_WEIGHTS = [   # (n, replicates, seed, block, lengths) -> rows
    ((7, 2, 7, 1, None), [[0, 0, 2, 1, 1, 0, 3], [1, 1, 1, 0, 1, 2, 1]]),
    ((7, 2, 7, 3, [3, 4]), [[1, 1, 1, 1, 2, 1, 2], [1, 1, 1, 2, 2, 1, 1]]),
    ((10, [3, 2 ** 32 + 3], HIGH_SEED, 4, None), [[2, 2, 0, 0, 1, 1, 1, 1, 2, 2], [1, 1, 1, 1, 2, 1, 1, 2, 1, 1]]),
]

# ---- device cases ----
# name: (n, C, R, score kind, weight kind).  Score kinds: 'normal' (distinct floats, some negative, a -0 and a +0),
# 'two' (rounded to two decimals: heavy ties), 'one' (label 0 distinct, label 1 ONE score).  Weight kinds: a dict of the
# rule's arguments, or 'explicit' (zeros on the top-scored windows, 255s, an all-zero replicate).
# Lengths the kernels use: 16 row loads per batch and 64 list elements per load of the walk, 64 rows per wave and 256 per
# workgroup of the sliding sum (more with a block above 64), 256 draws per workgroup of the start histogram, 32 x 32 tiles of
# the key pack, 64 x 64 of the explicit weights, 256 keys per workgroup.
_AT = lambda k: [(k - 1, 2, 2), (k, 2, 2), (k + 1, 2, 2)]
CASES = {
    "n1": (1, 1, 1, "normal", dict(seed=1, block=1)),
    "n2": (2, 2, 3, "normal", dict(seed=2, block=2)),
    "n63": (63, 3, 63, "normal", dict(seed=3, block=7)),
    "n64": (64, 3, 64, "normal", dict(seed=4, block=1)),
    "n65": (65, 3, 65, "normal", dict(seed=5, block=100)),   # a block longer than the stratum
    "n65_explicit": (65, 3, 65, "two", "explicit"),
    "n300": (300, 5, 130, "two", dict(seed=(5 << 32) | 11, block=7, lengths=[100, 0, 200])),   # 7 divides neither stratum
    "n300_explicit": (300, 5, 130, "two", "explicit"),
    "n4097": (4097, 2, 70, "one", dict(seed=HIGH_SEED, block=25, lengths=[10, 4000, 87], rep0=2 ** 32 + 3)),
    "n5000": (5000, 103, 64, "normal", dict(seed=6, block=50, lengths=[1500, 3500])),
}
for _k in (16, 32, 256):   # block 1 at 255 / 256 / 257: n draws, around the 256 threads of a workgroup of the start histogram
    for _n, _c, _r in _AT(_k):
        CASES["n%d" % _n] = (_n, _c, _r, "two", dict(seed=_n, block=1 if _k == 256 else 3))
# blocks above the 64 rows a wave of the sliding sum takes at least: its segment grows with the block
CASES["n1000_b65"] = (1000, 2, 3, "two", dict(seed=65, block=65, lengths=[500, 0, 64, 436]))
CASES["n1000_b300"] = (1000, 2, 3, "two", dict(seed=300, block=300, lengths=[700, 300]))   # the second stratum is one block
for _b in (4095, 4096, 4097):   # ... up to 4096 rows; a longer block forms its sums over more rows than the wave slides over
    CASES["n9000_b%d" % _b] = (9000, 1, 2, "two", dict(seed=_b, block=_b))
NAMES = sorted(CASES)


def scores_targets(name):
    """(probs float32 [n, C], targets float32 [n, C]); with C >= 3 label 0 has no positive, label 1 only positives and
    label 2 a single one"""
    n, C, R, kind, _ = CASES[name]
    rng = np.random.default_rng(abs(hash_name(name)))
    t = (rng.random((n, C)) < 0.3).astype(np.float32)
    s = rng.normal(size=(n, C)).astype(np.float32) + t * np.float32(0.7)
    if kind == "two":
        s = np.round(1.0 / (1.0 + np.exp(-s)), 2).astype(np.float32)
    elif kind == "one":
        s[:, 1] = np.float32(0.25)
    else:
        if n >= 2:
            s[0, 0], s[1, 0] = np.float32(-0.0), np.float32(0.0)
    if C >= 3:
        t[:, 0] = 0
        t[:, 1] = 1
        t[:, 2] = 0
        t[n // 2, 2] = 1
    return s, t


def hash_name(name):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name))


def rule_args(name):
    """(replicates, seed, block, lengths) of a case whose weights come from the rule, else None"""
    n, C, R, _, w = CASES[name]
    if w == "explicit":
        return None
    reps = R if "rep0" not in w else [w["rep0"] + r for r in range(R)]
    return reps, w["seed"], w["block"], w.get("lengths")


@functools.lru_cache(maxsize=None)
def weights(name):
    """int64 [R, n], read-only"""
    n, C, R, _, w = CASES[name]
    if w == "explicit":
        s, _ = scores_targets(name)
        rng = np.random.default_rng(hash_name(name) + 1)
        W = rng.integers(0, 4, size=(R, n)).astype(np.int64)
        top = np.argsort(-s[:, 0].astype(np.float64), kind="stable")[:max(1, n // 5)]
        W[0, top] = 0                       # the skipped leading runs (of label 0)
        W[1] = 0                            # an all-zero replicate
        W[2, rng.integers(0, n, 5)] = 255
        W[3] = 255
    else:
        reps, seed, block, lengths = rule_args(name)
        W = B.bootstrap_weights_host(n, reps, seed, block, lengths)
    W.setflags(write=False)
    return W


@functools.lru_cache(maxsize=None)
def host_sums(name, q=0.5):
    s, t = scores_targets(name)
    out = B.weighted_sums_host(s, t, weights(name), q)
    for v in out.values():
        v.setflags(write=False)
    return out


def sum_rtol(n):
    """S_ap and S_pr: at most n non-negative terms, each with at most three roundings of 2^-53, summed in any order on either
    side, fused multiply-add or not"""
    return (n + 4) * 2.0 ** -52
