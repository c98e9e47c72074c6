"""Distance sums and the expected vector of one chromosome's Hi-C contact records: what Juicer writes as `<chrom>_<res>.RAWexpected`
/ `KRexpected` and data/7create_graph_old.py:124, :153-154 divides a value by (commented out there, because the author had the
files only for some data), computed from the records themselves.  On the device: csrc/cgcn_hicdist.hip through
HicContacts.distance_sums / expected_vector (chromegcn_amd/hic.py); beside it the numpy restatement.  chromegcn_amd/hic.py's
docstring states the same definitions next to the scoring rule that uses them.

Definitions.  Records (pos1, pos2, count) of one chromosome in any order, res = resolution_bp, b1 = pos1 // res,
b2 = pos2 // res, d = |b1 - b2|.  n_bins defaults to the largest bin + 1; a smaller one is a ValueError, and so is a count
that is negative or not finite, or a negative position (as in hicnorm).
  1. Distance sums.  nv = the norm vector with NaN and 0 replaced by +inf (get_normalization_values), all ones without a
     vector; a bin outside the vector reads as +inf.  raw[d] = sum of count and act[d] = sum of count / (nv[b1] nv[b2]) over
     the records at distance d, diagonal records at d = 0; both float64 [n_bins].  Host statement: np.bincount(d, weights=...,
     minlength=n_bins), that is, record order; the device adds the same terms in another fixed order, so raw is bit-equal
     for integer counts below 2^53 and act[d] is within 2 (k_d - 1) 2^-53 relative, k_d the records at that distance.
     distance_sums_device_order_host restates the device's order in numpy, bit for bit.
  2. Expected vector.  poss[d] = n_bins - d.  For each d, w_d is the smallest w >= 0 whose window [max(d - w, 0),
     min(d + w, n_bins - 1)] has sum raw >= min_count; if no window reaches min_count the whole range is used.  min_count
     defaults to 400, Juicer's shot-noise mark.  The window is chosen from the RAW sums for every kind of norm: shot noise is a
     property of read counts, and for integer counts the choice is then exact in any summation order.
     expected[d] = sum_window act / sum_window poss.  expected_from_sums is the ONE float64 function that turns the sums into
     the vector (prefix sums, a vectorised binary search for w_d); the device path reads back raw and act (2 n_bins doubles),
     calls it and uploads the vector.
     Two differences from Juicer: no scale factor is applied (as for the norm vectors: the top-K selection does not see one),
     and the window rule is ours -- in the spirit of Juicer's ExpectedValueCalculation, but not its running-window loop."""
from __future__ import annotations

import numpy as np

from . import hicnorm

MIN_COUNT = 400


def clean_vector(v) -> np.ndarray:
    """a copy of an expected vector with NaN, 0 and negative entries mapped to +inf (what the scoring rule divides by)"""
    ex = np.array(v, dtype=np.float64).ravel()
    ex[~(ex > 0.0)] = np.inf
    return ex


def distance_sums_host(pos1, pos2, count, norm, resolution_bp, n_bins=None, norm_args=None):
    """(raw, act) of rule 1, float64 [n_bins] each, by np.bincount in record order"""
    res = int(resolution_bp)
    if res < 1:
        raise ValueError("resolution_bp must be positive")
    p1, p2 = np.asarray(pos1, dtype=np.int64).ravel(), np.asarray(pos2, dtype=np.int64).ravel()
    c = np.asarray(count, dtype=np.float64).ravel()
    if not (p1.shape == p2.shape == c.shape):
        raise ValueError("pos1, pos2 and count must be vectors of one length")
    hicnorm._bad_records((0 if np.all(np.isfinite(c) & (c >= 0)) else 1) | (2 if p1.size and min(p1.min(), p2.min()) < 0 else 0))
    i, j = p1 // res, p2 // res
    top = int(max(i.max(), j.max())) + 1 if i.size else 0
    n = top if n_bins is None else int(n_bins)
    if n < top:
        raise ValueError("n_bins=%d but the records reach bin %d" % (n, top - 1))
    d = np.abs(i - j)
    raw = np.bincount(d, weights=c, minlength=n).astype(np.float64)
    norm = hicnorm.resolve_norm_host(pos1, pos2, count, norm, res, n_bins, norm_args)
    if norm is None:
        return raw, raw.copy()
    nv = hicnorm.clean_norm(norm, n)   # n == 0: no records, nothing is read
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        w = c / (nv[i] * nv[j])
    return raw, np.bincount(d, weights=w, minlength=n).astype(np.float64)


def _device_order_sum(d_sorted, v_sorted, n):
    """out[d] = the sum of v over the records at distance d in the order of csrc/cgcn_hicdist.hip, from the values sorted by
    (distance, record): tiles of 64 sorted values, a segmented scan over a tile's lanes in six doubling steps, then per distance
    lane l adds the partials of its tiles l, l + 64, ... in tile order and one butterfly (32, 16, ..., 1) joins the lanes"""
    M = d_sorted.size
    out = np.zeros(n)
    if M == 0 or n == 0:
        return out
    T = (M + 63) // 64
    d = np.full(T * 64, -1, np.int64)
    v = np.zeros(T * 64)
    d[:M], v[:M] = d_sorted, v_sorted
    d, v = d.reshape(T, 64), v.reshape(T, 64)
    o = 1
    while o < 64:   # every lane reads the values of the step before
        nxt = v.copy()
        nxt[:, o:] = np.where(d[:, o:] == d[:, :-o], v[:, :-o] + v[:, o:], v[:, o:])
        v, o = nxt, o * 2
    v = v.reshape(-1)
    s = np.searchsorted(d_sorted, np.arange(n), side="left")
    e = np.searchsorted(d_sorted, np.arange(n), side="right")
    has = e > s
    t0, t1 = s // 64, (np.maximum(e, 1) - 1) // 64
    lane = np.arange(64, dtype=np.int64)[None, :]
    acc = np.zeros((n, 64))
    for k in range(int(np.max(np.where(has, t1 - t0, 0))) // 64 + 1):
        t = t0[:, None] + lane + 64 * k
        ok = has[:, None] & (t <= t1[:, None])
        at = np.minimum(e[:, None], 64 * (t + 1)) - 1          # the last lane of the run inside tile t
        acc += np.where(ok, v[np.clip(at, 0, v.size - 1)], 0.0)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, np.arange(64) ^ o]
    out[has] = acc[has, 0]
    return out


def distance_sums_device_order_host(pos1, pos2, count, norm, resolution_bp, n_bins=None, norm_args=None):
    """(raw, act) of rule 1 with the terms added in the DEVICE's fixed order (csrc/cgcn_hicdist.hip) instead of record order:
    bit for bit what HicContacts.distance_sums returns for the same records and vector.  For host restatements that must
    reproduce a device result that depends on the expected vector to the last bit (chromegcn_amd/loops.py)."""
    res = int(resolution_bp)
    raw, _ = distance_sums_host(pos1, pos2, count, norm, res, n_bins, norm_args)    # the checks; raw sizes the vectors
    n = raw.size
    p1, p2 = np.asarray(pos1, dtype=np.int64).ravel(), np.asarray(pos2, dtype=np.int64).ravel()
    c = np.asarray(count, dtype=np.float64).ravel()
    i, j = p1 // res, p2 // res
    d = np.abs(i - j)
    order = np.argsort(d, kind="stable")                                            # the key is (distance, record)
    norm = hicnorm.resolve_norm_host(pos1, pos2, count, norm, res, n_bins, norm_args)
    w = c
    if norm is not None:
        nv = hicnorm.clean_norm(norm, n)
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            w = c / (nv[i] * nv[j])
    return _device_order_sum(d[order], c[order], n), _device_order_sum(d[order], w[order], n)


def expected_from_sums(raw, act, min_count=MIN_COUNT, return_info=False):
    """Rule 2: the expected vector float64 [n_bins] from the distance sums.  return_info: (vector, {w: int64 [n_bins], w_max,
    whole_range: the number of distances whose window is the whole range})."""
    raw, act = np.asarray(raw, dtype=np.float64).ravel(), np.asarray(act, dtype=np.float64).ravel()
    if raw.shape != act.shape:
        raise ValueError("raw and act must be vectors of one length")
    n = raw.size
    if n == 0:
        out = np.zeros(0, np.float64)
        return (out, {"w": np.zeros(0, np.int64), "w_max": 0, "whole_range": 0}) if return_info else out
    c_raw = np.concatenate([np.zeros(1), np.cumsum(raw)])
    c_act = np.concatenate([np.zeros(1), np.cumsum(act)])
    c_pos = np.concatenate([np.zeros(1), np.cumsum((n - np.arange(n)).astype(np.float64))])
    d = np.arange(n, dtype=np.int64)

    def window(w):
        return np.maximum(d - w, 0), np.minimum(d + w, n - 1)

    def enough(w):   # monotone in w: raw >= 0, and the whole range is the last resort
        lo, hi = window(w)
        return (c_raw[hi + 1] - c_raw[lo] >= min_count) | ((lo == 0) & (hi == n - 1))

    lo_w, hi_w = np.zeros(n, np.int64), np.full(n, n - 1, np.int64)   # enough(n - 1) holds: the whole range
    while np.any(lo_w < hi_w):
        mid = (lo_w + hi_w) // 2
        ok = enough(mid)
        hi_w = np.where(ok, mid, hi_w)
        lo_w = np.where(ok, lo_w, mid + 1)
    lo, hi = window(lo_w)
    with np.errstate(over="ignore", invalid="ignore"):
        out = (c_act[hi + 1] - c_act[lo]) / (c_pos[hi + 1] - c_pos[lo])
    if not return_info:
        return out
    return out, {"w": lo_w, "w_max": int(lo_w.max()), "whole_range": int(np.sum((lo == 0) & (hi == n - 1)))}


def expected_vector_host(pos1, pos2, count, norm, resolution_bp, n_bins=None, min_count=MIN_COUNT, return_info=False,
                         norm_args=None):
    """The expected vector of the records on the host: expected_from_sums(*distance_sums_host(...)).  norm: None (RAW), a
    vector, or 'KR' / 'VC' / 'SQRTVC' (hicnorm.hic_norm_vector_host with norm_args)."""
    raw, act = distance_sums_host(pos1, pos2, count, norm, resolution_bp, n_bins, norm_args)
    out = expected_from_sums(raw, act, min_count, return_info=return_info)
    if return_info:
        out[1]["host_syncs"] = 0
    return out


def hic_expected_vector(pos1, pos2, count, norm, resolution_bp, n_bins=None, min_count=MIN_COUNT, device="cuda", return_info=False,
                        norm_args=None):
    """HicContacts.expected_vector for arrays (or a HicContacts as pos1: nothing is uploaded again)"""
    from .hic import HicContacts
    c = pos1 if isinstance(pos1, HicContacts) else HicContacts(pos1, pos2, count, device)
    return c.expected_vector(norm, resolution_bp, n_bins=n_bins, min_count=min_count, return_info=return_info, norm_args=norm_args)
