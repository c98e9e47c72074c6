"""Thresholded multi-label metrics on the GPU: what the reference computes
behind -br_threshold (config_args.py:28, utils/evals.py:94-100) with utils/metrics.py:29-109 -- subset accuracy (ACC),
1 - Hamming loss (HA), example-based F1 (ebF1), micro F1 (miF1), macro F1 (maF1) -- for a whole grid of thresholds, or one
threshold per label, in one stream over the [n, C] probabilities (cgcn_threshold_counts, csrc/cgcn_threshold.hip).

    Y[i, c] = targets[i, c] > 0.5          P[t, i, c] = probs[i, c] >= thresholds[t, c]   (float32; NaN is never predicted)

The device returns INTEGER counts (`ThresholdCounts`); one host function, `metrics_from_counts`, turns counts into the
metrics in float64, for the device path and for the numpy restatement alike (`threshold_counts_host`,
`threshold_metrics_host`: plain boolean arrays and np.bincount -- the specification the device counts are tested against,
exactly)."""
from __future__ import annotations

from typing import Dict, NamedTuple

import numpy as np
import torch

from . import _lib

MAX_T = 64          # thresholds per cgcn_threshold_counts call; more are served by several calls
METRIC_KEYS = ("ACC", "HA", "ebF1", "miF1", "maF1")


class ThresholdCounts(NamedTuple):
    """int64 counts of T thresholds (device tensors from threshold_counts, numpy arrays from threshold_counts_host):
      pos    [C]            rows with Y
      tp     [T, C]         rows with P and Y
      pp     [T, C]         rows with P (fp = pp - tp, fn = pos - tp)
      exact  [T]            rows whose C decisions all equal their C targets
      rows   [T, 2C + 1]    rows with |P_i| + |Y_i| = k
      tpsum  [T, 2C + 1]    sum of |P_i and Y_i| over those rows
    n, C: the shape; thresholds: the float32 [T, C] matrix that was applied."""
    pos: object
    tp: object
    pp: object
    exact: object
    rows: object
    tpsum: object
    n: int
    C: int
    thresholds: object


def threshold_matrix(thresholds, C: int) -> np.ndarray:
    """[T, C] float32 from a Python float (one threshold for every label), a 1-D [T] array or tensor (a grid shared by all
    labels) or a 2-D [T, C] one (per label).  Values are rounded to float32; a NaN raises ValueError."""
    if isinstance(thresholds, torch.Tensor):
        thresholds = thresholds.detach().cpu().numpy()
    with np.errstate(over="ignore"):
        a = np.asarray(thresholds, dtype=np.float64).astype(np.float32)
    if a.ndim == 0:
        a = a.reshape(1, 1)
    elif a.ndim == 1:
        a = a[:, None]
    elif a.ndim != 2 or a.shape[1] != C:
        raise ValueError("thresholds must be a float, [T] or [T, C=%d]; found shape %s" % (C, a.shape))
    if a.shape[0] == 0:
        raise ValueError("thresholds: no threshold given")
    if np.isnan(a).any():
        raise ValueError("thresholds: a threshold is NaN")
    return np.array(np.broadcast_to(a, (a.shape[0], C)), dtype=np.float32, order="C")     # a fresh, writable copy


def threshold_counts(probs: torch.Tensor, targets: torch.Tensor, thresholds) -> ThresholdCounts:
    """The counts of every threshold on the device.  probs, targets: [n, C] CUDA tensors, 1 <= C <= 1024; thresholds: see
    threshold_matrix.  Nothing is copied to the host."""
    if not isinstance(probs, torch.Tensor) or not isinstance(targets, torch.Tensor) or not probs.is_cuda or not targets.is_cuda:
        raise RuntimeError("chromegcn_amd.thresholds: tensors must be on the GPU (there is no CPU fallback; the numpy "
                           "restatement is threshold_counts_host)")
    probs = probs.contiguous().float()
    targets = targets.contiguous().float()
    if probs.dim() != 2 or tuple(targets.shape) != tuple(probs.shape):
        raise RuntimeError("probs and targets must both be [n, C]")
    n, C = probs.shape
    thr = torch.from_numpy(threshold_matrix(thresholds, C)).to(probs.device)
    T = thr.shape[0]
    K = 2 * C + 1
    dev = probs.device
    pos = torch.empty(C, device=dev, dtype=torch.int64)
    tp = torch.empty(T, C, device=dev, dtype=torch.int64)
    pp = torch.empty(T, C, device=dev, dtype=torch.int64)
    exact = torch.empty(T, device=dev, dtype=torch.int64)
    rows = torch.empty(T, K, device=dev, dtype=torch.int64)
    tpsum = torch.empty(T, K, device=dev, dtype=torch.int64)
    for t0 in range(0, T, MAX_T):
        t1 = min(T, t0 + MAX_T)
        ws, ws_bytes = _lib.workspace_for("cgcn_threshold_workspace_bytes", dev,
                                          "thresholded counts, n=%d C=%d T=%d" % (n, C, t1 - t0), n=n, C=C, T=t1 - t0)
        _lib.call("cgcn_threshold_counts", n=n, C=C, T=t1 - t0, probs=probs, targets=targets, thresholds=thr[t0:t1],
                  pos=pos, tp=tp[t0:t1], pp=pp[t0:t1], exact=exact[t0:t1], rows=rows[t0:t1], tpsum=tpsum[t0:t1],
                  workspace=ws, workspace_bytes=ws_bytes)
    return ThresholdCounts(pos, tp, pp, exact, rows, tpsum, int(n), int(C), thr)


def _host(counts: ThresholdCounts) -> ThresholdCounts:
    """the same counts as numpy arrays: the six count arrays come down in ONE device-to-host copy (the small threshold
    matrix in a second) when they live on the device"""
    fields = (counts.pos, counts.tp, counts.pp, counts.exact, counts.rows, counts.tpsum)
    if isinstance(counts.pos, torch.Tensor):
        flat = torch.cat([f.reshape(-1) for f in fields]).cpu().numpy()
        out, at = [], 0
        for f in fields:
            out.append(flat[at:at + f.numel()].reshape(tuple(f.shape)))
            at += f.numel()
        thr = counts.thresholds.cpu().numpy()
    else:
        out = [np.asarray(f, dtype=np.int64) for f in fields]
        thr = np.asarray(counts.thresholds, dtype=np.float32)
    return ThresholdCounts(*out, counts.n, counts.C, thr)


def _ratio(a, b):
    """a / b in float64, NaN where b == 0"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    out = np.full(np.broadcast(a, b).shape, np.nan)
    np.divide(a, b, out=out, where=b != 0)
    return out


def metrics_from_counts(counts: ThresholdCounts) -> Dict[str, np.ndarray]:
    """float64 metrics of every threshold, from integer counts; NaN wherever a denominator is zero (f1_score_from_stats'
    safe_div and example_f1_score's deletion of empty rows, utils/metrics.py:54-93):
      ACC   [T]  exact / n                                 HA    [T]  1 - sum_c (fp + fn) / (n C)
      miF1  [T]  2 sum tp / (2 sum tp + sum fp + sum fn)   maF1  [T]  mean of f1 over the labels where it is defined
      ebF1  [T]  (sum_{k >= 1} 2 tpsum[k] / k) / sum_{k >= 1} rows[k], k ascending
      precision, recall, f1  [T, C]  tp / pp, tp / pos, 2 tp / (2 tp + fp + fn)"""
    c = _host(counts)
    n, C = c.n, c.C
    pos, tp, pp = c.pos.astype(np.float64), c.tp.astype(np.float64), c.pp.astype(np.float64)
    fp, fn = pp - tp, pos[None, :] - tp
    f1 = _ratio(2 * tp, 2 * tp + fp + fn)
    defined = ~np.isnan(f1)
    k = np.arange(1, 2 * C + 1, dtype=np.float64)
    eb_num = np.cumsum(2.0 * c.tpsum[:, 1:].astype(np.float64) / k, axis=1)[:, -1]      # cumsum: k ascending
    return {
        "ACC": _ratio(c.exact, n),
        "HA": 1.0 - _ratio((fp + fn).sum(axis=1), float(n) * C),
        "ebF1": _ratio(eb_num, c.rows[:, 1:].sum(axis=1)),
        "miF1": _ratio(2 * tp.sum(axis=1), 2 * tp.sum(axis=1) + fp.sum(axis=1) + fn.sum(axis=1)),
        "maF1": _ratio(np.where(defined, f1, 0.0).sum(axis=1), defined.sum(axis=1)),
        "precision": _ratio(tp, pp), "recall": _ratio(tp, np.broadcast_to(pos, tp.shape)), "f1": f1,
    }


def threshold_metrics(probs: torch.Tensor, targets: torch.Tensor, thresholds=0.5) -> Dict[str, np.ndarray]:
    """metrics_from_counts(threshold_counts(...)): one stream over the device tensors, one device-to-host copy"""
    return metrics_from_counts(threshold_counts(probs, targets, thresholds))


def best_thresholds(counts: ThresholdCounts, criterion: str = "f1") -> np.ndarray:
    """[C] float32: per label the threshold of the grid row with the largest per-label F1 (the first such row), NaN where F1
    is undefined on every row.  Host arithmetic on the counts: tune on the validation split with a shared grid, then apply
    on the test split as a [1, C] matrix (`threshold_metrics(p, t, best[None])`)."""
    if criterion != "f1":
        raise ValueError("best_thresholds: the only criterion is 'f1'")
    c = _host(counts)
    f1 = metrics_from_counts(c)["f1"]
    defined = ~np.isnan(f1)
    row = np.argmax(np.where(defined, f1, -np.inf), axis=0)     # argmax: the first of equal maxima
    best = c.thresholds[row, np.arange(c.C)].astype(np.float32)
    best[~defined.any(axis=0)] = np.nan
    return best


# ---- numpy restatements: the specification --------------------------------------------------------------------------------
def threshold_counts_host(probs, targets, thresholds) -> ThresholdCounts:
    """ThresholdCounts of numpy int64 arrays from plain boolean arrays and np.bincount"""
    probs = np.ascontiguousarray(np.asarray(probs, dtype=np.float32))
    targets = np.asarray(targets, dtype=np.float32)
    if probs.ndim != 2 or targets.shape != probs.shape:
        raise ValueError("probs and targets must both be [n, C]")
    n, C = probs.shape
    thr = threshold_matrix(thresholds, C)
    T, K = thr.shape[0], 2 * C + 1
    Y = targets > np.float32(0.5)
    ny = Y.sum(axis=1)
    tp, pp = np.zeros((T, C), dtype=np.int64), np.zeros((T, C), dtype=np.int64)
    exact = np.zeros(T, dtype=np.int64)
    rows, tpsum = np.zeros((T, K), dtype=np.int64), np.zeros((T, K), dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for t in range(T):
            P = probs >= thr[t][None, :]
            both = P & Y
            tp[t], pp[t] = both.sum(axis=0), P.sum(axis=0)
            exact[t] = int((P == Y).all(axis=1).sum())
            k = P.sum(axis=1) + ny
            rows[t] = np.bincount(k, minlength=K)
            tpsum[t] = np.rint(np.bincount(k, weights=both.sum(axis=1), minlength=K)).astype(np.int64)
    return ThresholdCounts(Y.sum(axis=0).astype(np.int64), tp, pp, exact, rows, tpsum, int(n), int(C), thr)


def threshold_metrics_host(probs, targets, thresholds=0.5) -> Dict[str, np.ndarray]:
    return metrics_from_counts(threshold_counts_host(probs, targets, thresholds))
