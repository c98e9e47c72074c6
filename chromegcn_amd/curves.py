"""ROC and precision-recall curves of every label on the GPU: the
per_label_type / plot branches of the reference's compute_metrics (utils/evals.py:28-84), which call scikit-learn's
roc_curve / precision_recall_curve once per label (utils/metrics.py:255-303), and Find_Optimal_Cutoff
(utils/metrics.py:224-235).  One pack + segmented sort over all labels (the one chromegcn_amd.metrics runs), two
ordered compactions (cgcn_curves_count / cgcn_curves_fill), integer counts throughout.

Scores are probabilities: a negative score or a NaN raises ValueError (there is no general-scores path).  The numpy
functions at the end (`roc_curve_host`, `pr_curve_host`, `optimal_cutoff_host`) are the specification the device
arrays are tested against, bit for bit."""
from __future__ import annotations

from typing import Tuple

import numpy as np
import torch

from . import _lib


class Curves:
    """The curves of C labels as flat device arrays: label c's points are [offsets[c], offsets[c + 1]), in descending
    order of threshold.
      kind          "roc" or "pr"
      offsets       int64 [C + 1]
      tps, fps      int32: positives / negatives with a score >= the threshold
      thresholds    float32 (ROC: every label starts with the origin, threshold +inf)
      fpr, tpr      (ROC) float64: fps / N, tps / P -- all NaN for a label without negatives / positives
      precision, recall  (PR) float64: tps / (tps + fps) (0 where tps + fps == 0), tps / P (all 1 without positives)
    `curves[c]` is label c's triple as numpy arrays, as scikit-learn returns it."""

    def __init__(self, kind: str, offsets: torch.Tensor, tps: torch.Tensor, fps: torch.Tensor, thresholds: torch.Tensor):
        self.kind, self.offsets, self.tps, self.fps, self.thresholds = kind, offsets, tps, fps, thresholds
        lengths = offsets[1:] - offsets[:-1]
        label = torch.repeat_interleave(lengths, output_size=tps.numel())   # the label of every point
        last = offsets[1:] - 1                  # every label has a point; its last one holds all positives / negatives
        P, t = tps[last].double()[label], tps.double()
        if kind == "roc":
            self.fpr = fps.double() / fps[last].double()[label]   # 0 / 0: NaN throughout a label without negatives
            self.tpr = t / P
        else:
            ps = (tps + fps).double()
            self.precision = torch.where(ps != 0, t / ps, 0.0)
            self.recall = torch.where(P > 0, t / P, 1.0)
        self._host = None

    def __len__(self):
        return self.offsets.numel() - 1

    def __getitem__(self, c: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """ROC: (fpr, tpr, thresholds) as sklearn.metrics.roc_curve returns them; PR: (precision, recall, thresholds) as
        precision_recall_curve does -- ascending thresholds, the terminal (1, 0) appended.  The first call copies the
        arrays to the host, once."""
        if self._host is None:
            a, b = (self.fpr, self.tpr) if self.kind == "roc" else (self.precision, self.recall)
            self._host = (self.offsets.cpu().numpy(), a.cpu().numpy(), b.cpu().numpy(), self.thresholds.cpu().numpy())
        off, a, b, thr = self._host
        if not -len(self) <= c < len(self):
            raise IndexError("label %d of %d" % (c, len(self)))
        s = slice(int(off[c % len(self)]), int(off[c % len(self) + 1]))
        if self.kind == "roc":
            return a[s].copy(), b[s].copy(), _with_inf(thr[s][1:])
        return np.hstack((a[s][::-1], 1)), np.hstack((b[s][::-1], 0)), thr[s][::-1].copy()


def _with_inf(thresholds):
    # scikit-learn's own expression: the result type is numpy's for (python float, float32 array)
    return np.r_[np.inf, thresholds]


def _curves_raw(kind: str, probs: torch.Tensor, targets: torch.Tensor, drop_intermediate: bool):
    """(offsets, tps, fps, thresholds): count, the read of offsets[C] and `bad`, fill"""
    if not probs.is_cuda or not targets.is_cuda:
        raise RuntimeError("chromegcn_amd.curves: tensors must be on the GPU (there is no CPU fallback; the numpy "
                           "restatements are roc_curve_host / pr_curve_host)")
    probs = probs.contiguous().float()
    targets = targets.contiguous().float()
    if probs.dim() != 2 or tuple(targets.shape) != tuple(probs.shape):
        raise RuntimeError("probs and targets must both be [n, C]")
    n, C = probs.shape
    ws, ws_bytes = _lib.workspace_for("cgcn_curves_workspace_bytes", probs.device, "curves, n=%d C=%d" % (n, C), n=n, C=C)
    head = torch.zeros(C + 2, device=probs.device, dtype=torch.int64)   # offsets [C + 1], then the `bad` word
    offsets = head[:C + 1]
    _lib.call("cgcn_curves_count", n=n, C=C, probs=probs, targets=targets,
              kind=_lib.CURVE_ROC if kind == "roc" else _lib.CURVE_PR, drop_intermediate=int(bool(drop_intermediate)),
              offsets=offsets, bad=head.data_ptr() + 8 * (C + 1), workspace=ws, workspace_bytes=ws_bytes)
    total, bad = head[C:].tolist()   # the single host synchronisation: the outputs are sized by it
    if bad != 0:
        raise ValueError("chromegcn_amd.curves: a score is negative or NaN (scores must be probabilities)")
    tps = torch.empty(total, device=probs.device, dtype=torch.int32)
    fps = torch.empty(total, device=probs.device, dtype=torch.int32)
    thresholds = torch.empty(total, device=probs.device, dtype=torch.float32)
    _lib.call("cgcn_curves_fill", n=n, C=C, offsets=offsets, capacity=total, tps=tps, fps=fps, thresholds=thresholds,
              workspace=ws, workspace_bytes=ws_bytes)
    return offsets, tps, fps, thresholds


def _curves(kind: str, probs: torch.Tensor, targets: torch.Tensor, drop_intermediate: bool) -> Curves:
    return Curves(kind, *_curves_raw(kind, probs, targets, drop_intermediate))


def roc_curves(probs: torch.Tensor, targets: torch.Tensor, drop_intermediate: bool = True) -> Curves:
    """sklearn.metrics.roc_curve(targets[:, c], probs[:, c], drop_intermediate=...) for every label c at once.
    probs, targets: [n, C] CUDA tensors, probs non-negative, targets 0 / 1."""
    return _curves("roc", probs, targets, drop_intermediate)


def pr_curves(probs: torch.Tensor, targets: torch.Tensor) -> Curves:
    """sklearn.metrics.precision_recall_curve(targets[:, c], probs[:, c]) for every label c at once (the flat arrays are in
    descending order of threshold and without the terminal point; `curves[c]` is in scikit-learn's order and has it)."""
    return _curves("pr", probs, targets, False)


def _cutoffs(offsets, tps, fps, thresholds) -> torch.Tensor:
    out = torch.empty(offsets.numel() - 1, device=tps.device, dtype=torch.float32)
    _lib.call("cgcn_curves_cutoff", C=out.numel(), offsets=offsets, tps=tps, fps=fps, thresholds=thresholds, cutoffs=out)
    return out


def cutoffs_of(roc: Curves) -> torch.Tensor:
    """[C] float32: per label the threshold of the first point of `roc` that minimises |tpr - (1 - fpr)| (NaN without a
    positive or without a negative)"""
    if roc.kind != "roc":
        raise ValueError("cutoffs_of needs ROC curves")
    return _cutoffs(roc.offsets, roc.tps, roc.fps, roc.thresholds)


def optimal_cutoffs(probs: torch.Tensor, targets: torch.Tensor) -> torch.Tensor:
    """Find_Optimal_Cutoff (utils/metrics.py:224-235) for every label: [C] float32, the threshold where the ROC curve
    (roc_curve's default, drop_intermediate=True) comes closest to tpr = 1 - fpr.  See optimal_cutoff_host for the rule."""
    return _cutoffs(*_curves_raw("roc", probs, targets, True))


# ---- numpy restatements: the specification --------------------------------------------------------------------------------
def _binary_clf_curve_host(y_true, y_score):
    """(fps, tps, thresholds) of sklearn's _binary_clf_curve: int64 counts at the last element of each run of equal scores
    in the stable descending order, thresholds in the dtype of y_score"""
    y_true = np.asarray(y_true).ravel() > 0.5
    y_score = np.asarray(y_score).ravel()
    if y_true.size != y_score.size or y_score.size == 0:
        raise ValueError("y_true and y_score must have the same, non-zero length")
    order = np.argsort(y_score, kind="mergesort")[::-1]
    y_score, y_true = y_score[order], y_true[order]
    idx = np.r_[np.flatnonzero(np.diff(y_score)), y_true.size - 1]
    tps = np.cumsum(y_true, dtype=np.int64)[idx]
    return 1 + idx - tps, tps, y_score[idx]


def roc_points_host(y_true, y_score, drop_intermediate=True):
    """(fps, tps, thresholds) of one label as cgcn_curves_fill writes them for the ROC kind: int64 counts, the origin
    (0, 0, +inf) first"""
    fps, tps, thr = _binary_clf_curve_host(y_true, y_score)
    if drop_intermediate and fps.size > 2:
        keep = np.r_[True, np.logical_or(np.diff(fps, 2), np.diff(tps, 2)), True]
        fps, tps, thr = fps[keep], tps[keep], thr[keep]
    return np.r_[0, fps], np.r_[0, tps], _with_inf(thr)


def roc_curve_host(y_true, y_score, drop_intermediate=True):
    """sklearn.metrics.roc_curve restated: (fpr, tpr, thresholds), float64 quotients of integer counts; fpr / tpr all NaN
    without negatives / positives."""
    fps, tps, thr = roc_points_host(y_true, y_score, drop_intermediate)
    fpr = fps / fps[-1] if fps[-1] > 0 else np.full(fps.shape, np.nan)
    tpr = tps / tps[-1] if tps[-1] > 0 else np.full(tps.shape, np.nan)
    return fpr, tpr, thr


def pr_curve_host(y_true, y_score):
    """sklearn.metrics.precision_recall_curve restated: (precision, recall, thresholds) in ascending order of threshold, the
    terminal (1, 0) appended; recall all 1 without positives, precision 0 where tps + fps == 0."""
    fps, tps, thr = _binary_clf_curve_host(y_true, y_score)
    ps = tps + fps
    precision = np.zeros(tps.shape, dtype=np.float64)
    np.divide(tps, ps, out=precision, where=ps != 0)
    recall = tps / tps[-1] if tps[-1] > 0 else np.ones(tps.shape, dtype=np.float64)
    return np.hstack((precision[::-1], 1)), np.hstack((recall[::-1], 0)), thr[::-1]


def optimal_cutoff_host(y_true, y_score):
    """The threshold of the FIRST point of roc_curve(y_true, y_score) -- its default drop_intermediate=True, the origin
    included -- that minimises |tpr - (1 - fpr)|, with tpr = tps / P and fpr = fps / N in float64 in that operation
    order; NaN when the label has no positive or no negative.  Ties go to the earliest point, the highest threshold.
    This is the project's statement of the reference's Find_Optimal_Cutoff (utils/metrics.py:224-235), which itself no
    longer runs on current pandas (it indexes with .ix): it sorts the points by |tpr - (1 - fpr)| and takes the first."""
    fps, tps, thr = roc_points_host(y_true, y_score, True)
    if tps[-1] == 0 or fps[-1] == 0:
        return np.float32(np.nan)
    tpr, fpr = tps / tps[-1], fps / fps[-1]
    return np.float32(thr[int(np.argmin(np.abs(tpr - (1 - fpr))))])
