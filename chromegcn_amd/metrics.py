"""Multi-label metrics on the GPU: the build's counterpart of the reference's
compute_metrics (utils/evals.py:26-120) / utils/metrics.py, which calls scikit-learn once per label per metric on
the CPU after every split (runner.py:41,45,51) -- the dominant cost of an epoch once the GCN step takes
microseconds.  One device sort + one scan (cgcn_multilabel_metrics)."""
from __future__ import annotations

from typing import Dict

import numpy as np
import torch

from . import _lib


def _metrics_raw(probs: torch.Tensor, targets: torch.Tensor, fdr_cutoff: float, nonneg: bool) -> torch.Tensor:
    """one launch sequence; returns a flat device tensor: [4 * C] results, then (nonneg path) the `bad` word as element 4 C
    (bit pattern of an int32: nonzero = a score was negative or NaN and the results are to be discarded)"""
    if not probs.is_cuda or not targets.is_cuda:
        raise RuntimeError("chromegcn_amd.metrics: tensors must be on the GPU (there is no CPU fallback; "
                           "the reference's sklearn path is utils/metrics.py)")
    probs = probs.contiguous().float()
    targets = targets.contiguous().float()
    n, C = probs.shape
    if tuple(targets.shape) != (n, C):
        raise RuntimeError("probs and targets must both be [n, C]")
    ws_bytes = _lib.query("cgcn_metrics_workspace_bytes", n=n, C=C)
    if ws_bytes == 0:
        raise RuntimeError("chromegcn_amd.metrics: unsupported size n=%d C=%d" % (n, C))
    ws = torch.empty(ws_bytes, device=probs.device, dtype=torch.uint8)
    out = torch.empty(4 * C + 1, device=probs.device, dtype=torch.float32)
    args = dict(n=n, C=C, probs=probs, targets=targets, fdr_cutoff=float(fdr_cutoff), out=out, workspace=ws,
                workspace_bytes=ws_bytes)
    if nonneg:
        _lib.call("cgcn_multilabel_metrics_nonneg", bad=out.data_ptr() + 16 * C, **args)
    else:
        _lib.call("cgcn_multilabel_metrics", **args)
    return out


def _split(flat: torch.Tensor, C: int) -> Dict[str, torch.Tensor]:
    out = flat[:4 * C].view(4, C)
    return {"auroc": out[0], "aupr": out[1], "recall_at_fdr": out[2], "average_precision": out[3]}


def multilabel_metrics(probs: torch.Tensor, targets: torch.Tensor, fdr_cutoff: float = 0.5) -> Dict[str, torch.Tensor]:
    """probs, targets: [n, C] float32 CUDA tensors.  Returns per-label tensors [C] (NaN where undefined):
    'auroc', 'aupr', 'recall_at_fdr', 'average_precision'.
    Scores are taken for probabilities first (non-negative: 32-bit keys and the library's own segmented radix sort,
    cgcn_multilabel_metrics_nonneg); if the device reports a negative score or a NaN the general path (any float scores,
    64-bit keys) runs instead -- same results either way where both apply.
    `fdr_cutoff` is rounded to float32 on the way in (the C ABI takes a float): 0.1 means float32(0.1)."""
    C = probs.shape[1]
    flat = _metrics_raw(probs, targets, fdr_cutoff, nonneg=True)
    if int(flat[4 * C:].view(torch.int32).item()) != 0:
        flat = _metrics_raw(probs, targets, fdr_cutoff, nonneg=False)
    return _split(flat, C)


def group_means(per_label: Dict[str, np.ndarray], label_groups) -> Dict[str, float]:
    """{<group>_meanAUC, <group>_meanAUPR, <group>_meanFDR} for every group of `label_groups` (a mapping group name -> list
    of label indices, e.g. {"tfbs": [...], "hm": [...], "dnase": [...]}: utils/evals.py:38-71 averages over these three):
    means of per_label["auroc" / "aupr" / "recall_at_fdr"] ([C] arrays, NaN where undefined) over the group's labels with
    a defined value, NaN when it has none.  Pure host arithmetic."""
    out = {}
    for group, idx in label_groups.items():
        idx = np.asarray(list(idx), dtype=np.int64)
        for key, name in (("auroc", "meanAUC"), ("aupr", "meanAUPR"), ("recall_at_fdr", "meanFDR")):
            v = np.asarray(per_label[key], dtype=np.float64)[idx]
            v = v[~np.isnan(v)]
            out["%s_%s" % (group, name)] = float(np.mean(v)) if v.size else float("nan")
    return out


def compute_metrics(all_predictions, all_targets, loss, args=None, elapsed=0.0, data_dict=None, cell_type=None,
                    device="cuda", verbose=False, label_groups=None, br_threshold=None, bootstrap=None):
    """Same positional arguments and result keys as the reference's compute_metrics (utils/evals.py:26,107-120).
    Labels whose metric is undefined (a single class present) are skipped in the means, as the reference's try/except
    does.  Unlike the reference this does NOT threshold all_predictions in place (utils/evals.py:99-100).
    Of the per_label_type branch (utils/evals.py:28-84) the group means are here: with `label_groups` (see group_means;
    the caller supplies the index lists) the result also holds <group>_meanAUC / _meanAUPR / _meanFDR, from the per-label
    results of the same single metrics call.  The curves its plot branch draws are chromegcn_amd.curves.
    `br_threshold` (default: `args.br_threshold` where `args` has one, else off; config_args.py:28): with a value the result
    also holds the scalars ACC, HA, ebF1, miF1, maF1 of the decisions p >= br_threshold (chromegcn_amd.thresholds, one more
    stream over the device tensors); all_predictions is still not modified.
    `bootstrap` (default: off, nothing changes): a dict of bootstrap_metrics' arguments (n_boot, block, seed, lengths, level);
    the result then also holds mAP_ci, meanAUC_ci, meanAUPR_ci and meanFDR_ci, each the (low, high) percentile interval of
    the scalar under the block bootstrap of chromegcn_amd.bootstrap (NaN for an empty split)."""
    p = torch.as_tensor(all_predictions).to(device=device, dtype=torch.float32)
    t = torch.as_tensor(all_targets).to(device=device, dtype=torch.float32)
    C = p.shape[1]
    empty = p.shape[0] == 0   # a split without a chromosome (-synthetic_chroms chr21,chr22 has no validation one): all NaN
    if empty:
        m = {k: np.full(C, np.nan) for k in ("auroc", "aupr", "recall_at_fdr", "average_precision")}
    else:
        host = _metrics_raw(p, t, 0.5, nonneg=True).cpu()          # ONE device-to-host copy: results + the `bad` word
        if int(host[4 * C:].view(torch.int32).item()) != 0:        # scores that are not probabilities: the general path
            host = _metrics_raw(p, t, 0.5, nonneg=False).cpu()
        m = {k: v.double().numpy() for k, v in _split(host, C).items()}
    auc = m["auroc"][~np.isnan(m["auroc"])]
    aupr = m["aupr"][~np.isnan(m["aupr"])]
    fdr = m["recall_at_fdr"][~np.isnan(m["recall_at_fdr"])]
    out = {
        "mAP": float(np.mean(m["average_precision"])) if m["average_precision"].size else float("nan"),
        "meanAUC": float(np.mean(auc)) if auc.size else float("nan"),
        "medianAUC": float(np.median(auc)) if auc.size else float("nan"),
        "allAUC": auc, "allFDR": fdr,
        "meanAUPR": float(np.mean(aupr)) if aupr.size else float("nan"),
        "medianAUPR": float(np.median(aupr)) if aupr.size else float("nan"),
        "allAUPR": aupr,
        "meanFDR": float(np.mean(fdr)) if fdr.size else float("nan"),
        "medianFDR": float(np.median(fdr)) if fdr.size else float("nan"),
        "loss": loss, "time": elapsed,
    }
    if label_groups is not None:
        out.update(group_means(m, label_groups))
    if br_threshold is None:
        br_threshold = getattr(args, "br_threshold", None)
    if br_threshold is not None and not empty:
        from . import thresholds
        tm = thresholds.threshold_metrics(p, t, float(br_threshold))
        out.update({k: float(tm[k][0]) for k in thresholds.METRIC_KEYS})
    if bootstrap is not None:
        keys = ("mAP", "meanAUC", "meanAUPR", "meanFDR")
        if empty:
            out.update({k + "_ci": (float("nan"), float("nan")) for k in keys})
        else:
            from . import bootstrap as B
            res = B.bootstrap_metrics(p, t, **dict(bootstrap))
            out.update({k + "_ci": (res.scalars[k]["ci_low"], res.scalars[k]["ci_high"]) for k in keys})
    if verbose:  # utils/evals.py:102-105
        print("mAP:      " + str(round(out["mAP"], 3)))
        print("meanAUC:  " + str(round(out["meanAUC"], 3)))
        print("meanAUPR: " + str(round(out["meanAUPR"], 3)))
        print("meanFDR:  " + str(round(out["meanFDR"], 3)))
    return out


def per_chromosome_metrics(probs, targets, lengths, names=None, loss=0.0, device="cuda", **kwargs):
    """{chromosome: compute_metrics of that chromosome's rows} for predictions and targets that hold the chromosomes one after
    the other: lengths[i] rows for chromosome names[i] (default names: "0", "1", ...).  The slices are views of the device
    tensors, so the existing kernels run on them without a copy.  The reference's per-chromosome loop
    (scripts/analyze_results.py:288-307) selects every chromosome's rows and then hands the UNSLICED arrays to compute_metrics
    (:304), a slip that gives every chromosome the whole split's metrics; this slices.  `loss` and kwargs go to
    compute_metrics: with bootstrap=dict(n_boot=..., block=...) every chromosome's rows are resampled on their own (one
    stratum) and its result holds the <key>_ci pairs."""
    lengths = [int(k) for k in lengths]
    names = [str(i) for i in range(len(lengths))] if names is None else [str(c) for c in names]
    if len(names) != len(lengths) or len(set(names)) != len(names):
        raise ValueError("per_chromosome_metrics: one distinct name per length is needed")
    p = torch.as_tensor(probs).to(device=device, dtype=torch.float32)
    t = torch.as_tensor(targets).to(device=device, dtype=torch.float32)
    if min(lengths, default=0) < 0 or sum(lengths) != p.shape[0] or t.shape != p.shape:
        raise ValueError("per_chromosome_metrics: the lengths sum to %d but there are %d rows" % (sum(lengths), p.shape[0]))
    out, at = {}, 0
    for c, k in zip(names, lengths):
        out[c] = compute_metrics(p[at:at + k], t[at:at + k], loss, device=device, **kwargs)
        at += k
    return out
