"""Block-bootstrap confidence intervals for the multi-label ranking metrics, and paired comparison of two models.

Every other result of the package is a point estimate.  This module resamples the windows -- in circular blocks, because
neighbouring windows are correlated, and per chromosome where the caller gives the chromosomes' lengths -- and evaluates
AUROC, AUPR, recall at an FDR cut-off and average precision for every label under every replicate from ONE sort of the
scores (csrc/cgcn_bootstrap.hip).  The reference has nothing of the kind (utils/evals.py:89-92 computes the point values).

This docstring is the specification; `bootstrap_weights_host` and `weighted_sums_host` restate it in numpy and the device is
held to them (tests/test_gpu_bootstrap.py): weights and integer sums bit for bit, the two float64 sums to their rounding.

THE WEIGHTED-METRIC RULE.  One label: scores s_i (float32; -0 is folded onto +0), targets t_i (positive iff > 0.5), integer
weights w_i >= 0.  Sort by score descending; a RUN is a maximal group of equal scores.  For run k = 1 .. K, TOT_k is the sum
of w over runs 1 .. k, tp_k the same sum of w t, fp_k = TOT_k - tp_k.  Runs with TOT_k = 0 (they can only be leading ones)
are no curve points, which makes the result equal to the one on the resampled rows.  (tp_0, fp_0) = (0, 0), p_0 = 1,
p_k = tp_k / TOT_k in float64, P = sum w t, TOT = sum w.  The SUMS, each [R, C] for R weight vectors and C labels:
    A    int64    sum_k (fp_k - fp_{k-1}) (tp_k + tp_{k-1})
    P    int64
    TOT  int64
    F    int64    tp_k of the LAST k with (double) fp_k <= q * (double) TOT_k, 0 without one; q = fdr_cutoff, a float64 in
                  (0, 1); one IEEE product and one comparison
    S_ap float64  sum_k (tp_k - tp_{k-1}) p_k
    S_pr float64  sum_k (tp_k - tp_{k-1}) (p_k + p_{k-1})
At q = 0.5 the condition of F is exactly fp_k <= tp_k, which is exactly what 1 - p_k <= 0.5 decides; at other cut-offs it can
differ from the float form `1 - precision <= cutoff` of the reference (utils/metrics.py:148-166) in the last ulp.
`metrics_from_sums` turns the sums into the metrics, in float64, for the device path and the restatement alike:
    auroc = A / (2 P (TOT - P)), NaN where P (TOT - P) = 0;  average_precision = S_ap / P;  aupr = S_pr / (2 P);
    recall_at_fdr = F / P;  P = 0 < TOT gives average_precision 0, aupr 0.5, recall_at_fdr 0 (what multilabel_metrics returns
    for a label without positives);  TOT = 0 gives NaN for all four.
Every TOT must be below 2^31 (so that A < 2^62): the host raises ValueError; on the device a weight is a byte (0 .. 255, a
larger or a negative one is a ValueError, never saturated) and n < 2^23, which bounds TOT by 255 n < 2^31.

THE WEIGHT RULE: circular block bootstrap, optionally per stratum.  draw(t, seed, attempt, stream, R) of
chromegcn_amd/nullgraph.py (mix32 / dropout_key of csrc/cgcn_common.hpp) with stream 5 and attempt = the replicate's ABSOLUTE
index b, so that a replicate does not depend on how replicates are batched; seed and b are 64 bits and both halves matter.
The rows are split into strata of lengths[s] consecutive rows (lengths=None: one stratum of n rows); empty strata are
skipped.  A stratum of n_s rows at offset_s has block length L_s = min(block, n_s) and makes k_s = ceil(n_s / L_s) draws,
numbered globally g = (sum of k_s' over the strata before) + j; start = draw(g, seed, b, 5, n_s), and the draw adds 1 to the
rows offset_s + (start + q) mod n_s, q = 0 .. L_s - 1.  Every row has the expected weight k_s L_s / n_s (1 when block divides
n_s); block = 1 is the ordinary bootstrap.

THE STATISTICS (host, numpy).  `bootstrap_summary`: NaN replicates are dropped and counted (n_valid); the interval is
np.quantile(..., method="linear") at (1 -+ level) / 2 of the rest, se their standard deviation with ddof = 1.  The scalars
are compute_metrics' own: meanAUC / meanAUPR / meanFDR are means over the labels with a defined value, mAP is the plain mean
of average_precision, <group>_meanAUC / _meanAUPR / _meanFDR those of metrics.group_means; each is computed per replicate and
summarised like a label.  `bootstrap_compare` walks two models under the SAME weights; a difference is a - b, and its
two-sided p is min(1, 2 min((1 + #{d_b <= 0}) / (B + 1), (1 + #{d_b >= 0}) / (B + 1))) over the B replicates with a defined
difference."""
from __future__ import annotations

from typing import Dict, NamedTuple, Optional

import numpy as np

from .nullgraph import draw

METRICS = ("auroc", "aupr", "recall_at_fdr", "average_precision")   # metrics.multilabel_metrics, in its table's order
SUMS = ("A", "P", "TOT", "F", "S_ap", "S_pr")
SCALARS = (("meanAUC", "auroc"), ("meanAUPR", "aupr"), ("meanFDR", "recall_at_fdr"), ("mAP", "average_precision"))
STREAM_BOOTSTRAP = 5
FLAG_WEIGHT, FLAG_NEGATIVE, FLAG_STRATA = 1, 2, 4   # CGCN_BOOT_FLAG_* in include/chromegcn.h
MAX_WEIGHT = 255
WORKSPACE_CAP = 1536 << 20   # bytes of start histogram + weight tile that one batch of replicates may take (n = 250 000: 1 280)
LANES = 64


# ----------------------------------------------------------------------------------------------------------------------
# the rules, on the host (numpy only)
# ----------------------------------------------------------------------------------------------------------------------
def _strata(n: int, lengths) -> np.ndarray:
    """the offsets [S + 1] (int64) of the strata; ValueError unless the lengths are non-negative and sum to n"""
    n = int(n)
    if n < 0:
        raise ValueError("n must not be negative")
    if lengths is None:
        return np.array([0, n], np.int64)
    ln = np.asarray([int(k) for k in lengths], np.int64)
    if ln.size and ln.min() < 0:
        raise ValueError("a stratum's length must not be negative")
    if int(ln.sum()) != n:
        raise ValueError("the lengths sum to %d but there are %d rows" % (int(ln.sum()), n))
    if ln.size == 0:
        return np.array([0, 0], np.int64)
    return np.concatenate([[0], np.cumsum(ln)]).astype(np.int64)


def _n_draws(offsets, block: int) -> int:
    ns = np.diff(offsets)
    ns = ns[ns > 0]
    L = np.minimum(block, ns)
    return int(((ns + L - 1) // L).sum())


def _replicate_indices(replicates):
    """a count -> 0 .. count - 1; an array -> its entries (Python ints: 64 bits)"""
    if np.ndim(replicates) == 0:
        r = int(replicates)
        if r < 0:
            raise ValueError("the number of replicates must not be negative")
        return list(range(r))
    out = [int(b) for b in np.asarray(replicates, dtype=object).ravel()]
    if any(b < 0 or b >= 1 << 64 for b in out):
        raise ValueError("a replicate index must be in [0, 2^64)")
    return out


def _check_block(block) -> int:
    block = int(block)
    if block < 1:
        raise ValueError("block must be at least 1")
    return block


def bootstrap_weights_host(n, replicates, seed=0, block=1, lengths=None) -> np.ndarray:
    """The weight rule of the module docstring: int64 [R, n], row r the weights of replicate replicates[r] (or r, for a
    count).  Pure numpy."""
    block = _check_block(block)
    offsets = _strata(n, lengths)
    reps = _replicate_indices(replicates)
    out = np.zeros((len(reps), int(n)), np.int64)
    for r, b in enumerate(reps):
        g0 = 0
        for off, end in zip(offsets[:-1], offsets[1:]):
            ns = int(end - off)
            if ns == 0:
                continue
            L = min(block, ns)
            k = (ns + L - 1) // L
            start = draw(np.arange(g0, g0 + k, dtype=np.int64), seed, b, STREAM_BOOTSTRAP, ns)
            rows = int(off) + (start[:, None] + np.arange(L, dtype=np.int64)[None, :]) % ns
            np.add.at(out[r], rows.ravel(), 1)
            g0 += k
    return out


def _check_cutoff(q) -> float:
    q = float(q)
    if not (0.0 < q < 1.0):
        raise ValueError("fdr_cutoff must be inside (0, 1), got %r" % (q,))
    return q


def _host_weights(weights, n: int) -> np.ndarray:
    w = np.asarray(weights)
    if w.dtype.kind not in "iub":
        raise ValueError("weights must be integers")
    w = w.astype(np.int64)
    if w.ndim == 1:
        w = w[None, :]
    if w.ndim != 2 or w.shape[1] != n:
        raise ValueError("weights must be [R, n] with n = %d, got %s" % (n, w.shape))
    if w.size and w.min() < 0:
        raise ValueError("a weight is negative")
    if w.size and int(w.sum(1).max()) >= 2 ** 31:
        raise ValueError("a replicate's total weight must be below 2^31")
    return w


def _as_2d(x, dtype):
    x = np.asarray(x, dtype)
    return x[:, None] if x.ndim == 1 else x


def weighted_sums_host(probs, targets, weights, fdr_cutoff=0.5) -> Dict[str, np.ndarray]:
    """The weighted-metric rule of the module docstring in numpy: probs, targets [n, C] (or [n]), weights integer [R, n]
    (or [n]) -> {'A', 'P', 'TOT', 'F' (int64), 'S_ap', 'S_pr' (float64)}, each [R, C].  ValueError for a NaN score, a
    negative weight, a total of 2^31 or more, a cut-off outside (0, 1)."""
    q = _check_cutoff(fdr_cutoff)
    s = _as_2d(probs, np.float32)
    t = _as_2d(targets, np.float32)
    if s.ndim != 2 or s.shape != t.shape:
        raise ValueError("probs and targets must both be [n, C]")
    n, C = s.shape
    w = _host_weights(weights, n)
    if np.isnan(s).any():
        raise ValueError("a score is NaN")
    R = w.shape[0]
    s = np.where(s == 0, np.float32(0), s)   # -0 onto +0
    out = {k: np.zeros((R, C), np.int64) for k in SUMS[:4]}
    out.update({k: np.zeros((R, C), np.float64) for k in SUMS[4:]})
    if n == 0 or R == 0:
        return out
    for c in range(C):
        order = np.argsort(-s[:, c].astype(np.float64), kind="stable")
        ss, tt = s[order, c], (t[order, c] > 0.5).astype(np.int64)
        end = np.ones(n, bool)
        end[:-1] = ss[1:] != ss[:-1]
        wo = w[:, order]
        tot = np.cumsum(wo, 1)[:, end]          # [R, K]
        tp = np.cumsum(wo * tt[None, :], 1)[:, end]
        fp = tot - tp
        valid = tot > 0                         # a leading run without weight repeats the point (0, 0), p = 1
        p = np.where(valid, tp / np.maximum(tot, 1).astype(np.float64), 1.0)
        zero = np.zeros((R, 1), np.int64)
        tp0, fp0 = np.concatenate([zero, tp[:, :-1]], 1), np.concatenate([zero, fp[:, :-1]], 1)
        p0 = np.concatenate([np.ones((R, 1)), p[:, :-1]], 1)
        dtp = (tp - tp0).astype(np.float64)
        out["A"][:, c] = ((fp - fp0) * (tp + tp0)).sum(1)
        out["P"][:, c] = tp[:, -1]
        out["TOT"][:, c] = tot[:, -1]
        out["S_ap"][:, c] = (dtp * p).sum(1)
        out["S_pr"][:, c] = (dtp * (p + p0)).sum(1)
        ok = valid & (fp.astype(np.float64) <= q * tot.astype(np.float64))
        last = ok.shape[1] - 1 - np.argmax(ok[:, ::-1], 1)
        out["F"][:, c] = np.where(ok.any(1), tp[np.arange(R), last], 0)
    return out


def metrics_from_sums(sums) -> Dict[str, np.ndarray]:
    """The sums of the rule -> {'auroc', 'aupr', 'recall_at_fdr', 'average_precision'}, float64 arrays of the sums' shape
    (module docstring).  The one place where the device's sums and the restatement's become metrics."""
    A, P, TOT, F = (np.asarray(sums[k], np.int64).astype(np.float64) for k in SUMS[:4])
    S_ap, S_pr = np.asarray(sums["S_ap"], np.float64), np.asarray(sums["S_pr"], np.float64)
    neg = TOT - P
    with np.errstate(divide="ignore", invalid="ignore"):
        auroc = np.where(P * neg > 0, A / (2.0 * P * neg), np.nan)
        ap = np.where(P > 0, S_ap / P, 0.0)
        aupr = np.where(P > 0, S_pr / (2.0 * P), 0.5)
        rec = np.where(P > 0, F / P, 0.0)
    empty = TOT == 0
    return {"auroc": auroc, "aupr": np.where(empty, np.nan, aupr), "recall_at_fdr": np.where(empty, np.nan, rec),
            "average_precision": np.where(empty, np.nan, ap)}


def bootstrap_summary(point, replicates, level=0.95) -> Dict[str, np.ndarray]:
    """point [...], replicates [B, ...] -> {'point', 'ci_low', 'ci_high', 'se' (float64), 'n_valid' (int64)}, each [...]:
    the percentile interval of the module docstring.  NaN replicates are dropped and counted; without a valid replicate the
    interval is NaN, with fewer than two so is se.  Pure numpy."""
    level = float(level)
    if not (0.0 < level < 1.0):
        raise ValueError("level must be inside (0, 1)")
    point = np.asarray(point, np.float64)
    rep = np.asarray(replicates, np.float64)
    if rep.ndim < 1 or rep.shape[1:] != point.shape:
        raise ValueError("replicates must be [B, ...] over the shape of point")
    flat = rep.reshape(rep.shape[0], -1)
    lo, hi = np.full(flat.shape[1], np.nan), np.full(flat.shape[1], np.nan)
    se = np.full(flat.shape[1], np.nan)
    nv = np.zeros(flat.shape[1], np.int64)
    for j in range(flat.shape[1]):
        v = flat[:, j]
        v = v[~np.isnan(v)]
        nv[j] = v.size
        if v.size:
            lo[j], hi[j] = np.quantile(v, [(1.0 - level) / 2.0, (1.0 + level) / 2.0], method="linear")
        if v.size > 1:
            se[j] = np.std(v, ddof=1)
    sh = point.shape
    return {"point": point, "ci_low": lo.reshape(sh), "ci_high": hi.reshape(sh), "se": se.reshape(sh), "n_valid": nv.reshape(sh)}


def paired_p(differences) -> np.ndarray:
    """[B, ...] replicate differences -> the two-sided p of the module docstring, [...]; NaN differences are left out"""
    d = np.asarray(differences, np.float64)
    valid = ~np.isnan(d)
    B = valid.sum(0)
    le = ((d <= 0) & valid).sum(0)
    ge = ((d >= 0) & valid).sum(0)
    return np.minimum(1.0, 2.0 * np.minimum((1.0 + le) / (B + 1.0), (1.0 + ge) / (B + 1.0)))


def _nanmean(v, axis):
    ok = ~np.isnan(v)
    cnt = ok.sum(axis)
    tot = np.where(ok, v, 0.0).sum(axis)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(cnt > 0, tot / np.maximum(cnt, 1), np.nan)


def scalar_metrics(per_label: Dict[str, np.ndarray], label_groups=None) -> Dict[str, np.ndarray]:
    """{metric: [..., C]} -> the scalars compute_metrics prints, each [...]: meanAUC, meanAUPR, meanFDR (NaN labels left
    out), mAP (the plain mean) and, with label_groups, <group>_meanAUC / _meanAUPR / _meanFDR as metrics.group_means"""
    out = {}
    for name, key in SCALARS:
        v = np.asarray(per_label[key], np.float64)
        if name == "mAP":
            out[name] = v.mean(-1) if v.shape[-1] else np.full(v.shape[:-1], np.nan)
        else:
            out[name] = _nanmean(v, -1)
    for group, idx in (label_groups or {}).items():
        idx = np.asarray(list(idx), dtype=np.int64)
        for name, key in SCALARS[:3]:
            out["%s_%s" % (group, name)] = _nanmean(np.asarray(per_label[key], np.float64)[..., idx], -1)
    return out


class BootstrapResult(NamedTuple):
    """point, ci_low, ci_high, se, n_valid: {metric: [C]}; scalars: {name: {'point', 'ci_low', 'ci_high', 'se', 'n_valid'}}
    for meanAUC, meanAUPR, meanFDR, mAP and the group means; replicates / scalar_replicates: {metric: [n_boot, C]} /
    {name: [n_boot]} with keep_replicates, else None."""
    point: Dict[str, np.ndarray]
    ci_low: Dict[str, np.ndarray]
    ci_high: Dict[str, np.ndarray]
    se: Dict[str, np.ndarray]
    n_valid: Dict[str, np.ndarray]
    scalars: Dict[str, Dict[str, float]]
    replicates: Optional[Dict[str, np.ndarray]]
    scalar_replicates: Optional[Dict[str, np.ndarray]]
    n_boot: int
    seed: int
    block: int
    level: float


class BootstrapComparison(NamedTuple):
    """Model a against model b under the same weights.  a, b: {metric: [C]} point estimates; diff (a - b), ci_low, ci_high,
    se, n_valid, p: {metric: [C]}; scalars: {name: {'a', 'b', 'diff', 'ci_low', 'ci_high', 'se', 'n_valid', 'p'}};
    replicates / scalar_replicates: the replicate DIFFERENCES with keep_replicates, else None."""
    a: Dict[str, np.ndarray]
    b: Dict[str, np.ndarray]
    diff: Dict[str, np.ndarray]
    ci_low: Dict[str, np.ndarray]
    ci_high: Dict[str, np.ndarray]
    se: Dict[str, np.ndarray]
    n_valid: Dict[str, np.ndarray]
    p: Dict[str, np.ndarray]
    scalars: Dict[str, Dict[str, float]]
    replicates: Optional[Dict[str, np.ndarray]]
    scalar_replicates: Optional[Dict[str, np.ndarray]]
    n_boot: int
    seed: int
    block: int
    level: float


# ----------------------------------------------------------------------------------------------------------------------
# the device side
# ----------------------------------------------------------------------------------------------------------------------
class _Sorted(NamedTuple):
    order: object   # uint32-as-int32 [C n] on the device
    bad: object     # int32 [1]
    n: int
    C: int


def _device_pair(probs, targets):
    import torch
    if not (torch.is_tensor(probs) and torch.is_tensor(targets)) or not probs.is_cuda or not targets.is_cuda:
        raise RuntimeError("chromegcn_amd.bootstrap: tensors must be on the GPU (there is no CPU fallback; "
                           "weighted_sums_host is the host restatement)")
    if probs.dim() != 2 or tuple(targets.shape) != tuple(probs.shape):
        raise ValueError("probs and targets must both be [n, C]")
    n, C = int(probs.shape[0]), int(probs.shape[1])
    if n < 1 or C < 1:
        raise ValueError("at least one window and one label are needed")
    return probs.contiguous().float(), targets.contiguous().float(), n, C


def _workspace(n, C, R, dev):
    from . import _lib
    return _lib.workspace_for("cgcn_bootstrap_workspace_bytes", dev, "bootstrap n=%d C=%d R=%d" % (n, C, R), n=n, C=C, R=R)


def _sort(probs, targets) -> _Sorted:
    """one sort of every label's scores; enqueued, nothing read back"""
    import torch
    from . import _lib
    p, t, n, C = _device_pair(probs, targets)
    dev = p.device
    with torch.cuda.device(dev):
        wsp, need = _workspace(n, C, 0, dev)
        order = torch.empty(n * C, dtype=torch.int32, device=dev)
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.call("cgcn_bootstrap_sort", n=n, C=C, probs=p, targets=t, order=order, bad=bad, workspace=wsp, workspace_bytes=need)
    return _Sorted(order, bad, n, C)


def _groups(R: int) -> int:
    return (R + LANES - 1) // LANES


def _rule_tile(n, rep0, R, offsets_dev, n_strata, block, draws, seed, flags, dev):
    """the weight tile [G, n, 64] of replicates rep0 .. rep0 + R - 1; flags: address of the int32 flag word"""
    import torch
    from . import _lib
    signed = lambda x: x - (1 << 64) if x >= (1 << 63) else x
    with torch.cuda.device(dev):
        tile = torch.empty((_groups(R), n, LANES), dtype=torch.uint8, device=dev)
        wsp, need = _workspace(n, 1, R, dev)
        _lib.call("cgcn_bootstrap_weights", n=n, rep0=signed(int(rep0) & 0xFFFFFFFFFFFFFFFF), R=R, n_strata=n_strata,
                  offsets=offsets_dev, block=min(block, 2 ** 31 - 1), draws=draws, seed=signed(int(seed) & 0xFFFFFFFFFFFFFFFF),
                  tile=tile, flags=flags, workspace=wsp, workspace_bytes=need)
    return tile


def _explicit_tile(weights, n, flags, dev):
    """(tile, R) of explicit weights: anything integer [R, n] (or [n]); a host array is checked before any launch"""
    import torch
    from . import _lib
    if torch.is_tensor(weights) and weights.is_cuda:
        w = weights
        if w.dtype.is_floating_point or w.dtype.is_complex:
            raise ValueError("weights must be integers")
        if w.dim() == 1:
            w = w[None, :]
        if w.dim() != 2 or int(w.shape[1]) != n:
            raise ValueError("weights must be [R, n] with n = %d, got %s" % (n, tuple(w.shape)))
        # widened first (uint8 is what bootstrap_weights returns; bool, int8 ...), then clamped so that the int32 the kernel
        # reads still says negative or above 255: the device flags -1 and 256
        w = w.to(dev).to(torch.int64).clamp(-1, MAX_WEIGHT + 1).to(torch.int32).contiguous()
    else:
        hw = _host_weights(weights.numpy() if torch.is_tensor(weights) else weights, n)
        if hw.size and hw.max() > MAX_WEIGHT:
            raise ValueError("a weight is above %d" % MAX_WEIGHT)
        w = torch.from_numpy(np.ascontiguousarray(hw, np.int32)).to(dev)
    R = int(w.shape[0])
    if R < 1:
        raise ValueError("at least one weight vector is needed")
    with torch.cuda.device(dev):
        tile = torch.empty((_groups(R), n, LANES), dtype=torch.uint8, device=dev)
        _lib.call("cgcn_bootstrap_weights_in", n=n, R=R, weights=w, tile=tile, flags=flags)
    return tile, R


def _new_out(R, C, dev):
    """(out int64 [6 R C + 2], address of the flag word): the sums, the CGCN_BOOT_FLAG_* word and the sort's bad word"""
    import torch
    out = torch.zeros(6 * R * C + 2, dtype=torch.int64, device=dev)
    return out, out.data_ptr() + 8 * 6 * R * C


def _walk(srt: _Sorted, tile, R, q, out):
    import ctypes
    import torch
    from . import _lib
    with torch.cuda.device(srt.order.device):
        _lib.call("cgcn_bootstrap_sums", n=srt.n, C=srt.C, R=R, order=srt.order, tile=tile, fdr_cutoff=ctypes.c_double(q), out=out)
        out[-1:] |= srt.bad.to(out.dtype)


def _read(out, R, C) -> Dict[str, np.ndarray]:
    """the ONE device-to-host copy: the six arrays, and what the two flag words raise"""
    h = out.cpu().numpy()
    flags, bad = int(h[-2]), int(h[-1])
    if bad:
        raise ValueError("a score is NaN")
    if flags & FLAG_NEGATIVE:
        raise ValueError("a weight is negative")
    if flags & FLAG_WEIGHT:
        raise ValueError("a weight is above %d (weights are stored as bytes)" % MAX_WEIGHT)
    if flags & FLAG_STRATA:
        raise ValueError("the strata do not lie inside the rows")
    rc = R * C
    res = {k: h[j * rc:(j + 1) * rc].reshape(R, C).copy() for j, k in enumerate(SUMS[:4])}
    res.update({k: h[(4 + j) * rc:(5 + j) * rc].view(np.float64).reshape(R, C).copy() for j, k in enumerate(SUMS[4:])})
    return res


def _rule_setup(n, block, lengths, dev):
    import torch
    block = _check_block(block)
    offsets = _strata(n, lengths)
    draws = _n_draws(offsets, block)
    total = int(sum(((e - o + min(block, e - o) - 1) // min(block, e - o)) * min(block, e - o)
                    for o, e in zip(offsets[:-1].tolist(), offsets[1:].tolist()) if e > o))
    if total >= 2 ** 31:
        raise ValueError("a replicate's total weight must be below 2^31")
    off_dev = torch.from_numpy(offsets.astype(np.int32)).to(dev)
    return block, off_dev, int(offsets.size) - 1, draws


def batch_replicates(n: int, cap: int = WORKSPACE_CAP) -> int:
    """how many replicates one batch takes under the workspace cap: a multiple of 64, at least 64"""
    per_group = max(1, int(n)) * LANES * 5   # int32 start histogram + byte tile
    return int(min(1023, max(1, cap // per_group))) * LANES


def bootstrap_weights(n, replicates, seed=0, block=1, lengths=None, device="cuda"):
    """bootstrap_weights_host on the device: uint8 [R, n] on the device (a weight above 255 is a ValueError).  Reads the flag
    word back."""
    import torch
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("bootstrap_weights needs a GPU; bootstrap_weights_host is the host restatement")
    n = int(n)
    reps = _replicate_indices(replicates)
    if n < 1:
        raise ValueError("at least one window is needed")
    block, off_dev, n_strata, draws = _rule_setup(n, block, lengths, dev)
    parts, at = [], 0
    flags = torch.zeros(2, dtype=torch.int64, device=dev)
    while at < len(reps):   # runs of consecutive indices, each at most a batch long
        end = at + 1
        while end < len(reps) and reps[end] == reps[end - 1] + 1 and end - at < batch_replicates(n):
            end += 1
        R = end - at
        tile = _rule_tile(n, reps[at], R, off_dev, n_strata, block, draws, seed, flags.data_ptr(), dev)
        parts.append(tile.permute(0, 2, 1).reshape(-1, n)[:R])
        at = end
    _read(flags, 0, 0)
    return torch.cat(parts, 0) if parts else torch.empty((0, n), dtype=torch.uint8, device=dev)


def weighted_sums(probs, targets, weights, fdr_cutoff=0.5) -> Dict[str, np.ndarray]:
    """weighted_sums_host on the device: probs, targets [n, C] CUDA tensors, weights integer [R, n] (a tensor on either side
    or an array), each in 0 .. 255 -> the six host arrays [R, C], after ONE device-to-host copy.  ValueError for a NaN score
    (the device's `bad` word), a negative weight or one above 255."""
    q = _check_cutoff(fdr_cutoff)
    import torch
    p, t, n, C = _device_pair(probs, targets)
    dev = p.device
    # the tile first: a host array's weights are refused before anything is launched
    holder = torch.zeros(2, dtype=torch.int64, device=dev)
    tile, R = _explicit_tile(weights, n, holder.data_ptr(), dev)
    srt = _sort(p, t)
    out, _ = _new_out(R, C, dev)
    _walk(srt, tile, R, q, out)
    out[-2:-1] |= holder[:1]
    return _read(out, R, C)


def weighted_metrics(probs, targets, weights, fdr_cutoff=0.5) -> Dict[str, np.ndarray]:
    """metrics_from_sums(weighted_sums(...)): the four metrics [R, C] in float64 for any integer weights [R, n] in 0 .. 255.
    Rows of 0 / 1 give leave-one-chromosome-out for free; all ones give the point estimate in float64."""
    return metrics_from_sums(weighted_sums(probs, targets, weights, fdr_cutoff))


def _replicate_metrics(models, n_boot, seed, block, lengths, fdr_cutoff, batch):
    """[(point {metric: [C]}, replicates {metric: [n_boot, C]}) per model]: every model sorted once, every batch of weights
    generated once and walked for every model"""
    import torch
    q = _check_cutoff(fdr_cutoff)
    n_boot = int(n_boot)
    if n_boot < 1:
        raise ValueError("n_boot must be at least 1")
    pairs = [_device_pair(p, t) for p, t in models]
    n, C = pairs[0][2], pairs[0][3]
    dev = pairs[0][0].device
    block, off_dev, n_strata, draws = _rule_setup(n, block, lengths, dev)
    batch = batch_replicates(n) if batch is None else int(batch)
    if batch < 1:
        raise ValueError("batch must be at least 1")
    sorts = [_sort(p, t) for p, t, _, _ in pairs]
    ones = torch.ones((1, n), dtype=torch.int32, device=dev)
    points = []
    for srt in sorts:
        out, fl = _new_out(1, C, dev)
        tile, _ = _explicit_tile(ones, n, fl, dev)
        _walk(srt, tile, 1, q, out)
        points.append({k: v[0] for k, v in metrics_from_sums(_read(out, 1, C)).items()})
    reps = [{k: np.empty((n_boot, C), np.float64) for k in METRICS} for _ in sorts]
    for b0 in range(0, n_boot, batch):
        R = min(batch, n_boot - b0)
        outs = [_new_out(R, C, dev) for _ in sorts]
        tile = _rule_tile(n, b0, R, off_dev, n_strata, block, draws, seed, outs[0][1], dev)
        for srt, (out, _) in zip(sorts, outs):
            _walk(srt, tile, R, q, out)
        outs[-1][0][-2:-1] |= outs[0][0][-2:-1]   # the weights' flag word is the first model's: every read sees it
        for m, (out, _) in enumerate(outs):
            for k, v in metrics_from_sums(_read(out, R, C)).items():
                reps[m][k][b0:b0 + R] = v
    return list(zip(points, reps))


def _summaries(point, reps, level, label_groups):
    per = {k: bootstrap_summary(point[k], reps[k], level) for k in METRICS}
    sp, sr = scalar_metrics(point, label_groups), scalar_metrics(reps, label_groups)
    scal = {name: bootstrap_summary(sp[name], sr[name], level) for name in sp}
    return per, scal, sr


def _scalar_dict(s):
    return {k: (int(v) if k == "n_valid" else float(v)) for k, v in s.items()}


def bootstrap_metrics(probs, targets, n_boot=1000, seed=0, block=1, lengths=None, level=0.95, label_groups=None,
                      fdr_cutoff=0.5, keep_replicates=False, batch=None) -> BootstrapResult:
    """Percentile intervals of the four per-label metrics and of compute_metrics' scalars under the weight rule of the module
    docstring: probs, targets [n, C] CUDA tensors; `lengths` makes the chromosomes strata.  One sort; the replicates are
    generated and walked in batches of `batch` (default: what WORKSPACE_CAP allows), one device-to-host copy per batch -- the
    result does not depend on the batching.  The point estimate is the unit-weight walk, in float64."""
    (point, reps), = _replicate_metrics([(probs, targets)], n_boot, seed, block, lengths, fdr_cutoff, batch)
    per, scal, sr = _summaries(point, reps, level, label_groups)
    return BootstrapResult(point=point, ci_low={k: per[k]["ci_low"] for k in METRICS}, ci_high={k: per[k]["ci_high"] for k in METRICS},
                           se={k: per[k]["se"] for k in METRICS}, n_valid={k: per[k]["n_valid"] for k in METRICS},
                           scalars={name: _scalar_dict(s) for name, s in scal.items()},
                           replicates=reps if keep_replicates else None, scalar_replicates=sr if keep_replicates else None,
                           n_boot=int(n_boot), seed=int(seed), block=int(block), level=float(level))


def bootstrap_compare(probs_a, probs_b, targets, n_boot=1000, seed=0, block=1, lengths=None, level=0.95, label_groups=None,
                      fdr_cutoff=0.5, keep_replicates=False, batch=None) -> BootstrapComparison:
    """Model a against model b on the same targets, both walked under the SAME weights: per label and per scalar the
    difference a - b, its percentile interval and the two-sided p of the module docstring.  The replicate differences equal
    those of two bootstrap_metrics runs with this seed, subtracted."""
    (pa, ra), (pb, rb) = _replicate_metrics([(probs_a, targets), (probs_b, targets)], n_boot, seed, block, lengths, fdr_cutoff,
                                            batch)
    diff = {k: pa[k] - pb[k] for k in METRICS}
    dreps = {k: ra[k] - rb[k] for k in METRICS}
    per = {k: bootstrap_summary(diff[k], dreps[k], level) for k in METRICS}
    sa, sb = scalar_metrics(pa, label_groups), scalar_metrics(pb, label_groups)
    sra, srb = scalar_metrics(ra, label_groups), scalar_metrics(rb, label_groups)
    sdr = {name: sra[name] - srb[name] for name in sra}
    scal = {}
    for name in sa:
        s = _scalar_dict(bootstrap_summary(sa[name] - sb[name], sdr[name], level))
        s["diff"] = s.pop("point")
        s.update(a=float(sa[name]), b=float(sb[name]), p=float(paired_p(sdr[name])))
        scal[name] = s
    return BootstrapComparison(a=pa, b=pb, diff=diff, ci_low={k: per[k]["ci_low"] for k in METRICS},
                               ci_high={k: per[k]["ci_high"] for k in METRICS}, se={k: per[k]["se"] for k in METRICS},
                               n_valid={k: per[k]["n_valid"] for k in METRICS}, p={k: paired_p(dreps[k]) for k in METRICS},
                               scalars=scal, replicates=dreps if keep_replicates else None,
                               scalar_replicates=sdr if keep_replicates else None, n_boot=int(n_boot), seed=int(seed),
                               block=int(block), level=float(level))
