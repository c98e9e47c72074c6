"""A/B compartments of one chromosome's Hi-C contact matrix: the sign of the leading eigenvector of the Pearson correlation of
the observed / expected map (Juicer's `eigenvector`, cooltools' `E1`), and the compartment restriction and stratification of
the top-K contact graph and of the metrics.  The dense middle runs on the device (csrc/cgcn_compartment.hip); every stage has
a numpy restatement here, and what lies between the stages (the pair counts, sums -> expected, the orientation, the calls) is
host numpy shared by the device path and the restatement.

The rule, per chromosome.  res = resolution_bp (default 100 000); A = hicnorm's contact matrix at res (n bins, symmetric, fp64).
  1. Matrix and balancing.  B[a, b] = A[a, b] / (nv[a] * nv[b]), one float64 multiplication and one float64 division, exactly
     insulation's rule 1; nv = hicnorm.clean_norm(norm).  With norm = None, B = A.  norm: None, a vector, or 'KR' / 'VC' /
     'SQRTVC' (computed from the records); the default is 'VC', which cannot fail to converge.
  2. Kept bins.  valid = hicmap.valid_bins(VC, norm), VC the matrix's row sums; keep = the valid bins ascending,
     m = len(keep); everything dense is m x m over keep.  m > 8192 is a ValueError that names a coarser resolution (two m^2
     float64 arrays are allocated); m < 3 gives an all-NaN result with converged = False.
  3. Expected by distance.  For d = keep[j] - keep[i] >= 0 (i <= j): dsum[d] = sum of B[keep[i], keep[j]], cnt[d] = the number
     of such pairs (exact integers on the host; zeros count, each unordered pair once); e[d] = dsum[d] / cnt[d] where
     cnt[d] > 0, else 0 (expected_from_dist_sums, the one float64 numpy function behind both paths).  A plain mean per distance
     over the kept bins: this project's definition and cooltools' convention -- NOT Juicer's expected vector, no smoothing
     window, no scale factor (hicdist's expected vector is the smoothed one and is not used here).
  4. O/E.  M[i, j] = B[keep[i], keep[j]] / e[d] when d >= ignore_diags (default 2) and e[d] > 0, else 1.0, the neutral value.
     (Filling with 0 plants a band in every row: on planted maps it raised lambda_2 / lambda_1 from 0.05 to 0.23 and at n = 17
     lost the recovery.)
  5. Standardised rows.  mean[i] = (sum_j M[i, j]) / m; ss[i] = sum_j (M[i, j] - mean[i])^2; Z[i, j] = (M[i, j] - mean[i]) /
     sqrt(ss[i]): one subtraction, one square root, one division.  A row with ss[i] == 0 gets Z = 0, is counted in
     info["flat_rows"] and gets NaN in every eigenvector.
  6. Pearson map.  C = Z Z^T, m x m float64 (a device tensor from the device path), symmetric bit for bit.
  7. Eigenvectors.  n_eigs in 1 .. 3 (default 1) by deflated power iteration on C.  Start: v0[i] = cos(0.7 i) + 0.1 on the
     compact index, normalised (numpy, uploaded).  A step: y = C v; y -= sum_{p<j} (e_p . y) e_p over the vectors already
     found; lambda = v . y; r = |y - lambda v|_2; stop when r <= tol * lambda (tol default 1e-10) or at max_iter (default 1000);
     else v = y / |y|_2.  The vector returned is the v the residual was measured on.  The loop is the host's, as KR's is: the
     device path reads lambda, |y|^2 and r^2 back every check_every steps (default 4) and can stop only there; the restatement
     looks after every step.  info: converged, iterations, eigenvalue, residual (a list per vector), flat_rows, host_syncs.
     E[k] is float64 [n]: the vector on keep, NaN elsewhere.
  8. Orientation.  orient: a float vector [n] or None.  E[k] is flipped so that sum over keep of E[k][b] * (orient[b] -
     mean_keep(orient)) > 0 (NaN entries of E[k] take no part); with orient = None or that sum 0 the entry of largest |E|
     (the lowest bin on ties) is made positive.  label_density is the natural orient: A is the side that carries the peaks.
  9. Calls.  compartment_of_bin int8: +1 where E[0] > 0 (A), -1 where E[0] < 0 (B), 0 where NaN or 0.  as_domains() int32 [n]:
     0 for A, 1 for B, 2 + b for a bin b without a call, so that the builders' domains = (vec, res) restricts a graph to
     contacts within one compartment and a bin without a call keeps only its own records.

Sums on the device run in one fixed order (a wavefront per row or distance, lane l the terms l, l + 64, ... ascending, one
butterfly); wave_sum restates that order, so dist_sums_host and oe_rows_host give the device's bits."""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp
import torch

from . import hicmap, hicnorm

MAX_KEPT = 8192
RESOLUTION_BP, IGNORE_DIAGS, TOL, MAX_ITER, CHECK_EVERY, MAX_EIGS = 100000, 2, 1e-10, 1000, 4, 3
_RULE = ("n_eigs", "ignore_diags", "orient", "tol", "max_iter", "check_every")
_CHUNK = 1 << 22   # dist_sums_host: (distance, row) terms expanded at a time
_WAVE = 64


# ----------------------------------------------------------------------------------------------
# what both paths share
# ----------------------------------------------------------------------------------------------
def _rule(rule):
    unknown = set(rule) - set(_RULE)
    if unknown:
        raise TypeError("unknown argument(s) %s" % ", ".join(sorted(unknown)))
    n_eigs = int(rule.get("n_eigs", 1))
    if not 1 <= n_eigs <= MAX_EIGS:
        raise ValueError("n_eigs must be 1 to %d, not %d" % (MAX_EIGS, n_eigs))
    out = dict(n_eigs=n_eigs, ignore_diags=int(rule.get("ignore_diags", IGNORE_DIAGS)), orient=rule.get("orient"),
               tol=float(rule.get("tol", TOL)), max_iter=int(rule.get("max_iter", MAX_ITER)),
               check_every=int(rule.get("check_every", CHECK_EVERY)))
    if out["ignore_diags"] < 0 or out["tol"] <= 0 or out["max_iter"] < 1 or out["check_every"] < 1:
        raise ValueError("ignore_diags >= 0, tol > 0, max_iter >= 1 and check_every >= 1 are required")
    return out


def kept_bins(valid, resolution_bp):
    """rule 2: (keep int32 [m] ascending, rank int32 [n]: the place of a bin in keep or -1); more than 8192 kept bins is a
    ValueError before anything dense is allocated"""
    valid = np.asarray(valid, dtype=bool).ravel()
    keep = np.flatnonzero(valid).astype(np.int32)
    if keep.size > MAX_KEPT:
        raise ValueError("%d bins are kept at resolution_bp=%d but at most %d fit the dense Pearson map: use a coarser "
                         "resolution, %d bp or more" % (keep.size, int(resolution_bp), MAX_KEPT,
                                                        int(resolution_bp) * -(-keep.size // MAX_KEPT)))
    rank = np.full(valid.size, -1, np.int32)
    rank[keep] = np.arange(keep.size, dtype=np.int32)
    return keep, rank


def pair_counts(valid) -> np.ndarray:
    """rule 3's cnt int64 [n]: the pairs of valid bins d apart, each unordered pair once (d = 0: the valid bins)"""
    v = np.asarray(valid, dtype=bool).ravel().astype(np.int64)
    return np.correlate(v, v, "full")[v.size - 1:] if v.size else np.zeros(0, np.int64)


def expected_from_dist_sums(dsum, cnt) -> np.ndarray:
    """rule 3: e = dsum / cnt where cnt > 0, else 0 (float64)"""
    dsum, cnt = np.asarray(dsum, dtype=np.float64).ravel(), np.asarray(cnt, dtype=np.int64).ravel()
    if dsum.shape != cnt.shape:
        raise ValueError("dsum has %d distances but cnt has %d" % (dsum.size, cnt.size))
    e = np.zeros(dsum.size)
    np.divide(dsum, cnt, out=e, where=cnt > 0)
    return e


def start_vector(m) -> np.ndarray:
    """rule 7's v0, normalised"""
    v = np.cos(0.7 * np.arange(m, dtype=np.float64)) + 0.1
    return v / np.sqrt(np.sum(v * v))


def label_density(targets, window_start, resolution_bp, n_bins) -> np.ndarray:
    """positives per bin, float64 [n_bins] (a host bincount): the natural `orient`.  targets [N, C] (or [N]) of 0 / 1,
    window_start [N]; a window beyond n_bins takes no part"""
    t = targets.cpu().numpy() if torch.is_tensor(targets) else np.asarray(targets)
    per_window = t.reshape(t.shape[0], -1).astype(np.float64).sum(axis=1)
    b = np.asarray(window_start, dtype=np.int64).ravel() // int(resolution_bp)
    if b.shape != per_window.shape:
        raise ValueError("targets has %d windows but window_start has %d" % (per_window.size, b.size))
    inside = (b >= 0) & (b < int(n_bins))
    return np.bincount(b[inside], weights=per_window[inside], minlength=int(n_bins))[:int(n_bins)]


def _orient_sign(e, orient) -> float:
    """rule 8 for one vector [n] (NaN where it has no entry): +1.0 or -1.0"""
    have = ~np.isnan(e)
    if not have.any():
        return 1.0
    if orient is not None:
        o = np.asarray(orient, dtype=np.float64).ravel()
        if o.size != e.size:
            raise ValueError("orient has %d bins but the matrix has %d" % (o.size, e.size))
        s = float(np.sum(e[have] * (o[have] - np.mean(o[have]))))
        if s != 0.0 and not np.isnan(s):
            return 1.0 if s > 0 else -1.0
    return 1.0 if e[int(np.nanargmax(np.abs(e)))] >= 0 else -1.0


class Compartments:
    """The result: E float64 [n_eigs, n] (NaN off keep and on flat rows), eigenvalues float64 [n_eigs], pearson [m, m] (a
    device tensor from the device path, numpy from compartments_host), keep int32 [m], expected float64 [n] (rule 3's e),
    info (rule 7), resolution_bp, n."""

    def __init__(self, E, eigenvalues, pearson, keep, expected, info, resolution_bp):
        self.E, self.eigenvalues, self.pearson, self.keep, self.expected = E, eigenvalues, pearson, keep, expected
        self.info, self.resolution_bp, self.n = info, int(resolution_bp), int(E.shape[1])

    def oriented(self, orient) -> "Compartments":
        """the same result with every vector oriented by rule 8 (nothing is computed again; the Pearson map is shared)"""
        E = np.array(self.E)
        for k in range(E.shape[0]):
            E[k] *= _orient_sign(E[k], orient)
        return Compartments(E, self.eigenvalues, self.pearson, self.keep, self.expected, self.info, self.resolution_bp)

    @property
    def compartment_of_bin(self) -> np.ndarray:
        """rule 9: int8 [n], +1 A, -1 B, 0 no call"""
        with np.errstate(invalid="ignore"):
            return (self.E[0] > 0).astype(np.int8) - (self.E[0] < 0).astype(np.int8)

    def as_domains(self) -> np.ndarray:
        """rule 9: int32 [n] for the builders' domains = (as_domains(), resolution_bp)"""
        c = self.compartment_of_bin
        return np.where(c > 0, 0, np.where(c < 0, 1, 2 + np.arange(self.n))).astype(np.int32)

    def compartment_of_windows(self, window_start) -> np.ndarray:
        """the call of each graph window's bin (int8); 0 for a window beyond the matrix"""
        b = np.asarray(window_start, dtype=np.int64).ravel() // self.resolution_bp
        inside = (b >= 0) & (b < self.n)
        c = self.compartment_of_bin
        return np.where(inside, c[np.clip(b, 0, max(self.n - 1, 0))] if self.n else 0, 0).astype(np.int8)

    def a_share(self) -> float:
        """the A share of the called bins (NaN without a call)"""
        c = self.compartment_of_bin
        called = int(np.count_nonzero(c))
        return float(np.count_nonzero(c > 0)) / called if called else float("nan")


def _result(n, keep, expected, pearson, vectors, infos, flat, syncs, orient, resolution_bp) -> Compartments:
    """rules 7 (the scatter to [n], NaN on flat rows), 8 and 9 from the compact vectors"""
    E = np.full((len(infos), n), np.nan)
    for k, v in enumerate(vectors):
        if v is not None:
            E[k, keep] = np.where(flat, np.nan, v)
    info = {key: [i[key] for i in infos] for key in ("converged", "iterations", "eigenvalue", "residual")}
    info.update(flat_rows=int(np.count_nonzero(flat)), host_syncs=int(syncs))
    c = Compartments(E, np.array(info["eigenvalue"], dtype=np.float64), pearson, keep, expected, info, resolution_bp)
    return c.oriented(orient)


def _no_result(n, keep, expected, n_eigs, syncs, resolution_bp) -> Compartments:
    nan = float("nan")
    infos = [dict(converged=False, iterations=0, eigenvalue=nan, residual=nan) for _ in range(n_eigs)]
    return _result(n, keep, expected, None, [None] * n_eigs, infos, np.zeros(keep.size, bool), syncs, None, resolution_bp)


def _stopped(lam, r2, tol) -> bool:
    return bool(np.sqrt(r2) <= tol * lam)


# ----------------------------------------------------------------------------------------------
# host restatements, stage by stage
# ----------------------------------------------------------------------------------------------
def wave_sum(T) -> np.ndarray:
    """The row sums of T [R, K] in the device's order: 64 partial sums, lane l adding the terms l, l + 64, ... ascending from
    0.0, then the butterfly p[l] += p[l ^ o] for o = 32, 16, 8, 4, 2, 1.  Bit-equal to the kernels' sums of the same terms."""
    T = np.asarray(T, dtype=np.float64)
    R, K = T.shape
    P = np.zeros((R, _WAVE))
    for t in range(0, K, _WAVE):
        w = min(_WAVE, K - t)
        P[:, :w] += T[:, t:t + w]
    lanes = np.arange(_WAVE)
    for o in (32, 16, 8, 4, 2, 1):
        P = P + P[:, lanes ^ o]
    return P[:, 0].copy()


def balanced_dense_host(A, norm, keep) -> np.ndarray:
    """rule 1 over the kept bins: B float64 [m, m]"""
    A = sp.csr_matrix(A, dtype=np.float64)
    keep = np.asarray(keep, dtype=np.int64)
    B = A[keep][:, keep].toarray()
    if norm is not None:
        nv = hicnorm.clean_norm(norm, A.shape[0])[keep]
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            B = B / (nv[:, None] * nv[None, :])
    return B


def dist_sums_host(B, keep, n) -> np.ndarray:
    """rule 3's dsum float64 [n] from the dense B [m, m] and keep"""
    B = np.asarray(B, dtype=np.float64)
    keep = np.asarray(keep, dtype=np.int64).ravel()
    m, n = keep.size, int(n)
    rank = np.full(n, -1, np.int64)
    rank[keep] = np.arange(m)
    out = np.zeros(n)
    rows = np.arange(m)
    step = max(1, _CHUNK // max(m, 1))
    for d0 in range(0, n, step):
        d = np.arange(d0, min(d0 + step, n))
        b = keep[None, :] + d[:, None]
        r = rank[np.minimum(b, n - 1)]
        ok = (b < n) & (r >= 0)
        out[d] = wave_sum(np.where(ok, B[rows[None, :], np.maximum(r, 0)], 0.0))
    return out


def oe_rows_host(B, keep, e, ignore_diags=IGNORE_DIAGS):
    """rules 4 and 5's sums: (M [m, m], mean [m], ss [m])"""
    B = np.asarray(B, dtype=np.float64)
    keep = np.asarray(keep, dtype=np.int64).ravel()
    e = np.asarray(e, dtype=np.float64).ravel()
    m = keep.size
    d = np.abs(keep[:, None] - keep[None, :])
    ev = np.where(d < e.size, e[np.minimum(d, max(e.size - 1, 0))], 0.0) if e.size else np.zeros(d.shape)
    use = (d >= int(ignore_diags)) & (ev > 0)
    M = np.ones((m, m))
    np.divide(B, ev, out=M, where=use)
    mean = wave_sum(M) / float(m)
    t = M - mean[:, None]
    return M, mean, wave_sum(t * t)


def standardise_host(M, mean, ss) -> np.ndarray:
    """rule 5's Z from M, mean and ss, elementwise"""
    ss = np.asarray(ss, dtype=np.float64)
    Z = np.zeros_like(M)
    pos = ss > 0
    Z[pos] = (M[pos] - mean[pos, None]) / np.sqrt(ss[pos])[:, None]
    return Z


def pearson_host(Z) -> np.ndarray:
    """rule 6: C = Z Z^T, the lower triangle a copy of the upper one"""
    C = Z @ Z.T
    return np.triu(C) + np.triu(C, 1).T


def power_step_host(C, v, prev=()):
    """one step of rule 7: (y deflated, lambda, |y|^2, r^2, the dots with prev, v_next)"""
    y = C @ v
    dots = [float(p @ y) for p in prev]
    for dot, p in zip(dots, prev):
        y = y - dot * p
    lam = float(v @ y)
    nn = float(y @ y)
    t = y - lam * v
    length = np.sqrt(nn)
    return y, lam, nn, float(t @ t), dots, (y / length if length > 0 else y)


def power_iteration_host(C, n_eigs=1, tol=TOL, max_iter=MAX_ITER):
    """rule 7 on the host, looking at the residual after every step: (vectors [n_eigs][m], infos)"""
    vectors, infos = [], []
    for _ in range(n_eigs):
        v, it = start_vector(C.shape[0]), 0
        while True:
            _, lam, _, r2, _, v_next = power_step_host(C, v, vectors)
            it += 1
            stop = _stopped(lam, r2, tol)
            if stop or it >= max_iter:
                break
            v = v_next
        vectors.append(v)
        infos.append(dict(converged=bool(stop), iterations=it, eigenvalue=lam, residual=float(np.sqrt(r2))))
    return vectors, infos


def compartments_host(pos1, pos2, count, norm="VC", resolution_bp=RESOLUTION_BP, n_bins=None, n_eigs=1, ignore_diags=IGNORE_DIAGS,
                      orient=None, tol=TOL, max_iter=MAX_ITER, norm_args=None) -> Compartments:
    """The whole rule in numpy, with the same iteration and start vector as the device path (not eigh)."""
    rule = _rule(dict(n_eigs=n_eigs, ignore_diags=ignore_diags, tol=tol, max_iter=max_iter))
    A, vc, norm, _ = hicmap.resolve_host(pos1, pos2, count, norm, resolution_bp, n_bins, norm_args)
    n = A.shape[0]
    valid = hicmap.valid_bins(vc, norm)
    keep, _ = kept_bins(valid, resolution_bp)
    cnt = pair_counts(valid)
    if keep.size < 3:
        return _no_result(n, keep, np.zeros(n), rule["n_eigs"], 0, resolution_bp)
    B = balanced_dense_host(A, norm, keep)
    e = expected_from_dist_sums(dist_sums_host(B, keep, n), cnt)
    M, mean, ss = oe_rows_host(B, keep, e, rule["ignore_diags"])
    C = pearson_host(standardise_host(M, mean, ss))
    vectors, infos = power_iteration_host(C, rule["n_eigs"], rule["tol"], rule["max_iter"])
    return _result(n, keep, e, C, vectors, infos, ss == 0, 0, orient, resolution_bp)


# ----------------------------------------------------------------------------------------------
# device, stage by stage (each enqueues only)
# ----------------------------------------------------------------------------------------------
def _ld(m) -> int:
    """the leading dimension of B / M / Z: even, so that every row starts on 16 bytes"""
    return m + (m & 1)


def _i32(a, dev) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)


def _dense_arg(B):
    if not (torch.is_tensor(B) and B.is_cuda and B.dtype == torch.float64 and B.ndim == 2 and B.is_contiguous()
            and B.shape[1] == _ld(B.shape[0])):
        raise ValueError("B must be a contiguous float64 device tensor [m, m + (m & 1)]")
    return int(B.shape[0]), int(B.shape[1])


def balanced_dense(A: hicnorm.DeviceContactMatrix, norm, keep) -> torch.Tensor:
    """rule 1 on the device (cgcn_hiccomp_dense): B float64 [m, ld], ld = m + (m & 1); the columns beyond m stay 0.
    norm: None or a float64 device vector; keep: the kept bins ascending (host)."""
    from . import _lib
    dev = A.rowptr.device
    keep = np.asarray(keep, dtype=np.int64).ravel()
    m = int(keep.size)
    if m > MAX_KEPT or (m and (keep[0] < 0 or keep[-1] >= A.n or np.any(np.diff(keep) <= 0))):
        raise ValueError("keep must be at most %d strictly ascending bins of the matrix" % MAX_KEPT)
    hicmap.device_vector(norm, dev, "norm", optional=True)
    rank = np.full(A.n, -1, np.int32)
    rank[keep] = np.arange(m, dtype=np.int32)
    B = torch.zeros(m, _ld(m), dtype=torch.float64, device=dev)
    if m:
        with torch.cuda.device(dev):
            _lib.call("cgcn_hiccomp_dense", n=A.n, rowptr=A.rowptr, col=A.col, val=A.val, norm=norm,
                      n_norm=0 if norm is None else int(norm.numel()), rank=_i32(rank, dev), m=m, ld=_ld(m), B=B)
    return B


def dist_sums(B, keep, n) -> torch.Tensor:
    """rule 3's dsum float64 [n] on the device (cgcn_hiccomp_dist_sums)"""
    from . import _lib
    m, ld = _dense_arg(B)
    keep = np.asarray(keep, dtype=np.int64).ravel()
    if keep.size != m or (m and (keep.min() < 0 or keep.max() >= int(n))):
        raise ValueError("keep must hold B's %d bins, all below n" % m)
    rank = np.full(int(n), -1, np.int32)
    rank[keep] = np.arange(m, dtype=np.int32)
    out = torch.zeros(int(n), dtype=torch.float64, device=B.device)
    if n and m:
        with torch.cuda.device(B.device):
            _lib.call("cgcn_hiccomp_dist_sums", n=int(n), m=m, ld=ld, B=B, keep=_i32(keep, B.device), rank=_i32(rank, B.device),
                      dsum=out)
    return out


def oe_rows(B, keep, e, ignore_diags=IGNORE_DIAGS, stages=3, stats=None):
    """rules 4 and 5 in place on the device (cgcn_hiccomp_oe_rows): (mean, ss) float64 device vectors [m].  stages & 1: B
    becomes M, mean and ss are computed; stages & 2: M becomes Z from `stats` = (mean, ss) (stage 1's when both run)."""
    from . import _lib
    m, ld = _dense_arg(B)
    dev = B.device
    keep = np.asarray(keep, dtype=np.int64).ravel()
    if keep.size != m:
        raise ValueError("keep must hold B's %d bins" % m)
    if stages not in (1, 2, 3) or (stages == 2) != (stats is not None):
        raise ValueError("stages is 1, 2 or 3; stats goes with stages = 2 alone")
    mean, ss = stats if stats is not None else (torch.empty(m, dtype=torch.float64, device=dev) for _ in range(2))
    e = e if torch.is_tensor(e) else torch.from_numpy(np.ascontiguousarray(e, dtype=np.float64)).to(dev)
    if m:
        with torch.cuda.device(dev):
            _lib.call("cgcn_hiccomp_oe_rows", m=m, ld=ld, B=B, keep=_i32(keep, dev), e=e if e.numel() else None, n_e=int(e.numel()),
                      ignore_diags=int(ignore_diags), stages=int(stages), mean=mean, ss=ss)
    return mean, ss


def pearson(Z) -> torch.Tensor:
    """rule 6 on the device (cgcn_hiccomp_corr): C float64 [m, m]"""
    from . import _lib
    m, ld = _dense_arg(Z)
    C = torch.empty(m, m, dtype=torch.float64, device=Z.device)
    if m:
        with torch.cuda.device(Z.device):
            _lib.call("cgcn_hiccomp_corr", m=m, ld=ld, Z=Z, C=C)
    return C


def power_step(C, v, prev=None, y=None, v_next=None, rec=None):
    """one step of rule 7 on the device (cgcn_hiccomp_step): (y, v_next, rec) device tensors; rec float64 [8] = lambda,
    |y|^2, r^2, the dots with prev [n_prev, m].  Nothing is read back."""
    from . import _lib
    m, dev = int(C.shape[0]), C.device
    y = torch.empty(m, dtype=torch.float64, device=dev) if y is None else y
    v_next = torch.empty(m, dtype=torch.float64, device=dev) if v_next is None else v_next
    rec = torch.zeros(8, dtype=torch.float64, device=dev) if rec is None else rec
    with torch.cuda.device(dev):
        _lib.call("cgcn_hiccomp_step", m=m, C=C, v=v, prev=prev, n_prev=0 if prev is None else int(prev.shape[0]), y=y,
                  v_next=v_next, rec=rec)
    return y, v_next, rec


def power_iteration(C, n_eigs=1, tol=TOL, max_iter=MAX_ITER, check_every=CHECK_EVERY):
    """rule 7 with the steps on the device and the loop on the host: (vectors [n_eigs][m] numpy, infos, host syncs)"""
    m, dev = int(C.shape[0]), C.device
    v0 = torch.from_numpy(start_vector(m)).to(dev)
    found = torch.zeros(max(n_eigs - 1, 1), m, dtype=torch.float64, device=dev)
    y, rec = torch.empty(m, dtype=torch.float64, device=dev), torch.zeros(8, dtype=torch.float64, device=dev)
    vectors, infos, syncs = [], [], 0
    for k in range(n_eigs):
        a, b, it = v0.clone(), torch.empty_like(v0), 0
        while True:
            for _ in range(min(check_every, max_iter - it)):
                power_step(C, a, found[:k] if k else None, y, b, rec)
                a, b = b, a   # b: the vector this step measured, a: the next one
                it += 1
            lam, _, r2 = rec[:3].tolist()
            syncs += 1
            stop = _stopped(lam, r2, tol)
            if stop or it >= max_iter:
                break
        if k + 1 < n_eigs:
            found[k].copy_(b)
        vectors.append(b.cpu().numpy())
        syncs += 1
        infos.append(dict(converged=bool(stop), iterations=it, eigenvalue=lam, residual=float(np.sqrt(r2))))
    return vectors, infos, syncs


def compartments_of_matrix(A: hicnorm.DeviceContactMatrix, norm, resolution_bp=RESOLUTION_BP, **rule) -> Compartments:
    """Rules 2 to 9 from the device matrix and a device norm vector (or None).  Read back: the row sums and the vector, the n
    distance sums, the m row sums of squares, three doubles every check_every steps, the vectors."""
    rule = _rule(rule)
    nv = None if norm is None else norm.cpu().numpy()
    valid = hicmap.valid_bins(A.vc.cpu().numpy(), nv)
    keep, _ = kept_bins(valid, resolution_bp)
    if keep.size < 3:
        return _no_result(A.n, keep, np.zeros(A.n), rule["n_eigs"], 1, resolution_bp)
    B = balanced_dense(A, norm, keep)
    e = expected_from_dist_sums(dist_sums(B, keep, A.n).cpu().numpy(), pair_counts(valid))
    _, ss = oe_rows(B, keep, e, rule["ignore_diags"])
    C = pearson(B)
    del B
    flat = ss.cpu().numpy() == 0
    vectors, infos, syncs = power_iteration(C, rule["n_eigs"], rule["tol"], rule["max_iter"], rule["check_every"])
    return _result(A.n, keep, e, C, vectors, infos, flat, syncs + 3, rule["orient"], resolution_bp)


# ----------------------------------------------------------------------------------------------
# graphs and metrics by compartment
# ----------------------------------------------------------------------------------------------
def compartment_edge_share(graph_or_csr, comp_of_window) -> dict:
    """{"AA", "BB", "AB", "uncalled", "nnz"} as exact integers: the stored entries of a graph (hicmap.csr_of's
    inputs) by the calls of their two windows (+1 A, -1 B, 0 none; an entry with an end without a call is "uncalled")"""
    comp = np.asarray(comp_of_window, dtype=np.int64).ravel()
    row, col, nnz = hicmap.edge_rows(graph_or_csr, comp.size, "comp_of_window")
    a, b = comp[row], comp[col]
    return {"AA": int(np.sum((a > 0) & (b > 0))), "BB": int(np.sum((a < 0) & (b < 0))), "AB": int(np.sum(a * b < 0)),
            "uncalled": int(np.sum(a * b == 0)), "nnz": nnz}


def compartment_metrics(probs, targets, comp_of_window, fdr_cutoff=0.5, host=False) -> dict:
    """{"A": {metric: [C]}, "B": {metric: [C]}}: bootstrap.weighted_metrics (AUROC, AUPR, recall at the FDR cutoff, AP per
    label) with the two 0 / 1 rows comp > 0 and comp < 0.  probs, targets: device tensors [n, C], as weighted_metrics takes
    them; host = True: arrays or tensors, through bootstrap.weighted_sums_host instead of the device."""
    from . import bootstrap
    comp = np.asarray(comp_of_window).ravel()
    rows = np.stack([comp > 0, comp < 0]).astype(np.int32)
    if host:
        probs, targets = (x.cpu().numpy() if torch.is_tensor(x) else x for x in (probs, targets))
        got = bootstrap.metrics_from_sums(bootstrap.weighted_sums_host(probs, targets, rows, fdr_cutoff))
    else:
        got = bootstrap.weighted_metrics(probs, targets, rows, fdr_cutoff)
    return {name: {k: v[i] for k, v in got.items()} for i, name in enumerate(("A", "B"))}
