"""KR / VC / SQRTVC normalisation vectors of a Hi-C contact matrix, computed from the contact records themselves: what
Juicer writes next to a `RAWobserved` dump as `<chrom>_<res>kb.{KR,VC,SQRTVC}norm` and data/7create_graph_new.py:51-65
reads, for record sets that have no such file (KR that did not converge, HiChIP pairs, merged replicates).  On the
device: csrc/cgcn_hicnorm.hip, driven by kr_balance_device below; beside it the numpy / scipy restatement.

Definitions.  Records (pos1, pos2, count), any order, pos1 > pos2 and duplicates allowed; i = pos1 // res, j = pos2 // res.
  A (n_bins x n_bins, symmetric, fp64): i == j adds count to A[i, i]; otherwise to A[i, j] and A[j, i].  The records of one
  entry are added in record order.  A count that is negative or not finite, or a negative position, is a ValueError;
  n_bins defaults to the largest bin + 1 and a smaller one is a ValueError.  nnz_i = entries of row i that are > 0.
  VC_i = sum_j A[i, j];  SQRTVC_i = sqrt(VC_i);  every vector holds NaN where VC_i == 0 (Juicer writes NaN there and the
  graph builder maps NaN and 0 to "this contact is worth 0").
  KR: S = {i: VC_i > 0 and nnz_i >= min_row_nnz}; x > 0 on S with x_i (A_S x)_i = 1, A_S = A without the rows and columns
  outside S; the vector is 1 / x on S and NaN elsewhere, so count / (nv_i nv_j) = x_i count x_j is the balanced value.
  Stop at ||1 - x o (A_S x)||_2 <= tol, or when max_mvp matrix-vector products are spent (converged = False).
  Juicer rescales each of its vectors by one global factor; the top-K selection does not see such a factor and it is not
  reproduced: the vectors are not comparable number by number with Juicer's files.

The KR iteration (Knight & Ruiz 2013, inner-outer Newton with CG; delta = 0.1, Delta = 3, g = 0.9, etamax = 0.1):

    x = 1; v = x o (A x); rk = 1 - v; rho1 = rk.rk; rout = rold = rho1; eta = etamax; stop_tol = tol / 2; rt = tol^2
    while rout > rt and mvp < max_mvp:
        k = 0; y = 1; innertol = max(eta^2 rout, rt)
        while rho1 > innertol and mvp < max_mvp:
            k += 1
            if k == 1: Z = rk / v; p = Z; rho1 = rk.Z
            else:      beta = rho1 / rho2; p = Z + beta p
            w = x o (A (x o p)) + v o p;  alpha = rho1 / (p.w);  ap = alpha p;  ynew = y + ap
            if min(ynew) <= delta: gamma = min over ap < 0 of (delta - y) / ap;  y += gamma ap; break
            if max(ynew) >= Delta: gamma = min over ynew > Delta of (Delta - y) / ap;  y += gamma ap; break
            y = ynew; rk -= alpha w; rho2 = rho1; Z = rk / v; rho1 = rk.Z
        x = x o y; v = x o (A x); rk = 1 - v; rho1 = rk.rk; rout = rho1
        rat = rout / rold; rold = rout; eta_o = eta; eta = g rat
        if g eta_o^2 > 0.1: eta = max(eta, g eta_o^2)
        eta = max(min(eta, etamax), stop_tol / sqrt(rout))

Every product A z counts against max_mvp, the first one included; the outer update behind an inner loop that the cap has
stopped is still made (the listing does not gate it), so a run spends at most max_mvp + 1 products.  The host restatement follows the listing step by step on
the extracted A_S; the device keeps the control flow and works on the full vectors with a 0 / 1 mask inside the products
and the residual, the vector steps fused (cgcn_hicnorm_kr_step) and their scalars in a device record that the host reads
once per inner iteration and once per outer update.  Loop control is the host's.

Sparse rows (kr_retry): a run that does not converge is repeated with min_row_nnz raised to the nnz found at the 1, 2, 3,
5 and then 10 % quantile of the non-empty rows (sorted(nnz)[int(q cnt)]; at least the last value + 1): at most five more
runs of at most max_mvp + 1 products each, the first that converges wins, info["min_row_nnz"] names it (the last one tried when
none does).  Our own ladder, in the spirit of Juicer's; it does not reproduce Juicer's."""
from __future__ import annotations

import math

import numpy as np
import scipy.sparse as sp
import torch

KINDS = ("KR", "VC", "SQRTVC")
KR_DELTA, KR_DELTA_UP, KR_G, KR_ETAMAX = 0.1, 3.0, 0.9, 0.1
LADDER = (0.01, 0.02, 0.03, 0.05, 0.10)
# include/chromegcn.h: CGCN_HICNORM_*
_REC, _HDR = 32, 32 + 6 * 1024
_OP_MASK, _OP_RES, _OP_FIRST, _OP_DIR, _OP_W, _OP_Y, _OP_CLIP = range(7)
_V_MASK, _V_X, _V_V, _V_P, _V_W, _V_Y, _V_RK, _V_Z = 0, 1, 2, 3, 4, 5, 7, 9
_KR_DEFAULTS = dict(tol=1e-6, max_mvp=1000, min_row_nnz=1, kr_retry=True)


class HicNormError(RuntimeError):
    """KR did not converge (after the sparse-row ladder when kr_retry); `info` is the last run's"""

    def __init__(self, msg, info):
        super().__init__(msg)
        self.info = info


def _kind(kind) -> str:
    if kind not in KINDS:
        raise ValueError("norm kind %r is none of %s" % (kind, ", ".join(KINDS)))
    return kind


def _bad_records(flags: int):
    if flags & 1:
        raise ValueError("contact counts must be finite and non-negative")
    if flags & 2:
        raise ValueError("contact positions must be non-negative")


def _require_converged(info):
    if not info.get("converged", True):
        raise HicNormError("KR did not converge: %r" % (info,), info)


# ----------------------------------------------------------------------------------------------
# host restatement
# ----------------------------------------------------------------------------------------------
def contact_matrix_host(pos1, pos2, count, resolution_bp, n_bins=None) -> sp.csr_matrix:
    """A of the module docstring as a float64 CSR with sorted columns; the records of one entry are added in record order"""
    res = int(resolution_bp)
    if res < 1:
        raise ValueError("resolution_bp must be positive")
    p1, p2 = np.asarray(pos1, dtype=np.int64).ravel(), np.asarray(pos2, dtype=np.int64).ravel()
    c = np.asarray(count, dtype=np.float64).ravel()
    if not (p1.shape == p2.shape == c.shape):
        raise ValueError("pos1, pos2 and count must be vectors of one length")
    _bad_records((0 if np.all(np.isfinite(c) & (c >= 0)) else 1) | (2 if p1.size and min(p1.min(), p2.min()) < 0 else 0))
    i, j = p1 // res, p2 // res
    top = int(max(i.max(), j.max())) + 1 if i.size else 0
    n = top if n_bins is None else int(n_bins)
    if n < top:
        raise ValueError("n_bins=%d but the records reach bin %d" % (n, top - 1))
    # two slots per record, (i, j) and (j, i), the second one unused for a diagonal record: the device's order
    rows, cols = np.stack([i, j], 1).ravel(), np.stack([j, i], 1).ravel()
    vals = np.repeat(c, 2)
    keep = np.stack([np.ones(i.size, bool), i != j], 1).ravel()
    rows, cols, vals = rows[keep], cols[keep], vals[keep]
    order = np.lexsort((cols, rows))   # stable: equal (row, col) stay in record order
    rows, cols, vals = rows[order], cols[order], vals[order]
    head = np.ones(rows.size, bool)
    head[1:] = (rows[1:] != rows[:-1]) | (cols[1:] != cols[:-1])
    run = np.cumsum(head) - 1
    start = np.flatnonzero(head)
    data = np.zeros(start.size)
    if rows.size:
        at = np.arange(rows.size) - start[run]   # place inside the run
        for t in range(int(at.max()) + 1):       # one term of every run per step: a sequential sum per entry
            sel = at == t
            data[run[sel]] += vals[sel]
    indptr = np.zeros(n + 1, np.int64)
    np.add.at(indptr, rows[head] + 1, 1)
    return sp.csr_matrix((data, cols[head].astype(np.int32), np.cumsum(indptr).astype(np.int32)), shape=(n, n))


def _row_stats_host(A: sp.csr_matrix):
    vc = np.asarray(A.sum(axis=1)).ravel()
    pos = sp.csr_matrix(((A.data > 0).astype(np.int64), A.indices, A.indptr), shape=A.shape)
    return vc, np.asarray(pos.sum(axis=1)).ravel().astype(np.int64)


def _ladder_value(nnz_sorted, q, last):
    cnt = int(nnz_sorted.shape[0])
    v = int(nnz_sorted[min(int(q * cnt), cnt - 1)]) if cnt else 0
    return max(v, last + 1)


def _kr_run_host(A, tol, max_mvp):
    """the listing on one matrix without empty rows; (x, info)"""
    n = A.shape[0]
    mvp = [0]

    def mv(z):
        mvp[0] += 1
        return A @ z

    x = np.ones(n)
    outer, clips = 0, [0, 0]
    with np.errstate(all="ignore"):
        v = x * mv(x)
        rk = 1.0 - v
        rho1 = float(rk @ rk)
        rout = rold = rho1
        eta, stop_tol, rt = KR_ETAMAX, tol * 0.5, tol * tol
        rho2, Z, p = 0.0, None, None
        while rout > rt and mvp[0] < max_mvp:
            outer += 1
            k, y = 0, np.ones(n)
            innertol = max(eta * eta * rout, rt)
            while rho1 > innertol and mvp[0] < max_mvp:
                k += 1
                if k == 1:
                    Z = rk / v
                    p = Z.copy()
                    rho1 = float(rk @ Z)
                else:
                    p = Z + (rho1 / rho2) * p
                w = x * mv(x * p) + v * p
                alpha = rho1 / float(p @ w)
                ap = alpha * p
                ynew = y + ap
                if ynew.min() <= KR_DELTA:
                    sel = ap < 0
                    y = y + np.min((KR_DELTA - y[sel]) / ap[sel], initial=np.inf) * ap
                    clips[0] += 1
                    break
                if ynew.max() >= KR_DELTA_UP:
                    sel = ynew > KR_DELTA_UP
                    y = y + np.min((KR_DELTA_UP - y[sel]) / ap[sel], initial=np.inf) * ap
                    clips[1] += 1
                    break
                y = ynew
                rk = rk - alpha * w
                rho2 = rho1
                Z = rk / v
                rho1 = float(rk @ Z)
            x = x * y
            v = x * mv(x)
            rk = 1.0 - v
            rho1 = float(rk @ rk)
            rout = rho1
            rat = rout / rold
            rold = rout
            eta_o = eta
            eta = KR_G * rat
            if KR_G * eta_o * eta_o > 0.1:
                eta = max(eta, KR_G * eta_o * eta_o)
            eta = max(min(eta, KR_ETAMAX), stop_tol / math.sqrt(rout) if rout > 0 else KR_ETAMAX)
    return x, {"converged": bool(rout <= rt), "residual": math.sqrt(rout) if rout >= 0 else float("nan"), "mvp": mvp[0],
               "outer": outer, "clips": tuple(clips)}


def kr_balance_host(A, tol=1e-6, max_mvp=1000, min_row_nnz=1, kr_retry=True):
    """(x, info): x float64 [n], NaN outside the kept set S; info: converged, residual, mvp, outer, clips (how often the inner
    loop ended on the listing's lower and on its upper bound of y), kept, excluded (non-empty rows outside S), min_row_nnz
    (the value of the run reported), ladder (every value tried), host_syncs (0 here)"""
    A = sp.csr_matrix(A, dtype=np.float64)
    vc, nnz = _row_stats_host(A)
    full = vc > 0
    nnz_sorted = np.sort(nnz[full])
    tried, mrn = [], int(min_row_nnz)
    while True:
        tried.append(mrn)
        keep = full & (nnz >= mrn)
        idx = np.flatnonzero(keep)
        xs, info = _kr_run_host(A[idx][:, idx].tocsr(), float(tol), int(max_mvp))
        x = np.full(A.shape[0], np.nan)
        x[idx] = xs
        info.update(kept=int(idx.size), excluded=int(full.sum() - idx.size), min_row_nnz=mrn, ladder=list(tried), host_syncs=0)
        if info["converged"] or not kr_retry or len(tried) > len(LADDER):
            return x, info
        mrn = _ladder_value(nnz_sorted, LADDER[len(tried) - 1], mrn)


def _vector_from_stats_host(kind, vc):
    with np.errstate(invalid="ignore"):
        out = np.sqrt(vc) if kind == "SQRTVC" else vc.astype(np.float64, copy=True)
    out[~(vc > 0)] = np.nan
    return out


def hic_norm_vector_host(pos1, pos2, count, kind, resolution_bp, n_bins=None, **kr):
    """(vector float64 [n_bins], info) of the module docstring on the host; **kr: tol, max_mvp, min_row_nnz, kr_retry"""
    kind = _kind(kind)
    unknown = set(kr) - set(_KR_DEFAULTS)
    if unknown:
        raise TypeError("unknown argument(s) %s" % ", ".join(sorted(unknown)))
    A = contact_matrix_host(pos1, pos2, count, resolution_bp, n_bins)
    if kind != "KR":
        vc, _ = _row_stats_host(A)
        return _vector_from_stats_host(kind, vc), {"kind": kind}
    x, info = kr_balance_host(A, **{**_KR_DEFAULTS, **kr})
    with np.errstate(divide="ignore", invalid="ignore"):
        return 1.0 / x, info


def resolve_norm_host(pos1, pos2, count, norm, resolution_bp, n_bins=None, norm_args=None):
    """None or a vector: as given; 'KR' / 'VC' / 'SQRTVC': the vector computed from the records (hic_norm_vector_host with
    norm_args), HicNormError for a KR that did not converge"""
    if not isinstance(norm, str):
        return norm
    size = {} if n_bins is None else {"n_bins": n_bins}   # build_hic_graph_host's norm_args may name n_bins themselves
    v, info = hic_norm_vector_host(pos1, pos2, count, norm, resolution_bp, **size, **(norm_args or {}))
    _require_converged(info)
    return v


def clean_norm(norm, n):
    """the norm vector at n bins as a balanced value reads it: NaN, 0 and the bins beyond its length are +inf"""
    nv = np.full(n, np.inf)
    given = np.array(norm, dtype=np.float64).ravel()[:n]
    nv[:given.size] = given
    nv[np.isnan(nv) | (nv == 0.0)] = np.inf
    return nv


def pad_vector(v, n):
    """the vector with NaN bins appended up to n bins (windows beyond the last bin in contact)"""
    if torch.is_tensor(v):
        return v if v.numel() >= n else torch.cat([v, torch.full((n - v.numel(),), float("nan"), dtype=v.dtype, device=v.device)])
    return v if v.shape[0] >= n else np.concatenate([v, np.full(n - v.shape[0], np.nan)])


# ----------------------------------------------------------------------------------------------
# device
# ----------------------------------------------------------------------------------------------
class DeviceContactMatrix:
    """A on the device: rowptr int32 [n + 1], col int32 [nnz], val float64 [nnz], vc float64 [n], row_nnz int32 [n]"""

    def __init__(self, n, nnz, rowptr, col, val, vc, row_nnz):
        self.n, self.nnz, self.rowptr, self.col, self.val, self.vc, self.row_nnz = n, nnz, rowptr, col, val, vc, row_nnz

    def to_host(self) -> sp.csr_matrix:
        return sp.csr_matrix((self.val[:self.nnz].cpu().numpy(), self.col[:self.nnz].cpu().numpy(), self.rowptr.cpu().numpy()),
                             shape=(self.n, self.n))


def aggregate_contacts(pos1, pos2, count, resolution_bp, n_bins=None) -> DeviceContactMatrix:
    """records (device tensors: int32, int32, float64) -> A (cgcn_hicnorm_count, one read-back of the sizes and the
    bad-record flags, cgcn_hicnorm_fill).  The sort key holds row, column and record index: 2 bits(n_bins) + bits(M) + 1 must
    not exceed 64 (250 000 bins with 1.3e8 records fit), else RuntimeError: unsupported shape."""
    from . import _lib
    res, dev, m = int(resolution_bp), pos1.device, int(pos1.numel())
    if res < 1:
        raise ValueError("resolution_bp must be positive")
    given = 0 if n_bins is None else int(n_bins)
    if given < 0:
        raise ValueError("n_bins must not be negative")
    with torch.cuda.device(dev):
        # the bins are counted first: n_bins = 0
        wsp, need = _lib.workspace_for("cgcn_hicnorm_workspace_bytes", dev, "Hi-C norm aggregation, M=%d" % m, M=m, n_bins=0)
        sizes = torch.zeros(4, dtype=torch.int64, device=dev)
        _lib.call("cgcn_hicnorm_count", M=m, pos1=pos1, pos2=pos2, count=count, resolution_bp=res, n_bins=0, workspace=wsp,
                  workspace_bytes=need, sizes=sizes)
        entries, flags, top, _ = sizes.tolist()
        _bad_records(flags)
        n = top if n_bins is None else given
        if n < top:
            raise ValueError("n_bins=%d but the records reach bin %d" % (n, top - 1))
        if entries >= 2 ** 31 - 1 or n >= 2 ** 31 - 1:
            raise ValueError("the contact matrix has %d entries in %d bins: beyond int32" % (entries, n))
        rowptr = torch.zeros(n + 1, dtype=torch.int32, device=dev)
        col = torch.empty(max(entries, 1), dtype=torch.int32, device=dev)
        val = torch.empty(max(entries, 1), dtype=torch.float64, device=dev)
        vc = torch.zeros(n, dtype=torch.float64, device=dev)
        row_nnz = torch.zeros(n, dtype=torch.int32, device=dev)
        if n:
            need = _lib.query("cgcn_hicnorm_workspace_bytes", M=m, n_bins=n)
            if need > wsp.numel():
                wsp = _lib._workspace(need, dev, "Hi-C norm aggregation, M=%d n_bins=%d" % (m, n))
            _lib.call("cgcn_hicnorm_fill", M=m, pos1=pos1, pos2=pos2, count=count, resolution_bp=res, n_bins=n, capacity=entries,
                      workspace=wsp, workspace_bytes=need, rowptr=rowptr, col=col, val=val, vc=vc, row_nnz=row_nnz, sizes=sizes)
    return DeviceContactMatrix(n, entries, rowptr, col, val, vc, row_nnz)


def spmv(A: DeviceContactMatrix, x=None, p=None, mask=None, out=None, long_row_nnz: int = -1) -> torch.Tensor:
    """mask o (A (mask o x o p)) in float64 (cgcn_hicnorm_spmv); long_row_nnz: the route threshold (-1 = the default)"""
    from . import _lib
    y = torch.empty(A.n, dtype=torch.float64, device=A.rowptr.device) if out is None else out
    with torch.cuda.device(A.rowptr.device):
        _lib.call("cgcn_hicnorm_spmv", n=A.n, rowptr=A.rowptr, col=A.col, val=A.val, mask=mask, x=x, p=p, y=y,
                  long_row_nnz=int(long_row_nnz))
    return y


def _kr_run_device(A: DeviceContactMatrix, tol, max_mvp, min_row_nnz, long_row_nnz):
    """one run of the listing at one min_row_nnz: (state, info)"""
    from . import _lib
    n, dev = A.n, A.rowptr.device
    nbytes = _lib.query("cgcn_hicnorm_kr_state_bytes", n=n)
    state = torch.zeros(nbytes // 8, dtype=torch.float64, device=dev)
    ns = (n + 31) & ~31
    vec = lambda k: state[_HDR + k * ns:_HDR + k * ns + n]   # noqa: E731
    m, x, p, w = vec(_V_MASK), vec(_V_X), vec(_V_P), vec(_V_W)
    syncs = [0]

    def step(op, flag=0, parity=0):
        _lib.call("cgcn_hicnorm_kr_step", n=n, op=op, flag=int(flag), parity=parity, vc=A.vc, row_nnz=A.row_nnz, state=state,
                  state_bytes=nbytes)

    def record():
        syncs[0] += 1
        return state[:12].tolist()

    def product(pvec):
        spmv(A, x=x, p=pvec, mask=m, out=w, long_row_nnz=long_row_nnz)

    c, mvp, outer, clips = 0, 1, 0, [0, 0]
    step(_OP_MASK, min_row_nnz, c)
    product(None)
    step(_OP_RES, 0, c)
    rec = record()
    kept, nonempty = int(rec[10]), int(rec[11])
    rho1 = rout = rold = rec[8]
    eta, stop_tol, rt = KR_ETAMAX, tol * 0.5, tol * tol
    while rout > rt and mvp < max_mvp:
        outer += 1
        k = 0
        innertol = max(eta * eta * rout, rt)
        while rho1 > innertol and mvp < max_mvp:
            k += 1
            step(_OP_FIRST if k == 1 else _OP_DIR, 0, c)
            product(p)
            mvp += 1
            step(_OP_W, k > 1, c)
            step(_OP_Y, 0, c)
            rec = record()
            if rec[3] <= KR_DELTA:
                step(_OP_CLIP, 0, c)
                clips[0] += 1
                break
            if rec[4] >= KR_DELTA_UP:
                step(_OP_CLIP, 1, c)
                clips[1] += 1
                break
            c ^= 1   # accepted: ynew, the new rk and Z are the current copies
            rho1 = rec[7]
        product(vec(_V_Y + c))
        mvp += 1
        step(_OP_RES, 1, c)
        rout = rho1 = record()[8]
        rat = rout / rold if rold else 0.0
        rold = rout
        eta_o = eta
        eta = KR_G * rat
        if KR_G * eta_o * eta_o > 0.1:
            eta = max(eta, KR_G * eta_o * eta_o)
        eta = max(min(eta, KR_ETAMAX), stop_tol / math.sqrt(rout) if rout > 0 else KR_ETAMAX)
    info = {"converged": bool(rout <= rt), "residual": math.sqrt(rout) if rout >= 0 else float("nan"), "mvp": mvp, "outer": outer,
            "clips": tuple(clips), "kept": kept, "excluded": nonempty - kept, "min_row_nnz": int(min_row_nnz),
            "host_syncs": syncs[0]}
    return state, info


def kr_balance_device(A: DeviceContactMatrix, tol=1e-6, max_mvp=1000, min_row_nnz=1, kr_retry=True, long_row_nnz=-1):
    """(norm vector float64 [n] on the device: 1 / x on S, NaN elsewhere; info as kr_balance_host's)"""
    from . import _lib
    out = torch.empty(A.n, dtype=torch.float64, device=A.rowptr.device)
    if A.n == 0:
        return out, {"converged": True, "residual": 0.0, "mvp": 0, "outer": 0, "clips": (0, 0), "kept": 0, "excluded": 0,
                     "min_row_nnz": int(min_row_nnz), "ladder": [int(min_row_nnz)], "host_syncs": 0}
    tried, mrn, syncs, ladder = [], int(min_row_nnz), 0, None
    with torch.cuda.device(A.rowptr.device):
        while True:
            tried.append(mrn)
            state, info = _kr_run_device(A, float(tol), int(max_mvp), mrn, int(long_row_nnz))
            syncs += info["host_syncs"]
            if info["converged"] or not kr_retry or len(tried) > len(LADDER):
                break
            if ladder is None:   # the five quantiles at once: one more read-back, on this path only
                srt = torch.sort(A.row_nnz[A.vc > 0]).values
                cnt = int(srt.numel())
                syncs += 1
                ladder = srt[[min(int(q * cnt), cnt - 1) for q in LADDER]].tolist() if cnt else [0] * len(LADDER)
            mrn = max(int(ladder[len(tried) - 1]), mrn + 1)
        info.update(ladder=list(tried), host_syncs=syncs)
        _lib.call("cgcn_hicnorm_vector", n=A.n, kind=2, vc=A.vc, state=state, out=out)
    return out, info


def vector_from_matrix(A: DeviceContactMatrix, kind, long_row_nnz=-1, **kr):
    """(vector, info) of one kind from the aggregated matrix"""
    from . import _lib
    kind = _kind(kind)
    if kind == "KR":
        return kr_balance_device(A, long_row_nnz=long_row_nnz, **{**_KR_DEFAULTS, **kr})
    out = torch.empty(A.n, dtype=torch.float64, device=A.rowptr.device)
    with torch.cuda.device(A.rowptr.device):
        _lib.call("cgcn_hicnorm_vector", n=A.n, kind=1 if kind == "SQRTVC" else 0, vc=A.vc, state=None, out=out)
    return out, {"kind": kind}


def hic_norm_vector(pos1, pos2, count, kind, resolution_bp, n_bins=None, device="cuda", return_info=False, **kr):
    """HicContacts.norm_vector for arrays (or a HicContacts as pos1: nothing is uploaded again)"""
    from .hic import HicContacts
    c = pos1 if isinstance(pos1, HicContacts) else HicContacts(pos1, pos2, count, device)
    return c.norm_vector(kind, resolution_bp, n_bins=n_bins, return_info=return_info, **kr)
