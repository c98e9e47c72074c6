"""Two contact maps compared: the stratum-adjusted correlation coefficient (SCC) of HiCRep (Yang et al. 2017).  Both maps are
smoothed with a box filter, correlated diagonal by diagonal -- so that the distance decay, which every Hi-C map shares, cannot
pass for agreement -- and the strata's correlations are combined with fixed weights.  It answers how alike two cell lines are,
two sources of one cell line (a Juicer dump and HiChIP read pairs), two resolutions of one file, or a map and a control.  The
rule below is this project's definition, after the closed-form weights of HiCRep's Python re-implementation.  No `hicrep`
package exists where this runs, so NOTHING here is compared against HiCRep's own output.  OUT OF SCOPE: HiCRep's `htrain` (the
choice of h) and depth down-sampling, its tie-aware rank variances, a standard error of SCC, genome-wide pooling across
chromosomes, O/E as the compared value.  The smoothing and the sums per stratum run on the device (csrc/cgcn_mapcompare.hip);
the bands and the validity bytes are the shared front end's (hicmap); scc_from_sums is host code that both paths share.

The rule, per chromosome.  Two record sets a and b, one resolution_bp = res; n = max(n_a, n_b) bins unless n_bins says it: the
shorter map is zero beyond its end.  A = hicnorm's contact matrix of a map at res with n bins.
  1. Cell value.  norm = None: the observed count A[i, j] (HiCRep's input).  A norm vector or a name: A[i, j] / (nv[i] * nv[j]),
     nv = hicnorm.clean_norm(norm) (NaN, 0 and the bins beyond the vector read as +inf: the value is 0).  norm is one name for
     both maps -- each vector computed from its own records -- or a pair (one entry per map: None, a name or a vector).  HiCRep
     divides each map by its total first; that is left out: rho does not change when a map is scaled, and the weights do not
     read the values.
  2. Validity.  Bin i is valid iff hicmap.valid_bins holds for it in BOTH maps.  The smoothing reads every cell, valid or not.
  3. Smoothing.  The box SUM of half-width h, 0 <= h <= 20: S[i, d] = sum over da = -h .. h of R_da, R_da = sum over db = -h .. h
     of V(i + da, i + d + db), both plain sequential float64 sums from 0.0 in ascending index order, no fused multiply-add.
     V(p, q) is the value of the cell (min(p, q), max(p, q)) and 0 when p or q is outside [0, n): a cell across the main diagonal
     reads its mirror image, the diagonal cell itself appears once.  The sum, not the mean: (2 h + 1)^2 cancels in rho, and the
     sum is exact on integer counts.  The two levels make a direct sum and a separable one (row sums, then their sum) the same
     bits.  S is kept stratum-major, S[d][i], with a leading dimension ld = n rounded up to even and zeros from i = n - d on.
  4. Strata.  d = min_dist (default 1; 0 is allowed) .. D = min(max_distance_bp // res, n - 1); max_distance_bp = 5 Mb by
     default.  The cell (i, i + d) takes part iff both bins are valid and Sa != 0 or Sb != 0 (HiCRep drops the cells that are
     zero in both maps).
  5. Sums per stratum, in a fixed order.  The rows 0 .. n - d - 1 are cut into chunks of CHUNK = 2048 consecutive rows.  Inside
     a chunk, lane l of 64 adds the rows c0 + l, c0 + l + 64, ... in ascending order from 0.0 (a cell that takes no part adds
     nothing), then the xor butterfly 32 .. 1 (compartments.wave_sum); the stratum's sum is ONE sequential sum, from 0.0, of the
     chunk sums in chunk order.  Pass 1: N (int64), sum x, sum y; the means are sum x / N and sum y / N, one division each.  Pass
     2: sum (x - mx)^2, sum (y - my)^2, sum (x - mx)(y - my), every difference, product and sum rounded on its own.
  6. Scores (scc_from_sums, shared).  rho_d = sxy / sqrt(sxx * syy) if N_d >= 3, sxx > 0 and syy > 0, else NaN.  w_d =
     (N_d + 1) / 12: N_d times the variance (1 + 1 / N_d) / 12 of N_d ranks divided by N_d.  scc = sum w_d rho_d / sum w_d over
     the strata with a finite rho; NaN when there is none.
  7. Guards, ValueError before anything is allocated: h > 20 (or < 0); n (D + 2 h + 1) > 2^28 band elements; two different
     resolutions (resolution_bp given as a pair); min_dist < 0.  Empty record sets and n < 2 are legal: scc is NaN."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

from . import hicmap, hicnorm
from .compartments import wave_sum

CHUNK = 2048
MAX_H, MAX_ELEMS, MAX_DISTANCE_BP = 20, 1 << 28, 5000000
_SUMS = ("sx", "sy", "mx", "my", "sxx", "syy", "sxy")     # the rows of cgcn_mapcmp_sums' stats


class SccRule(NamedTuple):
    """the checked arguments of one comparison (scc_rule)"""
    res: int
    h: int
    min_dist: int
    max_dist: int     # D; -1 for a map without bins

    @property
    def width(self):
        """the raw band's width: the boxes of the stratum D reach 2 h further"""
        return max(self.max_dist, 0) + 2 * self.h + 1


def scc_rule(resolution_bp, n=0, h=5, max_distance_bp=None, min_dist=1) -> SccRule:
    """The rule's arguments, checked (rule 7's guards among them).  resolution_bp: one resolution, or a pair (one per map) that
    must agree.  n: the bins of the compared maps; D = min(max_distance_bp // res, n - 1)."""
    if isinstance(resolution_bp, (tuple, list, np.ndarray)):
        both = [int(r) for r in resolution_bp]
        if len(both) != 2 or both[0] != both[1]:
            raise ValueError("the two maps have different resolutions (%s): bin both at one resolution_bp"
                             % ", ".join(str(r) for r in both))
        resolution_bp = both[0]
    res = int(resolution_bp)
    if res < 1:
        raise ValueError("resolution_bp must be positive")
    h = int(h)
    if h > MAX_H:
        raise ValueError("h=%d: more than %d is not supported" % (h, MAX_H))
    if h < 0:
        raise ValueError("h must not be negative")
    md = int(min_dist)
    if md < 0:
        raise ValueError("min_dist must not be negative")
    reach = int(MAX_DISTANCE_BP if max_distance_bp is None else max_distance_bp) // res
    if reach < 0:
        raise ValueError("max_distance_bp must not be negative")
    n = int(n)
    D = min(reach, n - 1)
    if n * (max(D, 0) + 2 * h + 1) > MAX_ELEMS:
        raise ValueError("%d bins x %d distances are more than 2^28 band elements: take a coarser resolution_bp or a shorter "
                         "max_distance_bp" % (n, D + 2 * h + 1))
    return SccRule(res, h, md, D)


def leading_dim(n) -> int:
    """ld of rule 3: n rounded up to even"""
    return int(n) + (int(n) & 1)


class StratumSums(NamedTuple):
    """rule 5's sums, one entry per stratum 0 .. D: cells int64, the rest float64"""
    cells: np.ndarray
    sx: np.ndarray
    sy: np.ndarray
    mx: np.ndarray
    my: np.ndarray
    sxx: np.ndarray
    syy: np.ndarray
    sxy: np.ndarray


# ----------------------------------------------------------------------------------------------
# shared host functions
# ----------------------------------------------------------------------------------------------
def scc_from_sums(sums: StratumSums):
    """rule 6: (scc float, rho float64 [D + 1], weights float64 [D + 1]) of rule 5's sums"""
    N = np.asarray(sums.cells, dtype=np.int64)
    sxx, syy, sxy = (np.asarray(v, dtype=np.float64) for v in (sums.sxx, sums.syy, sums.sxy))
    ok = (N >= 3) & (sxx > 0) & (syy > 0)
    with np.errstate(all="ignore"):
        rho = np.where(ok, sxy / np.sqrt(np.where(ok, sxx * syy, 1.0)), np.nan)
    weights = (N + 1) / 12.0
    use = np.isfinite(rho)
    num = den = 0.0
    for d in np.nonzero(use)[0]:          # one sequential sum in stratum order
        num += weights[d] * rho[d]
        den += weights[d]
    return (num / den if den > 0 else float("nan")), rho, weights


class MapComparison:
    """The comparison of two maps: scc (float), rho float64 [D + 1] (NaN for a stratum that is not compared), cells int64
    [D + 1] (N_d), weights float64 [D + 1], valid bool [n] (rule 2), sums (StratumSums), rule (an SccRule)."""

    def __init__(self, sums: StratumSums, valid, rule: SccRule):
        self.sums, self.rule = sums, rule
        self.valid = np.asarray(valid, dtype=bool)
        self.cells = np.asarray(sums.cells, dtype=np.int64)
        self.scc, self.rho, self.weights = scc_from_sums(sums)

    @property
    def n_strata(self) -> int:
        """the strata with a finite rho"""
        return int(np.isfinite(self.rho).sum())

    def save(self, path):
        """everything as one .npz: scc, rho, cells, weights, valid, the sums and the rule's fields"""
        r = self.rule
        np.savez(path, scc=self.scc, rho=self.rho, cells=self.cells, weights=self.weights, valid=self.valid,
                 resolution_bp=r.res, h=r.h, min_dist=r.min_dist, max_dist=r.max_dist,
                 **{k: getattr(self.sums, k) for k in _SUMS})


def _empty_sums(D) -> StratumSums:
    L = max(int(D) + 1, 0)
    z = np.zeros(L)
    return StratumSums(np.zeros(L, np.int64), z, z.copy(), np.full(L, np.nan), np.full(L, np.nan), z.copy(), z.copy(), z.copy())


def norm_pair(norm):
    """rule 1's `norm` as (norm of a, norm of b): a pair is one entry per map, anything else serves both"""
    if isinstance(norm, (tuple, list)):
        if len(norm) != 2:
            raise ValueError("norm is None, a name, a vector for both maps, or a pair with one entry per map")
        return norm[0], norm[1]
    return norm, norm


# ----------------------------------------------------------------------------------------------
# host restatement
# ----------------------------------------------------------------------------------------------
def smooth_strata_host(band, norm, h, D) -> np.ndarray:
    """Rules 1 and 3 on the host: S float64 [D + 1, ld] from hicmap.band_host's raw band [n, >= D + 2 h + 1] and norm (None or
    a vector).  The separable form: the row sums tap by tap, then their sum row by row, every addition one vectorised numpy
    addition over all cells, in the rule's order."""
    band = np.asarray(band, dtype=np.float64)
    n, width = band.shape
    h, D = int(h), int(D)
    if not 0 <= h <= MAX_H:
        raise ValueError("h=%d: 0 .. %d are supported" % (h, MAX_H))
    if D < 0 or width < D + 2 * h + 1:
        raise ValueError("the band is %d wide but D=%d and h=%d need %d" % (width, D, h, D + 2 * h + 1))
    ld = leading_dim(n)
    S = np.zeros((D + 1, ld))
    if n == 0:
        return S
    W = D + 2 * h + 1
    e = np.arange(W, dtype=np.int64)[None, :]
    inside = np.arange(n, dtype=np.int64)[:, None] + e < n
    val = np.where(inside, band[:, :W], 0.0)
    if norm is not None:
        nv = hicnorm.clean_norm(norm, n)
        nq = np.lib.stride_tricks.sliding_window_view(np.concatenate([nv, np.ones(W)]), W)[:n]
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            val = np.where(inside, band[:, :W] / (nv[:, None] * nq), 0.0)
    # Vs[p + h, e + 2 h] = V(p, p + e) for p = -h .. n + h - 1 and e = -2 h .. D + 2 h
    Vs = np.zeros((n + 2 * h, D + 4 * h + 1))
    Vs[h:h + n, 2 * h:] = val
    for k in range(1, 2 * h + 1):           # below the diagonal: V(p, p - k) is the cell (p - k, p)
        if k < n:
            Vs[h + k:h + n, 2 * h - k] = val[:n - k, k]
    with np.errstate(over="ignore", invalid="ignore"):
        R = np.zeros((n + 2 * h, D + 2 * h + 1))            # R[p + h, e + h] = sum_db V(p, p + e + db), e = -h .. D + h
        for t in range(2 * h + 1):
            R = R + Vs[:, t:t + D + 2 * h + 1]
        out = np.zeros((n, D + 1))
        for t in range(2 * h + 1):                          # da = t - h: the row i + da at the distance d - da
            out = out + R[t:t + n, 2 * h - t:2 * h - t + D + 1]
    out = np.where(np.arange(n)[:, None] + np.arange(D + 1)[None, :] < n, out, 0.0)
    S[:, :n] = out.T
    return S


def stratum_sums_host(Sa, Sb, valid, n, min_dist=1) -> StratumSums:
    """Rules 4 and 5 on the host from two arrays of smoothed strata [D + 1, >= n] and the validity of the n bins"""
    Sa, Sb = np.asarray(Sa, dtype=np.float64), np.asarray(Sb, dtype=np.float64)
    valid = np.asarray(valid, dtype=bool).ravel()
    n, md = int(n), int(min_dist)
    if Sa.shape != Sb.shape or Sa.ndim != 2 or Sa.shape[1] < n or valid.size != n:
        raise ValueError("the strata must be two arrays [D + 1, >= n] of one shape, with one validity entry per bin")
    L = Sa.shape[0]
    nc = max((n + CHUNK - 1) // CHUNK, 1)
    x, y, part = np.zeros((L, nc * CHUNK)), np.zeros((L, nc * CHUNK)), np.zeros((L, nc * CHUNK), bool)
    for d in range(min(L, n)):
        rows = n - d
        x[d, :rows], y[d, :rows] = Sa[d, :rows], Sb[d, :rows]
        if d >= md:
            part[d, :rows] = valid[:rows] & valid[d:] & ((Sa[d, :rows] != 0) | (Sb[d, :rows] != 0))

    def total(T):
        """the masked terms summed per stratum: wave_sum per chunk, then the chunks in order"""
        P = wave_sum(np.where(part, T, 0.0).reshape(L * nc, CHUNK)).reshape(L, nc)
        s = np.zeros(L)
        for c in range(nc):
            s = s + P[:, c]
        return s

    cells = part.sum(axis=1).astype(np.int64)
    with np.errstate(all="ignore"):
        sx, sy = total(x), total(y)
        mx, my = sx / cells.astype(np.float64), sy / cells.astype(np.float64)
        dx, dy = x - mx[:, None], y - my[:, None]
        sxx, syy, sxy = total(dx * dx), total(dy * dy), total(dx * dy)
    return StratumSums(cells, sx, sy, mx, my, sxx, syy, sxy)


def _records(r):
    """(pos1, pos2, count) of a record set: a triple, or anything with these three attributes (hiccache.HostContacts)"""
    if isinstance(r, (tuple, list)):
        if len(r) != 3:
            raise ValueError("a record set is (pos1, pos2, count)")
        return r[0], r[1], r[2]
    return r.pos1, r.pos2, r.count


def map_scc_host(records_a, records_b, norm=None, resolution_bp=40000, h=5, max_distance_bp=MAX_DISTANCE_BP, min_dist=1,
                 n_bins=None, norm_args=None):
    """The whole rule on the host from the records of the two maps ((pos1, pos2, count) each).  norm: None, 'KR' / 'VC' /
    'SQRTVC' (each map's vector from its own records, with norm_args), a vector for both, or a pair.  h: one half-width (a
    MapComparison) or a sequence (a list, one per value; the matrices, bands and validity are formed once)."""
    many = isinstance(h, (tuple, list, np.ndarray))
    hs = [int(v) for v in h] if many else [int(h)]
    for v in hs:
        scc_rule(resolution_bp, 0, v, max_distance_bp, min_dist)
    res = scc_rule(resolution_bp, 0, hs[0] if hs else 0, max_distance_bp, min_dist).res
    recs = [_records(records_a), _records(records_b)]
    if n_bins is None:     # the bins of the longer map: its largest position's bin + 1 (matrix_host checks the records below)
        tops = [max(np.max(p1, initial=-1), np.max(p2, initial=-1)) for p1, p2 in ((np.asarray(r[0]), np.asarray(r[1])) for r in recs)]
        n = max(int(t) // res + 1 if t >= 0 else 0 for t in tops)
    else:
        n = int(n_bins)
    rules = [scc_rule(res, n, v, max_distance_bp, min_dist) for v in hs]      # the size guard, before the bands are formed
    mats = [hicmap.matrix_host(*r, res, n) for r in recs]
    norms = [hicnorm.resolve_norm_host(*r, nm, res, n, norm_args) for r, nm in zip(recs, norm_pair(norm))]
    valid = hicmap.valid_bins(mats[0][1], norms[0]) & hicmap.valid_bins(mats[1][1], norms[1]) if n else np.zeros(0, bool)
    out = []
    width = max([r.width for r in rules] or [1])
    bands = [hicmap.band_host(A, width) for A, _ in mats] if n else None
    for r in rules:
        if n == 0:
            out.append(MapComparison(_empty_sums(r.max_dist), valid, r))
            continue
        Sa, Sb = (smooth_strata_host(b, nv, r.h, r.max_dist) for b, nv in zip(bands, norms))
        out.append(MapComparison(stratum_sums_host(Sa, Sb, valid, n, r.min_dist), valid, r))
    return out if many else out[0]


# ----------------------------------------------------------------------------------------------
# device
# ----------------------------------------------------------------------------------------------
def smooth_strata(band, norm, h, D) -> torch.Tensor:
    """rules 1 and 3 on the device (cgcn_mapcmp_smooth: enqueue only): S float64 [D + 1, ld] from hicmap.device_band's raw band
    (at least D + 2 h + 1 wide) and norm, None or a float64 device vector"""
    from . import _lib
    h, D = int(h), int(D)
    if not 0 <= h <= MAX_H:
        raise ValueError("h=%d: 0 .. %d are supported" % (h, MAX_H))
    if D < 0:
        raise ValueError("D must not be negative")
    dev = band.device
    n, width = hicmap.check_band(band, None, D + 2 * h + 1)
    norm = hicmap.device_vector(norm, dev, "norm", optional=True)
    ld = leading_dim(n)
    if (D + 1) * (ld + 1) > MAX_ELEMS:
        raise ValueError("%d strata x %d bins are more than 2^28 elements" % (D + 1, ld))
    S = torch.empty(D + 1, ld, dtype=torch.float64, device=dev)
    if n:
        with torch.cuda.device(dev):
            _lib.call("cgcn_mapcmp_smooth", n=n, D=D, h=h, width=width, band=band, norm=norm,
                      n_norm=0 if norm is None else int(norm.numel()), ld=ld, S=S)
    return S


def valid_bins_device(vc, norm) -> torch.Tensor:
    """hicmap.valid_bins on the device: bool [n] from the row sums and the norm vector (or None), torch plumbing"""
    ok = vc > 0
    if norm is not None:
        n, m = int(vc.numel()), int(norm.numel())
        nv = norm[:n] if m >= n else torch.cat([norm, torch.full((n - m,), float("nan"), dtype=norm.dtype, device=norm.device)])
        ok = ok & torch.isfinite(nv) & (nv != 0)
    return ok


def stratum_sums_device(Sa, Sb, valid, n, min_dist=1):
    """rules 4 and 5 on the device, not read back: (cells int64 [D + 1], stats float64 [7, D + 1] in _SUMS' order).  Pass 1,
    its fold (which leaves the means on the device), pass 2 and its fold are enqueued back to back: no host read in between."""
    from . import _lib
    dev = Sa.device
    n = int(n)
    for S in (Sa, Sb):
        if not (torch.is_tensor(S) and S.dtype == torch.float64 and S.is_contiguous() and S.ndim == 2 and S.device == dev):
            raise ValueError("the strata must be contiguous float64 [D + 1, ld] tensors on one device")
    if Sa.shape != Sb.shape or int(Sa.shape[1]) < n or int(Sa.shape[0]) < 1:
        raise ValueError("the strata must be two tensors [D + 1, >= n] of one shape")
    if not (torch.is_tensor(valid) and valid.device == dev and valid.numel() == n and valid.dtype in (torch.bool, torch.uint8)):
        raise ValueError("valid must be a bool or uint8 device vector with one entry per bin")
    if int(min_dist) < 0:
        raise ValueError("min_dist must not be negative")
    D, ld = int(Sa.shape[0]) - 1, int(Sa.shape[1])
    v8 = valid.to(torch.uint8).contiguous()
    cells = torch.zeros(D + 1, dtype=torch.int64, device=dev)
    stats = torch.zeros(len(_SUMS), D + 1, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        wsp, need = _lib.workspace_for("cgcn_mapcmp_workspace_bytes", dev, "map comparison, n=%d D=%d" % (n, D), n=n, D=D)
        for pass_no in (1, 2):
            _lib.call("cgcn_mapcmp_sums", n=n, D=D, ld=ld, Sa=Sa, Sb=Sb, valid=v8, min_dist=int(min_dist), pass_no=pass_no,
                      workspace=wsp, workspace_bytes=need, cells=cells, stats=stats)
    return cells, stats


def _sums_of(cells, stats) -> StratumSums:
    """the one read-back of a comparison: cells and stats as a StratumSums"""
    L = int(cells.numel())
    back = torch.cat([cells.to(torch.float64).view(1, L), stats]).cpu().numpy()   # N <= 2^28: exact as float64
    return StratumSums(back[0].astype(np.int64), *(back[1 + k].copy() for k in range(len(_SUMS))))


def stratum_sums(Sa, Sb, valid, n, min_dist=1) -> StratumSums:
    """stratum_sums_device and its read-back (one)"""
    return _sums_of(*stratum_sums_device(Sa, Sb, valid, n, min_dist))


def scc_of_matrices(A, B, norm_a, norm_b, rules):
    """Rules 1 to 6 from two device matrices (hicnorm.DeviceContactMatrix) of one size: hicmap.device_band and the validity
    bytes once, then smooth_strata and stratum_sums per rule of `rules` (SccRules that differ in h alone), one read-back each.
    norm_a, norm_b: None or float64 device vectors.  A list of MapComparison."""
    if A.n != B.n:
        raise ValueError("the two matrices have %d and %d bins: aggregate both at n_bins = the larger" % (A.n, B.n))
    n, rules = A.n, list(rules)
    valid = valid_bins_device(A.vc, norm_a) & valid_bins_device(B.vc, norm_b)
    valid_host = valid.cpu().numpy()
    if n == 0:
        return [MapComparison(_empty_sums(r.max_dist), valid_host, r) for r in rules]
    width = max([r.width for r in rules] or [1])
    band_a, band_b = hicmap.device_band(A, width), hicmap.device_band(B, width)
    out = []
    for r in rules:
        Sa, Sb = smooth_strata(band_a, norm_a, r.h, r.max_dist), smooth_strata(band_b, norm_b, r.h, r.max_dist)
        out.append(MapComparison(stratum_sums(Sa, Sb, valid, n, r.min_dist), valid_host, r))
    return out


def map_scc(a, b, **kw):
    """a.scc(b, **kw) of two hic.HicContacts: the device path of map_scc_host"""
    return a.scc(b, **kw)


# ----------------------------------------------------------------------------------------------
# graphs
# ----------------------------------------------------------------------------------------------
def graph_edge_overlap(graph_a, graph_b, groups=None) -> dict:
    """The stored entries of two graphs over the same windows (hicmap.csr_of's inputs), as sets of (row, column): {shared,
    only_a, only_b (ints), jaccard = shared / (shared + only_a + only_b), NaN for two empty graphs}.  groups: ascending
    window distances e[0] < e[1] < ... as pileup.distance_groups takes them; the result then also holds `by_group`, the same
    four keys as arrays [len(groups) - 1], entry g over the entries with e[g] <= |column - row| < e[g + 1].  ValueError for
    graphs of different window counts."""
    n = hicmap.csr_of(graph_a)[0].size - 1
    ra, ca, _ = hicmap.edge_rows(graph_a, n, "the first graph")
    rb, cb, _ = hicmap.edge_rows(graph_b, n, "the first graph")
    ka, kb = np.unique(ra * n + ca), np.unique(rb * n + cb)
    both = np.intersect1d(ka, kb, assume_unique=True)

    def counts(sel_a, sel_b, sel_s):
        s, oa, ob = int(sel_s), int(sel_a) - int(sel_s), int(sel_b) - int(sel_s)
        return s, oa, ob, (s / (s + oa + ob) if s + oa + ob else float("nan"))

    s, oa, ob, j = counts(ka.size, kb.size, both.size)
    out = {"shared": s, "only_a": oa, "only_b": ob, "jaccard": j}
    if groups is not None:
        edges = np.asarray(groups, dtype=np.int64).ravel()
        if edges.size < 2 or np.any(np.diff(edges) <= 0):
            raise ValueError("groups must be at least two ascending window distances")
        G = edges.size - 1

        def per_group(k):
            d = np.abs(k % max(n, 1) - k // max(n, 1))
            g = np.searchsorted(edges, d, side="right") - 1
            return np.bincount(g[(g >= 0) & (g < G)], minlength=G)[:G]

        rows = [counts(a, b, c) for a, b, c in zip(per_group(ka), per_group(kb), per_group(both))]
        out["by_group"] = {"shared": np.array([r[0] for r in rows], np.int64), "only_a": np.array([r[1] for r in rows], np.int64),
                           "only_b": np.array([r[2] for r in rows], np.int64),
                           "jaccard": np.array([r[3] for r in rows], np.float64)}
    return out
