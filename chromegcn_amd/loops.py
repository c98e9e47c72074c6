"""Chromatin loops of one chromosome's Hi-C contact matrix -- pixels enriched over their LOCAL background -- and the loop
restriction of the top-K contact graph.  The top-K graph is a cut on a global score and cannot tell a focal contact from a
generally dense neighbourhood; the reference's HiChIP source (data/eqtl_data/HiChIP.py) is a loop assay.  The rule below is
this project's definition, after HiCCUPS (Rao et al. 2014): the four local neighbourhoods, the lambda chunks, the Poisson FDR
thresholds per chunk, the published ratio filters and greedy centroid clustering.  OUT OF SCOPE: HiCCUPS's adaptive widening
of the window where the neighbourhood is sparse, and its merge of the calls of several resolutions; one (p, w) at one
resolution is called.  The stencil runs on the device (csrc/cgcn_loops.hip); everything behind the histograms and behind the
enriched pixels is host code that the device path and the numpy restatement share (loop_thresholds, loops_from_pixels), as
insulation.insulation_from_sums is shared.

The rule, per chromosome.  res = resolution_bp (default 10 000); A = hicnorm's contact matrix at res (n bins); nv =
hicnorm.clean_norm(norm), norm None, a vector, or 'KR' / 'VC' / 'SQRTVC' (default 'VC'); ex = a per-distance expected vector
for the same norm (expected = "auto": HicContacts.expected_vector(norm, res), on the host its restatement in the device's
summation order, hicmap.resolve_host; or an explicit
float64 vector, which reads as 0 beyond its length and must reach min(n, D + 1) entries); p the peak half-width and w the window
half-width, 0 <= p < w <= 10, by default (4, 7) at 5 kb, (2, 5) at 10 kb, (1, 3) at 25 kb (any other resolution needs them
given); D = max_distance_bp // res, max_distance_bp = 2 Mb by default: a convention, not a measurement.
  1. Balanced value.  B[a, b] = A[a, b] / (nv[a] * nv[b]): insulation's rule 1.  valid = hicmap.valid_bins(VC, norm), VC
     the matrix's row sums.
  2. Cells.  A cell (a, b) takes part iff 0 <= a, b < n, b - a >= ignore_diags (default 2) and both bins are valid.
  3. Neighbourhoods of pixel (i, j), j = i + d; offsets (da, db) listed row-major, da ascending, then db ascending.
       donut:      |da|, |db| <= w, without the box |da| <= p and |db| <= p, without da == 0 and without db == 0
       lower-left: 1 <= da <= w, -w <= db <= -1, without da <= p and db >= -p
       horizontal: |da| <= 1, p < |db| <= w
       vertical:   p < |da| <= w, |db| <= 1
     Full sizes 4 (w^2 - p^2), w^2 - p^2, 6 (w - p), 6 (w - p): 32 / 8 / 12 / 12 at (1, 3).
  4. Sums.  S_x = the sum of B[i + da, j + db], T_x = the sum of ex[(j + db) - (i + da)] over the cells of neighbourhood x
     that take part: each ONE plain sequential float64 sum in the listed order, from 0.0; a cell that takes no part adds
     nothing.  C_x = the number of cells that take part.
  5. Candidates.  A pixel is a candidate iff both its bins are valid, min_dist <= d <= D (min_dist = p + ignore_diags + 1 by
     default) and, for all four x, T_x > 0 and 2 C_x >= the full size of x.
  6. Local expected, in raw counts.  lambda_x = ((S_x / T_x) * ex[d]) * (nv[i] * nv[j]), in exactly this order; NaN off the
     candidates.  Without a norm the last factor is 1.
  7. Chunks.  t_m = 2^(m / 3), m = 0 .. K - 2, K = 40, computed once on the host in float64 (chunk_boundaries) and uploaded;
     k_x = the number of t_m <= lambda_x = np.searchsorted(t, lambda_x, 'right') (K - 1 for a NaN).  The device compares
     against the table and takes no logarithm.
  8. Histograms.  o = min(rint(A[i, j]), W - 1), W = max_count + 1 = 10 001 by default; hist[x, k_x, o] += 1 over the
     candidates, int32 [4, K, W].  Pixels with a count of zero are included.
  9. Thresholds (loop_thresholds, shared).  For chunk k the upper lambda is t_min(k, K - 2); N_k the pixels of the chunk;
     exp_tail[o] = N_k * scipy.stats.poisson.sf(o - 1, lambda); obs_tail[o] = the pixels of the chunk with a count >= o;
     thr[x, k] = the least o with obs_tail > 0 and exp_tail <= fdr * obs_tail, W when there is none.  fdr = 0.1 by default.
 10. Enriched pixels.  A candidate with o >= thr[x, k_x] for all four x; the list (i, j, A[i, j], lambda_donut, lambda_ll,
     lambda_h, lambda_v) in ascending (i, j).
 11. Filters and clusters (loops_from_pixels, shared).  Keep a pixel iff A > 1.75 lambda_donut, A > 1.75 lambda_ll,
     A > 1.5 lambda_h and A > 1.5 lambda_v (HiCCUPS's published ratios; `ratios`).  Sort by A descending, stable on the (i, j)
     order.  Greedy clusters: the first unused pixel is the peak; absorb, in sorted order, any unused pixel whose Chebyshev
     distance to the running centroid (the mean of the members' bins) is <= radius_bins = max(1, cluster_radius_bp // res)
     (default 20 kb), updating the centroid after each absorption; rescan until a scan adds nothing.  A loop is the peak
     (i, j), the centroid, radius (the largest Chebyshev distance of a member from the final centroid), n_pixels, observed
     (A at the peak), the four lambda and the four k of the peak.  Clusters below min_cluster_pixels (default 1) are dropped.
 12. Loop-restricted graphs.  With loops = (loops, pad_bins), a source record takes part in the top-K build iff
     (pos1 // res, pos2 // res), lower bin first and res the loops' resolution, lies within Chebyshev distance pad_bins
     (default 1) of some loop's peak and inside the matrix (both bins < n).  The test is on the source record, before any
     window_bp expansion, as in insulation's rule 7; norm and expected vectors still come from ALL records; the kept records
     stay in file order; together with domains both tests must hold; loops = None is bit for bit what it was.
 13. Size guards, ValueError before anything is allocated: n (D + 1) > 2^28 band elements (take a larger resolution_bp or a
     smaller max_distance_bp); w > 10; K > 64; W > 65 536."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

from . import hicmap, hicnorm
from .hicmap import band_host, device_band as loop_band  # noqa: F401  (the tests of the commit before the move call them here)

NAMES = ("donut", "lower_left", "horizontal", "vertical")
N_CHUNKS, MAX_COUNT, FDR = 40, 10000, 0.1
MAX_DISTANCE_BP, CLUSTER_RADIUS_BP, IGNORE_DIAGS = 2000000, 20000, 2
RATIOS = (1.75, 1.75, 1.5, 1.5)
DEFAULT_PW = {5000: (4, 7), 10000: (2, 5), 25000: (1, 3)}
MAX_W, MAX_CHUNKS, MAX_W_COUNTS, MAX_PIXELS = 10, 64, 65536, 1 << 28
_KEY = 1 << 32   # footprint key = lower bin * 2^32 + upper bin
_RULE = ("p", "w", "max_distance_bp", "ignore_diags", "min_dist", "fdr", "max_count", "n_chunks", "ratios", "cluster_radius_bp",
         "min_cluster_pixels")


class LoopRule(NamedTuple):
    """the checked arguments of one call (loop_rule)"""
    res: int
    p: int
    w: int
    D: int
    ignore_diags: int
    min_dist: int
    fdr: float
    W: int
    K: int
    ratios: tuple
    radius_bins: int
    min_cluster_pixels: int

    @property
    def width(self):
        """the band's width: the neighbourhoods of the pixels at distance D reach 2 w further"""
        return self.D + 2 * self.w + 1


def _check_pw(p, w, ignore_diags, min_dist):
    p, w, ig = int(p), int(w), int(ignore_diags)
    if w > MAX_W:
        raise ValueError("w=%d: more than %d is not supported" % (w, MAX_W))
    if not 0 <= p < w:
        raise ValueError("the half-widths need 0 <= p < w, not p=%d w=%d" % (p, w))
    if ig < 0:
        raise ValueError("ignore_diags must not be negative")
    md = p + ig + 1 if min_dist is None else int(min_dist)
    if md < 0:
        raise ValueError("min_dist must not be negative")
    return p, w, ig, md


def loop_rule(resolution_bp, n=0, **rule) -> LoopRule:
    """The rule's arguments, checked (rule 13's guards among them): p, w, max_distance_bp, ignore_diags, min_dist, fdr,
    max_count, n_chunks, ratios, cluster_radius_bp, min_cluster_pixels."""
    unknown = set(rule) - set(_RULE)
    if unknown:
        raise TypeError("unknown argument(s) %s" % ", ".join(sorted(unknown)))
    res = int(resolution_bp)
    if res < 1:
        raise ValueError("resolution_bp must be positive")
    p, w = rule.get("p"), rule.get("w")
    if p is None or w is None:
        if res not in DEFAULT_PW:
            raise ValueError("resolution_bp=%d has no default half-widths (those are for %s): give p and w"
                             % (res, ", ".join(map(str, sorted(DEFAULT_PW)))))
        p, w = DEFAULT_PW[res][0] if p is None else p, DEFAULT_PW[res][1] if w is None else w
    p, w, ig, md = _check_pw(p, w, rule.get("ignore_diags", IGNORE_DIAGS), rule.get("min_dist"))
    D = int(rule.get("max_distance_bp", MAX_DISTANCE_BP)) // res
    if D < 0:
        raise ValueError("max_distance_bp must not be negative")
    K, W = int(rule.get("n_chunks", N_CHUNKS)), int(rule.get("max_count", MAX_COUNT)) + 1
    if K > MAX_CHUNKS or K < 2:
        raise ValueError("n_chunks=%d is outside [2, %d]" % (K, MAX_CHUNKS))
    if W > MAX_W_COUNTS or W < 1:
        raise ValueError("max_count + 1 = %d is outside [1, %d]" % (W, MAX_W_COUNTS))
    if int(n) * (D + 1) > MAX_PIXELS:
        raise ValueError("%d bins x %d distances are more than 2^28 band elements: take a larger resolution_bp or a smaller "
                         "max_distance_bp" % (int(n), D + 1))
    fdr = float(rule.get("fdr", FDR))
    if not 0.0 < fdr <= 1.0:
        raise ValueError("fdr must lie in (0, 1]")
    ratios = tuple(float(r) for r in rule.get("ratios", RATIOS))
    if len(ratios) != 4:
        raise ValueError("ratios are four numbers: donut, lower-left, horizontal, vertical")
    radius = max(1, int(rule.get("cluster_radius_bp", CLUSTER_RADIUS_BP)) // res)
    return LoopRule(res, p, w, D, ig, md, fdr, W, K, ratios, radius, int(rule.get("min_cluster_pixels", 1)))


# ----------------------------------------------------------------------------------------------
# shared host functions
# ----------------------------------------------------------------------------------------------
def neighbourhood_offsets(p, w):
    """rule 3: four int64 arrays [size, 2] of (da, db) in the listed order: donut, lower-left, horizontal, vertical"""
    p, w, _, _ = _check_pw(p, w, 0, 0)
    box = [(da, db) for da in range(-w, w + 1) for db in range(-w, w + 1)]
    inner = lambda da, db: abs(da) <= p and abs(db) <= p   # noqa: E731
    lists = ([o for o in box if not inner(*o) and o[0] != 0 and o[1] != 0],
             [o for o in box if o[0] >= 1 and o[1] <= -1 and not (o[0] <= p and o[1] >= -p)],
             [o for o in box if abs(o[0]) <= 1 and p < abs(o[1])],
             [o for o in box if p < abs(o[0]) and abs(o[1]) <= 1])
    return tuple(np.asarray(x, dtype=np.int64).reshape(-1, 2) for x in lists)


def chunk_boundaries(n_chunks=N_CHUNKS) -> np.ndarray:
    """rule 7: t_m = 2^(m / 3), m = 0 .. n_chunks - 2, float64"""
    return np.power(2.0, np.arange(int(n_chunks) - 1, dtype=np.float64) / 3.0)


def loop_thresholds(hist, fdr=FDR, bounds=None) -> np.ndarray:
    """rule 9: thr int32 [4, K] from the histograms int [4, K, W]"""
    from scipy.stats import poisson
    hist = np.asarray(hist)
    X, K, W = hist.shape
    t = chunk_boundaries(K) if bounds is None else np.asarray(bounds, dtype=np.float64)
    if t.size != K - 1:
        raise ValueError("%d chunks need %d boundaries, not %d" % (K, K - 1, t.size))
    thr = np.full((X, K), W, dtype=np.int32)
    o = np.arange(W)
    for x in range(X):
        for k in range(K):
            h = hist[x, k].astype(np.int64)
            total = int(h.sum())
            if total == 0:
                continue
            obs_tail = np.cumsum(h[::-1])[::-1]
            exp_tail = total * poisson.sf(o - 1, t[min(k, K - 2)])
            ok = (obs_tail > 0) & (exp_tail <= float(fdr) * obs_tail)
            if ok.any():
                thr[x, k] = int(np.argmax(ok))
    return thr


class Pixels(NamedTuple):
    """rule 10's list: i, j int64 [m], observed float64 [m], lam float64 [m, 4]"""
    i: np.ndarray
    j: np.ndarray
    observed: np.ndarray
    lam: np.ndarray


class Loops:
    """The loops of one chromosome: peak_i, peak_j int64 [L] (bins of resolution_bp, i < j), centroid float64 [L, 2], radius
    float64 [L], n_pixels int64 [L], observed float64 [L], lam float64 [L, 4] and k int64 [L, 4] (donut, lower-left,
    horizontal, vertical), n the bins of the matrix, info: candidates, enriched, kept_after_ratios, thresholds, host_syncs."""

    def __init__(self, resolution_bp, n, peak_i, peak_j, centroid, radius, n_pixels, observed, lam, k, info=None):
        self.resolution_bp, self.n = int(resolution_bp), int(n)
        self.peak_i, self.peak_j, self.centroid, self.radius = peak_i, peak_j, centroid, radius
        self.n_pixels, self.observed, self.lam, self.k = n_pixels, observed, lam, k
        self.info = dict(info or {})

    def __len__(self):
        return int(self.peak_i.size)

    def to_bedpe(self, chrom) -> str:
        """one BEDPE line per loop: the two peak bins, then observed, the four lambda, the centroid, radius and n_pixels"""
        res, out = self.resolution_bp, []
        for q in range(len(self)):
            i, j = int(self.peak_i[q]), int(self.peak_j[q])
            out.append("\t".join([str(chrom), str(i * res), str((i + 1) * res), str(chrom), str(j * res), str((j + 1) * res),
                                  "%.10g" % self.observed[q]] + ["%.10g" % v for v in self.lam[q]]
                                 + ["%.10g" % (self.centroid[q, 0] * res), "%.10g" % (self.centroid[q, 1] * res),
                                    "%.10g" % (self.radius[q] * res), str(int(self.n_pixels[q]))]))
        return "".join(line + "\n" for line in out)

    def anchors(self) -> np.ndarray:
        """the bins that are an end of some loop, ascending"""
        return np.unique(np.concatenate([self.peak_i, self.peak_j]).astype(np.int64))

    def footprint_keys(self, pad_bins=1) -> np.ndarray:
        """rule 12's footprints as sorted int64 keys a * 2^32 + b, a <= b: the pixels within Chebyshev distance pad_bins of a
        peak, inside the matrix"""
        pad = int(pad_bins)
        if pad < 0:
            raise ValueError("pad_bins must not be negative")
        o = np.arange(-pad, pad + 1, dtype=np.int64)
        a = (self.peak_i.astype(np.int64)[:, None, None] + o[None, :, None] + 0 * o[None, None, :]).ravel()
        b = (self.peak_j.astype(np.int64)[:, None, None] + 0 * o[None, :, None] + o[None, None, :]).ravel()
        ok = (a >= 0) & (b < self.n) & (a <= b)
        return np.unique(a[ok] * _KEY + b[ok])


def loops_from_pixels(pix: Pixels, resolution_bp, n, ratios=RATIOS, cluster_radius_bp=CLUSTER_RADIUS_BP, min_cluster_pixels=1,
                      bounds=None, info=None) -> Loops:
    """rule 11: the ratio filters and the greedy centroid clusters of the enriched pixels"""
    res = int(resolution_bp)
    radius = max(1, int(cluster_radius_bp) // res)
    t = chunk_boundaries() if bounds is None else np.asarray(bounds, dtype=np.float64)
    pi, pj = np.asarray(pix.i, dtype=np.int64), np.asarray(pix.j, dtype=np.int64)
    obs, lam = np.asarray(pix.observed, dtype=np.float64), np.asarray(pix.lam, dtype=np.float64).reshape(-1, 4)
    with np.errstate(invalid="ignore"):
        keep = np.ones(pi.size, bool)
        for x in range(4):
            keep &= obs > float(ratios[x]) * lam[:, x]
    pi, pj, obs, lam = pi[keep], pj[keep], obs[keep], lam[keep]
    order = np.argsort(-obs, kind="stable")
    pi, pj, obs, lam = pi[order], pj[order], obs[order], lam[order]
    fi, fj = pi.astype(np.float64), pj.astype(np.float64)
    unused = np.ones(pi.size, bool)
    peaks, cents, radii, sizes = [], [], [], []
    for s in range(pi.size):
        if not unused[s]:
            continue
        unused[s] = False
        members = [s]
        ci, cj = fi[s], fj[s]
        added = True
        while added:
            added, at = False, 0
            while True:
                near = unused[at:] & (np.maximum(np.abs(fi[at:] - ci), np.abs(fj[at:] - cj)) <= radius)
                if not near.any():
                    break
                q = at + int(np.argmax(near))
                unused[q] = False
                members.append(q)
                ci, cj = float(np.mean(fi[members])), float(np.mean(fj[members]))
                added, at = True, q + 1
        if len(members) >= int(min_cluster_pixels):
            m = np.asarray(members)
            peaks.append(s)
            cents.append((ci, cj))
            radii.append(float(np.max(np.maximum(np.abs(fi[m] - ci), np.abs(fj[m] - cj)))))
            sizes.append(len(members))
    pk = np.asarray(peaks, dtype=np.int64)
    out_info = dict(info or {})
    out_info["kept_after_ratios"] = int(keep.sum())
    return Loops(res, n, pi[pk], pj[pk], np.asarray(cents, dtype=np.float64).reshape(-1, 2), np.asarray(radii, dtype=np.float64),
                 np.asarray(sizes, dtype=np.int64), obs[pk], lam[pk].reshape(-1, 4),
                 np.searchsorted(t, lam[pk].reshape(-1, 4), side="right").astype(np.int64), out_info)


# ----------------------------------------------------------------------------------------------
# host restatement of the stencil: band-shaped [n, D + 1], vectorised over pixels, sequential over offsets
# ----------------------------------------------------------------------------------------------
def loop_lambdas_host(band, vc, norm, ex, p, w, D, ignore_diags=IGNORE_DIAGS, min_dist=None):
    """Rules 1 to 6 on the band: (lam float64 [4, n, D + 1], NaN off the candidates; candidate bool [n, D + 1]).  band is
    hicmap.band_host's with a width of at least D + 2 w + 1, vc the matrix's row sums, norm None or a vector, ex the expected vector."""
    band = np.asarray(band, dtype=np.float64)
    n, width = band.shape
    p, w, ig, md = _check_pw(p, w, ignore_diags, min_dist)
    D = int(D)
    if D < 0 or width < D + 2 * w + 1:
        raise ValueError("the band is %d wide but D=%d and w=%d need %d" % (width, D, w, D + 2 * w + 1))
    valid, nv = hicmap.bins_of_band_host(vc, norm, n)
    exv = hicmap.expected_at_host(ex, n, D + 2 * w + 1, D + 1, "pixels")
    lam, cand = np.full((4, n, D + 1), np.nan), np.zeros((n, D + 1), bool)
    if n == 0:
        return lam, cand
    # the padded planes: rows a = -w .. n + w - 1, distances dd = -2 w .. D + 2 w
    a, dd = np.arange(-w, n + w, dtype=np.int64)[:, None], np.arange(-2 * w, D + 2 * w + 1, dtype=np.int64)[None, :]
    b = a + dd
    inside = (a >= 0) & (a < n) & (b < n) & (dd >= ig)
    ac, bc, dc = np.clip(a, 0, n - 1), np.clip(b, 0, n - 1), np.clip(dd, 0, width - 1)
    part = inside & valid[ac] & valid[bc]
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        B = np.where(part, band[ac, dc] / (nv[ac] * nv[bc]), 0.0)
    E = np.where(part, exv[dc], 0.0)
    i, d = np.arange(n, dtype=np.int64)[:, None], np.arange(D + 1, dtype=np.int64)[None, :]
    jc = np.minimum(i + d, n - 1)
    cand = (i + d < n) & valid[i] & valid[jc] & (d >= md)
    sums = []
    for offs in neighbourhood_offsets(p, w):
        S, T, C = np.zeros((n, D + 1)), np.zeros((n, D + 1)), np.zeros((n, D + 1), np.int64)
        for da, db in offs.tolist():   # rule 4's order
            r0, c0 = w + da, 2 * w + db - da
            S += B[r0:r0 + n, c0:c0 + D + 1]
            T += E[r0:r0 + n, c0:c0 + D + 1]
            C += part[r0:r0 + n, c0:c0 + D + 1]
        cand &= (T > 0) & (2 * C >= offs.shape[0])
        sums.append((S, T))
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        nvij = nv[i] * nv[jc]
        for x, (S, T) in enumerate(sums):
            lam[x] = np.where(cand, ((S / T) * exv[d]) * nvij, np.nan)
    return lam, cand


def _counts(band, D, W):
    return np.minimum(np.rint(np.asarray(band, dtype=np.float64)[:, :D + 1]), W - 1).astype(np.int64)


def loop_histograms_host(band, lam, cand, bounds=None, max_count=MAX_COUNT) -> np.ndarray:
    """rules 7 and 8: hist int32 [4, K, W]"""
    t = chunk_boundaries() if bounds is None else np.asarray(bounds, dtype=np.float64)
    K, W = t.size + 1, int(max_count) + 1
    o = _counts(band, lam.shape[2] - 1, W)[cand]
    hist = np.zeros((4, K, W), np.int32)
    for x in range(4):
        k = np.searchsorted(t, lam[x][cand], side="right")
        hist[x] = np.bincount(k * W + o, minlength=K * W).reshape(K, W)
    return hist


def enriched_pixels_host(band, lam, cand, thr, bounds=None, max_count=MAX_COUNT) -> Pixels:
    """rule 10: the candidates at or above all four thresholds, in ascending (i, j)"""
    t = chunk_boundaries() if bounds is None else np.asarray(bounds, dtype=np.float64)
    thr = np.asarray(thr).reshape(4, t.size + 1)
    D = lam.shape[2] - 1
    o = _counts(band, D, int(max_count) + 1)
    hit = cand.copy()
    for x in range(4):
        k = np.searchsorted(t, lam[x], side="right")
        hit &= o >= thr[x][k]
    i, d = np.nonzero(hit)
    return Pixels(i.astype(np.int64), (i + d).astype(np.int64), np.asarray(band)[i, d], lam[:, i, d].T.copy())


def loops_host(pos1, pos2, count, norm="VC", resolution_bp=10000, expected="auto", n_bins=None, norm_args=None,
               expected_args=None, **rule) -> Loops:
    """The whole rule on the host.  norm: None, a vector at resolution_bp, or 'KR' / 'VC' / 'SQRTVC' (computed from the records);
    expected: "auto" (hicmap.resolve_host's, with expected_args = min_count: the vector HicContacts.expected_vector returns, bit
    for bit, so that the local expected values are the device's too) or a vector; **rule: loop_rule's."""
    res = int(resolution_bp)
    loop_rule(res, 0, **rule)
    A, vc = hicmap.matrix_host(pos1, pos2, count, res, n_bins)
    n = A.shape[0]
    r = loop_rule(res, n, **rule)
    norm, expected = hicmap.vectors_host(pos1, pos2, count, n, norm, res, n_bins, norm_args, expected, expected_args)
    band = hicmap.band_host(A, r.width)
    t = chunk_boundaries(r.K)
    lam, cand = loop_lambdas_host(band, vc, norm, expected, r.p, r.w, r.D, r.ignore_diags, r.min_dist)
    thr = loop_thresholds(loop_histograms_host(band, lam, cand, t, r.W - 1), r.fdr, t)
    pix = enriched_pixels_host(band, lam, cand, thr, t, r.W - 1)
    info = {"candidates": int(cand.sum()), "enriched": int(pix.i.size), "thresholds": thr, "host_syncs": 0}
    return loops_from_pixels(pix, res, n, r.ratios, r.radius_bins * res, r.min_cluster_pixels, t, info)


# ----------------------------------------------------------------------------------------------
# device
# ----------------------------------------------------------------------------------------------
def _stencil_args(band, vc, norm, ex, r: LoopRule):
    dev = band.device
    n, width = hicmap.check_band(band, vc, r.width, r.D + 1)
    norm, ex = hicmap.device_vector(norm, dev, "norm", optional=True), hicmap.device_vector(ex, dev, "the expected vector")
    hicmap.expected_reach(int(ex.numel()), n, r.D + 1, "pixels")
    return dict(n=n, D=r.D, width=width, band=band, vc=vc, norm=norm, n_norm=0 if norm is None else int(norm.numel()),
                expected=ex, n_expected=int(ex.numel()), p=r.p, w=r.w, ignore_diags=r.ignore_diags)


def loop_histograms(band, vc, norm, ex, r: LoopRule, bounds=None, want_lambda=False):
    """Pass 1 on the device (cgcn_hicloops_pass1: enqueue only): (hist int32 [4, K, W], flags uint32-as-int32 [n, D + 1]: the
    packed candidate bit and chunk indices that enriched_pixels reads, lambda float64 [4, n, D + 1] or None).  band: hicmap.device_band's,
    at least r.width wide; vc, norm (or None), ex: float64 device vectors; bounds: the chunk boundaries (host), K - 1 of them."""
    from . import _lib
    args = _stencil_args(band, vc, norm, ex, r)
    dev, n = band.device, args["n"]
    t = chunk_boundaries(r.K) if bounds is None else np.asarray(bounds, dtype=np.float64)
    if t.size != r.K - 1:
        raise ValueError("%d chunks need %d boundaries, not %d" % (r.K, r.K - 1, t.size))
    hist = torch.zeros(4, r.K, r.W, dtype=torch.int32, device=dev)
    flags = torch.zeros(n, r.D + 1, dtype=torch.int32, device=dev)
    lam = torch.empty(4, n, r.D + 1, dtype=torch.float64, device=dev) if want_lambda else None
    if n:
        with torch.cuda.device(dev):
            _lib.call("cgcn_hicloops_pass1", min_dist=r.min_dist, bounds=torch.from_numpy(t).to(dev), n_chunks=r.K, W=r.W,
                      hist=hist, flags=flags, lambda_out=lam, **args)
    return hist, flags, lam


def enriched_pixels(band, vc, norm, ex, r: LoopRule, flags, thr) -> Pixels:
    """Pass 2 on the device: the ordered count / scan / write of rule 10's list (cgcn_hicloops_count, ONE read-back of the
    count, cgcn_hicloops_write) and the read-back of the list.  thr: int32 [4, K] (host)."""
    from . import _lib
    args = _stencil_args(band, vc, norm, ex, r)
    dev, n = band.device, args["n"]
    thr_dev = torch.from_numpy(np.ascontiguousarray(np.asarray(thr, dtype=np.int32).reshape(4, r.K))).to(dev)
    if n == 0:
        return Pixels(np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0), np.zeros((0, 4)))
    with torch.cuda.device(dev):
        wsp, need = _lib.workspace_for("cgcn_hicloops_workspace_bytes", dev, "loop pixels, n=%d D=%d" % (n, r.D), n=n, D=r.D)
        total = torch.zeros(1, dtype=torch.int64, device=dev)
        _lib.call("cgcn_hicloops_count", n=n, D=r.D, width=args["width"], band=band, flags=flags, thr=thr_dev, n_chunks=r.K, W=r.W,
                  workspace=wsp, workspace_bytes=need, total=total)
        m = int(total.item())
        ij = torch.empty(max(m, 1), 2, dtype=torch.int32, device=dev)
        val = torch.empty(max(m, 1), 5, dtype=torch.float64, device=dev)
        _lib.call("cgcn_hicloops_write", flags=flags, thr=thr_dev, n_chunks=r.K, W=r.W, capacity=m, workspace=wsp,
                  workspace_bytes=need, pix_ij=ij, pix_val=val, **args)
        ij, val = ij[:m].cpu().numpy().astype(np.int64), val[:m].cpu().numpy()
    return Pixels(ij[:, 0].copy(), ij[:, 1].copy(), val[:, 0].copy(), val[:, 1:].copy())


def loops_of_matrix(A: hicnorm.DeviceContactMatrix, norm, ex, resolution_bp, **rule) -> Loops:
    """Rules 1 to 11 from the device matrix: the band and both passes on the device, the thresholds and the clusters in the
    shared host functions.  norm: None or a float64 device vector; ex: a float64 device vector.  Host syncs: the read-back of
    the histograms, of the count and of the list."""
    r = loop_rule(resolution_bp, A.n, **rule)
    t = chunk_boundaries(r.K)
    band = hicmap.device_band(A, r.width)
    hist, flags, _ = loop_histograms(band, A.vc, norm, ex, r, t)
    hist = hist.cpu().numpy()
    thr = loop_thresholds(hist, r.fdr, t)
    pix = enriched_pixels(band, A.vc, norm, ex, r, flags, thr)
    info = {"candidates": int(hist[0].sum()), "enriched": int(pix.i.size), "thresholds": thr, "host_syncs": 3}
    return loops_from_pixels(pix, r.res, A.n, r.ratios, r.radius_bins * r.res, r.min_cluster_pixels, t, info)


# ----------------------------------------------------------------------------------------------
# loops and graphs
# ----------------------------------------------------------------------------------------------
def check_loops(loops):
    """(Loops, pad_bins) of rule 12's argument: a Loops (pad_bins = 1) or the pair"""
    pad = 1
    if isinstance(loops, (tuple, list)):
        if len(loops) != 2:
            raise ValueError("loops must be a Loops, (Loops, pad_bins), a dict of HicContacts.loops' keywords, or None")
        loops, pad = loops
    if not isinstance(loops, Loops):
        raise ValueError("loops must be a Loops, (Loops, pad_bins), a dict of HicContacts.loops' keywords, or None")
    if int(pad) < 0:
        raise ValueError("pad_bins must not be negative")
    return loops, int(pad)


def same_loop_host(pos1, pos2, loops: Loops, pad_bins=1) -> np.ndarray:
    """rule 12's test per record (bool)"""
    res = loops.resolution_bp
    b1, b2 = np.asarray(pos1, dtype=np.int64) // res, np.asarray(pos2, dtype=np.int64) // res
    lo, hi = np.minimum(b1, b2), np.maximum(b1, b2)
    return (lo >= 0) & (hi < loops.n) & np.isin(lo * _KEY + hi, loops.footprint_keys(pad_bins))


def loop_edge_share(graph_or_csr, loops: Loops, window_start, pad_bins=1):
    """(entries in a footprint, nnz) as exact integers: the stored entries of a graph (hicmap.csr_of's inputs) whose two
    windows, binned at the loops' resolution and lower bin first, lie in some loop's footprint"""
    ws = np.asarray(window_start, dtype=np.int64).ravel()
    row, col, nnz = hicmap.edge_rows(graph_or_csr, ws.size, "window_start")
    return int(np.sum(same_loop_host(ws[row], ws[col], loops, pad_bins))), nnz
