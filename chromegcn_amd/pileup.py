"""Pile-ups (aggregate peak analysis, APA): the contact map summed in a small window around every pixel centre of a list, per
group of centres.  It is the usual companion of a HiCCUPS-style caller -- average the map around every call and check that the
centre stands out from its corners -- and, fed the edges of a top-K graph, it shows without a threshold whether the edges are
focal contacts or dense neighbourhoods; the same pass serves edges grouped by distance, by a quantile of adjacency saliency, the
edges of a null graph or a diagonally shifted control.  The rule below is this project's definition, after Juicer's `apa`
(Durand et al. 2016).  No Juicer output exists where this runs, so NOTHING here is compared against Juicer.  OUT OF SCOPE:
Juicer's normed and rank APA matrices, per-centre enhancement histograms, saddle plots, multi-resolution pile-ups.  The value
band, the slice sums and their fold run on the device (csrc/cgcn_pileup.hip); the keep test, the stable sort and the slice
table are torch plumbing there and numpy here; apa_scores is host code that both paths share.

The rule, per chromosome.  res = resolution_bp; A = hicnorm's contact matrix at res (n bins); nv = hicnorm.clean_norm(norm);
valid = hicmap.valid_bins(VC, norm), VC the matrix's row sums; ex = the expected vector exactly as hicmap.resolve_host resolves
`expected=` ("auto" or a float64 vector that reads as 0 beyond its length and reaches min(n, max_dist + 1) entries), needed for
value = "oe" alone; w the window half-width, 1 <= w <= 10 (by default 10 at res <= 10 kb and 5 above), S = 2 w + 1; c the corner
width, w // 2 + 1 by default (6 at w = 10), 1 <= c <= w.
  1. Cell value.  value = "observed": A[a, b]; "balanced": A[a, b] / (nv[a] * nv[b]); "oe" (default):
     (A[a, b] / (nv[a] * nv[b])) / ex[b - a], in exactly this order of operations.  A cell takes part iff both bins are valid,
     the value is finite and, for "oe", ex[b - a] > 0; ex reads as 0 beyond its length.  The VALUE BAND [n, max_dist + 2 w + 1]
     holds the value of the cell (a, a + dd) at [a, dd], NaN where the cell takes no part or lies beyond the matrix.
  2. Centres.  A centre (i, j) is given lower bin first; it is swapped if it is not.  It has a group g (default 0).  It is
     kept iff 0 <= g < G, i - w >= 0 and j + w <= n - 1, min_dist <= j - i, and j - i <= max_dist.  min_dist = 3 w by default
     and must be >= 2 w, so that no window cell crosses the diagonal (ValueError otherwise); max_dist = max_distance_bp // res,
     2 Mb by default (loops' convention).  Every other centre is skipped and counted under the FIRST test it fails, in this
     order: `group`, `edge`, `near`, `far`.  Duplicates are kept: a pile-up over edges is weighted by edges.
  3. Order.  The kept centres are sorted stably by group; within a group they stay in input order and are cut into slices of
     SLICE = 256 consecutive centres, the last of which may be short.
  4. Sums.  For group g and offset (da, db), |da|, |db| <= w: the slice partial is ONE plain sequential float64 sum, from 0.0
     and in centre order, of the values of the cells (i + da, j + db) that take part; P[g, da, db] is ONE plain sequential sum,
     from 0.0 and in slice order, of the slice partials; N[g, da, db] (int64) is the number of cells that took part; kept[g]
     the number of kept centres.  No fused multiply-add anywhere.  The same bits in every run, and exact whenever every value
     is an integer below 2^53 (value = "observed" on integer counts).
  5. Means and scores (apa_scores, shared).  mean = P / N, NaN where N == 0.  Rows are da = -w .. w, columns db = -w .. w: UL
     the first c rows x first c columns, UR the first c rows x last c columns, LL the last c rows x first c columns (the corner
     towards the diagonal), LR the last c rows x last c columns.  P2UL, P2UR, P2LL, P2LR = the centre divided by the np.nanmean
     of the corner; P2M = the centre divided by the np.nanmean of all other cells; ZscoreLL = (centre - mean(LL)) /
     std(LL, ddof=1), NaN for c = 1.
  6. Guards, ValueError before anything is allocated: w > 10; n (max_dist + 2 w + 1) > 2^28 band elements; G > 65 536; centre
     arrays of different lengths.  M = 0 and groups without kept centres are legal: zeros in P and N, NaN means."""
from __future__ import annotations

import warnings
from typing import NamedTuple

import numpy as np
import torch

from . import hicmap, hicnorm
from .loops import Loops

SLICE = 256
MAX_W, MAX_GROUPS, MAX_ELEMS, MAX_DISTANCE_BP = 10, 65536, 1 << 28, 2000000
VALUES = ("observed", "balanced", "oe")     # include/chromegcn.h: CGCN_PILEUP_*
REASONS = ("group", "edge", "near", "far")
SCORES = ("P2UL", "P2UR", "P2LL", "P2LR", "P2M", "ZscoreLL")
_RULE = ("value", "w", "corner", "min_dist", "max_distance_bp")


class PileupRule(NamedTuple):
    """the checked arguments of one call (pileup_rule)"""
    res: int
    value: str
    w: int
    corner: int
    min_dist: int
    max_dist: int

    @property
    def S(self):
        return 2 * self.w + 1

    @property
    def width(self):
        """the band's width: the windows of the centres at distance max_dist reach 2 w further"""
        return self.max_dist + 2 * self.w + 1


def pileup_rule(resolution_bp, n=0, n_groups=1, **rule) -> PileupRule:
    """The rule's arguments, checked (rule 6's guards among them): value, w, corner, min_dist, max_distance_bp."""
    unknown = set(rule) - set(_RULE)
    if unknown:
        raise TypeError("unknown argument(s) %s" % ", ".join(sorted(unknown)))
    res = int(resolution_bp)
    if res < 1:
        raise ValueError("resolution_bp must be positive")
    value = rule.get("value", "oe")
    if value not in VALUES:
        raise ValueError("value=%r is none of %s" % (value, ", ".join(VALUES)))
    w = rule.get("w")
    w = (10 if res <= 10000 else 5) if w is None else int(w)
    if w > MAX_W:
        raise ValueError("w=%d: more than %d is not supported" % (w, MAX_W))
    if w < 1:
        raise ValueError("w must be at least 1")
    c = rule.get("corner")
    c = w // 2 + 1 if c is None else int(c)
    if not 1 <= c <= w:
        raise ValueError("the corner width needs 1 <= corner <= w, not corner=%d w=%d" % (c, w))
    mbp = rule.get("max_distance_bp")
    D = int(MAX_DISTANCE_BP if mbp is None else mbp) // res
    if D < 0:
        raise ValueError("max_distance_bp must not be negative")
    md = rule.get("min_dist")
    md = 3 * w if md is None else int(md)
    if md < 2 * w:
        raise ValueError("min_dist=%d is below 2 w = %d: a window cell would cross the diagonal" % (md, 2 * w))
    if int(n) * (D + 2 * w + 1) > MAX_ELEMS:
        raise ValueError("%d bins x %d distances are more than 2^28 band elements: take a larger resolution_bp or a smaller "
                         "max_distance_bp" % (int(n), D + 2 * w + 1))
    if int(n_groups) > MAX_GROUPS:
        raise ValueError("%d groups are more than %d" % (int(n_groups), MAX_GROUPS))
    if int(n_groups) < 1:
        raise ValueError("n_groups must be at least 1")
    return PileupRule(res, value, w, c, md, D)


# ----------------------------------------------------------------------------------------------
# shared host functions
# ----------------------------------------------------------------------------------------------
def apa_scores(mean, corner) -> dict:
    """rule 5: {P2UL, P2UR, P2LL, P2LR, P2M, ZscoreLL} of a mean matrix float64 [S, S] (floats), or of a stack [G, S, S]
    (float64 arrays [G]).  NaN cells are ignored by the corner means; everything is NaN where the centre is."""
    mean = np.asarray(mean, dtype=np.float64)
    if mean.ndim == 3:
        rows = [apa_scores(m, corner) for m in mean]
        return {k: np.array([r[k] for r in rows], dtype=np.float64) for k in SCORES}
    if mean.ndim != 2 or mean.shape[0] != mean.shape[1] or mean.shape[0] % 2 != 1 or mean.shape[0] < 3:
        raise ValueError("the mean matrix must be square with an odd side of at least 3")
    S = mean.shape[0]
    w, c = S // 2, int(corner)
    if not 1 <= c <= w:
        raise ValueError("the corner width needs 1 <= corner <= w, not corner=%d w=%d" % (c, w))
    centre = mean[w, w]
    corners = {"UL": mean[:c, :c], "UR": mean[:c, S - c:], "LL": mean[S - c:, :c], "LR": mean[S - c:, S - c:]}
    others = np.ones((S, S), bool)
    others[w, w] = False
    out = {}
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore", RuntimeWarning)
        for k, v in corners.items():
            out["P2" + k] = float(centre / np.nanmean(v))
        out["P2M"] = float(centre / np.nanmean(mean[others]))
        ll = corners["LL"]
        out["ZscoreLL"] = float((centre - np.nanmean(ll)) / np.nanstd(ll, ddof=1)) if c > 1 else float("nan")
    return out


class Pileup:
    """The pile-up of one centre list: sum float64 [G, S, S] (P), count int64 [G, S, S] (N), mean = P / N (NaN where N == 0),
    kept int64 [G], skipped {group, edge, near, far}, rule (a PileupRule)."""

    def __init__(self, P, N, kept, skipped, rule: PileupRule):
        self.sum, self.count = np.asarray(P, dtype=np.float64), np.asarray(N, dtype=np.int64)
        self.kept, self.skipped, self.rule = np.asarray(kept, dtype=np.int64), dict(skipped), rule
        with np.errstate(invalid="ignore", divide="ignore"):
            self.mean = np.where(self.count > 0, self.sum / np.where(self.count > 0, self.count, 1), np.nan)

    def scores(self) -> dict:
        """rule 5's scores, one float64 array [G] each"""
        return apa_scores(self.mean, self.rule.corner)

    def save(self, path):
        """everything as one .npz: sum, count, mean, kept, skipped (in REASONS' order), the rule's fields and the scores"""
        r = self.rule
        np.savez(path, sum=self.sum, count=self.count, mean=self.mean, kept=self.kept,
                 skipped=np.array([self.skipped[k] for k in REASONS], dtype=np.int64), resolution_bp=r.res, value=r.value, w=r.w,
                 corner=r.corner, min_dist=r.min_dist, max_dist=r.max_dist, **self.scores())


def slice_table(kept):
    """rule 3: (slice_off int32 [n_slices + 1], group_off int32 [G + 1]) from the kept centres per group: the slices tile the
    sorted kept centres, group g owns the slices group_off[g] .. group_off[g + 1] - 1"""
    kept = np.asarray(kept, dtype=np.int64).ravel()
    per = (kept + SLICE - 1) // SLICE
    group_off = np.concatenate([[0], np.cumsum(per)])
    start = np.concatenate([[0], np.cumsum(kept)])
    ns = int(group_off[-1])
    g = np.repeat(np.arange(kept.size), per)
    lo = start[g] + (np.arange(ns) - group_off[g]) * SLICE
    slice_off = np.concatenate([lo, [start[-1]]]) if ns else np.zeros(1, np.int64)
    return slice_off.astype(np.int32), group_off.astype(np.int32)


def _centre_arrays(ci, cj, group):
    ci, cj = np.asarray(ci).ravel(), np.asarray(cj).ravel()
    if ci.size != cj.size or (group is not None and np.asarray(group).size != ci.size):
        raise ValueError("the centre arrays have different lengths")
    for a in (ci, cj):
        if a.size and not np.issubdtype(a.dtype, np.integer):
            raise ValueError("centres are integer bins")
    g = np.zeros(ci.size, np.int64) if group is None else np.asarray(group).ravel().astype(np.int64)
    return ci.astype(np.int64), cj.astype(np.int64), g


def keep_centres_host(ci, cj, group, G, n, rule: PileupRule):
    """rules 2 and 3 on the host: (i, j of the kept centres sorted stably by group, kept int64 [G], skipped)"""
    ci, cj, g = _centre_arrays(ci, cj, group)
    i, j = np.minimum(ci, cj), np.maximum(ci, cj)
    d = j - i
    fails = [(g < 0) | (g >= G), (i - rule.w < 0) | (j + rule.w > n - 1), d < rule.min_dist, d > rule.max_dist]
    alive, skipped = np.ones(i.size, bool), {}
    for name, f in zip(REASONS, fails):
        skipped[name] = int(np.sum(alive & f))
        alive &= ~f
    i, j, g = i[alive], j[alive], g[alive]
    order = np.argsort(g, kind="stable")
    return i[order], j[order], np.bincount(g, minlength=G).astype(np.int64)[:G], skipped


# ----------------------------------------------------------------------------------------------
# host restatement
# ----------------------------------------------------------------------------------------------
def value_band_host(band, vc, norm, ex, rule: PileupRule) -> np.ndarray:
    """rule 1: the value band float64 [n, width] from hicmap.band_host's raw band (at least rule.width wide; the result is as
    wide as the band), the matrix's row sums vc, norm None or a vector, ex the expected vector (None unless value = "oe")"""
    band = np.asarray(band, dtype=np.float64)
    n, width = band.shape
    if width < rule.width:
        raise ValueError("the band is %d wide but max_dist=%d and w=%d need %d" % (width, rule.max_dist, rule.w, rule.width))
    valid, nv = hicmap.bins_of_band_host(vc, norm, n)
    if rule.value == "oe":
        if ex is None:
            raise ValueError('value="oe" needs an expected vector')
        exv = hicmap.expected_at_host(ex, n, width, rule.max_dist + 1, "centres")
    if n == 0:
        return np.zeros((0, width))
    # bin b = a + dd of every cell as a window [n, width] over the vectors padded behind the matrix: a view, no index arrays
    window = np.lib.stride_tricks.sliding_window_view
    part = valid[:, None] & window(np.concatenate([valid, np.zeros(width, bool)]), width)[:n]
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        v = band
        if rule.value != "observed":
            v = band / (nv[:, None] * window(np.concatenate([nv, np.ones(width)]), width)[:n])
        if rule.value == "oe":
            part = part & (exv > 0)[None, :]
            v = v / np.where(exv > 0, exv, 1.0)[None, :]
    part = part & np.isfinite(v)
    return np.where(part, v, np.nan)


def pileup_sums_host(value_band, ci, cj, group, G, rule: PileupRule) -> Pileup:
    """Rules 2 to 4 on the host.  The slice partials are added position by position (an explicit loop over the SLICE positions,
    vectorised over slices and offsets) and folded slice by slice (an explicit loop over the slices of a group, vectorised over
    groups): np.sum adds pairwise and is not used."""
    vb = np.asarray(value_band, dtype=np.float64)
    n, width = vb.shape
    G = int(G)
    pileup_rule(rule.res, n, G, value=rule.value, w=rule.w, corner=rule.corner, min_dist=rule.min_dist,
                max_distance_bp=rule.max_dist * rule.res)
    if width < rule.width:
        raise ValueError("the value band is %d wide but the rule needs %d" % (width, rule.width))
    i, j, kept, skipped = keep_centres_host(ci, cj, group, G, n, rule)
    slice_off, group_off = slice_table(kept)
    ns, S, w = slice_off.size - 1, rule.S, rule.w
    part, cnt = np.zeros((ns, S, S)), np.zeros((ns, S, S), np.int64)
    o = np.arange(-w, w + 1, dtype=np.int64)
    da, db = o[None, :, None], o[None, None, :]
    lens = np.diff(slice_off.astype(np.int64))
    for pos in range(SLICE):                       # rule 4's centre order
        act = np.nonzero(lens > pos)[0]
        if act.size == 0:
            break
        at = slice_off[act].astype(np.int64) + pos
        a = i[at][:, None, None] + da
        dd = (j[at] - i[at])[:, None, None] + (db - da)
        v = vb[a + 0 * db, dd]
        took = ~np.isnan(v)
        part[act] = np.where(took, part[act] + np.where(took, v, 0.0), part[act])
        cnt[act] += took
    P, N = np.zeros((G, S, S)), np.zeros((G, S, S), np.int64)
    per = np.diff(group_off.astype(np.int64))
    for s in range(int(per.max()) if per.size else 0):   # rule 4's slice order
        act = np.nonzero(per > s)[0]
        P[act] = P[act] + part[group_off[act].astype(np.int64) + s]
        N[act] += cnt[group_off[act].astype(np.int64) + s]
    return Pileup(P, N, kept, skipped, rule)


def _centres_of(centres):
    """(ci, cj) of the `centres` argument: a Loops (its peaks) or a pair"""
    if isinstance(centres, Loops):
        return centres.peak_i, centres.peak_j
    if not isinstance(centres, (tuple, list)) or len(centres) != 2:
        raise ValueError("centres must be a Loops or a pair (i, j) of integer arrays or device tensors")
    return centres[0], centres[1]


def _n_groups(group, n_groups):
    if n_groups is not None:
        return int(n_groups)
    if group is None:
        return 1
    if torch.is_tensor(group):
        return int(group.max().item()) + 1 if group.numel() else 1
    group = np.asarray(group)
    return max(int(group.max()) + 1, 1) if group.size else 1


def pileup_host(pos1, pos2, count, centres, group=None, n_groups=None, norm="VC", resolution_bp=10000, expected="auto",
                n_bins=None, norm_args=None, expected_args=None, **rule) -> Pileup:
    """The whole rule on the host from the records.  norm: None, a vector at resolution_bp, or 'KR' / 'VC' / 'SQRTVC'; expected:
    "auto" (hicmap.resolve_host's: the distance sums in the device's order) or a vector, read for value = "oe" alone;
    **rule: pileup_rule's."""
    res = int(resolution_bp)
    G = _n_groups(group, n_groups)
    value = pileup_rule(res, 0, G, **rule).value   # decides whether an expected vector is read at all
    ci, cj = _centres_of(centres)
    _centre_arrays(ci, cj, group)
    A, vc = hicmap.matrix_host(pos1, pos2, count, res, n_bins)
    r = pileup_rule(res, A.shape[0], G, **rule)
    norm, expected = hicmap.vectors_host(pos1, pos2, count, A.shape[0], norm, res, n_bins, norm_args,
                                         expected if value == "oe" else None, expected_args)
    vb = value_band_host(hicmap.band_host(A, r.width), vc, norm, expected, r)
    return pileup_sums_host(vb, ci, cj, group, G, r)


# ----------------------------------------------------------------------------------------------
# device
# ----------------------------------------------------------------------------------------------
def value_band(band, vc, norm, ex, rule: PileupRule) -> torch.Tensor:
    """rule 1 on the device (cgcn_pileup_values: enqueue only): the value band float64 [n, width] from hicmap.device_band's raw
    band (at least rule.width wide); vc, norm (or None), ex (or None unless value = "oe"): float64 device vectors"""
    from . import _lib
    dev = band.device
    n, width = hicmap.check_band(band, vc, rule.width)
    norm = hicmap.device_vector(norm, dev, "norm", optional=True)
    if rule.value == "oe":
        ex = hicmap.device_vector(ex, dev, "the expected vector")
        hicmap.expected_reach(int(ex.numel()), n, rule.max_dist + 1, "centres")
    else:
        ex = None
    out = torch.empty(n, width, dtype=torch.float64, device=dev)
    if n:
        with torch.cuda.device(dev):
            _lib.call("cgcn_pileup_values", n=n, width=width, band=band, vc=vc, norm=norm,
                      n_norm=0 if norm is None else int(norm.numel()), expected=ex, n_expected=0 if ex is None else int(ex.numel()),
                      kind=VALUES.index(rule.value), vband=out)
    return out


def _device_centres(ci, cj, group, dev):
    def up(a):
        if torch.is_tensor(a):
            if a.dtype not in (torch.int32, torch.int64, torch.int16, torch.uint8, torch.int8):
                raise ValueError("centres are integer bins")
            return a.to(device=dev, dtype=torch.int64).ravel()
        a = np.asarray(a).ravel()
        if a.size and not np.issubdtype(a.dtype, np.integer):
            raise ValueError("centres are integer bins")
        return torch.from_numpy(a.astype(np.int64)).to(dev)
    ci, cj = up(ci), up(cj)
    g = torch.zeros_like(ci) if group is None else up(group)
    if ci.numel() != cj.numel() or g.numel() != ci.numel():
        raise ValueError("the centre arrays have different lengths")
    return ci, cj, g


def keep_centres(ci, cj, group, G, n, rule: PileupRule):
    """rules 2 and 3 on the device: (i, j int32 device tensors of the kept centres sorted stably by group, kept int64 numpy
    [G], skipped).  Masks, one stable sort and ONE read-back (the four skip counts and the kept centres per group)."""
    dev = ci.device
    i, j = torch.minimum(ci, cj), torch.maximum(ci, cj)
    d = j - i
    fails = [(group < 0) | (group >= G), (i - rule.w < 0) | (j + rule.w > n - 1), d < rule.min_dist, d > rule.max_dist]
    alive, counts = torch.ones_like(i, dtype=torch.bool), []
    for f in fails:
        counts.append((alive & f).sum())
        alive = alive & ~f
    key = torch.where(alive, group, torch.full_like(group, G))
    per = torch.zeros(G + 1, dtype=torch.int64, device=dev).scatter_add_(0, key, torch.ones_like(key))
    order = torch.sort(key, stable=True).indices
    back = torch.cat([torch.stack(counts), per[:G]]).cpu().numpy()          # the one sync
    kept = back[4:].astype(np.int64)
    K = int(kept.sum())
    return (i[order][:K].to(torch.int32).contiguous(), j[order][:K].to(torch.int32).contiguous(), kept,
            {name: int(c) for name, c in zip(REASONS, back[:4])})


def pileup_sums(value_band, ci, cj, group, G, rule: PileupRule) -> Pileup:
    """Rules 2 to 4 on the device: keep_centres, then cgcn_pileup_slices and cgcn_pileup_fold, and the read-back of P and N.
    value_band: value_band()'s tensor; ci, cj, group (or None): integer arrays or device tensors."""
    from . import _lib
    vb = value_band
    dev = vb.device
    n, G = int(vb.shape[0]), int(G)
    pileup_rule(rule.res, n, G, value=rule.value, w=rule.w, corner=rule.corner, min_dist=rule.min_dist,
                max_distance_bp=rule.max_dist * rule.res)
    n, width = hicmap.check_band(vb, None, rule.width, what="value band")
    S = rule.S
    with torch.cuda.device(dev):
        ci, cj, g = _device_centres(ci, cj, group, dev)
        i, j, kept, skipped = keep_centres(ci, cj, g, G, n, rule)
        slice_off, group_off = slice_table(kept)
        ns = slice_off.size - 1
        P = torch.empty(G, S, S, dtype=torch.float64, device=dev)
        N = torch.empty(G, S, S, dtype=torch.int64, device=dev)
        wsp, need = _lib.workspace_for("cgcn_pileup_workspace_bytes", dev, "pile-up, %d slices w=%d" % (ns, rule.w), n_slices=ns,
                                       w=rule.w)
        so, go = torch.from_numpy(slice_off).to(dev), torch.from_numpy(group_off).to(dev)
        _lib.call("cgcn_pileup_slices", n=n, width=width, vband=vb, w=rule.w, n_slices=ns, slice_off=so, n_centres=int(i.numel()),
                  ci=i, cj=j, workspace=wsp, workspace_bytes=need)
        _lib.call("cgcn_pileup_fold", n_groups=G, w=rule.w, n_slices=ns, group_off=go, workspace=wsp, workspace_bytes=need, P=P, N=N)
        return Pileup(P.cpu().numpy(), N.cpu().numpy(), kept, skipped, rule)


def pileup_of_matrix(A: hicnorm.DeviceContactMatrix, norm, ex, centres, group=None, n_groups=None, resolution_bp=10000,
                     **rule) -> Pileup:
    """Rules 1 to 4 from the device matrix: hicmap.device_band, value_band and pileup_sums.  norm: None or a float64 device
    vector; ex: a float64 device vector (None unless value = "oe")."""
    G = _n_groups(group, n_groups)
    r = pileup_rule(resolution_bp, A.n, G, **rule)
    ci, cj = _centres_of(centres)
    if not torch.is_tensor(ci):
        _centre_arrays(ci, cj, None if torch.is_tensor(group) else group)
    vb = value_band(hicmap.device_band(A, r.width), A.vc, norm, ex, r)
    return pileup_sums(vb, ci, cj, group, G, r)


# ----------------------------------------------------------------------------------------------
# centre lists
# ----------------------------------------------------------------------------------------------
def centres_of_graph(graph_or_csr, window_start, resolution_bp):
    """(i, j, entry) int64: one centre per stored entry of a graph (hicmap.csr_of's inputs) with col > row -- its two
    windows binned at resolution_bp as loops.loop_edge_share bins them, lower bin first -- and the entry's index into the
    graph's col / val arrays, so that per-entry values such as saliency can be carried along"""
    ws = np.asarray(window_start, dtype=np.int64).ravel()
    row, col, _ = hicmap.edge_rows(graph_or_csr, ws.size, "window_start")
    res = int(resolution_bp)
    if res < 1:
        raise ValueError("resolution_bp must be positive")
    entry = np.nonzero(col > row)[0].astype(np.int64)
    b1, b2 = ws[row[entry]] // res, ws[col[entry]] // res
    return np.minimum(b1, b2), np.maximum(b1, b2), entry


def shifted_centres(i, j, shift_bins):
    """the same-distance control: every centre moved by shift_bins along the diagonal (arrays or tensors)"""
    s = int(shift_bins)
    return i + s, j + s


def distance_groups(i, j, edges_bins):
    """group g where edges_bins[g] <= |j - i| < edges_bins[g + 1], -1 (skipped as `group`) outside; G = len(edges_bins) - 1"""
    edges = np.asarray(edges_bins, dtype=np.int64).ravel()
    if edges.size < 2 or np.any(np.diff(edges) <= 0):
        raise ValueError("edges_bins must be at least two ascending bin distances")
    if torch.is_tensor(i):
        d = (j - i).abs().to(torch.int64)
        g = torch.bucketize(d, torch.from_numpy(edges).to(d.device), right=True) - 1
        return torch.where((g < 0) | (g >= edges.size - 1), torch.full_like(g, -1), g)
    d = np.abs(np.asarray(j, dtype=np.int64) - np.asarray(i, dtype=np.int64))
    g = np.searchsorted(edges, d, side="right").astype(np.int64) - 1
    return np.where((g < 0) | (g >= edges.size - 1), -1, g)


def quantile_groups(values, q):
    """q groups of (nearly) equal size by ascending value: group = rank * q // M by a stable sort; -1 for a NaN"""
    v = np.asarray(values, dtype=np.float64).ravel()
    q = int(q)
    if q < 1:
        raise ValueError("q must be at least 1")
    g = np.full(v.size, -1, np.int64)
    ok = np.nonzero(~np.isnan(v))[0]
    order = ok[np.argsort(v[ok], kind="stable")]
    g[order] = np.arange(order.size, dtype=np.int64) * q // max(order.size, 1)
    return g
