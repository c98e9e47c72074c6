"""Insulation scores, TAD boundaries and domains of one chromosome's Hi-C contact matrix, and the domain restriction of the
top-K contact graph.  The reference meant to use domains: data/7create_graph_old.py:22,48,51-62 takes a `tad_file`, parses it
into tads[chrom] in a commented-out block and never uses the result.  Here the domains come from the records themselves: the
diamond sums on the device (csrc/cgcn_insulation.hip, diamond_sums below), everything behind the sums in ONE float64 numpy
function (insulation_from_sums) that the device path and the numpy restatement share, as hicdist.expected_from_sums is shared.

The rule, per chromosome.  res = resolution_bp; A = hicnorm's contact matrix at res (n bins, symmetric, fp64;
hicnorm.contact_matrix_host / aggregate_contacts).
  1. Balanced value.  B[a, b] = A[a, b] / (nv[a] * nv[b]), one float64 multiplication and one float64 division; nv = the norm
     vector with NaN and 0 mapped to +inf, as in the graph builder; bins beyond the vector's length read as +inf.  With
     norm = None, B = A.
  2. Diamond sums.  For a window of w >= 1 bins and bin i,
         S_w[i] = sum over a in [max(i - w, 0), i - 1], b in [i, min(i + w, n) - 1] of B[a, b]:
     the contacts across the junction left of bin i.  S_w[0] = 0; the diagonal never takes part.  Up to 8 windows go in one
     call, strictly ascending.  The host statement is np.bincount over the upper-triangle entries in (row, column) order; the
     device adds the same terms in another fixed order, so S is bit-equal for integer counts below 2^53 without a vector and
     otherwise within 2 (K - 1) 2^-53 relative, K the entries inside the diamond.
  3. Validity.  valid[b] = VC[b] > 0 and nv[b] finite, VC the matrix's row sums.  up_w[i] = the valid bins in
     [max(i - w, 0), i - 1], dn_w[i] = the valid bins in [i, min(i + w, n) - 1], npix = up * dn.  Bin i is DEFINED at w iff
     valid[i], npix >= ceil(min_valid_share * w * w) (default 0.66; the product is taken in float64) and S_w[i] > 0.
  4. Score.  score = S / npix on the defined bins and NaN elsewhere; L = log2(score / mean(score over the defined bins)).
  5. Boundaries.  With span s (default w), a defined bin i is a boundary iff L[i] < L[j] for every defined j in [i - s, i - 1],
     L[i] <= L[j] for every defined j in [i + 1, i + s] (the leftmost of equal minima wins), each side has at least one defined
     bin, and strength[i] = min(max L left, max L right) - L[i] >= min_strength (the maxima over the defined bins of the two
     ranges).  min_strength defaults to 0.5: a convention, not a measurement.
  6. Domains.  domain_of_bin[b] = the number of boundaries <= b (int32): domain k is [b_k, b_{k+1}).
  7. Domain-restricted graphs.  With domains = (domain_of_bin, domain_bp), a record takes part in the top-K build only if
     dom[pos1 // domain_bp] == dom[pos2 // domain_bp]; a position beyond the vector never matches.  The test is on the source
     record, before any window_bp expansion: the place where the minimum gap is tested.  domain_bp must be a multiple of
     resolution_bp (ValueError).  Named norms and expected = "auto" are still computed from ALL records; only the selection
     changes.  The kept records stay in file order, because ties in the top-K are taken in file order.
     (chromegcn_amd/hic.py: the `domains` argument of the builders, HicContacts.within_domains.)"""
from __future__ import annotations

import ctypes
import math

import numpy as np
import scipy.sparse as sp
import torch

from . import hicmap, hicnorm
from .hicmap import valid_bins  # noqa: F401  (the tests of the commit before the move call insulation.valid_bins / clean_norm)
from .hicnorm import clean_norm  # noqa: F401

MAX_WINDOWS = 8
MIN_VALID_SHARE, MIN_STRENGTH = 0.66, 0.5
_RULE = ("min_valid_share", "span", "min_strength")
_CHUNK = 1 << 22   # diamond_sums_host: (entry, bin) pairs expanded at a time


def _check_windows(windows):
    w = [int(x) for x in np.asarray(windows).ravel()]
    if not 1 <= len(w) <= MAX_WINDOWS:
        raise ValueError("1 to %d windows go in one call, not %d" % (MAX_WINDOWS, len(w)))
    if w[0] < 1 or any(b <= a for a, b in zip(w, w[1:])) or w[-1] >= 2 ** 31:
        raise ValueError("windows must be strictly ascending bin counts >= 1: %r" % (w,))
    return tuple(w)


def windows_in_bins(windows_bp, resolution_bp):
    """window sizes in bp -> bins; every size must be a positive multiple of resolution_bp"""
    res = int(resolution_bp)
    if res < 1:
        raise ValueError("resolution_bp must be positive")
    wbp = [int(x) for x in np.asarray(windows_bp).ravel()]
    if any(x < res or x % res for x in wbp):
        raise ValueError("every window must be a positive multiple of resolution_bp=%d: %r" % (res, wbp))
    return _check_windows([x // res for x in wbp])


# ----------------------------------------------------------------------------------------------
# host restatement of the sums
# ----------------------------------------------------------------------------------------------
def diamond_sums_host(A, norm, windows):
    """S float64 [len(windows), n] of rule 2 from the contact matrix (anything scipy makes a CSR of).  Every upper-triangle
    entry lists the bins whose diamond holds it -- (a, b) lies in the diamond of i iff max(a + 1, b - w + 1) <= i <=
    min(b, a + w) -- and np.bincount adds the weights per bin, entries in (row, column) order.  No difference array: it would
    cancel."""
    w_all = _check_windows(windows)
    A = sp.csr_matrix(A, dtype=np.float64)
    A.sort_indices()
    n = A.shape[0]
    coo = A.tocoo()
    up = coo.col > coo.row
    a, b, v = coo.row[up].astype(np.int64), coo.col[up].astype(np.int64), coo.data[up]
    if norm is not None:
        nv = hicnorm.clean_norm(norm, n)
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            v = v / (nv[a] * nv[b])
    S = np.zeros((len(w_all), n))
    for k, w in enumerate(w_all):
        lo = np.maximum(a + 1, b - w + 1)
        cnt = np.maximum(np.minimum(b, a + w) - lo + 1, 0)
        ends = np.cumsum(cnt)
        e0 = 0
        while e0 < a.size:   # whole entries up to _CHUNK pairs at a time; the partial sums are added in entry order
            e1 = max(int(np.searchsorted(ends, (ends[e0 - 1] if e0 else 0) + _CHUNK, side="right")), e0 + 1)
            c = cnt[e0:e1]
            first = np.cumsum(c) - c
            bins = np.repeat(lo[e0:e1] - first, c) + np.arange(int(c.sum()))
            S[k] += np.bincount(bins, weights=np.repeat(v[e0:e1], c), minlength=n)
            e0 = e1
    return S


# ----------------------------------------------------------------------------------------------
# rules 3 - 6: the one function behind the sums
# ----------------------------------------------------------------------------------------------
class InsulationProfile:
    """insulation_from_sums' result: npix int64 [W, n], defined bool [W, n], score and log2 float64 [W, n] (NaN where a bin
    is not defined), boundaries[k] int64 (ascending bins) and strength[k] float64 per window"""

    def __init__(self, npix, defined, score, log2, boundaries, strength):
        self.npix, self.defined, self.score, self.log2, self.boundaries, self.strength = npix, defined, score, log2, boundaries, strength


def _span_of(span, w, k):
    s = w if span is None else int(span[k]) if np.ndim(span) else int(span)
    if s < 1:
        raise ValueError("span must be at least 1 bin")
    return s


def insulation_from_sums(S, valid, windows, min_valid_share=MIN_VALID_SHARE, span=None, min_strength=MIN_STRENGTH) -> InsulationProfile:
    """Rules 3 to 5 in float64 numpy: the diamond sums S [W, n], valid bool [n] and the windows (bins) -> InsulationProfile.
    span: None (each window's own size), one number of bins, or one per window."""
    w_all = _check_windows(windows)
    S = np.asarray(S, dtype=np.float64).reshape(len(w_all), -1)
    valid = np.asarray(valid, dtype=bool).ravel()
    n = valid.size
    if S.shape[1] != n:
        raise ValueError("S has %d bins but valid has %d" % (S.shape[1], n))
    cv = np.concatenate([np.zeros(1, np.int64), np.cumsum(valid, dtype=np.int64)])
    i = np.arange(n, dtype=np.int64)
    npix, defined = np.zeros(S.shape, np.int64), np.zeros(S.shape, bool)
    score, L = np.full(S.shape, np.nan), np.full(S.shape, np.nan)
    boundaries, strength = [], []
    for k, w in enumerate(w_all):
        up = cv[i] - cv[np.maximum(i - w, 0)]
        dn = cv[np.minimum(i + w, n)] - cv[i]
        npix[k] = up * dn
        d = defined[k] = valid & (npix[k] >= math.ceil(float(min_valid_share) * float(w * w))) & (S[k] > 0)
        score[k, d] = S[k, d] / npix[k, d]
        if d.any():
            L[k, d] = np.log2(score[k, d] / np.mean(score[k, d]))
        s = _span_of(span, w, k)
        l_min, l_max = np.where(d, L[k], np.inf), np.where(d, L[k], -np.inf)
        left_min, right_min = np.full(n, np.inf), np.full(n, np.inf)
        left_max, right_max = np.full(n, -np.inf), np.full(n, -np.inf)
        for o in range(1, min(s, n - 1) + 1):   # the running extremes of the defined bins o to the left and o to the right
            left_min[o:] = np.minimum(left_min[o:], l_min[:-o])
            left_max[o:] = np.maximum(left_max[o:], l_max[:-o])
            right_min[:-o] = np.minimum(right_min[:-o], l_min[o:])
            right_max[:-o] = np.maximum(right_max[:-o], l_max[o:])
        with np.errstate(invalid="ignore"):
            st = np.minimum(left_max, right_max) - L[k]
            hit = d & (left_max > -np.inf) & (right_max > -np.inf) & (L[k] < left_min) & (L[k] <= right_min) & (st >= min_strength)
        boundaries.append(np.flatnonzero(hit))
        strength.append(st[hit])
    return InsulationProfile(npix, defined, score, L, boundaries, strength)


def domains_from_boundaries(boundaries, n) -> np.ndarray:
    """rule 6: domain_of_bin int32 [n], the number of boundaries <= b"""
    return np.searchsorted(np.asarray(boundaries, dtype=np.int64), np.arange(n), side="right").astype(np.int32)


class Insulation:
    """The insulation profile of one chromosome at `windows` (bins of resolution_bp): sums float64 [W, n] (a device tensor from
    HicContacts.insulation, numpy from insulation_host), valid bool [n], score and log2 float64 [W, n], boundaries[k] and
    strength[k] per window (numpy), domain_of_bin(k)."""

    def __init__(self, windows, resolution_bp, sums, valid, profile: InsulationProfile):
        self.windows, self.resolution_bp, self.sums, self.valid = tuple(windows), int(resolution_bp), sums, valid
        self.n = int(valid.size)
        self.npix, self.defined, self.score, self.log2 = profile.npix, profile.defined, profile.score, profile.log2
        self.boundaries, self.strength = profile.boundaries, profile.strength

    @property
    def windows_bp(self):
        return tuple(w * self.resolution_bp for w in self.windows)

    def index_of(self, window_bp) -> int:
        """the place of the window of window_bp base pairs among `windows`"""
        try:
            return self.windows_bp.index(int(window_bp))
        except ValueError:
            raise ValueError("window_bp=%r is none of %r" % (window_bp, self.windows_bp)) from None

    def domain_of_bin(self, k=0) -> np.ndarray:
        return domains_from_boundaries(self.boundaries[k], self.n)


def _rule(rule):
    unknown = set(rule) - set(_RULE)
    if unknown:
        raise TypeError("unknown argument(s) %s" % ", ".join(sorted(unknown)))
    return rule


def insulation_host(pos1, pos2, count, norm, resolution_bp, windows_bp, n_bins=None, norm_args=None, **rule) -> Insulation:
    """The whole rule on the host.  norm: None, a vector at resolution_bp, or 'KR' / 'VC' / 'SQRTVC' (computed from the records:
    hicnorm.hic_norm_vector_host with norm_args); **rule: min_valid_share, span, min_strength."""
    w = windows_in_bins(windows_bp, resolution_bp)
    A, vc, norm, _ = hicmap.resolve_host(pos1, pos2, count, norm, resolution_bp, n_bins, norm_args)
    S = diamond_sums_host(A, norm, w)
    valid = hicmap.valid_bins(vc, norm)
    return Insulation(w, resolution_bp, S, valid, insulation_from_sums(S, valid, w, **_rule(rule)))


def domains_host(pos1, pos2, count, window_bp, norm="VC", resolution_bp=10000, n_bins=None, norm_args=None, **rule):
    """(domain_of_bin int32 [n], resolution_bp) of one window on the host: HicContacts.domains' restatement"""
    ins = insulation_host(pos1, pos2, count, norm, resolution_bp, (int(window_bp),), n_bins, norm_args, **rule)
    return ins.domain_of_bin(0), int(resolution_bp)


# ----------------------------------------------------------------------------------------------
# device
# ----------------------------------------------------------------------------------------------
def diamond_sums(A: hicnorm.DeviceContactMatrix, norm, windows) -> torch.Tensor:
    """S float64 [len(windows), n] on the device (cgcn_hicinsul_sums: enqueue only).  norm: None or a float64 device vector."""
    from . import _lib
    w = _check_windows(windows)
    dev = A.rowptr.device
    out = torch.zeros(len(w), A.n, dtype=torch.float64, device=dev)
    if A.n == 0:
        return out
    hicmap.device_vector(norm, dev, "norm", optional=True)
    with torch.cuda.device(dev):
        _lib.call("cgcn_hicinsul_sums", n=A.n, rowptr=A.rowptr, col=A.col, val=A.val, norm=norm,
                  n_norm=0 if norm is None else int(norm.numel()), n_windows=len(w), windows=(ctypes.c_int32 * len(w))(*w), out=out)
    return out


def insulation_of_matrix(A: hicnorm.DeviceContactMatrix, norm, resolution_bp, windows, **rule) -> Insulation:
    """rules 2 to 5 from the device matrix: the sums on the device, one read-back of S, VC and the vector, the shared function"""
    S = diamond_sums(A, norm, windows)
    nv = None if norm is None else norm.cpu().numpy()
    valid = hicmap.valid_bins(A.vc.cpu().numpy(), nv)
    return Insulation(windows, resolution_bp, S, valid, insulation_from_sums(S.cpu().numpy(), valid, windows, **_rule(rule)))


# ----------------------------------------------------------------------------------------------
# domains and graphs
# ----------------------------------------------------------------------------------------------
def check_domains(domains, resolution_bp):
    """(domain_of_bin int32 numpy, domain_bp) of rule 7's argument"""
    try:
        dom, bp = domains
    except (TypeError, ValueError):
        raise ValueError("domains must be (domain_of_bin, domain_bp), a dict of HicContacts.domains' keywords, or None") from None
    dom = (dom.cpu().numpy() if torch.is_tensor(dom) else np.asarray(dom)).ravel().astype(np.int32)
    bp, res = int(bp), int(resolution_bp)
    if res < 1 or bp < 1 or bp % res:
        raise ValueError("domain_bp=%r is no multiple of resolution_bp=%r" % (bp, resolution_bp))
    return dom, bp


def same_domain_host(pos1, pos2, dom, domain_bp) -> np.ndarray:
    """rule 7's test per record (bool); a position beyond the vector never matches"""
    b1, b2 = np.asarray(pos1, dtype=np.int64) // domain_bp, np.asarray(pos2, dtype=np.int64) // domain_bp
    inside = (b1 >= 0) & (b2 >= 0) & (b1 < dom.size) & (b2 < dom.size)
    if dom.size == 0:
        return inside
    top = dom.size - 1
    return inside & (dom[np.clip(b1, 0, top)] == dom[np.clip(b2, 0, top)])


def domain_of_windows(window_start, domain_of_bin, domain_bp) -> np.ndarray:
    """the domain of each graph window (int64); -1 for a window beyond the vector"""
    dom = np.asarray(domain_of_bin).ravel()
    b = np.asarray(window_start, dtype=np.int64) // int(domain_bp)
    inside = (b >= 0) & (b < dom.size)
    return np.where(inside, dom[np.clip(b, 0, max(dom.size - 1, 0))] if dom.size else -1, -1).astype(np.int64)


def domain_edge_share(graph_or_csr, domain_of_window):
    """(same_domain_entries, nnz) as exact integers: the stored entries of a graph (hicmap.csr_of's inputs) whose two windows
    lie in one domain.  A negative domain never matches."""
    dom = np.asarray(domain_of_window, dtype=np.int64).ravel()
    row, col, nnz = hicmap.edge_rows(graph_or_csr, dom.size, "domain_of_window")
    return int(np.sum((dom[row] == dom[col]) & (dom[row] >= 0))), nnz
