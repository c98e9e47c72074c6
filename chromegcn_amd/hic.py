"""The top-K Hi-C contact graph from raw contact records: the reference's data/7create_graph_new.py
(get_normalization_values :51-65, get_contact_edge_pairs :67-91, get_top_contact_locs :93-104, create_adj_mat :108-120,
K = hic_edges / 2 :168) for any edge budget and any normalisation vector, on the device (csrc/cgcn_hic.hip) with a numpy
restatement beside it.

The rule, for one chromosome: a record (pos1, pos2, count) survives iff pos1 != pos2 and both positions are windows with
peaks; its value is count / (nv[pos1 // res] * nv[pos2 // res]) in float64, nv = the norm vector with NaN and 0 replaced by
+inf (count itself without a vector); the K survivors that come first in a STABLE descending sort by value are taken;
A[i, j] = A[j, i] = 1 for each of them, i, j the ranks of the two positions among the windows.  Outside the contract: two
records with the same ordered (pos1, pos2), NaN counts, 2 K >= 2^31.  Where a norm vector is taken, the names 'KR', 'VC' and
'SQRTVC' stand for the vector computed from the records themselves (chromegcn_amd/hicnorm.py; HicContacts.norm_vector).

Records coarser than the windows (K562: 5 kb records, 1 kb windows; data/extras/upsample_hic.py:36-44,
data/create_data.py:47-55): with `window_bp` dividing `resolution_bp`, up = resolution_bp / window_bp <= 8, the graph is the
rule above applied to the EXPANDED FILE -- for each record in file order, for a = 0 .. up - 1, for b = 0 .. up - 1, the record
(pos1 + a window_bp, pos2 + b window_bp, count) -- with the same norm, resolution_bp, window_start and K.  All up^2 children
of a record share its two norm bins and so its value; ties are taken in the order of the expanded file; a record (p, p)
yields the up^2 - up ordered pairs a != b, and (p + a, p + b) and (p + b, p + a) both count against K.  Contract: pos1 and
pos2 are multiples of resolution_bp (checked).  expand_contacts_host writes the expanded file out; nothing else here does:
the device filter and the host restatement both read the compact records and expand only the survivors.

Distance (min_distance_bp, expected).  Contact counts fall steeply with genomic distance, so a top-K
cut on the value above is mostly a cut on distance; the reference works around it with a minimum distance
(data/7create_graph_old.py:167, default 1000 in data/create_data.py:28) and a division by Juicer's expected vector
(7create_graph_old.py:124, :153-154, commented out).  Here, for one chromosome, res = resolution_bp, b1 = pos1 // res,
b2 = pos2 // res, d = |b1 - b2|, n_bins = the largest bin + 1 unless given (a smaller one is a ValueError):
  1. Distance sums: raw[d] = sum of count, act[d] = sum of count / (nv[b1] nv[b2]) over the records at distance d (diagonal
     records at d = 0; nv all ones without a vector), float64 [n_bins]; the host statement is np.bincount in record order.  A
     negative or non-finite count, or a negative position, is a ValueError, as in hicnorm.
  2. Expected vector: poss[d] = n_bins - d; w_d = the smallest w >= 0 whose window [max(d - w, 0), min(d + w, n_bins - 1)] has
     sum raw >= min_count (default 400, Juicer's shot-noise mark), the whole range if no window reaches it; the window is
     chosen from the RAW sums for every kind; expected[d] = sum_window act / sum_window poss (hicdist.expected_from_sums, one
     float64 numpy function shared by the device path and the restatement).  Not Juicer's: no scale factor is applied (as
     for the norm vectors; the top-K selection does not see one), and the window rule is ours, in the spirit of
     ExpectedValueCalculation but not its running-window loop.
  3. Scoring: v = (count / (nv[b1] nv[b2])) / ex[d], two IEEE float64 divisions in that order, ex = the expected vector with
     NaN, 0 and negative entries mapped to +inf; a distance outside the vector reads as +inf.  Without an expected vector the
     value is the one above, bit for bit.  With window_bp all up^2 children of a record share its value: d comes from the
     source record's two resolution_bp bins, the expected vector lives at the records' resolution.  expected = "auto": the
     vector of rule 2 computed from the records with the norm the call scores with.
  4. Minimum gap: a record takes part only if |pos1 - pos2| >= min_distance_bp (64-bit).  With window_bp the test is on the
     SOURCE record, before it is expanded (7create_graph_old.py:167-169: the test stands in front of the two `residuals`
     loops).  min_distance_bp = 0 is the rule above; everything else about survival stays; survivor counts count what
     survives both rules.

Contact TEXT becomes records by the rule of chromegcn_amd/hictext.py (HicContacts.from_text, parse_contacts_text_host); the
`.cghic` cache of the records is chromegcn_amd/hiccache.py's.  Their public names are still found here.

Domains (domains; DESIGN.md section 4.17, chromegcn_amd/insulation.py holds the rule).  domains = (domain_of_bin, domain_bp):
a record takes part only if dom[pos1 // domain_bp] == dom[pos2 // domain_bp], a position beyond the vector never matching;
the test is on the SOURCE record, where the minimum gap is tested.  domain_bp must be a multiple of resolution_bp.  A dict
stands for the vector computed from the records (HicContacts.domains / insulation.domains_host with these keywords).  Named
norms and expected = "auto" are still computed from ALL records; the kept records stay in file order.  domains = None is the
rule above, bit for bit.

Compartments (chromegcn_amd/compartments.py holds the rule).  HicContacts.compartments calls the A/B
compartments of the records; its as_domains() with its resolution is a `domains` pair like any other, so the restriction to
contacts within one compartment needs nothing of the builders.

Loops (loops; DESIGN.md section 4.19, chromegcn_amd/loops.py holds the rule).  loops = a Loops, (Loops, pad_bins) or a dict of
HicContacts.loops' keywords (plus pad_bins) computed from the records: a record takes part only if its pixel
(pos1 // res, pos2 // res), lower bin first and res the loops' resolution, lies within Chebyshev distance pad_bins (default 1)
of some loop's peak.  The test is on the SOURCE record; named norms, expected = "auto" and a dict of loops are still computed
from ALL records; the kept records stay in file order; with domains both tests must hold.  loops = None is the rule above, bit
for bit.

Pile-ups (chromegcn_amd/pileup.py holds the rule).  HicContacts.pileup sums the map in a window around
every centre of a list (loops, graph edges, their shifted controls), per group; it reads the records and changes no graph.

Two maps compared (chromegcn_amd/mapcompare.py holds the rule).  HicContacts.scc is the stratum-adjusted
correlation coefficient of this object's map and another's; it reads the records of both and changes no graph."""
from __future__ import annotations

from typing import Dict, NamedTuple, Optional

import numpy as np
import scipy.sparse as sp
import torch

from . import graph as G
# the names that lived here before the text rule, the cache format and the staging buffers got modules of their own
from ._textio import release_text_staging  # noqa: F401
from .compartments import (Compartments, compartment_edge_share, compartment_metrics, compartments_host,  # noqa: F401
                           compartments_of_matrix, label_density)
from .hiccache import (HostContacts, contact_cache_path, load_contacts_cache, load_contacts_text,  # noqa: F401
                       save_contacts_cache, windows_from_bed)
from .loops import Loops, loop_edge_share, loops_host, loops_of_matrix, same_loop_host  # noqa: F401
from .pileup import Pileup, apa_scores, centres_of_graph, pileup_host, pileup_of_matrix, shifted_centres  # noqa: F401
from .hictext import TEXT_LINE_MAX, TEXT_MALFORMED, TEXT_SLOW, parse_contacts_text, parse_contacts_text_host  # noqa: F401


# ----------------------------------------------------------------------------------------------
# host restatement (numpy / scipy only): the CPU path and the yardstick of the device build
# ----------------------------------------------------------------------------------------------
def _budget(hic_edges) -> int:
    k = int(hic_edges / 2.)  # data/7create_graph_new.py:168
    if k < 0 or 2 * k >= 2 ** 31:
        raise ValueError("hic_edges=%r is outside [0, 2^31)" % (hic_edges,))
    return k


def _windows(window_start) -> np.ndarray:
    ws = np.ascontiguousarray(np.asarray(window_start), dtype=np.int32)
    if ws.ndim != 1 or (ws.size > 1 and not np.all(ws[1:] > ws[:-1])):
        raise ValueError("window_start must be one strictly increasing vector")
    return ws


def _check_norm(norm, resolution_bp, ws):
    if norm is None:
        return
    if int(resolution_bp) < 1:
        raise ValueError("resolution_bp must be positive")
    if ws.size and int(ws[-1]) // int(resolution_bp) >= int(norm.shape[0]):
        raise ValueError("the norm vector has %d bins but the last window is in bin %d"
                         % (norm.shape[0], int(ws[-1]) // int(resolution_bp)))


def _upsample(resolution_bp, window_bp) -> int:
    """up = resolution_bp / window_bp (1 for window_bp = None: the records are at the windows' own resolution)"""
    if window_bp is None:
        return 1
    res, wbp = int(resolution_bp), int(window_bp)
    if res < 1 or wbp < 1 or res % wbp:
        raise ValueError("window_bp=%r does not divide resolution_bp=%r" % (window_bp, resolution_bp))
    if res // wbp > 8:
        raise ValueError("resolution_bp / window_bp = %d: more than 8 is not supported" % (res // wbp))
    return res // wbp


def _check_grid(p1, p2, resolution_bp):
    if np.any(p1 % int(resolution_bp)) or np.any(p2 % int(resolution_bp)):
        raise ValueError("pos1 / pos2 hold positions that are no multiple of resolution_bp=%d" % int(resolution_bp))


def expand_contacts_host(pos1, pos2, count, resolution_bp, window_bp):
    """The expanded file of rule 1 as arrays (int32 [up^2 M], int32 [up^2 M], count's dtype [up^2 M]): the loop of
    data/extras/upsample_hic.py:36-44, `a` outer and `b` inner.  up^2 times the memory: for tests and tools."""
    up = _upsample(resolution_bp, window_bp)
    p1, p2 = np.asarray(pos1, dtype=np.int64), np.asarray(pos2, dtype=np.int64)
    step = np.arange(up, dtype=np.int64) * (int(resolution_bp) // up)
    e1 = np.broadcast_to(p1[:, None, None] + step[None, :, None], (p1.size, up, up)).reshape(-1)
    e2 = np.broadcast_to(p2[:, None, None] + step[None, None, :], (p2.size, up, up)).reshape(-1)
    if e1.size and max(int(e1.max()), int(e2.max())) >= 2 ** 31:
        raise ValueError("an expanded position does not fit int32")
    return e1.astype(np.int32), e2.astype(np.int32), np.repeat(np.asarray(count), up * up)


_POPCOUNT8 = np.array([bin(x).count("1") for x in range(256)], dtype=np.int64)


def _gap(min_distance_bp) -> int:
    g = int(min_distance_bp)
    if g < 0:
        raise ValueError("min_distance_bp must not be negative")
    return g


def _auto_expected(expected) -> bool:
    """whether `expected` asks for the vector computed from the records; any string but "auto" is an error"""
    if isinstance(expected, str) and expected != "auto":
        raise ValueError("expected=%r is none of None, a vector, 'auto'" % (expected,))
    return isinstance(expected, str)


def _survivors_up(p1, p2, ws, wbp, up, keep=None):
    """(source record, child a, child b, i, j) of the survivors of the expanded file, in its order, from the compact records:
    per record the two up-bit masks of its children that are windows; only records with a survivor are expanded.  keep: the
    source records that take part (the minimum gap)."""
    n = ws.size

    def masks(p):
        m = np.zeros(p.size, np.uint8)
        for a in range(up):
            c = p + a * wbp
            m |= (ws[np.minimum(np.searchsorted(ws, c), n - 1)] == c).astype(np.uint8) << np.uint8(a)
        return m

    m1, m2 = masks(p1), masks(p2)
    if keep is not None:
        m1 = np.where(keep, m1, np.uint8(0))
    cnt = _POPCOUNT8[m1] * _POPCOUNT8[m2] - np.where(p1 == p2, _POPCOUNT8[m1 & m2], 0)
    rec = np.flatnonzero(cnt > 0)
    bit = np.arange(up, dtype=np.uint8)
    alive = (((m1[rec, None, None] >> bit[None, :, None]) & 1) & ((m2[rec, None, None] >> bit[None, None, :]) & 1)).astype(bool)
    alive &= ~((p1[rec] == p2[rec])[:, None, None] & np.eye(up, dtype=bool)[None])
    r, a, b = np.nonzero(alive)   # C order: record, a, b = the order of the expanded file
    src = rec[r]
    assert src.size == int(cnt.sum())
    return src, a, b, np.searchsorted(ws, p1[src] + a * wbp), np.searchsorted(ws, p2[src] + b * wbp)


def _host_domains(domains, pos1, pos2, count, resolution_bp):
    """the builders' `domains` on the host: None, or (domain_of_bin int32, domain_bp) -- a dict is computed from the records"""
    if domains is None:
        return None
    from . import insulation
    if isinstance(domains, dict):
        domains = insulation.domains_host(pos1, pos2, count, **domains)
    return insulation.check_domains(domains, resolution_bp)


def _host_loops(loops, pos1, pos2, count):
    """the builders' `loops` on the host: None, or (Loops, pad_bins) -- a dict is computed from the records"""
    if loops is None:
        return None
    from . import loops as LP
    if isinstance(loops, dict):
        kw = dict(loops)
        pad = kw.pop("pad_bins", 1)
        loops = (LP.loops_host(pos1, pos2, count, **kw), pad)
    return LP.check_loops(loops)


def survivor_values(pos1, pos2, count, norm, resolution_bp, window_start, window_bp=None, min_distance_bp=0, expected=None,
                    expected_args=None, domains=None, loops=None):
    """(record index, i, j, value) of the surviving records in file order (rules 1 and 2).  With window_bp: of the surviving
    records of the expanded file, the index being the position in it.  min_distance_bp, expected (None, a vector, or "auto":
    hicdist.expected_vector_host with this norm and expected_args): the minimum gap and the observed / expected value of the
    module docstring.  domains, loops: the module docstring's; the indices stay those of the whole file."""
    up = _upsample(resolution_bp, window_bp)
    domains = _host_domains(domains, pos1, pos2, count, resolution_bp)
    loops = _host_loops(loops, pos1, pos2, count)
    gap = _gap(min_distance_bp)
    ws = _windows(window_start).astype(np.int64)
    p1, p2 = np.asarray(pos1, dtype=np.int64), np.asarray(pos2, dtype=np.int64)
    if up > 1:
        _check_grid(p1, p2, resolution_bp)
    n = ws.size
    if n == 0 or p1.size == 0:
        e = np.zeros(0, np.int64)
        return e, e, e, np.zeros(0, np.float64)
    keep = (np.abs(p1 - p2) >= gap) if gap else None   # the source records that take part
    if domains is not None:
        from . import insulation
        same = insulation.same_domain_host(p1, p2, *domains)
        keep = same if keep is None else keep & same
    if loops is not None:
        near = same_loop_host(p1, p2, *loops)
        keep = near if keep is None else keep & near
    if up > 1:
        src, a, b, i, j = _survivors_up(p1, p2, ws, int(resolution_bp) // up, up, keep)
        idx = src * (up * up) + a * up + b
    else:
        i = np.minimum(np.searchsorted(ws, p1), n - 1)
        j = np.minimum(np.searchsorted(ws, p2), n - 1)
        idx = src = np.flatnonzero((p1 != p2) & (ws[i] == p1) & (ws[j] == p2) & (True if keep is None else keep))
        i, j = i[idx], j[idx]
    v = np.asarray(count)[src].astype(np.float64)
    if norm is not None:
        nv = np.array(norm, dtype=np.float64)
        _check_norm(nv, resolution_bp, ws)
        nv[np.isnan(nv) | (nv == 0.0)] = np.inf
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            v = v / (nv[p1[src] // int(resolution_bp)] * nv[p2[src] // int(resolution_bp)])
    if expected is not None:
        from . import hicdist
        if _auto_expected(expected):
            expected = hicdist.expected_vector_host(pos1, pos2, count, norm, resolution_bp, **(expected_args or {}))
        if int(resolution_bp) < 1:
            raise ValueError("resolution_bp must be positive")
        ex = hicdist.clean_vector(expected)
        d = np.abs(p1[src] // int(resolution_bp) - p2[src] // int(resolution_bp))
        e = np.where(d < ex.size, ex[np.minimum(d, max(ex.size - 1, 0))], np.inf) if ex.size else np.full(d.shape, np.inf)
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            v = v / e
    return idx, i, j, v


def build_hic_graph_host(pos1, pos2, count, norm, resolution_bp, window_start, hic_edges, window_bp=None,
                         norm_args=None, min_distance_bp=0, expected=None, expected_args=None, domains=None,
                         loops=None) -> sp.csr_matrix:
    """The {0,1} float64 CSR the reference's step 7 pickles (symmetric, zero diagonal, sorted columns).  With window_bp: of
    the expanded file, which is never written out (the CPU path for coarse records at full size).  norm = 'KR' / 'VC' /
    'SQRTVC': the vector computed from the records (hicnorm.hic_norm_vector_host with norm_args).  min_distance_bp, expected
    (None, a vector, or "auto": hicdist.expected_vector_host with the same norm and expected_args = n_bins / min_count).
    domains: None, (domain_of_bin, domain_bp), or a dict of insulation.domains_host's keywords (the module docstring).
    loops: None, a Loops, (Loops, pad_bins), or a dict of loops.loops_host's keywords plus pad_bins (the module docstring)."""
    ws = _windows(window_start)
    n = ws.size
    k = _budget(hic_edges)
    if _auto_expected(expected):
        from . import hicdist
        expected = hicdist.expected_vector_host(pos1, pos2, count, norm, resolution_bp, norm_args=norm_args, **(expected_args or {}))
    if isinstance(norm, str):
        from . import hicnorm
        norm = hicnorm.resolve_norm_host(pos1, pos2, count, norm, resolution_bp, norm_args=norm_args)
        norm = hicnorm.pad_vector(norm, int(ws[-1]) // int(resolution_bp) + 1 if n else 0)
    _, i, j, v = survivor_values(pos1, pos2, count, norm, resolution_bp, window_start, window_bp, min_distance_bp, expected,
                                 domains=domains, loops=loops)
    take = np.argsort(-v, kind="stable")[:k]
    i, j = i[take], j[take]
    a = sp.coo_matrix((np.ones(2 * i.size), (np.concatenate([i, j]), np.concatenate([j, i]))), shape=(n, n)).tocsr()
    a.sum_duplicates()
    a.data[:] = 1.0
    a.sort_indices()
    return sp.csr_matrix(a, dtype=np.float64)


# ----------------------------------------------------------------------------------------------
# device build
# ----------------------------------------------------------------------------------------------
class _Route(NamedTuple):
    """The top-K entry points of one (resolution_bp, window_bp): direct when the records are at the windows' resolution,
    else the `_up` forms.  HicContacts._route makes it; _count and build_raw add "_dist" for a gap or an expected vector."""
    suffix: str          # "" or "_up", behind cgcn_hic_count / cgcn_hic_build
    workspace_fn: str    # cgcn_hic_workspace_bytes or cgcn_hic_up_workspace_bytes
    extra: dict          # what the _up forms take besides: resolution_bp, window_bp, n_window_bins
    what: str            # how the workspace's unsupported-shape error starts


class HicContacts:
    """One chromosome's contact records resident on the device, so that a sweep over edge budgets and norm vectors
    uploads them once.  The survivor count of a window set (it sizes the build's buffers and depends on neither the
    budget nor the norm vector) is read back once per window set and kept."""

    def __init__(self, pos1, pos2, count, device="cuda"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("HicContacts needs a GPU; build_hic_graph_host is the CPU path")
        self.pos1 = self._up(pos1, torch.int32)
        self.pos2 = self._up(pos2, torch.int32)
        self.count = self._up(count, torch.float64)
        if not (self.pos1.ndim == 1 and self.pos1.shape == self.pos2.shape == self.count.shape):
            raise ValueError("pos1, pos2 and count must be vectors of one length")
        self.M = int(self.pos1.numel())
        self._ws_host = self._ws_dev = None
        self._survivors = {}     # of the current window set, per (resolution_bp, window_bp, min_distance_bp); direct: (None, None, gap)
        self._on_grid = set()    # the resolutions of which every position is known to be a multiple
        self._vectors = []   # (the caller's object, its device copy): a sweep passes the same vector again
        self._matrices = {}  # (resolution_bp, n_bins or None) -> hicnorm.DeviceContactMatrix
        self._norms = {}     # norm_vector's argument tuple -> (vector, info)
        self._dist_sums = {}       # distance_sums' argument tuple -> (raw, act, host syncs)
        self._expected = {}        # expected_vector's argument tuple -> (vector, info)
        self._insulations = {}     # insulation's argument tuple -> insulation.Insulation
        self._compartments = {}    # compartments' argument tuple (without orient) -> compartments.Compartments
        self._within = []          # (domain_of_bin, domain_bp, the HicContacts of the kept records): the last few selections
        self._loops = {}           # loops' argument tuple -> loops.Loops
        self._within_loops = []    # (Loops, pad_bins, the HicContacts of the kept records): the last few selections
        self._pileup_bands = {}    # (resolution_bp, n_bins, width) -> the raw band of pileup()
        self._pileup_values = {}   # pileup's norm, band and value tuple -> the value band
        self.text_info = None   # from_text: {n_bytes, slow_lines, parse_calls}

    @classmethod
    def from_host(cls, c: HostContacts, device="cuda") -> "HicContacts":
        return cls(c.pos1, c.pos2, c.count, device)

    def to_host(self, norms=None, resolution_bp: int = 1000, window_start=None) -> HostContacts:
        """the records as a HostContacts (one read-back), so that save_contacts_cache can write them"""
        return HostContacts(self.pos1.cpu().numpy(), self.pos2.cpu().numpy(), self.count.cpu().numpy(), dict(norms or {}),
                            int(resolution_bp), None if window_start is None else _windows(window_start))

    @classmethod
    def from_text(cls, path_or_bytes, device="cuda", chunk_bytes: int = 32 << 20, flag_capacity: int = 1 << 16,
                  timings: Optional[dict] = None) -> "HicContacts":
        """The records of contact text (a path, or bytes / bytearray / memoryview) by the rule of hictext's docstring, parsed
        on the device: the file is read in chunks of `chunk_bytes` through two pinned staging buffers into one device text
        buffer, cgcn_text_count sizes the arrays (one sync), cgcn_text_parse fills them and lists the lines that are not fast
        (a second call when more than `flag_capacity` are), those alone are parsed on the host and patched in, and the text
        buffer is released.  The records never visit the host.  The two staging buffers (2 x chunk_bytes of pinned host
        memory) stay allocated for the next call until release_text_staging(); they are module state, so from_text must not
        run in two threads at once.  Every line that is not fast costs a Python-level seek, readline and float() here, after
        the device pass: a file that is slow throughout (a 17-digit normalised dump) is read faster by load_contacts_text.
        `text_info` of the result: n_bytes, slow_lines (int64, the
        records parsed on the host), parse_calls.  timings: a dict that receives the seconds of every stage (with a device
        sync behind each)."""
        return parse_contacts_text(cls, path_or_bytes, device, chunk_bytes, flag_capacity, timings)

    def _up(self, a, dtype) -> torch.Tensor:
        t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
        return t.to(device=self.device, dtype=dtype).contiguous()

    def contact_matrix(self, resolution_bp, n_bins=None):
        """the symmetric fp64 contact matrix of the records on the device (hicnorm.DeviceContactMatrix), aggregated once per
        (resolution_bp, n_bins) and kept"""
        from . import hicnorm
        key = (int(resolution_bp), None if n_bins is None else int(n_bins))
        if key not in self._matrices:
            a = hicnorm.aggregate_contacts(self.pos1, self.pos2, self.count, key[0], key[1])
            self._matrices[key] = self._matrices[(key[0], a.n)] = a
        return self._matrices[key]

    def norm_vector(self, kind, resolution_bp, n_bins=None, tol=1e-6, max_mvp=1000, min_row_nnz=1, kr_retry=True,
                    return_info=False, long_row_nnz=-1):
        """The 'KR', 'VC' or 'SQRTVC' vector of the records (hicnorm's docstring) as a float64 device tensor [n_bins]; NaN
        at empty (KR: and excluded) bins.  The three kinds share one aggregation; vectors are kept per argument tuple.  A KR
        that did not converge is returned as it is with info["converged"] False: build(norm="KR") raises instead.
        return_info: (vector, info) -- KR: converged, residual, mvp, outer, kept, excluded, min_row_nnz, ladder, host_syncs."""
        from . import hicnorm
        kr = dict(tol=float(tol), max_mvp=int(max_mvp), min_row_nnz=int(min_row_nnz), kr_retry=bool(kr_retry))
        key = (hicnorm._kind(kind), int(resolution_bp), None if n_bins is None else int(n_bins), int(long_row_nnz))
        key += tuple(sorted(kr.items())) if kind == "KR" else ()
        if key not in self._norms:
            a = self.contact_matrix(resolution_bp, n_bins)
            self._norms[key] = hicnorm.vector_from_matrix(a, kind, long_row_nnz=int(long_row_nnz), **(kr if kind == "KR" else {}))
        v, info = self._norms[key]
        return (v, dict(info)) if return_info else v

    def _named_norm(self, norm, resolution_bp, norm_args, **size):
        """'KR' / 'VC' / 'SQRTVC' -> the vector computed from the records (HicNormError for a KR that did not converge);
        size: n_bins, where the caller and not norm_args says it"""
        from . import hicnorm
        v, info = self.norm_vector(norm, resolution_bp, return_info=True, **size, **(norm_args or {}))
        hicnorm._require_converged(info)
        return v

    def _map_vectors(self, a, norm, resolution_bp, norm_args, expected=None, expected_args=None):
        """(nv, ex): the device norm vector (or None) and expected vector of an analysis of the map `a` = contact_matrix(...).
        norm: None, a vector, or a name (_named_norm at a's size); expected: None (the analysis reads none: ex is None), a
        vector, or "auto" (expected_vector with this norm and expected_args).  A caller's own vector is uploaded, never kept."""
        ex = None
        if isinstance(expected, str):
            ex = self.expected_vector(norm, resolution_bp, n_bins=a.n, norm_args=norm_args, **(expected_args or {}))
        elif expected is not None:
            ex = self._norm(expected)
        nv = self._named_norm(norm, resolution_bp, norm_args, n_bins=a.n) if isinstance(norm, str) else self._norm(norm)
        return nv, ex

    @staticmethod
    def _norm_key(norm, norm_args):
        """the part of a cache key that names the norm; None for a caller's vector (not cached)"""
        if norm is None:
            return ("RAW",)
        if isinstance(norm, str):
            return (norm,) + tuple(sorted((norm_args or {}).items()))
        return None

    def distance_sums(self, norm, resolution_bp, n_bins=None, norm_args=None):
        """(raw, act) of the module docstring's rule 1 as float64 device tensors [n_bins] (cgcn_hicdist_sums).  norm: None
        (RAW), a vector, or 'KR' / 'VC' / 'SQRTVC' (norm_vector with norm_args; a KR that did not converge raises
        HicNormError).  One read-back of the bad-record flags, and one more of the largest bin when n_bins is None and no
        contact matrix of this resolution is resident.  Kept per argument tuple for None and the three names."""
        return self._distance_sums(norm, resolution_bp, n_bins, norm_args)[:2]

    def _distance_sums(self, norm, resolution_bp, n_bins, norm_args):
        from . import _lib, hicnorm
        res = int(resolution_bp)
        if res < 1:
            raise ValueError("resolution_bp must be positive")
        given = None if n_bins is None else int(n_bins)
        if given is not None and given < 0:
            raise ValueError("n_bins must not be negative")
        nk = self._norm_key(norm, norm_args)
        key = None if nk is None else nk + (res, given)
        if key is not None and key in self._dist_sums:
            return self._dist_sums[key]
        nv = self._named_norm(norm, res, norm_args, n_bins=given) if isinstance(norm, str) else self._norm(norm)
        syncs = 0
        with torch.cuda.device(self.device):
            sizes = torch.zeros(2, dtype=torch.int64, device=self.device)
            args = dict(M=self.M, pos1=self.pos1, pos2=self.pos2, count=self.count, norm=nv,
                        n_norm=0 if nv is None else int(nv.numel()), resolution_bp=res)
            n = given
            if n is None and (res, None) in self._matrices:
                n = self._matrices[(res, None)].n   # aggregate_contacts has checked the records and counted the bins
            if n is None:
                wsp, need = _lib.workspace_for("cgcn_hicdist_workspace_bytes", self.device, "Hi-C distance sums, M=%d" % self.M,
                                               M=self.M, n_bins=0)
                _lib.call("cgcn_hicdist_sums", n_bins=0, workspace=wsp, workspace_bytes=need, raw_out=None, act_out=None,
                          sizes=sizes, **args)
                flags, n = sizes.tolist()
                syncs += 1
                hicnorm._bad_records(flags)
            raw = torch.zeros(n, dtype=torch.float64, device=self.device)
            act = torch.zeros(n, dtype=torch.float64, device=self.device)
            if n:
                wsp, need = _lib.workspace_for("cgcn_hicdist_workspace_bytes", self.device,
                                               "Hi-C distance sums, M=%d n_bins=%d" % (self.M, n), M=self.M, n_bins=n)
                _lib.call("cgcn_hicdist_sums", n_bins=n, workspace=wsp, workspace_bytes=need, raw_out=raw, act_out=act, sizes=sizes,
                          **args)
                flags, top = sizes.tolist()
                syncs += 1
                hicnorm._bad_records(flags)
                if flags & 4:
                    raise ValueError("n_bins=%d but the records reach bin %d" % (n, top - 1))
            elif self.M:
                raise ValueError("n_bins=0 but there are records")
        out = (raw, act, syncs)
        if key is not None:
            self._dist_sums[key] = out
        return out

    def expected_vector(self, norm, resolution_bp, n_bins=None, min_count=400, return_info=False, norm_args=None):
        """The expected vector of the module docstring's rule 2 as a float64 device tensor [n_bins]: distance_sums, one
        read-back of raw and act (2 n_bins doubles), hicdist.expected_from_sums on the host, one upload.  return_info:
        (vector, {w_max, whole_range: the distances whose window is the whole range, host_syncs}).  Kept per argument tuple
        for None and the three names."""
        from . import hicdist
        nk = self._norm_key(norm, norm_args)
        key = None if nk is None else nk + (int(resolution_bp), None if n_bins is None else int(n_bins), float(min_count))
        if key is None or key not in self._expected:
            raw, act, syncs = self._distance_sums(norm, resolution_bp, n_bins, norm_args)
            sums = torch.stack([raw, act]).cpu().numpy()
            ex, info = hicdist.expected_from_sums(sums[0], sums[1], min_count, return_info=True)
            info = {"w_max": info["w_max"], "whole_range": info["whole_range"], "host_syncs": syncs + 1}
            hit = (torch.from_numpy(ex).to(self.device), info)
            if key is None:
                return (hit[0], dict(info)) if return_info else hit[0]
            self._expected[key] = hit
        v, info = self._expected[key]
        return (v, dict(info)) if return_info else v

    def insulation(self, norm="VC", resolution_bp=10000, windows_bp=(100000, 250000), n_bins=None, norm_args=None, **rule):
        """The insulation profile of the records (chromegcn_amd/insulation.py's rule) at the windows `windows_bp`, multiples of
        resolution_bp: the diamond sums on the device from contact_matrix(resolution_bp, n_bins) (cgcn_hicinsul_sums), one
        read-back of the sums, the row sums and the vector, then insulation.insulation_from_sums.  norm: None, a vector at
        resolution_bp, or 'KR' / 'VC' / 'SQRTVC' (norm_vector with norm_args; a KR that did not converge raises HicNormError);
        VC is the default because it cannot fail to converge.  **rule: min_valid_share, span, min_strength.  Kept per
        argument tuple for None and the three names."""
        from . import insulation as INS
        res = int(resolution_bp)
        w = INS.windows_in_bins(windows_bp, res)
        INS._rule(rule)
        nk = self._norm_key(norm, norm_args)
        span = rule.get("span")
        key = None if nk is None else nk + (res, w, None if n_bins is None else int(n_bins)) + tuple(
            sorted({**rule, "span": tuple(np.ravel(span).tolist()) if span is not None else None}.items()))
        if key is not None and key in self._insulations:
            return self._insulations[key]
        a = self.contact_matrix(res, n_bins)
        nv, _ = self._map_vectors(a, norm, res, norm_args)
        out = INS.insulation_of_matrix(a, nv, res, w, **rule)
        if key is not None:
            self._insulations[key] = out
        return out

    def domains(self, window_bp, norm="VC", resolution_bp=10000, n_bins=None, norm_args=None, **rule):
        """(domain_of_bin int32 numpy [n_bins], resolution_bp) of insulation(...) at the one window `window_bp`: what the
        builders' `domains` takes"""
        ins = self.insulation(norm, resolution_bp, (int(window_bp),), n_bins=n_bins, norm_args=norm_args, **rule)
        return ins.domain_of_bin(0), int(resolution_bp)

    def compartments(self, norm="VC", resolution_bp=100000, n_bins=None, norm_args=None, **rule):
        """The A/B compartments of the records (chromegcn_amd/compartments.py's rule): the dense O/E Pearson map and its
        leading eigenvectors on the device from contact_matrix(resolution_bp, n_bins).  norm: None, a vector at resolution_bp,
        or 'KR' / 'VC' / 'SQRTVC' (norm_vector with norm_args; a KR that did not converge raises HicNormError).  **rule: n_eigs,
        ignore_diags, orient, tol, max_iter, check_every.  Kept per argument tuple for None and the three names; `orient` is
        applied to the kept result and takes no part in the tuple."""
        from . import compartments as CP
        res = int(resolution_bp)
        orient = rule.pop("orient", None)
        checked = CP._rule(rule)
        nk = self._norm_key(norm, norm_args)
        key = None if nk is None else nk + (res, None if n_bins is None else int(n_bins)) + tuple(
            sorted((k, v) for k, v in checked.items() if k != "orient"))
        out = None if key is None else self._compartments.get(key)
        if out is None:
            a = self.contact_matrix(res, n_bins)
            nv, _ = self._map_vectors(a, norm, res, norm_args)
            out = CP.compartments_of_matrix(a, nv, res, **rule)
            if key is not None:
                self._compartments[key] = out
        return out if orient is None else out.oriented(orient)

    def within_domains(self, domain_of_bin, domain_bp) -> "HicContacts":
        """the records whose two ends lie in one domain (a position beyond the vector never matches), in file order, as a
        HicContacts of their own.  Boolean indexing: one host sync for the size."""
        bp = int(domain_bp)
        if bp < 1:
            raise ValueError("domain_bp must be positive")
        dom = self._up(domain_of_bin, torch.int32).ravel()
        with torch.cuda.device(self.device):
            b1 = torch.div(self.pos1, bp, rounding_mode="floor").long()
            b2 = torch.div(self.pos2, bp, rounding_mode="floor").long()
            n = int(dom.numel())
            keep = (b1 >= 0) & (b2 >= 0) & (b1 < n) & (b2 < n)
            if n:
                keep &= dom[b1.clamp(0, n - 1)] == dom[b2.clamp(0, n - 1)]
            return HicContacts(self.pos1[keep], self.pos2[keep], self.count[keep], self.device)

    def _selection(self, domains, resolution_bp) -> "HicContacts":
        """within_domains for the builders' `domains` (a pair or a dict of domains' keywords); the last few are kept, so
        that a sweep over budgets or norms selects once"""
        from . import insulation as INS
        if isinstance(domains, dict):
            domains = self.domains(**domains)
        dom, bp = INS.check_domains(domains, resolution_bp)
        for d, b, c in self._within:
            if b == bp and d.shape == dom.shape and np.array_equal(d, dom):
                return c
        c = self.within_domains(dom, bp)
        self._within = self._within[-3:] + [(dom, bp, c)]
        return c

    def loops(self, norm="VC", resolution_bp=10000, expected="auto", n_bins=None, norm_args=None, expected_args=None, **rule):
        """The chromatin loops of the records (chromegcn_amd/loops.py's rule): the band and the two stencil passes on the device
        from contact_matrix(resolution_bp, n_bins), thresholds and clusters on the host.  norm: None, a vector at resolution_bp,
        or 'KR' / 'VC' / 'SQRTVC' (norm_vector with norm_args; a KR that did not converge raises HicNormError); expected: "auto"
        (expected_vector with this norm and expected_args = min_count) or a float64 vector.  **rule: loops.loop_rule's.  Kept per
        argument tuple for None and the three names with expected = "auto"."""
        from . import hicmap, loops as LP
        res = int(resolution_bp)
        checked = LP.loop_rule(res, 0, **rule)
        nk = self._norm_key(norm, norm_args) if hicmap.auto_expected(expected) else None
        key = None if nk is None else nk + (res, None if n_bins is None else int(n_bins), checked) + tuple(
            sorted((expected_args or {}).items()))
        if key is not None and key in self._loops:
            return self._loops[key]
        a = self.contact_matrix(res, n_bins)
        LP.loop_rule(res, a.n, **rule)   # the size guard, before anything is allocated
        nv, ex = self._map_vectors(a, norm, res, norm_args, expected, expected_args)
        out = LP.loops_of_matrix(a, nv, ex, res, **rule)
        if key is not None:
            self._loops[key] = out
        return out

    def pileup(self, centres, group=None, n_groups=None, norm="VC", resolution_bp=10000, expected="auto", value="oe", w=None,
               corner=None, min_dist=None, max_distance_bp=2_000_000, n_bins=None, norm_args=None, expected_args=None):
        """The pile-up of the map around `centres` (chromegcn_amd/pileup.py's rule): a Loops (its peaks), a pair of integer
        arrays or a pair of device tensors, in bins of resolution_bp; group: a group id per centre (None: one group), n_groups
        its range (None: the largest id + 1, one read-back for a device tensor).  norm, expected: loops()'s; expected is read
        for value = "oe" alone.  The raw band and the value band are kept per argument tuple for None and the three names with
        expected = "auto", so that loops, graph edges and their controls on one map share them."""
        from . import hicmap, pileup as PU
        res = int(resolution_bp)
        G = PU._n_groups(group, n_groups)
        rule = dict(value=value, w=w, corner=corner, min_dist=min_dist, max_distance_bp=max_distance_bp)
        PU.pileup_rule(res, 0, G, **rule)
        ci, cj = PU._centres_of(centres)
        if not torch.is_tensor(ci):
            PU._centre_arrays(ci, cj, None if torch.is_tensor(group) else group)
        auto = hicmap.auto_expected(expected)
        a = self.contact_matrix(res, n_bins)
        r = PU.pileup_rule(res, a.n, G, **rule)   # the size guard, before anything is allocated
        bkey = (res, a.n, r.width)
        if bkey not in self._pileup_bands:
            self._pileup_bands[bkey] = hicmap.device_band(a, r.width)
        nk = self._norm_key(norm, norm_args) if (auto or r.value != "oe") else None
        key = None if nk is None else nk + bkey + (r.value,) + (tuple(sorted((expected_args or {}).items())) if r.value == "oe"
                                                                 else ())
        vb = None if key is None else self._pileup_values.get(key)
        if vb is None:
            nv, ex = self._map_vectors(a, norm, res, norm_args, expected if r.value == "oe" else None, expected_args)
            vb = PU.value_band(self._pileup_bands[bkey], a.vc, nv, ex, r)
            if key is not None:
                self._pileup_values[key] = vb
        return PU.pileup_sums(vb, ci, cj, group, G, r)

    def scc(self, other: "HicContacts", norm=None, resolution_bp=40000, h=5, max_distance_bp=5_000_000, min_dist=1, n_bins=None,
            norm_args=None):
        """The stratum-adjusted correlation coefficient of this map and `other` (chromegcn_amd/mapcompare.py's rule), a
        MapComparison.  Both are binned at resolution_bp with n_bins = the larger of the two unless n_bins says it.  norm: None
        (the observed counts), 'KR' / 'VC' / 'SQRTVC' (each map's vector from its own records, norm_vector with norm_args), a
        vector for both, or a pair with one entry per map.  h: the box half-width, or a sequence of them: a list with one
        result per value, the bands and the validity bytes formed once.  One read-back of the sums per h (and one of the
        validity bytes)."""
        from . import mapcompare as MC
        many = isinstance(h, (tuple, list, np.ndarray))
        hs = [int(v) for v in h] if many else [int(h)]
        for v in hs:
            MC.scc_rule(resolution_bp, 0, v, max_distance_bp, min_dist)
        res = int(MC.scc_rule(resolution_bp, 0, 0, max_distance_bp, min_dist).res)
        if n_bins is None:
            n = max(self.contact_matrix(res).n, other.contact_matrix(res).n)
        else:
            n = int(n_bins)
        rules = [MC.scc_rule(res, n, v, max_distance_bp, min_dist) for v in hs]   # the size guard, before anything is allocated
        a, b = self.contact_matrix(res, n), other.contact_matrix(res, n)
        norm_a, norm_b = MC.norm_pair(norm)
        nva, _ = self._map_vectors(a, norm_a, res, norm_args)
        nvb, _ = other._map_vectors(b, norm_b, res, norm_args)
        out = MC.scc_of_matrices(a, b, nva, nvb, rules)
        return out if many else out[0]

    def within_loops(self, loops, pad_bins=1) -> "HicContacts":
        """the records whose pixel lies in some loop's footprint (loops.py's rule 12), in file order, as a HicContacts of their
        own: a sorted int64 key table, torch.searchsorted, boolean indexing -- one host sync for the size"""
        from . import loops as LP
        loops, pad = LP.check_loops((loops, pad_bins))
        res = loops.resolution_bp
        with torch.cuda.device(self.device):
            keys = torch.from_numpy(loops.footprint_keys(pad)).to(self.device)
            b1 = torch.div(self.pos1, res, rounding_mode="floor").long()
            b2 = torch.div(self.pos2, res, rounding_mode="floor").long()
            lo, hi = torch.minimum(b1, b2), torch.maximum(b1, b2)
            keep = (lo >= 0) & (hi < loops.n)
            if keys.numel():
                key = lo * LP._KEY + hi
                at = torch.searchsorted(keys, key).clamp(max=keys.numel() - 1)
                keep &= keys[at] == key
            else:
                keep &= False
            return HicContacts(self.pos1[keep], self.pos2[keep], self.count[keep], self.device)

    def _resolve_loops(self, loops):
        """(Loops, pad_bins) of the builders' `loops`; a dict is computed from THESE records"""
        from . import loops as LP
        if isinstance(loops, dict):
            kw = dict(loops)
            pad = kw.pop("pad_bins", 1)
            loops = (self.loops(**kw), pad)
        return LP.check_loops(loops)

    def _loop_selection(self, loops, pad) -> "HicContacts":
        """within_loops, the last few kept"""
        for lp, pd, c in self._within_loops:
            if lp is loops and pd == pad:
                return c
        c = self.within_loops(loops, pad)
        self._within_loops = self._within_loops[-3:] + [(loops, pad, c)]
        return c

    def _norm(self, norm) -> Optional[torch.Tensor]:
        if norm is None:
            return None
        if torch.is_tensor(norm) and norm.device == self.device and norm.dtype == torch.float64 and norm.is_contiguous():
            return norm
        for src, dev in self._vectors:
            if src is norm:
                return dev
        dev = self._up(norm, torch.float64)
        self._vectors = self._vectors[-7:] + [(norm, dev)]
        return dev

    def _set_windows(self, window_start):
        ws = _windows(window_start.cpu().numpy() if torch.is_tensor(window_start) else window_start)
        if self._ws_host is None or not np.array_equal(ws, self._ws_host):
            self._ws_host, self._ws_dev = ws, torch.from_numpy(ws).to(self.device)
            self._survivors = {}

    def _window_bins(self, wbp) -> int:
        """the extent of the window bitmap (cgcn_hic_count_up's n_window_bins)"""
        return max(0, int(self._ws_host[-1]) // wbp + 1) if self._ws_host.size else 0

    def survivors(self, window_start, resolution_bp=None, window_bp=None, min_distance_bp=0, expected=None,
                  expected_args=None) -> int:
        """records with pos1 != pos2 and both ends among the windows (cgcn_hic_count; one host sync per window set).  With
        window_bp: of the expanded file (cgcn_hic_count_up; one host sync per window set and window_bp).  min_distance_bp:
        of the records at least that far apart (the *_dist forms; one host sync per window set, window_bp and gap).  expected,
        expected_args: taken like the builders' and without effect: a value does not decide survival."""
        _upsample(resolution_bp, window_bp)
        gap = _gap(min_distance_bp)
        self._set_windows(window_start)
        return self._count(self._route(resolution_bp, window_bp), gap)

    def _route(self, resolution_bp, window_bp) -> _Route:
        """which of the top-K entry points serve records of resolution_bp and windows of window_bp (of the current window set)"""
        if window_bp is None or int(window_bp) == int(resolution_bp):
            return _Route("", "cgcn_hic_workspace_bytes", {}, "Hi-C build, M=%d" % self.M)
        res, wbp = int(resolution_bp), int(window_bp)
        return _Route("_up", "cgcn_hic_up_workspace_bytes",
                      dict(resolution_bp=res, window_bp=wbp, n_window_bins=self._window_bins(wbp)),
                      "Hi-C build, M=%d up=%d" % (self.M, res // wbp))

    def _count(self, route: _Route, gap: int) -> int:
        """the survivors of the current window set on `route` with the minimum gap `gap`: counted and read back once, then kept"""
        from . import _lib
        res = route.extra.get("resolution_bp")
        key = (res, route.extra.get("window_bp"), gap)
        if key not in self._survivors:
            n = int(self._ws_host.size)
            dist = dict(min_distance_bp=gap) if gap else {}
            with torch.cuda.device(self.device):
                wsp, need = _lib.workspace_for(route.workspace_fn, self.device, route.what, M=self.M, N=n, capacity=0, K=0,
                                               **route.extra)
                # [0]: survivors; the up forms add [1]: positions off the grid
                out = torch.zeros(2 if route.suffix else 1, dtype=torch.int64, device=self.device)
                if route.suffix and res not in self._on_grid:   # read back with the count: still one sync
                    out[1] = ((self.pos1 % res) != 0).sum() + ((self.pos2 % res) != 0).sum()
                _lib.call("cgcn_hic_count" + route.suffix + ("_dist" if gap else ""), M=self.M, pos1=self.pos1, pos2=self.pos2,
                          window_start=self._ws_dev, N=n, workspace=wsp, workspace_bytes=need, n_survivors=out, **route.extra,
                          **dist)
                if route.suffix:
                    s, off = out.tolist()
                    if off:
                        raise ValueError("pos1 / pos2 hold %d positions that are no multiple of resolution_bp=%d" % (off, res))
                    self._on_grid.add(res)
                else:
                    s = out.item()
            self._survivors[key] = int(s)
        return self._survivors[key]

    def build_raw(self, norm, resolution_bp, window_start, hic_edges, window_bp=None, norm_args=None, min_distance_bp=0,
                  expected=None, expected_args=None, domains=None, loops=None):
        """(rowptr int32 [N + 1], col int32 [>= nnz], sizes int64 [2] = (nnz, survivors)), all on the device, enqueued
        on the current stream: the {0,1} CSR of the reference's matrix.  No host sync beyond survivors() -- and, for
        norm = 'KR' / 'VC' / 'SQRTVC', those of norm_vector(norm, resolution_bp, **norm_args) when it is not cached; a KR
        that did not converge raises HicNormError.  min_distance_bp, expected (None, a vector, or "auto": expected_vector
        with the same norm and expected_args = n_bins / min_count): the module docstring's rules 3 and 4; with the defaults
        the entry points and the graph are the ones without them.  domains (None, (domain_of_bin, domain_bp), or a dict of
        domains()' keywords): names and "auto" are resolved on all records, then the same entry points build from the
        records within domains (within_domains; one more host sync per new selection).  loops (None, a Loops, (Loops,
        pad_bins), or a dict of loops()' keywords plus pad_bins): resolved on all records like domains, then the records within
        the loops' footprints are selected (within_loops; one more host sync per new selection), after those within domains."""
        from . import _lib
        k = _budget(hic_edges)
        gap = _gap(min_distance_bp)
        if _auto_expected(expected):
            expected = self.expected_vector(norm, resolution_bp, norm_args=norm_args, **(expected_args or {}))
        if isinstance(norm, str):
            from . import hicnorm
            norm = self._named_norm(norm, resolution_bp, norm_args)
            ws_last = _windows(window_start.cpu().numpy() if torch.is_tensor(window_start) else window_start)
            norm = hicnorm.pad_vector(norm, int(ws_last[-1]) // int(resolution_bp) + 1 if ws_last.size else 0)
        if domains is not None or loops is not None:
            sel = self
            found = None if loops is None else self._resolve_loops(loops)
            if domains is not None:
                sel = self._selection(domains, resolution_bp)
            if found is not None:
                sel = sel._loop_selection(*found)
            return sel.build_raw(norm, resolution_bp, window_start, hic_edges, window_bp=window_bp, min_distance_bp=gap,
                                 expected=expected)
        _upsample(resolution_bp, window_bp)
        self._set_windows(window_start)
        route = self._route(resolution_bp, window_bp)
        cap = self._count(route, gap)
        ws, n = self._ws_dev, int(self._ws_host.size)
        nv = self._norm(norm)
        if nv is not None:
            _check_norm(nv, resolution_bp, self._ws_host)
        ex = self._norm(expected)
        if ex is not None and (ex.ndim != 1 or int(resolution_bp) < 1):
            raise ValueError("expected must be a vector and resolution_bp positive")
        dist = {}
        if gap or ex is not None:   # the *_dist entry points; an empty vector scores as +inf everywhere, like one of NaN
            if ex is not None and ex.numel() == 0:
                ex = torch.full((1,), float("nan"), dtype=torch.float64, device=self.device)
            dist = dict(min_distance_bp=gap, expected=ex, n_expected=0 if ex is None else int(ex.numel()))
        with torch.cuda.device(self.device):
            rowptr = torch.empty(n + 1, dtype=torch.int32, device=self.device)
            col = torch.empty(max(2 * min(k, cap), 1), dtype=torch.int32, device=self.device)
            sizes = torch.zeros(2, dtype=torch.int64, device=self.device)   # [0]: nnz (its low int32 half), [1]: survivors
            wsp, need = _lib.workspace_for(route.workspace_fn, self.device, "%s capacity=%d K=%d" % (route.what, cap, k),
                                           M=self.M, N=n, capacity=cap, K=k, **route.extra)
            # every build takes resolution_bp (the norm bins); the _up forms have it in route.extra already
            _lib.call("cgcn_hic_build" + route.suffix + ("_dist" if dist else ""), M=self.M, pos1=self.pos1, pos2=self.pos2,
                      count=self.count, norm=nv, n_bins=0 if nv is None else int(nv.numel()), window_start=ws, N=n, K=k,
                      capacity=cap, workspace=wsp, workspace_bytes=need, rowptr_out=rowptr, col_out=col,
                      nnz_out=sizes.data_ptr(), n_survivors=sizes.data_ptr() + 8,
                      **{"resolution_bp": int(resolution_bp), **route.extra}, **dist)
        return rowptr, col, sizes

    def build(self, norm, resolution_bp, window_start, hic_edges, adj_type="hic", return_raw=False, window_bp=None,
              norm_args=None, min_distance_bp=0, expected=None, expected_args=None, null=None, domains=None, loops=None):
        """ChromGraph of process_graph(adj_type, ...) over the top-K contact matrix; the matrix itself never visits the
        host.  return_raw=True: (graph, the {0,1} scipy CSR the reference pickles) -- one more read-back.  norm: a vector,
        None, or 'KR' / 'VC' / 'SQRTVC' (computed from the records; norm_args: norm_vector's keywords).  min_distance_bp,
        expected, expected_args, domains, loops: build_raw's.  null = (model, seed): the matrix is replaced by its null graph
        (chromegcn_amd.nullgraph) before the normalisation; return_raw then returns the null matrix."""
        rowptr, col, sizes = self.build_raw(norm, resolution_bp, window_start, hic_edges, window_bp=window_bp,
                                            norm_args=norm_args, min_distance_bp=min_distance_bp, expected=expected,
                                            expected_args=expected_args, domains=domains, loops=loops)
        if null is not None:
            from . import nullgraph
            rowptr, col, sizes = nullgraph.null_graph((rowptr, col), model=null[0], seed=null[1], device=self.device)
        n = int(rowptr.numel()) - 1
        g = G.normalize_device_csr(adj_type, n, rowptr, col, None, self.device)
        if not return_raw:
            return g
        nnz = int(sizes[0].item())
        raw = sp.csr_matrix((np.ones(nnz, np.float64), col[:nnz].cpu().numpy(), rowptr.cpu().numpy()), shape=(n, n))
        return g, raw


def build_hic_graph(pos1, pos2, count, norm, resolution_bp, window_start, hic_edges, adj_type="hic", device="cuda",
                    return_raw=False, window_bp=None, norm_args=None, min_distance_bp=0, expected=None, expected_args=None,
                    null=None, domains=None, loops=None):
    """build_hic_graph_host on the device, handed straight to the device normaliser: contacts in, ChromGraph out.
    `pos1` may be a HicContacts (then pos2 and count are ignored): nothing is uploaded again.  window_bp: the records are
    coarser than the windows and stand for their expanded file (the module's docstring).  min_distance_bp, expected (None, a
    vector, "auto"), expected_args: the minimum gap and the observed / expected value (the module's docstring).  null,
    domains, loops: HicContacts.build's."""
    _upsample(resolution_bp, window_bp)
    c = pos1 if isinstance(pos1, HicContacts) else HicContacts(pos1, pos2, count, device)
    return c.build(norm, resolution_bp, window_start, hic_edges, adj_type=adj_type, return_raw=return_raw, window_bp=window_bp,
                   norm_args=norm_args, min_distance_bp=min_distance_bp, expected=expected, expected_args=expected_args, null=null,
                   domains=domains, loops=loops)


def contacts_from_text(path_or_bytes, device="cuda", **kw) -> HicContacts:
    """HicContacts.from_text: contact text in, device-resident records out"""
    return HicContacts.from_text(path_or_bytes, device=device, **kw)


def graphs_from_contact_caches(root: str, chroms, hicsize, hicnorm: str, adj_type: str = "hic", device="cuda",
                               sizes: Optional[Dict[str, int]] = None, window_bp=None,
                               compute_norm: bool = False, min_distance_bp=0, expected=None,
                               expected_args=None, null=None, domains=None,
                               domain_report: Optional[dict] = None, compartments: Optional[dict] = None,
                               compartment_report: Optional[dict] = None, loops: Optional[dict] = None,
                               loop_report: Optional[dict] = None, apa: Optional[dict] = None,
                               apa_report: Optional[dict] = None, compare: Optional[dict] = None,
                               compare_report: Optional[dict] = None) -> Dict[str, G.ChromGraph]:
    """{chrom: ChromGraph} from `<root>/<chrom>.cghic` (save_contacts_cache, with the chromosome's windows) for the edge
    budget `hicsize` and the norm vector named `hicnorm` ('' = none): what `chromegcn_amd.train -hic_contacts` loads
    instead of `{split}_graphs_{hicsize}_{hicnorm}norm.pkl`.  sizes: the expected window count per chromosome.  window_bp
    (`-hic_upsample`): the window size; a cache whose resolution_bp is coarser is built as its expanded file.  compute_norm
    (`-hic_compute_norm`): a `hicnorm` of 'KR' / 'VC' / 'SQRTVC' that the cache lacks is computed from its records.
    min_distance_bp (`-hic_min_distance`), expected (`-hic_expected`: "auto", the vector computed from each cache's records
    with the vector the call scores with; any other name: the vector the cache stores under it, tools/hic_ingest.py
    --compute-expected writes eRAW / eKR / eVC / eSQRTVC), expected_args: build_hic_graph's.  null = (model, seed)
    (`-hic_null`, `-hic_null_seed`): every matrix is replaced by its null graph before the normalisation, chromosome index c
    of the list with nullgraph.replicate_seed(seed, 0, c, len(chroms)).  domains (`-hic_domains`): a dict of
    HicContacts.domains' keywords; every graph is built from the records within the domains computed from its cache's records.
    domain_report: a dict that receives {chrom: (boundaries, same-domain entries, nnz)} of the UNRESTRICTED top-K matrix
    (insulation.domain_edge_share).  compartments (`-hic_compartments`): a dict of HicContacts.compartments' keywords plus
    `targets` ({chrom: label matrix}: every vector is oriented by compartments.label_density of the chromosome's windows) and
    `restrict` (`-hic_compartment_restrict`: every graph is built with domains = as_domains(), the contacts within one
    compartment; not together with `domains`).  compartment_report: a dict that receives {chrom: (Compartments,
    compartment_of_windows, compartments.compartment_edge_share of the graph that is returned)}.  loops (`-hic_loops`): a dict
    of HicContacts.loops' keywords plus `pad_bins` and `restrict` (`-hic_loop_restrict`: every graph is built from the records
    inside the footprints of the loops called from its cache's records; with `domains` both tests hold).  loop_report: a dict
    that receives {chrom: (Loops, entries in a footprint, nnz)} of the UNRESTRICTED top-K matrix (loops.loop_edge_share).
    apa (`-hic_apa`): a dict of HicContacts.pileup's keywords; apa_report: a dict that receives {chrom: {"edges", "control"[,
    "loops"]: Pileup}}: the pile-up around the edges of the UNRESTRICTED top-K matrix (pileup.centres_of_graph), around the
    same edges shifted by 3 w bins along the diagonal and, with `loops`, around the loops.  No graph depends on it.
    compare (`-hic_compare`): a dict of HicContacts.scc's keywords plus `root`, a second cache directory; compare_report: a dict
    that receives {chrom: (MapComparison of this cache's records and `<compare root>/<chrom>.cghic`'s, mapcompare.
    graph_edge_overlap of the two UNRESTRICTED top-K matrices, the second one built from the second cache's records, windows and
    `hicnorm` vector with the same budget and distance rule)}.  No graph depends on it."""
    from . import hicnorm as HN
    from . import nullgraph
    out = {}
    chroms = list(chroms)
    for ci, chrom in enumerate(chroms):
        c = load_contacts_cache(contact_cache_path(root, chrom))
        if c.window_start is None:
            raise ValueError("%s holds no window list" % contact_cache_path(root, chrom))
        computed = bool(compute_norm) and hicnorm in HN.KINDS and hicnorm not in c.norms
        if hicnorm and hicnorm not in c.norms and not computed:
            raise ValueError("%s holds no %r norm vector (has: %s)" % (contact_cache_path(root, chrom), hicnorm,
                                                                       ", ".join(sorted(c.norms)) or "none"))
        if sizes is not None and sizes[chrom] != c.window_start.size:
            raise ValueError("%s has %d windows but the chromosome's features have %d rows"
                             % (contact_cache_path(root, chrom), c.window_start.size, sizes[chrom]))
        up = {"window_bp": int(window_bp)} if window_bp is not None and c.resolution_bp > int(window_bp) else {}
        norm = hicnorm if computed else c.norms[hicnorm] if hicnorm else None
        ex = expected
        if isinstance(expected, str) and expected != "auto":
            if expected not in c.norms:
                raise ValueError("%s holds no %r vector (has: %s)" % (contact_cache_path(root, chrom), expected,
                                                                     ", ".join(sorted(c.norms)) or "none"))
            ex = c.norms[expected]
        rec, dom = (c.pos1, c.pos2, c.count), None
        if domains is not None:
            from . import insulation as INS
            rec = (HicContacts(c.pos1, c.pos2, c.count, device), None, None)
            dom = rec[0].domains(**domains)
            if domain_report is not None:   # what the restriction removes: the unrestricted top-K matrix against the domains
                rp, ci_, _ = rec[0].build_raw(norm, c.resolution_bp, c.window_start, int(hicsize), min_distance_bp=min_distance_bp,
                                              expected=ex, expected_args=expected_args, **up)
                domain_report[chrom] = (int(dom[0].max()) if dom[0].size else 0,) + INS.domain_edge_share(
                    (rp, ci_), INS.domain_of_windows(c.window_start, *dom))
        if compartments is not None:
            from . import compartments as CP
            kw = dict(compartments)
            restrict, labels = kw.pop("restrict", False), kw.pop("targets", None)
            if restrict and dom is not None:
                raise ValueError("a graph is restricted to domains or to compartments, not both")
            if not isinstance(rec[0], HicContacts):
                rec = (HicContacts(c.pos1, c.pos2, c.count, device), None, None)
            comp = rec[0].compartments(**kw)
            comp = comp.oriented(None if labels is None else
                                 CP.label_density(labels[chrom], c.window_start, comp.resolution_bp, comp.n))
            if restrict:
                dom = (comp.as_domains(), comp.resolution_bp)
        found = None
        if loops is not None:
            kw = dict(loops)
            restrict, pad = kw.pop("restrict", False), kw.pop("pad_bins", 1)
            if not isinstance(rec[0], HicContacts):
                rec = (HicContacts(c.pos1, c.pos2, c.count, device), None, None)
            called = rec[0].loops(**kw)
            if loop_report is not None:
                rp, ci_, _ = rec[0].build_raw(norm, c.resolution_bp, c.window_start, int(hicsize), min_distance_bp=min_distance_bp,
                                              expected=ex, expected_args=expected_args, **up)
                loop_report[chrom] = (called,) + loop_edge_share((rp, ci_), called, c.window_start, pad)
            found = (called, pad) if restrict else None
        if apa is not None:
            from . import pileup as PU
            kw = dict(apa)
            if not isinstance(rec[0], HicContacts):
                rec = (HicContacts(c.pos1, c.pos2, c.count, device), None, None)
            rp, ci_, _ = rec[0].build_raw(norm, c.resolution_bp, c.window_start, int(hicsize), min_distance_bp=min_distance_bp,
                                          expected=ex, expected_args=expected_args, **up)
            ei, ej, _ = PU.centres_of_graph((rp, ci_), c.window_start, kw.get("resolution_bp", 10000))
            w = PU.pileup_rule(kw.get("resolution_bp", 10000), **{k: v for k, v in kw.items() if k in PU._RULE}).w
            piles = {"edges": rec[0].pileup((ei, ej), **kw), "control": rec[0].pileup(PU.shifted_centres(ei, ej, 3 * w), **kw)}
            if loops is not None:
                piles["loops"] = rec[0].pileup(called, **kw)
            if apa_report is not None:
                apa_report[chrom] = piles
        if compare is not None:
            from . import mapcompare as MC
            kw = dict(compare)
            c2 = load_contacts_cache(contact_cache_path(kw.pop("root"), chrom))
            if c2.window_start is None:
                raise ValueError("%s holds no window list" % contact_cache_path(compare["root"], chrom))
            if hicnorm and hicnorm not in c2.norms and not (bool(compute_norm) and hicnorm in HN.KINDS):
                raise ValueError("%s holds no %r norm vector (has: %s)" % (contact_cache_path(compare["root"], chrom), hicnorm,
                                                                           ", ".join(sorted(c2.norms)) or "none"))
            if not isinstance(rec[0], HicContacts):
                rec = (HicContacts(c.pos1, c.pos2, c.count, device), None, None)
            other = HicContacts(c2.pos1, c2.pos2, c2.count, device)
            up2 = {"window_bp": int(window_bp)} if window_bp is not None and c2.resolution_bp > int(window_bp) else {}
            ga = rec[0].build_raw(norm, c.resolution_bp, c.window_start, int(hicsize), min_distance_bp=min_distance_bp,
                                  expected=ex, expected_args=expected_args, **up)
            gb = other.build_raw(c2.norms[hicnorm] if hicnorm in c2.norms else (hicnorm or None), c2.resolution_bp,
                                 c2.window_start, int(hicsize), min_distance_bp=min_distance_bp,
                                 expected=c2.norms.get(expected, expected) if isinstance(expected, str) else expected,
                                 expected_args=expected_args, **up2)
            pair = (rec[0].scc(other, **kw), MC.graph_edge_overlap(ga[:2], gb[:2]))
            if compare_report is not None:
                compare_report[chrom] = pair
        out[chrom] = build_hic_graph(*rec, norm, c.resolution_bp,
                                     c.window_start, int(hicsize), adj_type=adj_type, device=device,
                                     min_distance_bp=min_distance_bp, expected=ex, expected_args=expected_args,
                                     null=None if null is None else (null[0], nullgraph.replicate_seed(null[1], 0, ci, len(chroms))),
                                     domains=dom, loops=found, **up)
        if compartments is not None and compartment_report is not None:
            cw = comp.compartment_of_windows(c.window_start)
            compartment_report[chrom] = (comp, cw, CP.compartment_edge_share(out[chrom], cw))
    return out
