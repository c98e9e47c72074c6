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

Contact TEXT (a Juicer `RAWobserved` dump, which the reference reads with int() and float(), :71-76) becomes records by one
rule, restated by parse_contacts_text_host and run on the device by HicContacts.from_text (csrc/cgcn_text.hip):
  * a file is a sequence of lines, each ended by LF or CR LF, the last one possibly by nothing (a CR belongs to the terminator
    only in front of an LF); record r is the r-th line; the empty piece behind a final terminator is no line; a line is
    F1 TAB F2 TAB F3;
  * FAST: at most TEXT_LINE_MAX = 64 bytes without the terminator; F1, F2 one to ten decimal digits below 2^31; F3 is
    [+-]? digits [. digits]? ([eE] [+-]? digits)?; its digits without leading zeros and without trailing zeros of the fraction
    are at most 15 and form the integer w < 10^15 < 2^53; e = exponent - (fraction digits that remain in w), |e| <= 22; the
    value is float(w) * 10^e (e >= 0) or float(w) / 10^-e, negated behind '-': one correctly rounded operation on two exact
    operands, so it IS float(F3);
  * SLOW: not fast, but int(float(F1)), int(float(F2)) and float(F3) accept the fields and the positions fit int32 (16 or more
    digits, |e| > 22, nan, inf, 1e3 as a position, blanks around a field, a line beyond the bound): parsed by exactly those
    calls, on the host in both paths; 17-digit normalised dumps are of this kind throughout: load_contacts_text reads
    those faster;
  * MALFORMED: everything else (an empty line, a field count other than three, a '#' comment, a field float() rejects):
    ValueError naming the first such line, 1-based, the same text from both paths."""
from __future__ import annotations

import csv
import os
import time
from dataclasses import dataclass, field
from typing import Dict, Optional

import numpy as np
import scipy.sparse as sp
import torch

from . import graph as G


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


def survivor_values(pos1, pos2, count, norm, resolution_bp, window_start, window_bp=None, min_distance_bp=0, expected=None,
                    expected_args=None):
    """(record index, i, j, value) of the surviving records in file order (rules 1 and 2).  With window_bp: of the surviving
    records of the expanded file, the index being the position in it.  min_distance_bp, expected (None, a vector, or "auto":
    hicdist.expected_vector_host with this norm and expected_args): the minimum gap and the observed / expected value of the
    module docstring."""
    up = _upsample(resolution_bp, window_bp)
    gap = _gap(min_distance_bp)
    ws = _windows(window_start).astype(np.int64)
    p1, p2 = np.asarray(pos1, dtype=np.int64), np.asarray(pos2, dtype=np.int64)
    if up > 1:
        _check_grid(p1, p2, resolution_bp)
    n = ws.size
    if n == 0 or p1.size == 0:
        e = np.zeros(0, np.int64)
        return e, e, e, np.zeros(0, np.float64)
    if up > 1:
        src, a, b, i, j = _survivors_up(p1, p2, ws, int(resolution_bp) // up, up, (np.abs(p1 - p2) >= gap) if gap else None)
        idx = src * (up * up) + a * up + b
    else:
        i = np.minimum(np.searchsorted(ws, p1), n - 1)
        j = np.minimum(np.searchsorted(ws, p2), n - 1)
        idx = src = np.flatnonzero((p1 != p2) & (ws[i] == p1) & (ws[j] == p2) & (np.abs(p1 - p2) >= gap))
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
        if isinstance(expected, str):
            if expected != "auto":
                raise ValueError("expected=%r is none of None, a vector, 'auto'" % (expected,))
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
                         norm_args=None, min_distance_bp=0, expected=None, expected_args=None) -> sp.csr_matrix:
    """The {0,1} float64 CSR the reference's step 7 pickles (symmetric, zero diagonal, sorted columns).  With window_bp: of
    the expanded file, which is never written out (the CPU path for coarse records at full size).  norm = 'KR' / 'VC' /
    'SQRTVC': the vector computed from the records (hicnorm.hic_norm_vector_host with norm_args).  min_distance_bp, expected
    (None, a vector, or "auto": hicdist.expected_vector_host with the same norm and expected_args = n_bins / min_count)."""
    ws = _windows(window_start)
    n = ws.size
    k = _budget(hic_edges)
    if isinstance(expected, str):
        from . import hicdist
        if expected != "auto":
            raise ValueError("expected=%r is none of None, a vector, 'auto'" % (expected,))
        expected = hicdist.expected_vector_host(pos1, pos2, count, norm, resolution_bp, norm_args=norm_args, **(expected_args or {}))
    if isinstance(norm, str):
        from . import hicnorm
        norm, info = hicnorm.hic_norm_vector_host(pos1, pos2, count, norm, resolution_bp, **(norm_args or {}))
        if not info.get("converged", True):
            raise hicnorm.HicNormError("KR did not converge: %r" % (info,), info)
        norm = hicnorm.pad_vector(norm, int(ws[-1]) // int(resolution_bp) + 1 if n else 0)
    _, i, j, v = survivor_values(pos1, pos2, count, norm, resolution_bp, window_start, window_bp, min_distance_bp, expected)
    take = np.argsort(-v, kind="stable")[:k]
    i, j = i[take], j[take]
    a = sp.coo_matrix((np.ones(2 * i.size), (np.concatenate([i, j]), np.concatenate([j, i]))), shape=(n, n)).tocsr()
    a.sum_duplicates()
    a.data[:] = 1.0
    a.sort_indices()
    return sp.csr_matrix(a, dtype=np.float64)


# ----------------------------------------------------------------------------------------------
# contact records of one chromosome on the host: text parser and flat binary cache
# ----------------------------------------------------------------------------------------------
@dataclass
class HostContacts:
    pos1: np.ndarray                 # int32 [M]
    pos2: np.ndarray                 # int32 [M]
    count: np.ndarray                # float64 [M]
    norms: Dict[str, np.ndarray] = field(default_factory=dict)   # name ('KR', 'VC', 'SQRTVC') -> float64 [n_bins]
    resolution_bp: int = 1000
    window_start: Optional[np.ndarray] = None   # int32 [N]: the chromosome's windows with peaks, when known

    @property
    def M(self) -> int:
        return int(self.pos1.shape[0])


def load_contacts_text(raw_path: str, norm_paths: Optional[Dict[str, str]] = None, resolution_bp: int = 1000,
                       window_start=None) -> HostContacts:
    """Parse a `RAWobserved` file (`start_pos1<TAB>start_pos2<TAB>count` per line) and its norm files (one value per line,
    'NaN' allowed) once, with numpy.  Slow and simple on purpose: the result goes into the binary cache."""
    raw = np.loadtxt(raw_path, dtype=np.float64, delimiter="\t", ndmin=2)
    if raw.size == 0:
        raw = raw.reshape(0, 3)
    if raw.shape[1] != 3:
        raise ValueError("%s: expected three columns, found %d" % (raw_path, raw.shape[1]))
    norms = {name: np.loadtxt(p, dtype=np.float64, ndmin=1) for name, p in (norm_paths or {}).items()}
    return HostContacts(raw[:, 0].astype(np.int32), raw[:, 1].astype(np.int32), np.ascontiguousarray(raw[:, 2]), norms,
                        int(resolution_bp), None if window_start is None else _windows(window_start))


# ----------------------------------------------------------------------------------------------
# contact text -> records: the rule of the module docstring on the host
# ----------------------------------------------------------------------------------------------
TEXT_LINE_MAX = 64   # include/chromegcn.h: CGCN_TEXT_LINE_MAX
TEXT_SLOW, TEXT_MALFORMED = 1, 2
_P10 = np.array([float("1e%d" % k) for k in range(23)])           # the 23 powers of ten that are exact in fp64
_P10U = np.array([10 ** k for k in range(16)], dtype=np.uint64)


def _malformed(record: int) -> ValueError:
    return ValueError("contact text: line %d is not `pos1<TAB>pos2<TAB>count`" % (record + 1))


def _slow_line(raw: bytes):
    """(pos1, pos2, count) of one line without its terminator by Python's own int(float(.)) and float(.); None = malformed"""
    f = raw.split(b"\t")
    if len(f) != 3:
        return None
    try:
        a, b, v = int(float(f[0])), int(float(f[1])), float(f[2])
    except (ValueError, OverflowError):
        return None
    if not (-2 ** 31 <= a < 2 ** 31 and -2 ** 31 <= b < 2 ** 31):
        return None
    return a, b, v


def _text_bytes(data) -> np.ndarray:
    if isinstance(data, np.ndarray):
        if data.dtype != np.uint8 or data.ndim != 1:
            raise TypeError("contact text as an array must be a uint8 vector")
        return np.ascontiguousarray(data)
    return np.frombuffer(data, dtype=np.uint8)


def _text_lines(buf):
    """(start, end) int64 [M] of every line: its first byte and the byte behind its last (terminator excluded)"""
    n = buf.size
    lf = np.flatnonzero(buf == 10)
    start = np.concatenate([np.zeros(1, np.int64), lf + 1])
    start = start[start < n]
    end = np.concatenate([lf, np.full(1, n, np.int64)])[:start.size]
    cr = (end < n) & (end > start) & (buf[np.maximum(end - 1, 0)] == 13)
    return start, end - cr


def _text_fast(buf, start, end):
    """The fast form, all lines at once, one byte of every line per step (the walk of cgcn_text.hip's text_parse_line):
    (fast bool [M], pos1 int64 [M], pos2 int64 [M], count float64 [M]); the last three mean nothing where fast is False."""
    n, m_lines = buf.size, start.size
    bufp = np.concatenate([buf, np.zeros(1, np.uint8)])

    def at(p):
        return bufp[np.minimum(p, n)].astype(np.int64)

    ok = (end - start >= 1) & (end - start <= TEXT_LINE_MAX)
    p = start.copy()
    pos = []
    for _ in range(2):   # one to ten digits below 2^31, then the TAB
        x, nd, run = np.zeros(m_lines, np.int64), np.zeros(m_lines, np.int64), ok.copy()
        for _ in range(11):
            d = at(p) - 48
            run = run & (p < end) & (d >= 0) & (d <= 9)
            if not run.any():
                break
            x = np.where(run, x * 10 + d, x)
            nd += run
            p += run
        ok &= (nd >= 1) & (nd <= 10) & (x < 2 ** 31) & (p < end) & (at(p) == 9)
        p += 1
        pos.append(x)
    c = at(p)
    sign = ok & (p < end) & ((c == 43) | (c == 45))
    neg = sign & (c == 45)
    p += sign
    st = np.ones(m_lines, np.int8)   # 1 integer digits, 2 fraction digits, 3 behind [eE], 4 exponent digits
    w = np.zeros(m_lines, np.uint64)
    nsig, nint, nfr, fr, z, ex, nex = (np.zeros(m_lines, np.int64) for _ in range(7))
    eneg = np.zeros(m_lines, bool)
    for _ in range(TEXT_LINE_MAX):
        act = ok & (p < end)
        if not act.any():
            break
        c = at(p)
        d = c - 48
        isd = (d >= 0) & (d <= 9)
        du = np.where(isd, d, 0).astype(np.uint64)
        is_e = (c | 32) == 101
        in1, in2, in3, in4 = act & (st == 1), act & (st == 2), act & (st == 3), act & (st == 4)
        # integer part: leading zeros do not count
        dig = in1 & isd
        grow = dig & ((nsig > 0) | (d != 0))
        nsig += grow
        w = np.where(grow & (nsig <= 15), w * np.uint64(10) + du, w)   # never beyond 15 digits: w does not wrap
        nint += dig
        # fraction: zeros wait in z until a digit follows them
        dig2 = in2 & isd
        nfr += dig2
        nz = dig2 & (d != 0)
        first = nz & (nsig == 0)
        more = nz & (nsig > 0)
        nsig = np.where(first, 1, np.where(more, nsig + z + 1, nsig))
        w = np.where(first, du, np.where(more & (nsig <= 15), w * _P10U[np.minimum(z + 1, 15)] + du, w))
        fr += np.where(nz, z + 1, 0)
        z = np.where(nz, 0, z + (dig2 & (d == 0)))
        # exponent
        esign = in3 & ((c == 43) | (c == 45))
        eneg |= esign & (c == 45)
        dig4 = (in3 | in4) & isd
        ex = np.where(dig4 & (ex < 10000), ex * 10 + d, ex)
        nex += dig4
        # what ends a part
        end1, end2 = in1 & ~isd, in2 & ~isd
        to2 = end1 & (nint >= 1) & (c == 46)
        to3 = (end1 & (nint >= 1) & is_e) | (end2 & (nfr >= 1) & is_e)
        ok &= ~((end1 & ~to2 & ~to3) | (end2 & ~to3) | (in3 & ~esign & ~isd) | (in4 & ~isd))
        st = np.where(to2, 2, np.where(to3, 3, np.where(esign | dig4, 4, st))).astype(np.int8)
        p += act
    ok &= np.where(st == 1, nint >= 1, np.where(st == 2, nfr >= 1, nex >= 1))
    e = np.where(eneg, -ex, ex) - fr
    ok &= (nsig <= 15) & (e >= -22) & (e <= 22)
    mant = w.astype(np.float64)   # exact: w < 10^15
    with np.errstate(all="ignore"):
        val = np.where(e >= 0, mant * _P10[np.clip(e, 0, 22)], mant / _P10[np.clip(-e, 0, 22)])   # one rounding
    return ok, pos[0], pos[1], np.where(neg, -val, val)


def parse_contacts_text_host(data):
    """The rule of the module docstring on bytes (bytes, bytearray, memoryview or a uint8 vector): (pos1 int32 [M], pos2 int32
    [M], count float64 [M], slow_lines int64: the 0-based records that are SLOW, ascending).  Fast lines are parsed by the
    walk the device kernel does, every other line by int(float(.)) and float(.); ValueError at the first malformed line."""
    buf = _text_bytes(data)
    start, end = _text_lines(buf)
    fast, a, b, v = _text_fast(buf, start, end)
    pos1, pos2, count = a.astype(np.int32), b.astype(np.int32), np.ascontiguousarray(v, dtype=np.float64)
    slow = np.flatnonzero(~fast)
    for r in slow.tolist():
        rec = _slow_line(buf[start[r]:end[r]].tobytes())
        if rec is None:
            raise _malformed(r)
        pos1[r], pos2[r], count[r] = rec
    return pos1, pos2, count, slow.astype(np.int64)


def windows_from_bed(path: str, chroms) -> Dict[str, np.ndarray]:
    """{chrom: int32 window starts, ascending} of a windows bed (chrom<TAB>start<TAB>...): create_bin_dict of
    data/7create_graph_new.py:14-47 -- the distinct start positions of every chromosome of `chroms`; a window's node index
    is its rank.  Host only."""
    starts = {c: set() for c in chroms}
    with open(path, newline="") as f:
        for row in csv.reader(f, delimiter="\t"):
            if row and row[0] in starts:
                starts[row[0]].add(int(row[1]))
    return {c: np.array(sorted(s), dtype=np.int32) for c, s in starts.items()}


_MAGIC = b"CGHIC01\0"


def save_contacts_cache(path: str, c: HostContacts):
    """Flat little-endian file: magic, int64 header [M, n_norms, resolution_bp, N or -1], pos1 int32[M], pos2 int32[M],
    count fp64[M], per norm vector (name 16 bytes, int64 n_bins, fp64[n_bins]), window_start int32[N]."""
    n = -1 if c.window_start is None else int(c.window_start.shape[0])
    with open(path, "wb") as f:
        f.write(_MAGIC)
        f.write(np.array([c.M, len(c.norms), c.resolution_bp, n], dtype="<i8").tobytes())
        f.write(np.ascontiguousarray(c.pos1, dtype="<i4").tobytes())
        f.write(np.ascontiguousarray(c.pos2, dtype="<i4").tobytes())
        f.write(np.ascontiguousarray(c.count, dtype="<f8").tobytes())
        for name, v in c.norms.items():
            b = name.encode()
            if not 0 < len(b) <= 16:
                raise ValueError("norm name %r does not fit 16 bytes" % name)
            f.write(b.ljust(16, b"\0"))
            f.write(np.array([v.shape[0]], dtype="<i8").tobytes())
            f.write(np.ascontiguousarray(v, dtype="<f8").tobytes())
        if n >= 0:
            f.write(np.ascontiguousarray(c.window_start, dtype="<i4").tobytes())


def load_contacts_cache(path: str) -> HostContacts:
    def take(f, dtype, k):
        raw = f.read(np.dtype(dtype).itemsize * k)
        if len(raw) != np.dtype(dtype).itemsize * k:
            raise ValueError("%s is truncated" % path)
        return np.frombuffer(raw, dtype=dtype).copy()

    with open(path, "rb") as f:
        if f.read(8) != _MAGIC:
            raise ValueError("%s is not a chromegcn contact cache" % path)
        m, n_norms, res, n = take(f, "<i8", 4).tolist()
        if m < 0 or n_norms < 0 or res < 1 or n < -1:
            raise ValueError("%s is corrupt" % path)
        pos1, pos2, count = take(f, "<i4", m), take(f, "<i4", m), take(f, "<f8", m)
        norms = {}
        for _ in range(n_norms):
            name = f.read(16).rstrip(b"\0").decode()
            norms[name] = take(f, "<f8", int(take(f, "<i8", 1)[0]))
        ws = None if n < 0 else _windows(take(f, "<i4", n))
    return HostContacts(pos1, pos2, count, norms, int(res), ws)


# ----------------------------------------------------------------------------------------------
# device build
# ----------------------------------------------------------------------------------------------
def _find_lf(mem, off: int) -> int:
    """index of the first LF at or behind `off` in a byte memoryview, or its length - 1"""
    step = 4096
    for lo in range(off, len(mem), step):
        k = bytes(mem[lo:lo + step]).find(b"\n")
        if k >= 0:
            return lo + k
    return len(mem) - 1


_staging = {}   # (device, chunk_bytes) -> the two pinned staging buffers of from_text (release_text_staging frees them)


def release_text_staging():
    """Free the two pinned staging buffers HicContacts.from_text keeps between calls (2 x chunk_bytes of page-locked host
    memory, 64 MiB at the default; kept because pinning costs more than a chunk's copy, replaced when chunk_bytes or the
    device changes)."""
    _staging.clear()



def _stage_text(src, is_path, n, text, chunk_bytes) -> float:
    """Copy the n bytes of a file or a memoryview into the device buffer `text`, chunk by chunk through two pinned buffers:
    chunk k + 1 is read while chunk k is on its way.  Returns the seconds spent reading."""
    key = (text.device, chunk_bytes)
    if key not in _staging:
        _staging.clear()
        _staging[key] = [torch.empty(chunk_bytes, dtype=torch.uint8, pin_memory=True) for _ in range(2)]
    pinned, busy, t_read = _staging[key], [None, None], 0.0
    f = open(src, "rb", buffering=0) if is_path else None
    try:
        off, k = 0, 0
        while off < n:
            if busy[k] is not None:
                busy[k].synchronize()
            want = min(chunk_bytes, n - off)
            t0 = time.perf_counter()
            if is_path:
                got, view = 0, memoryview(pinned[k].numpy())
                while got < want:
                    r = f.readinto(view[got:want])
                    if not r:
                        raise ValueError("%s ended after %d of %d bytes" % (src, off + got, n))
                    got += r
            else:
                pinned[k].numpy()[:want] = np.frombuffer(src[off:off + want], dtype=np.uint8)
            t_read += time.perf_counter() - t0
            text[off:off + want].copy_(pinned[k][:want], non_blocking=True)
            busy[k] = torch.cuda.Event()
            busy[k].record()
            off, k = off + want, k ^ 1
        for e in busy:
            if e is not None:
                e.synchronize()   # the buffers are shared with the next call
    finally:
        if f is not None:
            f.close()
    return t_read


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
        self._survivors = None   # of the current window set, records at the windows' resolution
        self._survivors_up = {}  # of the current window set, per (resolution_bp, window_bp)
        self._on_grid = set()    # the resolutions of which every position is known to be a multiple
        self._vectors = []   # (the caller's object, its device copy): a sweep passes the same vector again
        self._matrices = {}  # (resolution_bp, n_bins or None) -> hicnorm.DeviceContactMatrix
        self._norms = {}     # norm_vector's argument tuple -> (vector, info)
        self._gap_survivors = {}   # of the current window set, per (min_distance_bp, resolution_bp, window_bp) with a gap > 0
        self._dist_sums = {}       # distance_sums' argument tuple -> (raw, act, host syncs)
        self._expected = {}        # expected_vector's argument tuple -> (vector, info)
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
        """The records of contact text (a path, or bytes / bytearray / memoryview) by the rule of the module docstring, parsed
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
        from . import _lib
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("HicContacts.from_text needs a GPU; parse_contacts_text_host is the CPU path")
        if int(chunk_bytes) < 1 or int(flag_capacity) < 0:
            raise ValueError("chunk_bytes must be positive and flag_capacity non-negative")
        is_path = isinstance(path_or_bytes, (str, os.PathLike))
        mem = None if is_path else memoryview(path_or_bytes).cast("B")
        n = os.path.getsize(path_or_bytes) if is_path else len(mem)
        t = [time.perf_counter()]

        def lap(name):
            if timings is not None:
                torch.cuda.synchronize(device)
                t.append(time.perf_counter())
                timings[name] = t[-1] - t[-2]

        def line_at(src, off):   # the line that starts at byte `off`, without its terminator
            if is_path:
                src.seek(off)
                raw = src.readline()
            else:
                stop = _find_lf(mem, off)
                raw = bytes(mem[off:stop + 1])
            return raw[:-2] if raw.endswith(b"\r\n") else raw[:-1] if raw.endswith(b"\n") else raw

        with torch.cuda.device(device):
            text = torch.empty(max(n, 1), dtype=torch.uint8, device=device)
            t_read = _stage_text(path_or_bytes if is_path else mem, is_path, n, text, int(chunk_bytes))
            if timings is not None:
                torch.cuda.synchronize(device)
                t.append(time.perf_counter())
                timings["read"], timings["h2d"] = t_read, t[-1] - t[-2] - t_read
            need = _lib.query("cgcn_text_workspace_bytes", n_bytes=n)
            wsp = _lib._workspace(need, device, "contact text, %d bytes" % n)
            out = torch.zeros(1, dtype=torch.int64, device=device)
            _lib.call("cgcn_text_count", text=text, n_bytes=n, workspace=wsp, workspace_bytes=need, n_records=out)
            m = int(out.item())
            lap("count")
            if m >= 2 ** 31:
                raise ValueError("contact text: %d records, more than 2^31 - 1" % m)
            pos1 = torch.empty(m, dtype=torch.int32, device=device)
            pos2 = torch.empty(m, dtype=torch.int32, device=device)
            count = torch.empty(m, dtype=torch.float64, device=device)
            cap, calls = int(flag_capacity), 0
            while True:
                flags = torch.empty((max(cap, 1), 3), dtype=torch.int64, device=device)
                totals = torch.zeros(2, dtype=torch.int64, device=device)
                _lib.call("cgcn_text_parse", text=text, n_bytes=n, M=m, pos1_out=pos1, pos2_out=pos2, count_out=count,
                          flags=flags, flag_capacity=cap, flag_totals=totals, workspace=wsp, workspace_bytes=need)
                calls += 1
                flagged = int(totals.sum().item())
                if flagged <= cap:
                    break
                if calls == 2:
                    raise RuntimeError("chromegcn_amd: cgcn_text_parse reported %d flagged lines for a capacity of %d" % (flagged, cap))
                cap = flagged   # once more, with room for every one of them
            lap("parse")
            fl = flags[:flagged].cpu().numpy()
            del text, flags, wsp
            fl = fl[np.argsort(fl[:, 0], kind="stable")]
            if flagged:
                recs = []
                src = open(path_or_bytes, "rb") if is_path else None
                try:
                    for r, off, _ in fl.tolist():   # ascending records: the first line that fails is the first malformed one
                        rec = _slow_line(line_at(src, off))
                        if rec is None:
                            raise _malformed(r)
                        recs.append(rec)
                finally:
                    if src is not None:
                        src.close()
                idx = torch.from_numpy(fl[:, 0].copy()).to(device)
                pos1.index_copy_(0, idx, torch.tensor([x[0] for x in recs], dtype=torch.int32).to(device))
                pos2.index_copy_(0, idx, torch.tensor([x[1] for x in recs], dtype=torch.int32).to(device))
                count.index_copy_(0, idx, torch.tensor([x[2] for x in recs], dtype=torch.float64).to(device))
            lap("patch")
        c = cls(pos1, pos2, count, device)
        c.text_info = {"n_bytes": int(n), "slow_lines": fl[:, 0].astype(np.int64), "parse_calls": calls}
        return c

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

    def _named_norm(self, norm, resolution_bp, n_bins=None, norm_args=None):
        """'KR' / 'VC' / 'SQRTVC' -> the vector computed from the records (HicNormError for a KR that did not converge)"""
        from . import hicnorm
        v, info = self.norm_vector(norm, resolution_bp, n_bins=n_bins, return_info=True, **(norm_args or {}))
        if not info.get("converged", True):
            raise hicnorm.HicNormError("KR did not converge: %r" % (info,), info)
        return v

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
        nv = self._named_norm(norm, res, given, norm_args) if isinstance(norm, str) else self._norm(norm)
        syncs = 0
        with torch.cuda.device(self.device):
            sizes = torch.zeros(2, dtype=torch.int64, device=self.device)
            args = dict(M=self.M, pos1=self.pos1, pos2=self.pos2, count=self.count, norm=nv,
                        n_norm=0 if nv is None else int(nv.numel()), resolution_bp=res)
            n = given
            if n is None and (res, None) in self._matrices:
                n = self._matrices[(res, None)].n   # aggregate_contacts has checked the records and counted the bins
            if n is None:
                need = _lib.query("cgcn_hicdist_workspace_bytes", M=self.M, n_bins=0)
                wsp = _lib._workspace(need, self.device, "Hi-C distance sums, M=%d" % self.M)
                _lib.call("cgcn_hicdist_sums", n_bins=0, workspace=wsp, workspace_bytes=need, raw_out=None, act_out=None,
                          sizes=sizes, **args)
                flags, n = sizes.tolist()
                syncs += 1
                err = hicnorm._bad_records(flags)
                if err is not None:
                    raise err
            raw = torch.zeros(n, dtype=torch.float64, device=self.device)
            act = torch.zeros(n, dtype=torch.float64, device=self.device)
            if n:
                need = _lib.query("cgcn_hicdist_workspace_bytes", M=self.M, n_bins=n)
                wsp = _lib._workspace(need, self.device, "Hi-C distance sums, M=%d n_bins=%d" % (self.M, n))
                _lib.call("cgcn_hicdist_sums", n_bins=n, workspace=wsp, workspace_bytes=need, raw_out=raw, act_out=act, sizes=sizes,
                          **args)
                flags, top = sizes.tolist()
                syncs += 1
                err = hicnorm._bad_records(flags)
                if err is not None:
                    raise err
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
            self._survivors, self._survivors_up, self._gap_survivors = None, {}, {}

    def _window_bins(self, wbp) -> int:
        """the extent of the window bitmap (cgcn_hic_count_up's n_window_bins)"""
        return max(0, int(self._ws_host[-1]) // wbp + 1) if self._ws_host.size else 0

    def survivors(self, window_start, resolution_bp=None, window_bp=None, min_distance_bp=0, expected=None,
                  expected_args=None) -> int:
        """records with pos1 != pos2 and both ends among the windows (cgcn_hic_count; one host sync per window set).  With
        window_bp: of the expanded file (cgcn_hic_count_up; one host sync per window set and window_bp).  min_distance_bp:
        of the records at least that far apart (the *_dist forms; one host sync per window set, window_bp and gap).  expected,
        expected_args: taken like the builders' and without effect: a value does not decide survival."""
        from . import _lib
        up = _upsample(resolution_bp, window_bp)
        gap = _gap(min_distance_bp)
        self._set_windows(window_start)
        n = int(self._ws_host.size)
        if gap:
            return self._survivors_with_gap(n, up, resolution_bp, window_bp, gap)
        if window_bp is None or int(window_bp) == int(resolution_bp):
            if self._survivors is None:
                with torch.cuda.device(self.device):
                    need = _lib.query("cgcn_hic_workspace_bytes", M=self.M, N=n, capacity=0, K=0)
                    wsp = _lib._workspace(need, self.device, "Hi-C build, M=%d" % self.M)
                    out = torch.zeros(1, dtype=torch.int64, device=self.device)
                    _lib.call("cgcn_hic_count", M=self.M, pos1=self.pos1, pos2=self.pos2, window_start=self._ws_dev, N=n,
                              workspace=wsp, workspace_bytes=need, n_survivors=out)
                    self._survivors = int(out.item())
            return self._survivors
        res, wbp = int(resolution_bp), int(window_bp)
        if (res, wbp) not in self._survivors_up:
            with torch.cuda.device(self.device):
                bins = self._window_bins(wbp)
                need = _lib.query("cgcn_hic_up_workspace_bytes", M=self.M, N=n, capacity=0, K=0, resolution_bp=res, window_bp=wbp,
                                  n_window_bins=bins)
                wsp = _lib._workspace(need, self.device, "Hi-C build, M=%d up=%d" % (self.M, up))
                out = torch.zeros(2, dtype=torch.int64, device=self.device)   # [0]: survivors, [1]: positions off the grid
                if res not in self._on_grid:   # read back with the count: still one sync
                    out[1] = ((self.pos1 % res) != 0).sum() + ((self.pos2 % res) != 0).sum()
                _lib.call("cgcn_hic_count_up", M=self.M, pos1=self.pos1, pos2=self.pos2, window_start=self._ws_dev, N=n,
                          resolution_bp=res, window_bp=wbp, n_window_bins=bins, workspace=wsp, workspace_bytes=need,
                          n_survivors=out)
                s, off = out.tolist()
            if off:
                raise ValueError("pos1 / pos2 hold %d positions that are no multiple of resolution_bp=%d" % (off, res))
            self._on_grid.add(res)
            self._survivors_up[(res, wbp)] = int(s)
        return self._survivors_up[(res, wbp)]

    def _survivors_with_gap(self, n, up, resolution_bp, window_bp, gap) -> int:
        from . import _lib
        direct = window_bp is None or int(window_bp) == int(resolution_bp)
        key = (gap, None, None) if direct else (gap, int(resolution_bp), int(window_bp))
        if key in self._gap_survivors:
            return self._gap_survivors[key]
        with torch.cuda.device(self.device):
            if direct:
                need = _lib.query("cgcn_hic_workspace_bytes", M=self.M, N=n, capacity=0, K=0)
                wsp = _lib._workspace(need, self.device, "Hi-C build, M=%d" % self.M)
                out = torch.zeros(1, dtype=torch.int64, device=self.device)
                _lib.call("cgcn_hic_count_dist", M=self.M, pos1=self.pos1, pos2=self.pos2, window_start=self._ws_dev, N=n,
                          min_distance_bp=gap, workspace=wsp, workspace_bytes=need, n_survivors=out)
                s = int(out.item())
            else:
                res, wbp = key[1], key[2]
                bins = self._window_bins(wbp)
                need = _lib.query("cgcn_hic_up_workspace_bytes", M=self.M, N=n, capacity=0, K=0, resolution_bp=res, window_bp=wbp,
                                  n_window_bins=bins)
                wsp = _lib._workspace(need, self.device, "Hi-C build, M=%d up=%d" % (self.M, up))
                out = torch.zeros(2, dtype=torch.int64, device=self.device)   # [0]: survivors, [1]: positions off the grid
                if res not in self._on_grid:   # read back with the count: still one sync
                    out[1] = ((self.pos1 % res) != 0).sum() + ((self.pos2 % res) != 0).sum()
                _lib.call("cgcn_hic_count_up_dist", M=self.M, pos1=self.pos1, pos2=self.pos2, window_start=self._ws_dev, N=n,
                          resolution_bp=res, window_bp=wbp, n_window_bins=bins, min_distance_bp=gap, workspace=wsp,
                          workspace_bytes=need, n_survivors=out)
                s, off = out.tolist()
                if off:
                    raise ValueError("pos1 / pos2 hold %d positions that are no multiple of resolution_bp=%d" % (off, res))
                self._on_grid.add(res)
        self._gap_survivors[key] = int(s)
        return self._gap_survivors[key]

    def build_raw(self, norm, resolution_bp, window_start, hic_edges, window_bp=None, norm_args=None, min_distance_bp=0,
                  expected=None, expected_args=None):
        """(rowptr int32 [N + 1], col int32 [>= nnz], sizes int64 [2] = (nnz, survivors)), all on the device, enqueued
        on the current stream: the {0,1} CSR of the reference's matrix.  No host sync beyond survivors() -- and, for
        norm = 'KR' / 'VC' / 'SQRTVC', those of norm_vector(norm, resolution_bp, **norm_args) when it is not cached; a KR
        that did not converge raises HicNormError.  min_distance_bp, expected (None, a vector, or "auto": expected_vector
        with the same norm and expected_args = n_bins / min_count): the module docstring's rules 3 and 4; with the defaults
        the entry points and the graph are the ones without them."""
        from . import _lib
        k = _budget(hic_edges)
        gap = _gap(min_distance_bp)
        if isinstance(expected, str):
            if expected != "auto":
                raise ValueError("expected=%r is none of None, a vector, 'auto'" % (expected,))
            expected = self.expected_vector(norm, resolution_bp, norm_args=norm_args, **(expected_args or {}))
        if isinstance(norm, str):
            from . import hicnorm
            norm, info = self.norm_vector(norm, resolution_bp, return_info=True, **(norm_args or {}))
            if not info.get("converged", True):
                raise hicnorm.HicNormError("KR did not converge: %r" % (info,), info)
            ws_last = _windows(window_start.cpu().numpy() if torch.is_tensor(window_start) else window_start)
            norm = hicnorm.pad_vector(norm, int(ws_last[-1]) // int(resolution_bp) + 1 if ws_last.size else 0)
        up = _upsample(resolution_bp, window_bp)
        direct = window_bp is None or int(window_bp) == int(resolution_bp)
        cap = (self.survivors(window_start, min_distance_bp=gap) if direct
               else self.survivors(window_start, resolution_bp, window_bp, min_distance_bp=gap))
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
            if direct:
                need = _lib.query("cgcn_hic_workspace_bytes", M=self.M, N=n, capacity=cap, K=k)
                wsp = _lib._workspace(need, self.device, "Hi-C build, M=%d capacity=%d K=%d" % (self.M, cap, k))
                _lib.call("cgcn_hic_build_dist" if dist else "cgcn_hic_build", M=self.M, pos1=self.pos1, pos2=self.pos2, count=self.count, norm=nv,
                          n_bins=0 if nv is None else int(nv.numel()), resolution_bp=int(resolution_bp), window_start=ws, N=n,
                          K=k, capacity=cap, workspace=wsp, workspace_bytes=need, rowptr_out=rowptr, col_out=col,
                          nnz_out=sizes.data_ptr(), n_survivors=sizes.data_ptr() + 8, **dist)
            else:
                res, wbp = int(resolution_bp), int(window_bp)
                bins = self._window_bins(wbp)
                need = _lib.query("cgcn_hic_up_workspace_bytes", M=self.M, N=n, capacity=cap, K=k, resolution_bp=res,
                                  window_bp=wbp, n_window_bins=bins)
                wsp = _lib._workspace(need, self.device, "Hi-C build, M=%d up=%d capacity=%d K=%d" % (self.M, up, cap, k))
                _lib.call("cgcn_hic_build_up_dist" if dist else "cgcn_hic_build_up", M=self.M, pos1=self.pos1, pos2=self.pos2, count=self.count, norm=nv,
                          n_bins=0 if nv is None else int(nv.numel()), resolution_bp=res, window_bp=wbp, n_window_bins=bins,
                          window_start=ws, N=n, K=k, capacity=cap, workspace=wsp, workspace_bytes=need, rowptr_out=rowptr,
                          col_out=col, nnz_out=sizes.data_ptr(), n_survivors=sizes.data_ptr() + 8, **dist)
        return rowptr, col, sizes

    def build(self, norm, resolution_bp, window_start, hic_edges, adj_type="hic", return_raw=False, window_bp=None,
              norm_args=None, min_distance_bp=0, expected=None, expected_args=None):
        """ChromGraph of process_graph(adj_type, ...) over the top-K contact matrix; the matrix itself never visits the
        host.  return_raw=True: (graph, the {0,1} scipy CSR the reference pickles) -- one more read-back.  norm: a vector,
        None, or 'KR' / 'VC' / 'SQRTVC' (computed from the records; norm_args: norm_vector's keywords).  min_distance_bp,
        expected, expected_args: build_raw's."""
        rowptr, col, sizes = self.build_raw(norm, resolution_bp, window_start, hic_edges, window_bp=window_bp,
                                            norm_args=norm_args, min_distance_bp=min_distance_bp, expected=expected,
                                            expected_args=expected_args)
        n = int(rowptr.numel()) - 1
        g = G.normalize_device_csr(adj_type, n, rowptr, col, None, self.device)
        if not return_raw:
            return g
        nnz = int(sizes[0].item())
        raw = sp.csr_matrix((np.ones(nnz, np.float64), col[:nnz].cpu().numpy(), rowptr.cpu().numpy()), shape=(n, n))
        return g, raw


def build_hic_graph(pos1, pos2, count, norm, resolution_bp, window_start, hic_edges, adj_type="hic", device="cuda",
                    return_raw=False, window_bp=None, norm_args=None, min_distance_bp=0, expected=None, expected_args=None):
    """build_hic_graph_host on the device, handed straight to the device normaliser: contacts in, ChromGraph out.
    `pos1` may be a HicContacts (then pos2 and count are ignored): nothing is uploaded again.  window_bp: the records are
    coarser than the windows and stand for their expanded file (the module's docstring).  min_distance_bp, expected (None, a
    vector, "auto"), expected_args: the minimum gap and the observed / expected value (the module's docstring)."""
    _upsample(resolution_bp, window_bp)
    c = pos1 if isinstance(pos1, HicContacts) else HicContacts(pos1, pos2, count, device)
    return c.build(norm, resolution_bp, window_start, hic_edges, adj_type=adj_type, return_raw=return_raw, window_bp=window_bp,
                   norm_args=norm_args, min_distance_bp=min_distance_bp, expected=expected, expected_args=expected_args)


def contacts_from_text(path_or_bytes, device="cuda", **kw) -> HicContacts:
    """HicContacts.from_text: contact text in, device-resident records out"""
    return HicContacts.from_text(path_or_bytes, device=device, **kw)


def contact_cache_path(root: str, chrom: str) -> str:
    return os.path.join(root, "%s.cghic" % chrom)


def graphs_from_contact_caches(root: str, chroms, hicsize, hicnorm: str, adj_type: str = "hic", device="cuda",
                               sizes: Optional[Dict[str, int]] = None, window_bp=None,
                               compute_norm: bool = False, min_distance_bp=0, expected=None,
                               expected_args=None) -> Dict[str, G.ChromGraph]:
    """{chrom: ChromGraph} from `<root>/<chrom>.cghic` (save_contacts_cache, with the chromosome's windows) for the edge
    budget `hicsize` and the norm vector named `hicnorm` ('' = none): what `chromegcn_amd.train -hic_contacts` loads
    instead of `{split}_graphs_{hicsize}_{hicnorm}norm.pkl`.  sizes: the expected window count per chromosome.  window_bp
    (`-hic_upsample`): the window size; a cache whose resolution_bp is coarser is built as its expanded file.  compute_norm
    (`-hic_compute_norm`): a `hicnorm` of 'KR' / 'VC' / 'SQRTVC' that the cache lacks is computed from its records.
    min_distance_bp (`-hic_min_distance`), expected (`-hic_expected`: "auto", the vector computed from each cache's records
    with the vector the call scores with; any other name: the vector the cache stores under it, tools/hic_ingest.py
    --compute-expected writes eRAW / eKR / eVC / eSQRTVC), expected_args: build_hic_graph's."""
    from . import hicnorm as HN
    out = {}
    for chrom in chroms:
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
        out[chrom] = build_hic_graph(c.pos1, c.pos2, c.count, norm, c.resolution_bp,
                                     c.window_start, int(hicsize), adj_type=adj_type, device=device,
                                     min_distance_bp=min_distance_bp, expected=ex, expected_args=expected_args, **up)
    return out
