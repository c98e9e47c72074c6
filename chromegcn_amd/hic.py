"""The top-K Hi-C contact graph from raw contact records: the reference's data/7create_graph_new.py
(get_normalization_values :51-65, get_contact_edge_pairs :67-91, get_top_contact_locs :93-104, create_adj_mat :108-120,
K = hic_edges / 2 :168) for any edge budget and any normalisation vector, on the device (csrc/cgcn_hic.hip) with a numpy
restatement beside it.

The rule, for one chromosome: a record (pos1, pos2, count) survives iff pos1 != pos2 and both positions are windows with
peaks; its value is count / (nv[pos1 // res] * nv[pos2 // res]) in float64, nv = the norm vector with NaN and 0 replaced by
+inf (count itself without a vector); the K survivors that come first in a STABLE descending sort by value are taken;
A[i, j] = A[j, i] = 1 for each of them, i, j the ranks of the two positions among the windows.  Outside the contract: two
records with the same ordered (pos1, pos2), NaN counts, 2 K >= 2^31."""
from __future__ import annotations

import os
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


def survivor_values(pos1, pos2, count, norm, resolution_bp, window_start):
    """(record index, i, j, value) of the surviving records in file order (rules 1 and 2)."""
    ws = _windows(window_start).astype(np.int64)
    p1, p2 = np.asarray(pos1, dtype=np.int64), np.asarray(pos2, dtype=np.int64)
    n = ws.size
    if n == 0 or p1.size == 0:
        e = np.zeros(0, np.int64)
        return e, e, e, np.zeros(0, np.float64)
    i = np.minimum(np.searchsorted(ws, p1), n - 1)
    j = np.minimum(np.searchsorted(ws, p2), n - 1)
    idx = np.flatnonzero((p1 != p2) & (ws[i] == p1) & (ws[j] == p2))
    v = np.asarray(count)[idx].astype(np.float64)
    if norm is not None:
        nv = np.array(norm, dtype=np.float64)
        _check_norm(nv, resolution_bp, ws)
        nv[np.isnan(nv) | (nv == 0.0)] = np.inf
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            v = v / (nv[p1[idx] // int(resolution_bp)] * nv[p2[idx] // int(resolution_bp)])
    return idx, i[idx], j[idx], v


def build_hic_graph_host(pos1, pos2, count, norm, resolution_bp, window_start, hic_edges) -> sp.csr_matrix:
    """The {0,1} float64 CSR the reference's step 7 pickles (symmetric, zero diagonal, sorted columns)."""
    n = _windows(window_start).size
    k = _budget(hic_edges)
    _, i, j, v = survivor_values(pos1, pos2, count, norm, resolution_bp, window_start)
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
        self._survivors = 0
        self._vectors = []   # (the caller's object, its device copy): a sweep passes the same vector again

    @classmethod
    def from_host(cls, c: HostContacts, device="cuda") -> "HicContacts":
        return cls(c.pos1, c.pos2, c.count, device)

    def _up(self, a, dtype) -> torch.Tensor:
        t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
        return t.to(device=self.device, dtype=dtype).contiguous()

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

    def survivors(self, window_start) -> int:
        """records with pos1 != pos2 and both ends among the windows (cgcn_hic_count; one host sync per window set)"""
        from . import _lib
        ws = _windows(window_start.cpu().numpy() if torch.is_tensor(window_start) else window_start)
        if self._ws_host is not None and np.array_equal(ws, self._ws_host):
            return self._survivors
        ws_dev = torch.from_numpy(ws).to(self.device)
        with torch.cuda.device(self.device):
            need = _lib.query("cgcn_hic_workspace_bytes", M=self.M, N=int(ws.size), capacity=0, K=0)
            wsp = _lib._workspace(need, self.device, "Hi-C build, M=%d" % self.M)
            out = torch.zeros(1, dtype=torch.int64, device=self.device)
            _lib.call("cgcn_hic_count", M=self.M, pos1=self.pos1, pos2=self.pos2, window_start=ws_dev, N=int(ws.size),
                      workspace=wsp, workspace_bytes=need, n_survivors=out)
            self._survivors = int(out.item())
        self._ws_host, self._ws_dev = ws, ws_dev
        return self._survivors

    def build_raw(self, norm, resolution_bp, window_start, hic_edges):
        """(rowptr int32 [N + 1], col int32 [>= nnz], sizes int64 [2] = (nnz, survivors)), all on the device, enqueued
        on the current stream: the {0,1} CSR of the reference's matrix.  No host sync beyond survivors()."""
        from . import _lib
        k = _budget(hic_edges)
        cap = self.survivors(window_start)
        ws, n = self._ws_dev, int(self._ws_host.size)
        nv = self._norm(norm)
        if nv is not None:
            _check_norm(nv, resolution_bp, self._ws_host)
        with torch.cuda.device(self.device):
            need = _lib.query("cgcn_hic_workspace_bytes", M=self.M, N=n, capacity=cap, K=k)
            wsp = _lib._workspace(need, self.device, "Hi-C build, M=%d capacity=%d K=%d" % (self.M, cap, k))
            rowptr = torch.empty(n + 1, dtype=torch.int32, device=self.device)
            col = torch.empty(max(2 * min(k, cap), 1), dtype=torch.int32, device=self.device)
            sizes = torch.zeros(2, dtype=torch.int64, device=self.device)   # [0]: nnz (its low int32 half), [1]: survivors
            _lib.call("cgcn_hic_build", M=self.M, pos1=self.pos1, pos2=self.pos2, count=self.count, norm=nv,
                      n_bins=0 if nv is None else int(nv.numel()), resolution_bp=int(resolution_bp), window_start=ws, N=n, K=k,
                      capacity=cap, workspace=wsp, workspace_bytes=need, rowptr_out=rowptr, col_out=col,
                      nnz_out=sizes.data_ptr(), n_survivors=sizes.data_ptr() + 8)
        return rowptr, col, sizes

    def build(self, norm, resolution_bp, window_start, hic_edges, adj_type="hic", return_raw=False):
        """ChromGraph of process_graph(adj_type, ...) over the top-K contact matrix; the matrix itself never visits the
        host.  return_raw=True: (graph, the {0,1} scipy CSR the reference pickles) -- one more read-back."""
        rowptr, col, sizes = self.build_raw(norm, resolution_bp, window_start, hic_edges)
        n = int(rowptr.numel()) - 1
        g = G.normalize_device_csr(adj_type, n, rowptr, col, None, self.device)
        if not return_raw:
            return g
        nnz = int(sizes[0].item())
        raw = sp.csr_matrix((np.ones(nnz, np.float64), col[:nnz].cpu().numpy(), rowptr.cpu().numpy()), shape=(n, n))
        return g, raw


def build_hic_graph(pos1, pos2, count, norm, resolution_bp, window_start, hic_edges, adj_type="hic", device="cuda",
                    return_raw=False):
    """build_hic_graph_host on the device, handed straight to the device normaliser: contacts in, ChromGraph out.
    `pos1` may be a HicContacts (then pos2 and count are ignored): nothing is uploaded again."""
    c = pos1 if isinstance(pos1, HicContacts) else HicContacts(pos1, pos2, count, device)
    return c.build(norm, resolution_bp, window_start, hic_edges, adj_type=adj_type, return_raw=return_raw)


def contact_cache_path(root: str, chrom: str) -> str:
    return os.path.join(root, "%s.cghic" % chrom)


def graphs_from_contact_caches(root: str, chroms, hicsize, hicnorm: str, adj_type: str = "hic", device="cuda",
                               sizes: Optional[Dict[str, int]] = None) -> Dict[str, G.ChromGraph]:
    """{chrom: ChromGraph} from `<root>/<chrom>.cghic` (save_contacts_cache, with the chromosome's windows) for the edge
    budget `hicsize` and the norm vector named `hicnorm` ('' = none): what `chromegcn_amd.train -hic_contacts` loads
    instead of `{split}_graphs_{hicsize}_{hicnorm}norm.pkl`.  sizes: the expected window count per chromosome."""
    out = {}
    for chrom in chroms:
        c = load_contacts_cache(contact_cache_path(root, chrom))
        if c.window_start is None:
            raise ValueError("%s holds no window list" % contact_cache_path(root, chrom))
        if hicnorm and hicnorm not in c.norms:
            raise ValueError("%s holds no %r norm vector (has: %s)" % (contact_cache_path(root, chrom), hicnorm,
                                                                       ", ".join(sorted(c.norms)) or "none"))
        if sizes is not None and sizes[chrom] != c.window_start.size:
            raise ValueError("%s has %d windows but the chromosome's features have %d rows"
                             % (contact_cache_path(root, chrom), c.window_start.size, sizes[chrom]))
        out[chrom] = build_hic_graph(c.pos1, c.pos2, c.count, c.norms[hicnorm] if hicnorm else None, c.resolution_bp,
                                     c.window_start, int(hicsize), adj_type=adj_type, device=device)
    return out
