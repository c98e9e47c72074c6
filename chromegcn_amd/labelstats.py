"""Label and Hi-C neighbourhood statistics: for a label matrix and the chromosomes' graphs, how many
Hi-C neighbours the windows of a label have (scripts/analyze_results.py:226-266, get_label_weights: the x axis of the paper's
per-label improvement figure), how often a contact joins a window of label a to a window of label b (exactly the entries the
label-pair ablation removes for that pair), and the reference's -summarize_data numbers (utils/util_methods.py:24-74: labels
per window, windows per label, label correlation).

All counts are exact integers, made on the device from tensors that already live there (cgcn_labelstats_windows /
cgcn_labelstats_graph, csrc/cgcn_labelstats.hip).  Window u is positive for label c iff targets[u, c] != 0 (the ablation's
rule; NaN counts as positive); P_c is the set of such windows.

    label_count[c]       |P_c|                                             int64 [C]
    labels_hist[k]       windows with exactly k positive labels, k = 0..C  int64 [C + 1]
    cooccurrence[a, b]   |P_a and P_b|                                     int64 [C, C]
    n_entries            neighbour entries of the graph                    int64 [1]
    degree_sum[c]        sum over P_c of deg[u]                            int64 [C]
    contact_pairs[a, b]  neighbour entries (u, v), u in P_a, v in P_b      int64 [C, C]

A NEIGHBOUR ENTRY is a stored entry (u, v) of the graph with u != v and, where the graph has values, val > 0; deg[u] is the
number of them in row u.  For a ChromGraph of adj_type 'hic' that is the reference's row sum of the raw pickle matrix
(analyze_results.py:254-260): the self loop process_graph adds is not counted, entries the ablation zeroed are not counted;
for 'both' the band entries count, they are edges of that graph.  The reference clips values above 1 and SUMS values
(:256,260); this counts ENTRIES.  The two agree for the {0, 1} pickles and for any values >= 1, and differ for fractional
values (an entry of 0.5 adds 0.5 there and 1 here).

The statistics of several chromosomes add element-wise (`+`, or on the device with label_stats_split), which is how the
reference pools the test chromosomes.  Everything derived (average degree, Pearson correlation, medians, enrichment) is
float64 host arithmetic on the integers alone.  label_stats_host is the numpy / scipy restatement: the same integers."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Optional

import numpy as np
import scipy.sparse as sp
import torch

from . import _lib
from .graph import ChromGraph, HostCSR

MAX_C = 256   # CGCN_LABELSTATS_MAX_C

_WINDOW_FIELDS = ("label_count", "labels_hist", "cooccurrence")
_GRAPH_FIELDS = ("n_entries", "degree_sum", "contact_pairs")


def _ratio(a, b):
    """a / b in float64, NaN where b == 0"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    out = np.full(np.broadcast(a, b).shape, np.nan)
    np.divide(a, b, out=out, where=b != 0)
    return out


def _lower_median_of_counts(hist: np.ndarray) -> int:
    """lower median of the multiset that holds the value k hist[k] times (torch.median's choice of two middle values)"""
    total = int(hist.sum())
    if total == 0:
        raise ValueError("median of no values")
    return int(np.searchsorted(np.cumsum(hist), (total - 1) // 2 + 1))


@dataclass
class LabelStats:
    """The integer arrays of the module docstring (device tensors from label_stats / label_stats_split, numpy arrays from
    label_stats_host or host()), the number of windows and of labels.  The three graph arrays are None when no graph was
    given.  `a + b` pools two of them."""
    n_windows: int
    C: int
    label_count: object
    labels_hist: object
    cooccurrence: object
    n_entries: object = None
    degree_sum: object = None
    contact_pairs: object = None

    @property
    def has_graph(self) -> bool:
        return self.degree_sum is not None

    def host(self) -> "LabelStats":
        """the same statistics as numpy int64 arrays (one device-to-host copy when they live on the device)"""
        names = _WINDOW_FIELDS + (_GRAPH_FIELDS if self.has_graph else ())
        fields = [getattr(self, k) for k in names]
        if isinstance(self.label_count, torch.Tensor):
            flat = torch.cat([f.reshape(-1) for f in fields]).cpu().numpy()
            out, at = {}, 0
            for k, f in zip(names, fields):
                out[k] = flat[at:at + f.numel()].reshape(tuple(f.shape)).copy()
                at += f.numel()
        else:
            out = {k: np.asarray(f, dtype=np.int64) for k, f in zip(names, fields)}
        return LabelStats(self.n_windows, self.C, **out)

    def __add__(self, other: "LabelStats") -> "LabelStats":
        if not isinstance(other, LabelStats):
            return NotImplemented
        if self.C != other.C:
            raise ValueError("LabelStats of %d and %d labels cannot be pooled" % (self.C, other.C))
        if self.has_graph != other.has_graph:
            raise ValueError("LabelStats with and without graph statistics cannot be pooled")
        a, b = self, other
        if isinstance(a.label_count, torch.Tensor) != isinstance(b.label_count, torch.Tensor):
            a, b = a.host(), b.host()
        names = _WINDOW_FIELDS + (_GRAPH_FIELDS if self.has_graph else ())
        return LabelStats(a.n_windows + b.n_windows, a.C, **{k: getattr(a, k) + getattr(b, k) for k in names})

    # ---- derived on the host, float64, from the integers only ----------------------------------------------------------------
    def _need_graph(self, what: str) -> "LabelStats":
        if not self.has_graph:
            raise ValueError("LabelStats.%s needs graph statistics (label_stats was called without a graph)" % what)
        return self.host()

    def average_degree(self) -> np.ndarray:
        """[C] degree_sum / label_count, NaN where the count is 0: the reference's normalized_label_weights
        (analyze_results.py:264)"""
        h = self._need_graph("average_degree")
        return _ratio(h.degree_sum, h.label_count)

    def pearson(self) -> np.ndarray:
        """[C, C] Pearson correlation of the label columns, (n co - c_a c_b) / sqrt(c_a (n - c_a) c_b (n - c_b)), NaN where
        a factor under the root is 0: np.corrcoef(targets.T) of {0, 1} targets (utils/util_methods.py:48)"""
        h = self.host()
        n = float(h.n_windows)
        c = h.label_count.astype(np.float64)
        var = c * (n - c)
        num = n * h.cooccurrence.astype(np.float64) - np.outer(c, c)
        den = np.sqrt(np.outer(var, var))
        out = _ratio(num, den)
        out[(var == 0)[:, None] | (var == 0)[None, :]] = np.nan
        return out

    def labels_per_window(self) -> Dict[str, float]:
        """mean, (lower) median and max of the number of positive labels of a window (utils/util_methods.py:60-66), from
        labels_hist"""
        h = self.host().labels_hist
        k = np.arange(h.shape[0], dtype=np.int64)
        total = int(h.sum())
        if total == 0:
            return {"mean": float("nan"), "median": float("nan"), "max": float("nan")}
        return {"mean": float(int((k * h).sum()) / total), "median": float(_lower_median_of_counts(h)),
                "max": float(k[h > 0].max())}

    def samples_per_label(self) -> Dict[str, float]:
        """mean, (lower) median and max of the number of positive windows of a label (utils/util_methods.py:68-74), from
        label_count"""
        c = np.sort(self.host().label_count)
        return {"mean": float(int(c.sum()) / c.shape[0]), "median": float(c[(c.shape[0] - 1) // 2]), "max": float(c[-1])}

    def contact_enrichment(self) -> np.ndarray:
        """[C, C] contact_pairs[a, b] n_entries / (degree_sum[a] degree_sum[b]), NaN where a factor is 0: observed over
        expected under a degree-preserving null"""
        h = self._need_graph("contact_enrichment")
        d = h.degree_sum.astype(np.float64)
        return _ratio(h.contact_pairs.astype(np.float64) * float(h.n_entries[0]), np.outer(d, d))


# ---- the graphs a caller may hand over ----------------------------------------------------------------------------------------
def _host_csr_arrays(graph):
    """(n, rowptr int32, col int32, val float32 or None) numpy arrays of a HostCSR or a scipy sparse matrix; the matrix is
    taken as is (a raw pickle entry: no + I, no normalisation)"""
    if isinstance(graph, HostCSR):
        return graph.n, graph.rowptr, graph.col, graph.val
    if sp.issparse(graph):
        a = sp.csr_matrix(graph)
        if a.shape[0] != a.shape[1]:
            raise ValueError("label_stats: the graph must be square, got %s" % (a.shape,))
        if a.nnz >= 2 ** 31:
            raise ValueError("label_stats: graph too large for int32 CSR")
        val = a.data.astype(np.float32)
        if np.any((a.data > 0) != (val > 0)):
            raise ValueError("label_stats: a positive graph value rounds to 0 in float32")
        return (a.shape[0], a.indptr.astype(np.int32), a.indices.astype(np.int32), None if np.all(val == 1) else val)
    raise TypeError("label_stats: graph must be a ChromGraph, a HostCSR or a scipy sparse matrix, got %r" % type(graph))


def _device_csr(graph, dev):
    """(n, nnz, rowptr, col, val or None) on the device"""
    if isinstance(graph, ChromGraph):
        if graph.device != dev:
            raise RuntimeError("label_stats: the graph is on %s but the targets are on %s" % (graph.device, dev))
        return graph.n, graph.nnz, graph.rowptr, graph.col, graph.val
    n, rowptr, col, val = _host_csr_arrays(graph)
    if rowptr.shape[0] != n + 1 or int(rowptr[0]) != 0 or int(rowptr[-1]) != col.shape[0] or np.any(np.diff(rowptr) < 0):
        raise ValueError("label_stats: invalid CSR row pointers")
    if col.shape[0] and (int(col.min()) < 0 or int(col.max()) >= n):
        raise ValueError("label_stats: a column index lies outside [0, %d)" % n)   # the kernels trust the structure

    def up(a, dt):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dt)
    return n, int(col.shape[0]), up(rowptr, torch.int32), up(col, torch.int32), up(val, torch.float32)


def _device_targets(targets) -> torch.Tensor:
    if not isinstance(targets, torch.Tensor) or not targets.is_cuda:
        raise RuntimeError("chromegcn_amd.labelstats: targets must be a tensor on the GPU (there is no CPU fallback; the "
                           "numpy restatement is label_stats_host)")
    if targets.dim() != 2:
        raise RuntimeError("targets must be [n, C], got %s" % (tuple(targets.shape),))
    if targets.dtype != torch.float32:
        targets = (targets != 0).to(torch.float32)     # bool and integer input: nonzero = positive
    return targets.contiguous()


class _Accumulator:
    """the device outputs of a pooled run: the first add zeroes them (accumulate = 0), every later one adds"""

    def __init__(self, C: int, dev, with_graph: bool):
        if not 1 <= C <= MAX_C:
            raise RuntimeError("chromegcn_amd.labelstats: unsupported number of labels C = %d (1 .. %d)" % (C, MAX_C))
        self.C, self.dev, self.n_windows, self.calls = C, dev, 0, 0
        e = lambda *shape: torch.empty(shape, device=dev, dtype=torch.int64)
        self.window = (e(C), e(C + 1), e(C, C))
        self.graph = (e(1), e(C), e(C, C)) if with_graph else None

    def add(self, targets, graph):
        tg = _device_targets(targets)
        n, C = tg.shape
        if C != self.C or tg.device != self.dev:
            raise RuntimeError("label_stats: every label matrix must be [n, %d] on %s" % (self.C, self.dev))
        acc = int(self.calls > 0)
        with torch.cuda.device(self.dev):
            ws, ws_bytes = _lib.workspace_for("cgcn_labelstats_workspace_bytes", self.dev,
                                              "label statistics, n=%d C=%d" % (n, C), n=n, C=C)
            cnt, hist, co = self.window
            _lib.call("cgcn_labelstats_windows", n=n, C=C, targets=tg, workspace=ws, workspace_bytes=ws_bytes, label_count=cnt,
                      labels_hist=hist, cooccurrence=co, accumulate=acc)
            if self.graph is not None:
                gn, nnz, rowptr, col, val = _device_csr(graph, self.dev)
                if gn != n:
                    raise ValueError("the graph has %d nodes but the label matrix %d rows" % (gn, n))
                ent, dsum, pairs = self.graph
                _lib.call("cgcn_labelstats_graph", n=n, C=C, nnz=nnz, rowptr=rowptr, col=col, val=val, label_bits=ws,
                          label_bits_bytes=ws_bytes, degree_sum=dsum, contact_pairs=pairs, n_entries=ent, accumulate=acc)
        self.n_windows += n
        self.calls += 1

    def result(self) -> LabelStats:
        cnt, hist, co = self.window
        ent, dsum, pairs = self.graph if self.graph is not None else (None, None, None)
        return LabelStats(self.n_windows, self.C, cnt, hist, co, ent, dsum, pairs)


def label_stats(targets: torch.Tensor, graph=None) -> LabelStats:
    """LabelStats of one chromosome on the device.  targets: [n, C] CUDA tensor, 1 <= C <= 256 (float32 is taken as is, bool
    and integer input is converted: nonzero = positive).  graph: None (only the window statistics are filled), a ChromGraph
    on the same device, a HostCSR, or a scipy sparse matrix (taken as is, a raw pickle entry: no + I, no normalisation).
    Neither the label matrix nor a device graph is copied to the host."""
    tg = _device_targets(targets)
    acc = _Accumulator(int(tg.shape[1]), tg.device, graph is not None)
    acc.add(tg, graph)
    return acc.result()


def _pairs_of(targets_by_chrom, graphs_by_chrom):
    if isinstance(targets_by_chrom, dict):
        if graphs_by_chrom is not None and not isinstance(graphs_by_chrom, dict):
            raise TypeError("label_stats_split: targets by name need graphs by name")
        return [(t, None if graphs_by_chrom is None else graphs_by_chrom[c]) for c, t in targets_by_chrom.items()]
    ts = list(targets_by_chrom)
    gs = [None] * len(ts) if graphs_by_chrom is None else list(graphs_by_chrom)
    if len(gs) != len(ts):
        raise ValueError("label_stats_split: %d label matrices but %d graphs" % (len(ts), len(gs)))
    return list(zip(ts, gs))


def label_stats_split(targets_by_chrom, graphs_by_chrom=None) -> LabelStats:
    """The pooled LabelStats of a split: the loop over chromosomes of get_label_weights (analyze_results.py:250-262), pooled on
    the device (`accumulate`).  Both arguments are dicts keyed by chromosome, or sequences in the same order;
    graphs_by_chrom = None leaves the graph statistics out."""
    pairs = _pairs_of(targets_by_chrom, graphs_by_chrom)
    if not pairs:
        raise ValueError("label_stats_split: no chromosome given")
    first = _device_targets(pairs[0][0])
    acc = _Accumulator(int(first.shape[1]), first.device, graphs_by_chrom is not None)
    for t, g in pairs:
        if graphs_by_chrom is not None and g is None:
            raise ValueError("label_stats_split: a chromosome has no graph")
        acc.add(t, g)
    return acc.result()


# ---- numpy / scipy restatement: the specification -----------------------------------------------------------------------------
def label_stats_host(targets, graph=None) -> LabelStats:
    """LabelStats of numpy int64 arrays from T.T @ T, T.T @ (A @ T) and np.bincount, T the {0, 1} matrix of targets != 0 and A
    the {0, 1} matrix of the neighbour entries.  graph: as label_stats (a ChromGraph is downloaded)."""
    if isinstance(targets, torch.Tensor):
        targets = targets.detach().cpu().numpy()
    targets = np.asarray(targets)
    if targets.ndim != 2:
        raise ValueError("targets must be [n, C], got %s" % (targets.shape,))
    n, C = targets.shape
    if not 1 <= C <= MAX_C:
        raise ValueError("unsupported number of labels C = %d (1 .. %d)" % (C, MAX_C))
    T = sp.csr_matrix((targets != 0).astype(np.int64))      # NaN != 0: positive
    Td = T.toarray()
    out = dict(label_count=Td.sum(axis=0).astype(np.int64),
               labels_hist=np.bincount(Td.sum(axis=1), minlength=C + 1).astype(np.int64),
               cooccurrence=np.asarray((T.T @ T).todense(), dtype=np.int64))
    if graph is not None:
        if isinstance(graph, ChromGraph):
            gn, rowptr, col = graph.n, graph.rowptr.cpu().numpy(), graph.col.cpu().numpy()
            val = None if graph.val is None else graph.val.cpu().numpy()
        else:
            gn, rowptr, col, val = _host_csr_arrays(graph)
        if gn != n:
            raise ValueError("the graph has %d nodes but the label matrix %d rows" % (gn, n))
        rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr.astype(np.int64)))
        keep = rows != col
        if val is not None:
            keep &= val > 0
        A = sp.csr_matrix((np.ones(int(keep.sum()), dtype=np.int64), (rows[keep], col[keep].astype(np.int64))), shape=(n, n))
        deg = np.asarray(A.sum(axis=1), dtype=np.int64).ravel()     # stored duplicates, if any, count once each: summed
        out.update(n_entries=np.array([deg.sum()], dtype=np.int64), degree_sum=(Td * deg[:, None]).sum(axis=0).astype(np.int64),
                   contact_pairs=np.asarray((T.T @ (A @ T)).todense(), dtype=np.int64))
    return LabelStats(int(n), int(C), **out)


def label_stats_split_host(targets_by_chrom, graphs_by_chrom=None) -> LabelStats:
    """label_stats_split with label_stats_host and `+`"""
    total: Optional[LabelStats] = None
    for t, g in _pairs_of(targets_by_chrom, graphs_by_chrom):
        s = label_stats_host(t, g)
        total = s if total is None else total + s
    if total is None:
        raise ValueError("label_stats_split_host: no chromosome given")
    return total
