"""Label-pair Hi-C edge ablation: the TF-TF interaction map of scripts/visualize.py:79-119, on the sparsity pattern.

For every pair of labels (i, j): remove every Hi-C edge from a window positive for i (P_i) to a window positive for j (P_j),
renormalise those rows, run the model on both strands and record how far the mean predicted probability of label i on P_i
drops relative to the full graph:  M[i, j] = (base_i - abl_ij) / base_i.

The reference builds a dense n x n adjacency per pair (133 MB at chr21 size, 3.6 GB at chr1 size) and runs two whole
forwards.  Here:
  * restricted route (L <= 2, the default there): an ablation changes only the rows of P_i, in every layer, so the
    (j, u in P_i) row instances are recomputed from the unablated forward's layer inputs (cgcn_ablation_layer) and only
    label i's head is evaluated on them (cgcn_ablation_head); a bounded number of launches per row label, never per pair;
  * composed route (any L; the cross-check): per pair, the masked values and row scales on the unchanged pattern
    (cgcn_ablation_mask), the library's eval forward over them, and one reduction (cgcn_ablation_reduce).
Special cases: M[i, i], an empty P_j and pairs outside rows x cols are 0; an empty P_i gives NaN (the reference's mean of
an empty tensor); a pair that removes no stored entry gives exactly 0."""
from __future__ import annotations

from typing import Iterable, List, Optional

import torch

from . import graph as G
from . import ops
from .graph import ChromGraph, as_graph

ROUTES = ("auto", "restricted", "composed")
_S = 2   # both strands (visualize.py:110-112)


def _align(b: int) -> int:
    return (b + 255) & ~255


def _labels(sel: Optional[Iterable[int]], C: int, what: str) -> List[int]:
    if sel is None:
        return list(range(C))
    out = []
    for c in sel:
        c = int(c)
        if not 0 <= c < C:
            raise ValueError("label_pair_ablation: %s label %d outside [0, %d)" % (what, c, C))
        if c not in out:
            out.append(c)
    return out


def _eval_stack(model, x: torch.Tensor, graph: ChromGraph) -> List[torch.Tensor]:
    """[X^0, X^1, ..., X^L] of the unablated eval forward ([S, n, d] each; cgcn_layer_fwd without Z / H)"""
    xs = [x]
    for k in range(1, model.n_layers + 1):
        gc, wk = getattr(model, "GC%d" % k), getattr(model, "W%d" % k)
        xn, _ = ops.layer_fwd(xs[-1], ops._layer_params(gc.weight, gc.bias, wk.weight, wk.bias),
                              (graph.rowptr, graph.col, graph.val, graph.row_scale), None, None)
        xs.append(xn)
    return xs


class RestrictedAblation:
    """The restricted route (L <= 2) for one model, chromosome and label set.  Construction runs the unablated forward and
    fills `base` [C]; `workspace(n_inst)` allocates the instance buffers; `run_row` enqueues the launches of one row
    label and one batch of column labels -- no allocation, no host synchronisation, so it can be captured into a graph."""

    def __init__(self, model, x: torch.Tensor, graph: ChromGraph, bits, lists, ranks, counts):
        self.L = model.n_layers
        if self.L > 2:
            raise ValueError("the restricted route covers models of at most 2 layers")
        self.model, self.graph = model, graph
        self.S, self.n, self.d = x.shape
        self.C = model.out.weight.shape[0]
        self.bits, self.lists, self.ranks, self.counts = bits, lists, ranks, counts
        self.params = []
        for k in range(1, self.L + 1):
            gc, wk = getattr(model, "GC%d" % k), getattr(model, "W%d" % k)
            self.params.append(ops._layer_params(gc.weight.detach(), gc.bias.detach(), wk.weight.detach(), wk.bias.detach()))
        self.xs = _eval_stack(model, x, graph)
        self.base = torch.empty(self.C, device=x.device, dtype=torch.float32)
        ops.ablation_head(self.xs[-1], None, model.batch_norm, model.out, lists, counts, -1, 0, None, 0, None, self.base,
                          None, self.d)

    def workspace(self, n_inst: int):
        """(X1, X2 or None, removed) instance buffers for up to n_inst instances (cgcn_ablation_workspace_bytes layout)"""
        nbytes = ops.ablation_workspace_bytes(n_inst, self.S, self.d, self.L)
        if nbytes == 0:
            raise RuntimeError("chromegcn_amd: label_pair_ablation: unsupported shape (S=%d, d=%d, L=%d)" % (self.S, self.d, self.L))
        ws = torch.empty(nbytes, device=self.base.device, dtype=torch.uint8)
        feat, fb = n_inst * self.S * self.d, _align(n_inst * self.S * self.d * 4)
        x1 = ws[:4 * feat].view(torch.float32)
        x2 = ws[fb:fb + 4 * feat].view(torch.float32) if self.L == 2 else None
        off = fb * self.L
        removed = ws[off:off + 4 * n_inst].view(torch.int32)
        return x1, x2, removed

    def run_row(self, i: int, n_pos: int, cols: torch.Tensor, n_cols: int, ws, M: torch.Tensor):
        """M[i, cols[:n_cols]] for row label i with |P_i| = n_pos; cols: int32 device view; ws from workspace() with room
        for n_cols * n_pos instances"""
        x1, x2, removed = ws
        pl, pr = self.lists[i], self.ranks[i]
        g = self.graph
        ops.ablation_layer(g, self.xs[0], None, self.params[0], self.bits, self.C, pl, pr, n_pos, cols, n_cols, x1, removed)
        last = x1
        if self.L == 2:
            ops.ablation_layer(g, self.xs[1], x1, self.params[1], self.bits, self.C, pl, pr, n_pos, cols, n_cols, x2, None)
            last = x2
        ops.ablation_head(None, last, self.model.batch_norm, self.model.out, self.lists, None, i, n_pos, cols, n_cols,
                          removed, self.base, M, self.d)


def label_pair_ablation(model, x_f: torch.Tensor, x_r: torch.Tensor, adj, targets: torch.Tensor, rows=None, cols=None,
                        route: str = "auto", max_workspace_bytes: int = 256 << 20, return_base: bool = False):
    """M [C, C] float32 on the device: M[i, j] = (base_i - abl_ij) / base_i for i in rows, j in cols (scripts/visualize.py:
    79-119 generalised; the reference's own call is rows = cols = range(10, 80)).
    model: eval-mode chromegcn_amd.ChromeGCN (d in {128, 256}); x_f, x_r: [n, d]; adj: what as_graph accepts (not None);
    targets: [n, C], nonzero = positive.  route: "auto" (restricted for L <= 2, else composed), "restricted" or "composed".
    max_workspace_bytes caps the restricted route's instance buffers (column labels are batched under it).
    return_base: also return base [C] (NaN for a label without positives)."""
    if model.training:
        raise RuntimeError("label_pair_ablation needs an eval-mode model (model.eval()): dropout and batch statistics would "
                           "make every entry random and non-local")
    if adj is None:
        raise ValueError("label_pair_ablation needs the chromosome's graph (adj=None has no edges to ablate)")
    if route not in ROUTES:
        raise ValueError("route must be one of %s, got %r" % (ROUTES, route))
    L = model.n_layers
    if route == "auto":
        route = "restricted" if L <= 2 else "composed"
    if route == "restricted" and L > 2:
        raise ValueError("route='restricted' covers models of at most 2 layers (this one has %d); use 'composed'" % L)
    ops._require_cuda(x_f, "x_f")
    ops._require_cuda(x_r, "x_r")
    n, d = x_f.shape
    C = model.out.weight.shape[0]
    if ops.ablation_workspace_bytes(1, _S, d, min(L, 2)) == 0:
        raise RuntimeError("chromegcn_amd: label_pair_ablation: unsupported shape (d = %d; the library supports 128 and 256)" % d)
    dev = x_f.device
    x = ops._dense(torch.stack([x_f.detach(), x_r.detach()]))
    graph = as_graph(adj, dev)
    if graph.n != n:
        raise ValueError("the graph has %d nodes but the features %d" % (graph.n, n))
    if tuple(targets.shape) != (n, C):
        raise ValueError("targets must be [n, C] = [%d, %d], got %s" % (n, C, tuple(targets.shape)))
    rows, cols = _labels(rows, C, "row"), _labels(cols, C, "column")
    with torch.no_grad():
        tg = (targets.to(dev) != 0).to(torch.float32).contiguous()
        bits, lists, ranks, counts_d = ops.ablation_prepare(tg)
        counts = counts_d.cpu().tolist()                              # the call's one host synchronisation
        M = torch.zeros((C, C), device=dev, dtype=torch.float32)
        work, nan_idx = [], []
        for i in rows:
            js = [j for j in cols if j != i and counts[j] > 0]
            if not js:
                continue
            if counts[i] == 0:
                nan_idx += [i * C + j for j in js]
            else:
                work.append((i, js))
        if nan_idx:
            M.view(-1)[torch.tensor(nan_idx, dtype=torch.int64).to(dev)] = float("nan")
        if route == "restricted":
            base = _run_restricted(model, x, graph, bits, lists, ranks, counts_d, counts, work, M, max_workspace_bytes)
        else:
            base = _run_composed(model, x, graph, bits, lists, counts_d, work, M)
    return (M, base) if return_base else M


def _run_restricted(model, x, graph, bits, lists, ranks, counts_d, counts, work, M, cap):
    ra = RestrictedAblation(model, x, graph, bits, lists, ranks, counts_d)
    if not work:
        return ra.base
    per_inst = ra.S * ra.d * 4 * ra.L + 4
    max_pos = max(counts[i] for i, _ in work)
    inst_cap = max(max_pos, int(cap) // per_inst)
    batches = [min(len(js), max(1, inst_cap // counts[i])) for i, js in work]
    n_inst = max(b * counts[i] for b, (i, _) in zip(batches, work))
    ws = ra.workspace(n_inst)
    width = max(len(js) for _, js in work)
    table = torch.full((len(work), width), -1, dtype=torch.int32)
    for r, (_, js) in enumerate(work):
        table[r, :len(js)] = torch.tensor(js, dtype=torch.int32)
    table = table.to(x.device)                                         # every row label's column labels, one upload
    for r, ((i, js), nb) in enumerate(zip(work, batches)):
        for s in range(0, len(js), nb):
            k = min(nb, len(js) - s)
            ra.run_row(i, counts[i], table[r, s:s + k], k, ws, M)
    return ra.base


def _run_composed(model, x, graph, bits, lists, counts_d, work, M):
    C = M.shape[0]
    base = torch.empty(C, device=x.device, dtype=torch.float32)
    logits = model._head(_eval_stack(model, x, graph)[-1]).contiguous()
    ops.ablation_reduce(logits, lists, counts_d, -1, 0, None, base, None)
    if not work:
        return base
    val = torch.empty(max(graph.nnz, 1), device=x.device, dtype=torch.float32)[:graph.nnz]
    rs = torch.empty(graph.n, device=x.device, dtype=torch.float32)
    removed = torch.zeros(1, device=x.device, dtype=torch.int32)
    mg = G.masked_graph(graph, val, rs)
    for i, js in work:
        for j in js:
            ops.ablation_mask(graph, bits, C, i, j, val, rs, removed)
            logits = model._head(_eval_stack(model, x, mg)[-1]).contiguous()
            ops.ablation_reduce(logits, lists, counts_d, i, j, removed, base, M)
    return base
