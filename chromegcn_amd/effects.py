"""Window effects through the Hi-C graph: how the predictions change, at a window and at its 3D contacts, when the
features of that one window change (a variant's alternative allele, or a knock-out by a neutral feature).

M independent variants; variant m replaces row u = windows[m] of x_f and x_r by alt_f[m], alt_r[m]:
    ref = sigmoid((logits_f + logits_r) / 2) on x,   alt = the same on x with row u replaced,   effect = alt - ref,
with the model in eval mode (running BatchNorm statistics, no dropout).  Reported for the variant's INSTANCES, in this order:
instance 0 is u itself; after it every v != u with a stored entry A[v, u], in the stored order of row u of the transpose
(ChromGraph.rowptr_t / col_t / val_t -- the graph's own arrays when it is symmetric, which every builder's output is).  A self
loop does not repeat u and a graph without a stored diagonal still reports u.

Those are exactly the rows layer 1 changes.  For L >= 2 layers, windows two or more hops away change as well;
scope="contacts" does NOT report them (a full forward per variant does: window_effects_host).

  * restricted route (L <= 2, d in {128, 256}; what "auto" picks there): the unperturbed forward runs once and keeps every
    layer's input X^k and aggregation H^k; an instance's new aggregate is H_v + w_vu (x'_u - x_u), one fused multiply-add per
    element and no gather (cgcn_effects_rows1; layer 2: cgcn_effects_rows2), the dense gated part is cgcn_layer_fwd's
    row-local route on the instance table, the head cgcn_head_logits.  About deg(u) row instances per layer instead of n.
  * composed route (any L; the definition on the device and the cross-check): per variant, row u overwritten in a copy of
    the stacked features, the library's eval forward, the rows gathered, the row restored.

`ref` comes from the unperturbed forward and, on the restricted route, `alt` from the instance path: alt_f[m] == x_f[u] gives
an alt that equals ref within rounding, not bit for bit, and entries of alt - ref below the tolerance
are noise."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np
import scipy.sparse as sp
import torch

from . import graph as G
from . import ops
from .ablation import _align, _eval_stack
from .graph import ChromGraph, HostCSR, as_graph

ROUTES = ("auto", "restricted", "composed")
SCOPES = ("own", "contacts")
_S = 2   # both strands


@dataclass
class WindowEffects:
    """offsets int64 [M + 1]; rows int32 [total] (the window of every reported row); ref, alt float32 [total, C].
    we[m] -> (rows, ref, alt) of variant m.  Device tensors from window_effects, numpy arrays (float64) from
    window_effects_host."""
    offsets: object
    rows: object
    ref: object
    alt: object

    def __len__(self):
        return int(self.offsets.shape[0]) - 1

    def __getitem__(self, m):
        if not -len(self) <= m < len(self):
            raise IndexError("variant %d of %d" % (m, len(self)))
        m %= len(self)
        a, b = int(self.offsets[m]), int(self.offsets[m + 1])
        return self.rows[a:b], self.ref[a:b], self.alt[a:b]


# ---- the definition on the host, float64 --------------------------------------------------------------------------------
def _host_csr(graph) -> HostCSR:
    if isinstance(graph, HostCSR):
        return graph
    if isinstance(graph, ChromGraph):
        return G.to_host(graph)
    if isinstance(graph, torch.Tensor) and graph.layout == torch.sparse_coo:
        a = graph.detach().cpu().coalesce()
        i = a.indices().numpy()
        return G.host_csr_from_matrix(sp.coo_matrix((a.values().numpy(), (i[0], i[1])), shape=tuple(a.shape)).tocsr())
    if sp.issparse(graph):
        return G.host_csr_from_matrix(graph)
    raise TypeError("graph must be a HostCSR, a ChromGraph, a torch sparse COO tensor or a scipy matrix, got %r" % type(graph))


def _host_transpose(h: HostCSR):
    """(rowptr_t, col_t) of the stored pattern's transpose, sorted rows (the graph's own arrays when it is symmetric)"""
    if h.symmetric:
        return np.asarray(h.rowptr, np.int64), np.asarray(h.col, np.int64)
    at = sp.csr_matrix((np.arange(1, h.nnz + 1, dtype=np.float64), h.col, h.rowptr), shape=(h.n, h.n)).T.tocsr()
    at.sort_indices()
    return at.indptr.astype(np.int64), at.indices.astype(np.int64)


def _windows_host(windows, n: int) -> np.ndarray:
    """windows as a checked int64 numpy vector (ValueError: not integers, not a vector, outside [0, n))"""
    if isinstance(windows, torch.Tensor):
        windows = windows.detach().cpu().numpy()
    w = np.asarray(windows)
    if w.ndim != 1:
        raise ValueError("windows must be a vector, got shape %s" % (tuple(w.shape),))
    if w.size and w.dtype.kind not in "iu":
        raise ValueError("windows must hold integers, got dtype %s" % w.dtype)
    w = w.astype(np.int64)
    if w.size and (int(w.min()) < 0 or int(w.max()) >= n):
        raise ValueError("windows must lie in [0, %d), got %d .. %d" % (n, int(w.min()), int(w.max())))
    return w


def effect_rows_host(graph, windows):
    """(offsets int64 [M + 1], rows int32 [total]): the instance enumeration of every variant -- u first, then every v != u
    with a stored A[v, u] in the stored order of row u of the transpose."""
    h = _host_csr(graph)
    rp, ct = _host_transpose(h)
    out, offsets = [], [0]
    for u in _windows_host(windows, h.n):
        nb = ct[rp[u]:rp[u + 1]]
        out.append(np.concatenate([[u], nb[nb != u]]))
        offsets.append(offsets[-1] + out[-1].shape[0])
    rows = np.concatenate(out).astype(np.int32) if out else np.zeros(0, np.int32)
    return np.asarray(offsets, np.int64), rows


def _params64(model):
    def a(t):
        return t.detach().double().cpu().numpy()
    layers = []
    for k in range(1, model.n_layers + 1):
        gc, wk = getattr(model, "GC%d" % k), getattr(model, "W%d" % k)
        layers.append((a(gc.weight), a(gc.bias), a(wk.weight).reshape(-1), float(wk.bias.detach().double().item())))
    bn, out = model.batch_norm, model.out
    return layers, (a(bn.weight), a(bn.bias), a(bn.running_mean), a(bn.running_var), float(bn.eps), a(out.weight), a(out.bias))


def _sigmoid64(x):
    return 1.0 / (1.0 + np.exp(-x))


def _forward64(params, A, x):
    """eval logits [n, C] of one strand in float64 (models/ChromeModels.py:37-51 with running statistics)"""
    layers, (bw, bb, mu, var, eps, wo, bo) = params
    for W, b, wg, cg in layers:
        z = np.tanh(A @ (x @ W) + b)
        g = _sigmoid64(z @ wg + cg)[:, None]
        x = (1.0 - g) * x + g * z
    y = (np.maximum(x, 0.0) - mu) / np.sqrt(var + eps) * bw + bb
    return y @ wo.T + bo


def _prob64(params, A, x_f, x_r):
    return _sigmoid64((_forward64(params, A, x_f) + _forward64(params, A, x_r)) / 2.0)


def _matrix64(h: HostCSR):
    a = h.ahat().astype(np.float64)
    return sp.csr_matrix(sp.diags(h.row_scale.astype(np.float64)) @ a) if h.row_scale is not None else sp.csr_matrix(a)


def _np64(t):
    return t.detach().double().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, np.float64)


def window_effects_host(model, x_f, x_r, adj, windows, alt_f, alt_r, scope: str = "own") -> WindowEffects:
    """The definition in float64 numpy: one whole eval forward per variant, nothing restricted.  model: anything with the
    reference's parameter names (ChromeGCN, the oracle); adj: what effect_rows_host accepts, taken with the float32 values
    and row scales the kernels get.  Returns a WindowEffects of numpy arrays (ref, alt float64)."""
    if scope not in SCOPES:
        raise ValueError("scope must be one of %s, got %r" % (SCOPES, scope))
    h = _host_csr(adj)
    x_f, x_r, alt_f, alt_r = map(_np64, (x_f, x_r, alt_f, alt_r))
    win = _windows_host(windows, h.n)
    params, A = _params64(model), _matrix64(h)
    base = _prob64(params, A, x_f, x_r)
    offsets, rows = effect_rows_host(h, win)
    if scope == "own":
        offsets, rows = np.arange(win.shape[0] + 1, dtype=np.int64), win.astype(np.int32)
    ref, alt = base[rows], np.empty((rows.shape[0], base.shape[1]))
    for m, u in enumerate(win):
        xf, xr = x_f.copy(), x_r.copy()
        xf[u], xr[u] = alt_f[m], alt_r[m]
        alt[offsets[m]:offsets[m + 1]] = _prob64(params, A, xf, xr)[rows[offsets[m]:offsets[m + 1]]]
    return WindowEffects(offsets, rows, ref, alt)


def _entry_positions(rp, ct, offsets, rows, windows):
    """for every instance its position in (rowptr_t, col_t), or -1 (instance 0 without a stored diagonal) -- host arrays"""
    pos = np.full(rows.shape[0], -1, np.int64)
    for m, u in enumerate(windows):
        seg = ct[rp[u]:rp[u + 1]]
        for k in range(offsets[m], offsets[m + 1]):
            j = np.flatnonzero(seg == rows[k])
            if j.size:
                pos[k] = rp[u] + j[0]
    return pos


def knockout_map_host(model, x_f, x_r, adj, fill=None, labels=None):
    """float64 [nnz_t] aligned with (rowptr_t, col_t): the entry of stored A[v, u] is sum over `labels` of |alt(v, c) -
    ref(v, c)| when window u alone is replaced by fill ([2, d]; default: the per-strand column mean of the features)."""
    h = _host_csr(adj)
    x_f, x_r = _np64(x_f), _np64(x_r)
    fill = np.stack([x_f.mean(0), x_r.mean(0)]) if fill is None else _np64(fill)
    win = np.arange(h.n)
    we = window_effects_host(model, x_f, x_r, h, win, np.broadcast_to(fill[0], x_f.shape), np.broadcast_to(fill[1], x_r.shape),
                             scope="contacts")
    rp, ct = _host_transpose(h)
    d = np.abs(we.alt - we.ref)
    s = (d if labels is None else d[:, list(labels)]).sum(1)
    pos = _entry_positions(rp, ct, we.offsets, we.rows, win)
    out = np.zeros(ct.shape[0])
    out[pos[pos >= 0]] = s[pos >= 0]
    return out


# ---- the device routes ------------------------------------------------------------------------------------------------------
def _prob(logits):
    return torch.sigmoid((logits[0] + logits[1]) * 0.5)


def _plan_torch(graph: ChromGraph):
    """diag_rel int64 [n]: the position of the stored (u, u) inside row u of the transpose, -1 without one -- torch
    operators only, no host synchronisation (the composed route and the knock-out map's scatter)"""
    n, dev = graph.n, graph.rowptr_t.device
    rp = graph.rowptr_t.to(torch.int64)
    nnz = int(graph.col_t.numel())
    diag = torch.full((n,), -1, dtype=torch.int64, device=dev)
    if nnz:
        row_of = torch.repeat_interleave(torch.arange(n, device=dev), rp[1:] - rp[:-1], output_size=nnz)
        rel = torch.arange(nnz, device=dev) - rp[row_of]
        rel = torch.where(graph.col_t.to(torch.int64) == row_of, rel, torch.full_like(rel, -1))
        diag = diag.scatter_reduce(0, row_of, rel, "amax", include_self=True)
    return diag


def _instances_torch(graph: ChromGraph, diag_rel, windows, offsets, total):
    """(variant, instance number, window, position in (rowptr_t, col_t) or -1) of every instance, int64 [total] each"""
    dev = windows.device
    M = int(windows.numel())
    counts = offsets[1:] - offsets[:-1]
    var = torch.repeat_interleave(torch.arange(M, device=dev), counts, output_size=total)
    k = torch.arange(total, device=dev) - offsets[var]
    u = windows.to(torch.int64)[var]
    dp = diag_rel[u]
    j = torch.where(k == 0, dp, k - 1 + ((dp >= 0) & (k - 1 >= dp)).to(torch.int64))
    pos = torch.where(j >= 0, graph.rowptr_t.to(torch.int64)[u] + j, torch.full_like(j, -1))
    v = torch.where(k == 0, u, graph.col_t.to(torch.int64)[pos.clamp(min=0)]) if graph.col_t.numel() else u
    return var, k, v, pos


class _Baseline:
    """The unperturbed eval forward of one model, chromosome and feature pair: layer inputs xs [X^0 .. X^L], with keep_h the
    aggregations hs [H^1 .. H^L] too, and prob [n, C] = ref of every window."""

    def __init__(self, model, x, graph: ChromGraph, keep_h: bool):
        self.model, self.graph, self.x = model, graph, x
        self.S, self.n, self.d = x.shape
        self.L = model.n_layers
        self.C = model.out.weight.shape[0]
        self.params, self.hs = [], []
        if keep_h:
            self.xs = [x]
            for k in range(1, self.L + 1):
                gc, wk = getattr(model, "GC%d" % k), getattr(model, "W%d" % k)
                p = ops._layer_params(gc.weight.detach(), gc.bias.detach(), wk.weight.detach(), wk.bias.detach())
                h = torch.empty_like(x)
                xn, _ = ops.layer_fwd(self.xs[-1], p, (graph.rowptr, graph.col, graph.val, graph.row_scale), None, h)
                self.params.append(p)
                self.hs.append(h)
                self.xs.append(xn)
        else:
            self.xs = _eval_stack(model, x, graph)
        self.prob = _prob(model._head(self.xs[-1]))


def _batches(cost, cap):
    """consecutive variants in batches whose summed cost stays under cap; one variant above the cap gets a batch to itself"""
    out, m0, acc = [], 0, 0
    for m, c in enumerate(cost):
        if m > m0 and acc + c > cap:
            out.append((m0, m, acc))
            m0, acc = m, 0
        acc += c
    if len(cost) > m0:
        out.append((m0, len(cost), acc))
    return out


def _run_restricted(base: _Baseline, win_d, alt, scope, cap) -> WindowEffects:
    g, model, S, d, L, C = base.graph, base.model, base.S, base.d, base.L, base.C
    dev = alt.device
    M = int(win_d.numel())
    own = scope == "own"
    counts, diag = ops.effects_plan(g, win_d)
    offsets = torch.zeros(M + 1, dtype=torch.int64, device=dev)
    offsets[1:] = torch.cumsum(counts, 0)
    off_h = offsets.cpu().numpy()                                      # the call's one host synchronisation
    total = M if own else int(off_h[-1])
    l1_own = own and L == 1                                            # layer 1 is the read-out: instance 0 alone
    rows = win_d.clone() if own else torch.empty(max(total, 1), dtype=torch.int32, device=dev)[:total]
    alt_out = torch.empty((total, C), dtype=torch.float32, device=dev)
    cost = [1] * M if l1_own else np.diff(off_h).tolist()
    per_inst = S * d * 4 * (2 + L) + S * 4
    hard = min((1 << 32) // (S * d * 4) - 1, 1 << 28)                  # rows of one feature table (cgcn_layer_fwd's limit)
    batches = _batches(cost, max(1, min(int(cap) // per_inst, hard)))
    n_max = max((b[2] for b in batches), default=0)
    nbytes = ops.effects_workspace_bytes(n_max, S, d, L)
    if nbytes == 0:
        raise RuntimeError("chromegcn_amd: window_effects: unsupported shape (S=%d, d=%d, L=%d, %d instances)" % (S, d, L, n_max))
    ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    fb = _align(n_max * S * d * 4)

    def table(part, r):
        return ws[part * fb:part * fb + 4 * S * r * d].view(torch.float32).view(S, r, d)

    def gate(r):
        return ws[(2 + L) * fb:(2 + L) * fb + 4 * S * r].view(torch.float32).view(S, r)

    for m0, m1, ni in batches:
        nv = m1 - m0
        o0 = m0 if own else int(off_h[m0])
        hi, xi, x1 = table(0, ni), table(1, ni), table(2, ni)
        ops.effects_rows1(g, base.xs[0], base.hs[0], win_d[m0:], alt[m0:], offsets[m0:], diag[m0:], nv, l1_own, ni, hi, xi,
                          None if own else rows[o0:])
        ops.layer_dense_rows(hi, xi, base.params[0], g, x1, gate(ni))
        last = x1
        if L == 2:
            no = nv if own else ni
            ho, xr, x2 = table(0, no), (table(1, no) if own else None), table(3, no)
            ops.effects_rows2(g, base.xs[1], base.hs[1], win_d[m0:], offsets[m0:], diag[m0:], nv, own, ni, x1, ho, xr)
            ops.layer_dense_rows(ho, xr if own else x1, base.params[1], g, x2, gate(no))
            last = x2
        alt_out[o0:o0 + last.shape[1]] = _prob(model._head(last))
    ref = base.prob.index_select(0, rows.to(torch.int64))
    return WindowEffects(torch.arange(M + 1, device=dev) if own else offsets, rows, ref, alt_out)


def _run_composed(base: _Baseline, win_h, win_d, alt, scope) -> WindowEffects:
    g, model, C = base.graph, base.model, base.C
    dev = alt.device
    M = int(win_d.numel())
    if scope == "own":
        off_h = np.arange(M + 1, dtype=np.int64)
        offsets, rows = torch.arange(M + 1, device=dev), win_d.clone()
    else:
        diag_rel = _plan_torch(g)
        rp = g.rowptr_t.to(torch.int64)
        u = win_d.to(torch.int64)
        counts = rp[u + 1] - rp[u] + (diag_rel[u] < 0).to(torch.int64)
        offsets = torch.zeros(M + 1, dtype=torch.int64, device=dev)
        offsets[1:] = torch.cumsum(counts, 0)
        off_h = offsets.cpu().numpy()                                  # the call's one host synchronisation
        rows = _instances_torch(g, diag_rel, win_d, offsets, int(off_h[-1]))[2].to(torch.int32)
    total = int(off_h[-1])
    rows64 = rows.to(torch.int64)
    alt_out = torch.empty((total, C), dtype=torch.float32, device=dev)
    xc = base.x.clone()
    for m in range(M):
        u, a, b = int(win_h[m]), int(off_h[m]), int(off_h[m + 1])
        xc[:, u] = alt[m]
        p = _prob(model._head(_eval_stack(model, xc, g)[-1]))
        alt_out[a:b] = p.index_select(0, rows64[a:b])
        xc[:, u] = base.x[:, u]
    return WindowEffects(offsets, rows, base.prob.index_select(0, rows64), alt_out)


def _check_call(model, x_f, x_r, adj, scope, route, what, variants=None):
    if model.training:
        raise RuntimeError("%s needs an eval-mode model (model.eval()): dropout and batch statistics would make every "
                           "effect random and non-local" % what)
    if adj is None:
        raise ValueError("%s needs the chromosome's graph (adj=None has no contacts)" % what)
    if scope not in SCOPES:
        raise ValueError("scope must be one of %s, got %r" % (SCOPES, scope))
    if route not in ROUTES:
        raise ValueError("route must be one of %s, got %r" % (ROUTES, route))
    L = model.n_layers
    if route == "auto":
        route = "restricted" if L <= 2 else "composed"
    if route == "restricted" and L > 2:
        raise ValueError("route='restricted' covers models of at most 2 layers (this one has %d); use 'composed'" % L)
    if x_f.dim() != 2 or x_f.shape != x_r.shape:
        raise ValueError("x_f and x_r must both be [n, d], got %s and %s" % (tuple(x_f.shape), tuple(x_r.shape)))
    win_h = None
    if variants is not None:
        windows, alt_f, alt_r = variants
        n, d = x_f.shape
        win_h = _windows_host(windows, n)
        M = win_h.shape[0]
        if tuple(alt_f.shape) != (M, d) or tuple(alt_r.shape) != (M, d):
            raise ValueError("alt_f and alt_r must be [M, d] = [%d, %d], got %s and %s"
                             % (M, d, tuple(alt_f.shape), tuple(alt_r.shape)))
    graph = as_graph(adj, x_f.device)
    if graph.n != x_f.shape[0]:
        raise ValueError("the graph has %d nodes but the features %d" % (graph.n, x_f.shape[0]))
    return route, graph, win_h


def _baseline(model, x_f, x_r, graph, route, what):
    ops._require_cuda(x_f, "x_f")
    ops._require_cuda(x_r, "x_r")
    d = x_f.shape[1]
    if route == "restricted" and ops.effects_workspace_bytes(1, _S, d, min(model.n_layers, 2)) == 0:
        raise RuntimeError("chromegcn_amd: %s: unsupported shape (d = %d; the restricted route supports 128 and 256)" % (what, d))
    x = ops._dense(torch.stack([x_f.detach(), x_r.detach()]))
    return _Baseline(model, x, graph, keep_h=route == "restricted")


def _effects(base, route, win_h, alt, scope, cap):
    if win_h.shape[0] == 0:
        e = torch.empty((0, base.C), dtype=torch.float32, device=alt.device)
        return WindowEffects(torch.zeros(1, dtype=torch.int64, device=alt.device),
                             torch.empty(0, dtype=torch.int32, device=alt.device), e, e.clone())
    win_d = torch.from_numpy(win_h.astype(np.int32)).to(alt.device)
    if route == "restricted":
        return _run_restricted(base, win_d, alt, scope, cap)
    return _run_composed(base, win_h, win_d, alt, scope)


def window_effects(model, x_f: torch.Tensor, x_r: torch.Tensor, adj, windows, alt_f: torch.Tensor, alt_r: torch.Tensor,
                   scope: str = "own", route: str = "auto", max_workspace_bytes: int = 256 << 20) -> WindowEffects:
    """ref and alt probabilities of M independent single-window replacements (module docstring), as a WindowEffects on the
    device: offsets int64 [M + 1], rows int32 [total], ref / alt float32 [total, C].
    model: eval-mode chromegcn_amd.ChromeGCN; x_f, x_r: [n, d]; adj: what as_graph accepts (not None); windows: M integers in
    [0, n) on the host (a list, a numpy array or a CPU tensor; a device tensor is copied to the host first); alt_f, alt_r:
    [M, d], the replacement rows of the two strands.
    scope: "own" reports instance 0 (window u) alone, total = M; "contacts" reports every instance: u, then the windows v
    with a stored A[v, u].  With two or more layers, windows two or more hops from u change as well: they are NOT reported.
    route: "restricted" (L <= 2, d in {128, 256}; "auto" picks it there), "composed" (any L; a whole forward per variant).
    max_workspace_bytes caps the restricted route's instance buffers: variants are processed in batches under it; a variant
    is never split, one larger than the cap gets a batch to itself.  One host synchronisation per call (the instance total).
    ref is the unperturbed forward's; on the restricted route alt comes from the instance path, so alt_f[m] == x_f[u] gives
    alt == ref within rounding only."""
    route, graph, win_h = _check_call(model, x_f, x_r, adj, scope, route, "window_effects", (windows, alt_f, alt_r))
    ops._require_cuda(alt_f, "alt_f")
    ops._require_cuda(alt_r, "alt_r")
    with torch.no_grad():
        base = _baseline(model, x_f, x_r, graph, route, "window_effects")
        alt = ops._dense(torch.stack([alt_f.detach(), alt_r.detach()], 1))       # [M, S, d]
        return _effects(base, route, win_h, alt, scope, max_workspace_bytes)


def knockout_map(model, x_f: torch.Tensor, x_r: torch.Tensor, adj, fill: Optional[torch.Tensor] = None, labels=None,
                 route: str = "auto", max_workspace_bytes: int = 256 << 20) -> torch.Tensor:
    """float32 [nnz_t] on the device, aligned with (rowptr_t, col_t) of the graph: the entry of stored A[v, u] is
    sum over `labels` (default: all) of |alt(v, c) - ref(v, c)| when window u alone is replaced by fill -- the
    finite-difference counterpart of the adjacency saliency, on the same pattern.  fill: [2, d] (forward, reverse); default
    the per-strand column mean of the features.  Every window in turn goes through window_effects(scope="contacts"), in
    batches of windows whose reported rows (ref and alt) stay under max_workspace_bytes, which also caps the instance
    buffers; the sums are torch operators.  route: as in window_effects ("composed": a whole forward per window, any L)."""
    route, graph, _ = _check_call(model, x_f, x_r, adj, "contacts", route, "knockout_map")
    n, d = x_f.shape
    C = model.out.weight.shape[0]
    if fill is not None and tuple(fill.shape) != (_S, d):
        raise ValueError("fill must be [2, d] = [2, %d], got %s" % (d, tuple(fill.shape)))
    sel = None
    if labels is not None:
        sel = [int(c) for c in labels]
        if any(not 0 <= c < C for c in sel):
            raise ValueError("labels must lie in [0, %d)" % C)
    with torch.no_grad():
        base = _baseline(model, x_f, x_r, graph, route, "knockout_map")
        dev = base.x.device
        fill = base.x.mean(1) if fill is None else fill.detach().to(dev, torch.float32)
        nnz = int(graph.col_t.numel())
        diag_rel = _plan_torch(graph)
        deg = (graph.rowptr_t[1:] - graph.rowptr_t[:-1]).cpu().numpy().astype(np.int64)
        out = torch.zeros(nnz + 1, dtype=torch.float32, device=dev)             # (slot nnz takes instance 0 without a diagonal)
        sel_d = None if sel is None else torch.tensor(sel, dtype=torch.int64, device=dev)
        for m0, m1, _ in _batches(((deg + 1) * (C * 8)).tolist(), max(1, int(max_workspace_bytes))):
            win_h = np.arange(m0, m1, dtype=np.int64)
            alt = fill.unsqueeze(0).expand(m1 - m0, _S, d).contiguous()
            we = _effects(base, route, win_h, alt, "contacts", max_workspace_bytes)
            dlt = (we.alt - we.ref).abs_()
            s = (dlt if sel_d is None else dlt.index_select(1, sel_d)).sum(1)
            win_d = torch.from_numpy(win_h.astype(np.int32)).to(dev)
            pos = _instances_torch(graph, diag_rel, win_d, we.offsets, int(s.numel()))[3]
            out.index_copy_(0, torch.where(pos >= 0, pos, torch.full_like(pos, nnz)), s)
    return out[:nnz]
