"""The label-pair Hi-C edge ablation of scripts/visualize.py:79-119 restated on the host, and the graphs, targets and models
that tests/test_ablation_ref_host.py and tests/test_gpu_ablation_cases.py share.  Three levels, all float64 and none near a GPU:

  * the dense method as the reference writes it (reference_matrix: a dense adjacency per pair, masked_fill, row sums with
    0 -> 1, two whole forwards);
  * one restatement per cgcn_ablation_* entry point, written from the contracts in include/chromegcn.h (prepare_ref,
    layer_ref, head_ref, mask_ref, reduce_ref);
  * restricted_matrix_ref, the whole M composed from those pieces: it recomputes the rows of P_i only, so C = 103 labels at
    n = 300 take seconds.

The contracts leave a row that loses nothing as it is (its row scale, or 1 without one), the dense method divides EVERY row
by its sum.  The two are the same operation where the rows of A sum to 1, so the host test compares them on graphs normalised
in float64 (graph_arrays(..., exact=True)); the kernels get the float32 graph and are held to the pieces."""
import functools
from collections import namedtuple

import numpy as np
import scipy.sparse as sp
import torch

import saliency_ref as S
from chromegcn_amd import graph as G
from oracle import chromegcn_oracle as O


# ---- the dense method ------------------------------------------------------------------------------------------------------
def _dense_forward(orc, adj, x):
    h = x
    for k in range(1, orc.n_layers + 1):
        gc, wk = getattr(orc, "GC%d" % k), getattr(orc, "W%d" % k)
        z = torch.tanh(adj @ (h @ gc.weight) + gc.bias)
        g = torch.sigmoid(wk(z))
        h = (1 - g) * h + g * z
    return orc.out(orc.batch_norm(torch.relu(h)))


def reference_matrix(orc, adj, x_f, x_r, targets, rows=None, cols=None):
    """scripts/visualize.py:79-119 restated in float64 (adj: the dense normalised adjacency)"""
    c = targets.shape[1]
    rows = range(c) if rows is None else rows
    cols = range(c) if cols is None else cols
    x_f, x_r = x_f.double(), x_r.double()
    with torch.no_grad():
        pred = (_dense_forward(orc, adj, x_f) + _dense_forward(orc, adj, x_r)) / 2
        mat = torch.zeros(c, c, dtype=torch.float64)
        zero_mat = torch.zeros(adj.shape, dtype=torch.bool)
        for i in rows:
            pi = targets[:, i].nonzero().view(-1)
            base = pred[pi, i].sigmoid().mean()
            pi_mat = zero_mat.index_fill(0, pi, True)
            for j in cols:
                pj = targets[:, j].nonzero().view(-1)
                if len(pj) > 0 and i != j:
                    adj2 = adj.masked_fill(pi_mat & zero_mat.index_fill(1, pj, True), 0)
                    s = adj2.sum(1).view(-1, 1)
                    s[s == 0] = 1
                    adj2 = adj2 / s
                    p = (_dense_forward(orc, adj2, x_f) + _dense_forward(orc, adj2, x_r)) / 2
                    mat[i, j] = (base - p[pi, i].sigmoid().mean()) / base
    return mat.numpy()


def _dense_adj(adj_type, a, n):
    return torch.from_numpy(O.normalized_adjacency(adj_type, a, n).toarray()).double()


# ---- graphs and models as plain arrays ---------------------------------------------------------------------------------------
Graph = namedtuple("Graph", "rowptr col val row_scale")        # A = diag(row_scale or 1) * (val or 1 on the pattern)
Prep = namedtuple("Prep", "bits lists ranks counts")
LayerParams = namedtuple("LayerParams", "W b wg cg")           # U = H W + b, g = sigmoid(Z . wg + cg)
HeadParams = namedtuple("HeadParams", "bn_w bn_b mean var eps W_out b_out")


def graph_arrays(h, exact=False):
    """A HostCSR as a Graph of float64 arrays.  exact=False: the float32 values and row scales the kernels get.  exact=True:
    the same operator normalised in float64 (row scale 1 / row sum; without a row scale the values divided by the row sum),
    whose rows sum to 1 within an ulp -- the form on which the contracts and the dense method are the same operation."""
    rowptr, col = np.asarray(h.rowptr, np.int64), np.asarray(h.col, np.int64)
    val = None if h.val is None else np.asarray(h.val, np.float64)
    rs = None if h.row_scale is None else np.asarray(h.row_scale, np.float64)
    if exact:
        rows = S.rows_of(rowptr)
        rowsum = np.bincount(rows, weights=np.ones(col.shape[0]) if val is None else val, minlength=h.n)
        inv = np.where(rowsum != 0, 1.0 / np.where(rowsum != 0, rowsum, 1.0), 0.0)
        if rs is not None:
            rs = inv
        else:
            val = val * np.where(rowsum != 0, inv, 1.0)[rows]
    return Graph(rowptr, col, val, rs)


def dense_of(g):
    """the dense float64 adjacency of a Graph, as a torch tensor"""
    n = g.rowptr.shape[0] - 1
    a = sp.csr_matrix((np.ones(g.col.shape[0]) if g.val is None else g.val, g.col, g.rowptr), shape=(n, n)).toarray()
    if g.row_scale is not None:
        a = a * g.row_scale[:, None]
    return torch.from_numpy(a)


def model_params(orc):
    """([LayerParams per layer], HeadParams) of an oracle model, float64"""
    def a(t):
        return t.detach().double().numpy().copy()
    layers = []
    for k in range(1, orc.n_layers + 1):
        gc, wk = getattr(orc, "GC%d" % k), getattr(orc, "W%d" % k)
        layers.append(LayerParams(a(gc.weight), a(gc.bias), a(wk.weight).reshape(-1), float(wk.bias.item())))
    bn = orc.batch_norm
    return layers, HeadParams(a(bn.weight), a(bn.bias), a(bn.running_mean), a(bn.running_var), float(bn.eps),
                              a(orc.out.weight), a(orc.out.bias))


def _sigmoid(x):
    one = np.ones((), x.dtype)
    return one / (one + np.exp(-x))


# ---- cgcn_ablation_prepare -------------------------------------------------------------------------------------------------
def positives(targets):
    """bool [n, C]: targets != 0 (so -0.0 is negative, NaN and a denormal positive)"""
    return np.asarray(targets) != 0


def prepare_ref(targets):
    """label_bits uint32 [n][(C + 31) / 32], pos_lists int32 [C][n] (ascending, -1 past the count), pos_ranks int32 [C][n]
    (-1 outside P_c) and pos_counts int32 [C]"""
    pos = positives(targets)
    n, C = pos.shape
    bits = np.zeros((n, (C + 31) // 32), np.uint32)
    lists, ranks = np.full((C, n), -1, np.int32), np.full((C, n), -1, np.int32)
    counts = np.zeros(C, np.int32)
    for c in range(C):
        bits[:, c >> 5] |= pos[:, c].astype(np.uint32) << np.uint32(c & 31)
        p = np.flatnonzero(pos[:, c])
        counts[c] = p.size
        lists[c, :p.size] = p
        ranks[c, p] = np.arange(p.size)
    return Prep(bits, lists, ranks, counts)


# ---- the gated layer: whole, and for the instances of one row label -------------------------------------------------------
def _gated(H, xin, p):
    Z = np.tanh(H @ p.W + p.b)
    g = _sigmoid(Z @ p.wg + p.cg)[..., None]
    return (1 - g) * xin + g * Z


def full_layer_ref(g, X, p):
    """one unablated gated layer, X [S, n, d] -> [S, n, d]"""
    n = g.rowptr.shape[0] - 1
    A = sp.csr_matrix((np.ones(g.col.shape[0]) if g.val is None else g.val, g.col, g.rowptr), shape=(n, n))
    H = np.stack([A @ X[s] for s in range(X.shape[0])])
    if g.row_scale is not None:
        H = H * g.row_scale[None, :, None]
    return _gated(H, X, p)


def layer_ref(g, X, p, pos, pos_list, cols, X_inst=None, dtype=np.float64):
    """cgcn_ablation_layer: the instances (b, k) of the rows u = pos_list[k] under the mask of column label cols[b].
    Kept entries (u, v), v not in P_cols[b], are gathered with their values (1 without); the scale is the row's own (1
    without) when nothing was removed, else 1 / kept sum -- and where that sum is 0 the dense method's `s == 0 -> 1` leaves
    the row scale: all-zero kept values, or none kept at all, aggregate to exactly 0.  A neighbour in P_i, and the row itself
    as the residual input, are read from X_inst [n_cols][n_pos][S][d] when it is given (layer 2), else from X [S, n, d].
    dtype=np.float32 runs every array and operation in float32.  Returns (instances [n_cols][n_pos][S][d] in dtype,
    removed int32 [n_cols][n_pos])."""
    dt = np.dtype(dtype)
    X = np.asarray(X, dt)
    p = LayerParams(np.asarray(p.W, dt), np.asarray(p.b, dt), np.asarray(p.wg, dt), dt.type(p.cg))
    Sn, n, d = X.shape
    u = np.asarray(pos_list, np.int64)
    n_pos, n_cols = u.shape[0], len(cols)
    lens = g.rowptr[u + 1] - g.rowptr[u]
    lp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ent = np.concatenate([np.arange(g.rowptr[a], g.rowptr[a + 1]) for a in u] + [np.zeros(0, np.int64)]).astype(np.int64)
    m = ent.shape[0]
    vs = g.col[ent]
    w = np.ones(m, dt) if g.val is None else np.asarray(g.val[ent], dt)
    rs_u = np.ones(n_pos, dt) if g.row_scale is None else np.asarray(g.row_scale[u], dt)
    rowid = np.repeat(np.arange(n_pos), lens)
    rank = np.full(n, -1, np.int64)
    rank[u] = np.arange(n_pos)
    rv = rank[vs]
    xsrc = X[:, vs, :]
    out = np.zeros((n_cols, n_pos, Sn, d), dt)
    removed = np.zeros((n_cols, n_pos), np.int32)
    if n_pos == 0 or n_cols == 0:
        return out, removed
    if X_inst is not None:
        X_inst = np.asarray(X_inst, dt)
    cols = np.asarray(cols, np.int64)
    seg = sp.csr_matrix((np.ones(m, dt), np.arange(m), lp), shape=(n_pos, m))       # row k sums the entries of pos_list[k]
    in_p = np.flatnonzero(rv >= 0)
    step = max(1, (1 << 23) // max(1, m * Sn * d))                                  # column labels per batch
    for b0 in range(0, n_cols, step):
        jb = cols[b0:b0 + step]
        B = jb.shape[0]
        drop = pos[vs][:, jb].T                                                     # [B, m]
        wk = np.where(drop, dt.type(0), w[None, :])
        rem = np.rint(seg @ drop.T.astype(np.float64)).astype(np.int32).T           # [B, n_pos]
        wsum = np.asarray(seg @ wk.T, dt).T
        nz = wsum != 0
        sc = np.where((rem == 0) | ~nz, rs_u[None, :], dt.type(1) / np.where(nz, wsum, dt.type(1)))
        indptr = (lp[None, :-1] + m * np.arange(B)[:, None]).ravel()
        indptr = np.concatenate([indptr, [B * m]])
        if X_inst is None:                                                          # every label reads the same neighbours
            A = sp.csr_matrix((wk.ravel(), np.tile(np.arange(m), B), indptr), shape=(B * n_pos, m))
            xv = xsrc
            xin = np.broadcast_to(X[:, None, u, :], (Sn, B, n_pos, d)).reshape(Sn, B * n_pos, d)
        else:
            A = sp.csr_matrix((wk.ravel(), np.arange(B * m), indptr), shape=(B * n_pos, B * m))
            xv = np.broadcast_to(xsrc[:, None], (Sn, B, m, d)).copy()
            xv[:, :, in_p, :] = X_inst[b0:b0 + B][:, rv[in_p]].transpose(2, 0, 1, 3)
            xv = xv.reshape(Sn, B * m, d)
            xin = X_inst[b0:b0 + B].transpose(2, 0, 1, 3).reshape(Sn, B * n_pos, d)
        H = np.stack([A @ xv[s] for s in range(Sn)]).astype(dt, copy=False) * sc.reshape(1, -1, 1)
        out[b0:b0 + B] = _gated(H, xin, p).reshape(Sn, B, n_pos, d).transpose(1, 2, 0, 3)
        removed[b0:b0 + B] = rem
    return out, removed


# ---- cgcn_ablation_head / cgcn_ablation_reduce -----------------------------------------------------------------------------
def head_prob(hp, rows, label):
    """sigmoid of the strand-mean logit of `label` on rows [..., S, d] (ReLU, eval BatchNorm, W_out[label] . y + b_out)"""
    y = np.maximum(np.asarray(rows, np.float64), 0.0)
    z = (y - hp.mean) / np.sqrt(hp.var + hp.eps) * hp.bn_w + hp.bn_b
    return _sigmoid((z @ hp.W_out[label] + hp.b_out[label]).mean(-1))


def _pair_entry(base_i, mean, removed_total):
    return 0.0 if removed_total == 0 else (base_i - mean) / base_i


def head_ref(hp, prep, label=-1, X=None, inst=None, removed=None, cols=None, base=None):
    """cgcn_ablation_head.  label < 0: base [C] from the unablated last-layer output X [S, n, d] (NaN for an empty label).
    label = i: row i of M [C] from the instance rows inst [n_cols][n_pos][S][d], zero outside cols."""
    C = prep.counts.shape[0]
    if label < 0:
        out = np.full(C, np.nan)
        for c in range(C):
            if prep.counts[c] > 0:
                rows = np.asarray(X, np.float64)[:, prep.lists[c, :prep.counts[c]], :].transpose(1, 0, 2)
                out[c] = head_prob(hp, rows, c).mean()
        return out
    row = np.zeros(C)
    for b, j in enumerate(cols):
        row[j] = _pair_entry(base[label], head_prob(hp, inst[b], label).mean(), int(np.sum(removed[b])))
    return row


def reduce_ref(logits, prep, label=-1, col_label=None, removed_total=None, base=None):
    """cgcn_ablation_reduce on logits [2, n, C].  label < 0: base [C]; label = i: the entry M[i, col_label]."""
    lg = np.asarray(logits, np.float64)

    def mean(c):
        rows = prep.lists[c, :prep.counts[c]]
        return _sigmoid((lg[0, rows, c] + lg[1, rows, c]) * 0.5).mean() if rows.size else np.nan
    if label < 0:
        return np.array([mean(c) for c in range(prep.counts.shape[0])])
    return _pair_entry(base[label], mean(label), removed_total)


# ---- cgcn_ablation_mask ----------------------------------------------------------------------------------------------------
def mask_ref(g, pos, i, j, dtype=np.float32):
    """cgcn_ablation_mask: (val_out [nnz], row_scale_out [n], removed total) of pair (i, j) on the unchanged pattern.  The
    kept sum of a touched row is a sequential sum in CSR order in `dtype` (float32: the kernel's own, so the comparison can be
    tight; float64 for the host comparison with the dense method).  A touched row whose kept sum is 0 keeps its row scale
    (`s == 0 -> 1`), or gets exactly 0 when it keeps nothing."""
    dt = np.dtype(dtype)
    n = g.rowptr.shape[0] - 1
    rows = S.rows_of(g.rowptr)
    w = np.ones(g.col.shape[0], dt) if g.val is None else np.asarray(g.val, dt)
    drop = pos[rows, i] & pos[g.col, j]
    val_out = np.where(drop, dt.type(0), w)
    rs_out = np.ones(n, dt) if g.row_scale is None else np.asarray(g.row_scale, dt).copy()
    for u in np.unique(rows[drop]):
        k0, k1 = g.rowptr[u], g.rowptr[u + 1]
        s = dt.type(0)
        for v in val_out[k0:k1][~drop[k0:k1]]:
            s = dt.type(s + v)
        if s != 0:
            rs_out[u] = dt.type(1) / s
        elif drop[k0:k1].all():
            rs_out[u] = 0
    return val_out, rs_out, int(drop.sum())


def masked_dense(g, val_out, rs_out):
    return dense_of(Graph(g.rowptr, g.col, np.asarray(val_out, np.float64), np.asarray(rs_out, np.float64)))


# ---- the whole matrix from the pieces ----------------------------------------------------------------------------------------
def _labels(sel, C):
    return list(range(C)) if sel is None else list(dict.fromkeys(int(c) for c in sel))


def restricted_matrix_ref(mp, g, x, targets, rows=None, cols=None):
    """(M [C, C], base [C]) in float64, by the restricted route's decomposition (at most 2 layers): the unablated forward
    once, then per row label i the instances of the rows of P_i through layer_ref (layer 2 reading layer 1's) and label i's
    head.  mp = model_params(oracle); g a Graph; x [2, n, d]; M[i, i], an empty P_j and pairs outside rows x cols are 0, an
    empty P_i gives NaN."""
    layers, hp = mp
    assert 1 <= len(layers) <= 2
    pos = positives(targets)
    prep = prepare_ref(targets)
    C = pos.shape[1]
    xs = [np.asarray(x, np.float64)]
    for p in layers:
        xs.append(full_layer_ref(g, xs[-1], p))
    base = head_ref(hp, prep, X=xs[-1])
    M = np.zeros((C, C))
    for i in _labels(rows, C):
        js = [j for j in _labels(cols, C) if j != i and prep.counts[j] > 0]
        if not js:
            continue
        if prep.counts[i] == 0:
            M[i, js] = np.nan
            continue
        pl = prep.lists[i, :prep.counts[i]]
        inst, removed = layer_ref(g, xs[0], layers[0], pos, pl, js)
        if len(layers) == 2:
            inst, _ = layer_ref(g, xs[1], layers[1], pos, pl, js, X_inst=inst)
        M[i] = head_ref(hp, prep, i, inst=inst, removed=removed, cols=js, base=base)
    return M, base


# ---- cases: graphs ---------------------------------------------------------------------------------------------------------
N, C_FULL = 300, 103
GRAPH_KINDS = ("hic", "both", "hub", "coo")
ROW_LABELS = (3, 33, 64, 102)                                  # one row label per word of the bitmask
SUBSET_COLS = tuple(int(c) for c in np.round(np.linspace(0, 102, 40)).astype(np.int64))
COO_EMPTY_ROW, COO_ZERO_ROW = 150, 12                          # of coo_matrix: no stored entry / a row with stored zeros


@functools.lru_cache(maxsize=None)
def coo_matrix(n=N):
    """The explicit-value operator a reference caller hands over as a torch sparse COO tensor: saliency_ref.
    asymmetric_valued restricted to non-negative values (|v|), each row divided by its sum, asymmetric, rows of 65 and 200
    entries, row COO_EMPTY_ROW without a stored entry, and in row COO_ZERO_ROW three STORED zeros next to three values."""
    a = S.asymmetric_valued(n, 0.04, 21, lengths=(65, 200), empty_row=COO_EMPTY_ROW).astype(np.float64)
    a.data = np.abs(a.data)
    z = COO_ZERO_ROW
    assert z not in (2, 4, COO_EMPTY_ROW)
    a = a.tolil()
    a[z, :] = 0
    a = sp.csr_matrix(a)
    a.eliminate_zeros()
    a = a.tolil()
    for c, v in zip((5, z, 40, 77, 130, 299), (0.5, 1.0, 0.25, 1e-30, 1e-30, 1e-30)):
        a[z, c] = v
    a = sp.csr_matrix(a)
    a.sort_indices()
    k0 = a.indptr[z]
    assert a.indptr[z + 1] - k0 == 6
    a.data[k0 + 3:k0 + 6] = 0.0                                 # columns 77, 130, 299: stored, valued 0
    rowsum = np.asarray(a.sum(1)).ravel()
    a.data /= np.where(rowsum != 0, rowsum, 1.0)[S.rows_of(a.indptr)]
    assert (abs(a - a.T)).nnz > 0 and a.data.min() == 0.0
    return a


def coo_tensor(n=N):
    """coo_matrix as the float32 torch sparse COO tensor (stored zeros included)"""
    a = coo_matrix(n).tocoo()
    idx = torch.from_numpy(np.vstack((a.row, a.col)).astype(np.int64))
    return torch.sparse_coo_tensor(idx, torch.from_numpy(a.data.astype(np.float32)), torch.Size(a.shape))


@functools.lru_cache(maxsize=None)
def raw_hic(kind, n=N):
    if kind == "hub":
        return S.hub_hic(n, "hic")[0]
    return O.random_symmetric_graph(n, 2000, {"hic": 31, "both": 32}[kind])


@functools.lru_cache(maxsize=None)
def host_graph(kind, n=N):
    """HostCSR of the case graph: 'hic' implicit values with a row scale; 'both' explicit values 1/2/3 with a row scale; 'hub'
    implicit with rows of 63 .. 200 entries and one row without an entry (row scale 0); 'coo' explicit values, NO row scale"""
    if kind == "coo":
        h = G.host_csr_from_matrix(coo_matrix(n))
        assert h.row_scale is None and h.nnz == coo_matrix(n).nnz
        return h
    h = G.normalize_graph("both" if kind == "both" else "hic", raw_hic(kind, n), n)
    assert (h.val is not None) == (kind == "both")
    return h


# ---- cases: targets --------------------------------------------------------------------------------------------------------
# planted labels of case_targets, spread over the four words of the bitmask and apart from ROW_LABELS
L_HUB, L_ALL_NB, L_BUT_ONE, L_U0, L_V0, L_EMPTY, L_EVERY, L_ZERO_I, L_ZERO_J = 40, 71, 7, 97, 20, 50, 60, 66, 99
Planted = namedtuple("Planted", "hub keep_one u0 v0")


@functools.lru_cache(maxsize=None)
def case_targets(kind, n=N, C=C_FULL, seed=0, rate=0.05):
    """(targets float32 [n, C] as a torch tensor, Planted): every label positive at `rate`, then
      L_HUB = {hub}, the longest row; L_ALL_NB = its stored neighbours (itself included): (L_HUB, L_ALL_NB) loses every entry;
      L_BUT_ONE = all of them but keep_one: (L_HUB, L_BUT_ONE) keeps exactly one;
      L_U0 = {u0}, L_V0 = {v0} with no stored entry between them: both pairs remove nothing;
      L_EMPTY positive nowhere, L_EVERY on every row;
      'coo' only: L_ZERO_I = {COO_ZERO_ROW}, L_ZERO_J = its neighbours with a nonzero value: the row keeps stored zeros only."""
    h = host_graph(kind, n)
    g = torch.Generator().manual_seed(1000 + seed)
    t = (torch.rand(n, C, generator=g) < rate).float()
    lens = np.diff(h.rowptr)
    hub = int(np.argmax(lens))
    nb = h.col[h.rowptr[hub]:h.rowptr[hub + 1]].astype(np.int64)
    stored = sp.csr_matrix((np.ones(h.nnz), h.col, h.rowptr), shape=(n, n)).toarray() != 0
    u0 = next(u for u in range(n) if u not in (hub, COO_ZERO_ROW) and lens[u] > 0)
    v0 = next(v for v in range(n) if v not in (u0, hub) and lens[v] > 0 and not stored[u0, v] and not stored[v, u0])
    keep_one = int(nb[len(nb) // 2])
    for lab, rows in ((L_HUB, [hub]), (L_ALL_NB, nb), (L_BUT_ONE, nb[nb != keep_one]), (L_U0, [u0]), (L_V0, [v0]),
                      (L_EMPTY, []), (L_EVERY, np.arange(n))):
        t[:, lab] = 0
        t[torch.as_tensor(np.asarray(rows, np.int64)), lab] = 1
    if kind == "coo":
        z = COO_ZERO_ROW
        k0, k1 = h.rowptr[z], h.rowptr[z + 1]
        t[:, L_ZERO_I] = 0
        t[z, L_ZERO_I] = 1
        t[:, L_ZERO_J] = 0
        t[torch.as_tensor(h.col[k0:k1][h.val[k0:k1] != 0].astype(np.int64)), L_ZERO_J] = 1
    return t, Planted(hub, keep_one, u0, v0)


def count_targets(n, counts, seed):
    """float32 [n, len(counts)]: label c positive on exactly counts[c] rows, drawn without replacement"""
    rng = np.random.RandomState(seed)
    t = np.zeros((n, len(counts)), np.float32)
    for c, k in enumerate(counts):
        t[rng.choice(n, k, replace=False), c] = 1
    return t


HEAD_COUNTS = (1, 2, 3, 4, 5, 8, 9, 300)       # k_abl_head: four waves take positions w, w + 4, ...
REDUCE_COUNTS = (1, 255, 256, 257, 300)        # k_abl_reduce: 256 threads take positions t, t + 256, ...
PREPARE_N = (1, 255, 256, 257, 300)            # k_abl_lists: chunks of 256 rows
PREPARE_C = (1, 31, 32, 33, 64, 65, 103)       # words of the bitmask


def prepare_targets(n, C, seed=0):
    return (np.random.RandomState(100 * n + C + seed).rand(n, C) < 0.3).astype(np.float32)


# ---- cases: models and inputs ------------------------------------------------------------------------------------------------
OUT_SCALE = 6.0      # on the classifier's default init: logits of a few units, so that base_i stays inside (0.05, 0.95)


def make_oracle(d, c, layers, seed, out_scale=OUT_SCALE):
    """float32 oracle in eval mode: GC weights randn / sqrt(d) * 1.5, the classifier scaled, BatchNorm statistics drawn"""
    torch.manual_seed(seed)
    orc = O.GatedGCNOracle(d, c, 0.0, layers)
    with torch.no_grad():
        for k, p in orc.named_parameters():
            if "GC" in k and k.endswith("weight"):
                p.copy_(torch.randn_like(p) / np.sqrt(d) * 1.5)
        orc.out.weight.mul_(out_scale)
        orc.batch_norm.running_mean.copy_(torch.randn(d) * 0.1)
        orc.batch_norm.running_var.copy_(torch.rand(d) + 0.5)
        orc.batch_norm.weight.copy_(torch.rand(d) + 0.5)
        orc.batch_norm.bias.copy_(torch.randn(d) * 0.1)
    return orc.eval()


def features(n, d, seed):
    """x [2, n, d] float32 (forward and reverse strand)"""
    g = torch.Generator().manual_seed(2000 + seed)
    return torch.stack([torch.randn(n, d, generator=g), torch.randn(n, d, generator=g)])


MATRIX_KINDS = ("hic", "coo")                  # the whole-matrix cases of the GPU test
MATRIX_D, MATRIX_LAYERS = 128, 2


@functools.lru_cache(maxsize=None)
def matrix_case(kind):
    """The C = 103, n = 300, rate 0.05, L = 2, d = 128 case on graph `kind`: oracle (float32), inputs, targets and -- once, for
    every test that needs it -- the float64 (M, base) of restricted_matrix_ref on the float32 graph"""
    seed = GRAPH_KINDS.index(kind)
    orc = make_oracle(MATRIX_D, C_FULL, MATRIX_LAYERS, 10 + seed)
    x = features(N, MATRIX_D, seed)
    t, planted = case_targets(kind)
    M, base = restricted_matrix_ref(model_params(orc), graph_arrays(host_graph(kind)), x.numpy(), t.numpy())
    M.setflags(write=False)
    base.setflags(write=False)
    return dict(orc=orc, x=x, targets=t, planted=planted, M=M, base=base)


def removes_something(h, pos):
    """bool [C, C]: pair (i, j) removes at least one stored entry"""
    A = sp.csr_matrix((np.ones(h.nnz), h.col, h.rowptr), shape=(h.n, h.n))
    p = pos.astype(np.float64)
    return (p.T @ (A @ p)) > 0


# ---- cases: the head and the reduction alone -----------------------------------------------------------------------------
HEAD_LABELS = HEAD_COUNTS + (0,) + (15,) * 11       # C = 20: the counts under test, an empty label, column labels to spare
HEAD_SEEDS = {128: 192, 256: 317}                  # model seeds that keep every base_i inside (0.05, 0.95)
REDUCE_LABELS = REDUCE_COUNTS + (0,)


@functools.lru_cache(maxsize=None)
def head_case(d):
    """targets with |P_c| = HEAD_LABELS[c], a one-layer oracle (its BatchNorm and classifier are the head), unablated rows x
    [2, n, d] and the float64 base of head_ref on them"""
    t = count_targets(N, HEAD_LABELS, 1)
    prep = prepare_ref(t)
    orc = make_oracle(d, len(HEAD_LABELS), 1, HEAD_SEEDS[d])
    x = features(N, d, 61).numpy()
    base = head_ref(model_params(orc)[1], prep, X=x)
    base.setflags(write=False)
    return dict(targets=t, prep=prep, orc=orc, hp=model_params(orc)[1], x=x, base=base)


@functools.lru_cache(maxsize=None)
def reduce_case():
    """targets with |P_c| = REDUCE_LABELS[c], logits [2, n, C] for the base, other logits for the pairs, the float64 base"""
    t = count_targets(N, REDUCE_LABELS, 2)
    prep = prepare_ref(t)
    c = len(REDUCE_LABELS)
    logits = (np.random.RandomState(5).randn(2, N, c) * 1.5).astype(np.float32)
    logits2 = (logits * 0.5 + np.random.RandomState(6).randn(2, N, c) * 0.7).astype(np.float32)
    base = reduce_ref(logits, prep)
    base.setflags(write=False)
    return dict(targets=t, prep=prep, logits=logits, logits2=logits2, base=base)


# ---- cases: the layer kernel alone -------------------------------------------------------------------------------------------
LAYER_N_COLS = (1, 15, 16, 17, 32, 33, 102)    # k_abl_layer: blocks of 16 column labels
LAYER_CASES = tuple((kind, nc, 128) for kind in GRAPH_KINDS for nc in LAYER_N_COLS) + \
    tuple((kind, nc, 256) for kind in GRAPH_KINDS for nc in (17, 102))
# max |float32 - float64| of layer_ref's instance rows over LAYER_CASES, both layers (tests/test_ablation_ref_host.py
# measures it again and holds it to this figure): what float32 arithmetic alone does to a layer
LAYER_F32_YARDSTICK = 8.62e-07


def layer_params(d, seed):
    """two LayerParams (float32 values as float64) that differ, for layer 1 and layer 2"""
    rng = np.random.RandomState(3000 + seed)
    out = []
    for _ in range(2):
        W = (rng.randn(d, d) / np.sqrt(d) * 1.5).astype(np.float32)
        b, wg = (rng.randn(d) * 0.1).astype(np.float32), (rng.randn(d) / np.sqrt(d)).astype(np.float32)
        out.append(LayerParams(W.astype(np.float64), b.astype(np.float64), wg.astype(np.float64), float(np.float32(rng.randn() * 0.1))))
    return out


def layer_cols(i, n_cols, C=C_FULL):
    """n_cols column labels for row label i: the other labels in a seeded order that takes the words of the bitmask in turn,
    so that four labels or more cover every word"""
    rng = np.random.RandomState(7 + i)
    words = [[int(c) for c in rng.permutation(np.arange(w, min(w + 32, C))) if c != i] for w in range(0, C, 32)]
    order = [w[k] for k in range(32) for w in words if k < len(w)]
    return order[:n_cols]


@functools.lru_cache(maxsize=None)
def layer_case(kind, n_cols, d):
    """Inputs and float64 results of the layer kernel alone, for every row label of ROW_LABELS: X1 / X2 [2, n, d] are unrelated
    draws (a swap of X and X_inst shows), layer 2 reads layer 1's float64 instances ROUNDED to float32 (what the kernel is
    handed).  Returns dict(x1, x2, params, pos, per_label = {i: (pos_list, cols, inst1, removed, inst1_f32, inst2)})."""
    seed = 10 * GRAPH_KINDS.index(kind) + (d == 256)
    g = graph_arrays(host_graph(kind))
    t, _ = case_targets(kind)
    pos = positives(t.numpy())
    x1, x2 = features(N, d, 50 + seed).numpy(), features(N, d, 90 + seed).numpy()
    params = layer_params(d, seed)
    per = {}
    for i in ROW_LABELS:
        pl = np.flatnonzero(pos[:, i])
        cols = layer_cols(i, n_cols)
        inst1, removed = layer_ref(g, x1, params[0], pos, pl, cols)
        inst1_f32 = inst1.astype(np.float32)
        inst2, removed2 = layer_ref(g, x2, params[1], pos, pl, cols, X_inst=inst1_f32)
        assert np.array_equal(removed, removed2)
        per[i] = (pl, cols, inst1, removed, inst1_f32, inst2)
    return dict(g=g, x1=x1, x2=x2, params=params, pos=pos, per_label=per)
