"""Planted graphs, tables and numpy restatements for the per-kernel tests of csrc/cgcn_effects.hip
(tests/test_effects_kernels_host.py on the CPU, tests/test_gpu_effects_kernels.py on the device).  CPU only.

The restatements follow the definition in the header comment of cgcn_effects.hip, as plain loops over variants and
instances: variant m replaces row u = windows[m]; its instances are u, then every v != u with a stored A[v, u] in ascending v.
    layer 1   H_inst = H1[v] + row_scale[v] Ahat[v, u] (alt[m] - X0[u])     residual: alt[m] for instance 0, else X0[v]
    layer 2   H_out  = H2[v] + row_scale[v] sum_w Ahat[v, w] (X1_inst[w's instance] - X1[w])   over the stored w of row v that
              are instances of the same variant, in ascending w
They never look at the transposed arrays the kernels search: the in-edges of a window come from one pass over the rows.

`wrong=` selects one deliberately wrong rule (WRONG_RULES): tests/test_effects_kernels_host.py shows that every one of them
changes an element of the exact cases, i.e. that those cases would catch a kernel that followed it."""
import functools

import numpy as np

from chromegcn_amd import graph as G

S = 2
CHUNK = 64                                   # stored entries k_eff_rows2 takes per step, one per lane
PATTERNS = ("lanes", "asymdiag")
FIELDS = [(False, False), (True, False), (False, True), (True, True)]       # (with val, with row_scale)
SCALES = np.array([0.25, 0.5, 1.0, 2.0], np.float32)
U32 = 2.0 ** -24                             # unit roundoff of float32

# ---- 'lanes': symmetric 0/1 pattern, n = 440 -------------------------------------------------------------------------
N_LANES = 440
HUB = 220                                    # its instances hold a row of every planted length
EMPTY, ALONE = 300, 301                      # no stored entry at all / the diagonal alone
V2, V63, V64, V65, V127, V128, V129, VGAP, V200 = 10, 150, 160, 170, 230, 240, 250, 260, 430
_SPECIAL = {V2: (2, True), V63: (63, True), V64: (64, False), V65: (65, True), V127: (127, True), V128: (128, False),
            V129: (129, True), V200: (200, True)}                           # window: (stored length, stored diagonal)
PLANTED_LENGTHS = (2, 63, 64, 65, 127, 128, 129)
# ---- 'asymdiag': asymmetric pattern with some stored diagonals, n = 320 ------------------------------------------------
N_ASYM = 320
NO_IN, NO_OUT, LONG_ROW, LONG_COL = 9, 21, 100, 101


def _lanes_pattern():
    n = N_LANES
    rng = np.random.RandomState(31)
    b = np.zeros((n, n), bool)
    not_filler = set(_SPECIAL) | {HUB, EMPTY, ALONE, VGAP}
    out_range = set(range(60, 140)) | set(range(300, 380))                  # fillers that are NOT neighbours of the hub
    fillers = np.array([f for f in range(n) if f not in not_filler])
    f_in = np.array([f for f in fillers if f not in out_range])
    f_out = np.array([f for f in fillers if f in out_range])

    def link(v, ws):
        b[v, ws] = True
        b[ws, v] = True

    link(HUB, f_in)
    b[HUB, HUB] = True
    b[ALONE, ALONE] = True
    for f in fillers:
        b[f, f] = f % 3 != 1
    pairs = rng.choice(fillers, (500, 2))
    for x, y in pairs[pairs[:, 0] != pairs[:, 1]]:
        link(x, y)
    for v, (length, diag) in _SPECIAL.items():
        pool = fillers[fillers < v] if v == V200 else fillers               # V200: its diagonal is the row's last entry
        k = length - 1 - int(diag)
        link(v, HUB)
        link(v, rng.choice(pool, k, replace=False) if k else [])
        b[v, v] = diag
    # VGAP, 129 entries and no diagonal: members of window HUB at lane 0 of chunk 0 (window 0), at lane 63 of chunk 0 (the
    # hub itself), none in chunk 1 (64 windows the hub has no edge to), one in the partial chunk 2 (window 400)
    gap = [0] + list(range(60, 122)) + [HUB] + list(range(302, 366)) + [400]
    assert len(gap) == 129 and all(g in f_in or g == HUB for g in (0, HUB, 400))
    assert all(g in f_out for g in gap[1:63] + gap[64:128])
    link(VGAP, gap)
    assert np.array_equal(b, b.T) and not b[EMPTY].any() and not b[:, EMPTY].any()
    return b


def _asym_pattern():
    n = N_ASYM
    rng = np.random.RandomState(32)
    b = rng.rand(n, n) < 0.04
    np.fill_diagonal(b, np.arange(n) % 4 == 0)
    b[LONG_ROW, rng.choice(n, 150, replace=False)] = True
    b[rng.choice(n, 150, replace=False), LONG_COL] = True
    b[:, NO_IN] = False
    b[NO_OUT, :] = False
    b[[3, 50, 200], NO_OUT] = True
    return b


def members(h, u, v):
    """positions inside stored row v of the entries w that are instances of window u (u itself, or a stored A[w, u])"""
    rp, col = h.rowptr, h.col
    inst = {u} | {w for w in range(h.n) if u in col[rp[w]:rp[w + 1]]}
    return [p for p, w in enumerate(col[rp[v]:rp[v + 1]]) if w in inst]


def _check_lanes(h):
    rp, col = h.rowptr, h.col
    length = np.diff(rp)
    assert length[ALONE] == 1 and col[rp[ALONE]] == ALONE and length[EMPTY] == 0
    for v, (want, diag) in _SPECIAL.items():
        assert length[v] == want and (v in col[rp[v]:rp[v + 1]]) == diag, v
    assert length[VGAP] == 129
    # symmetric: row HUB lists the hub's instances.  (A row of length 1 holds its diagonal alone and is nobody else's
    # instance: ALONE is its own window's only one.)
    inst_len = {int(length[v]) for v in col[rp[HUB]:rp[HUB + 1]]}
    assert set(PLANTED_LENGTHS) <= inst_len and max(inst_len) >= 193 and length[V200] >= 193 and length[HUB] >= 193
    mem = members(h, HUB, VGAP)
    assert mem == [0, 63, 128], mem                                        # lane 0, lane 63, nothing in chunk 1, partial chunk
    rel = []                                                                # (position of the stored diagonal, row length)
    for u in range(h.n):
        row = col[rp[u]:rp[u + 1]]
        hit = np.flatnonzero(row == u)
        rel.append((int(hit[0]) if hit.size else -1, row.shape[0]))
    assert any(dp == 0 and ln > 1 for dp, ln in rel) and any(dp == ln - 1 and ln > 1 for dp, ln in rel)
    assert any(0 < dp < ln - 1 for dp, ln in rel) and 0 < rel[HUB][0] < rel[HUB][1] - 1
    assert rel[ALONE] == (0, 1) and rel[V2][0] == 0 and rel[V200][0] == rel[V200][1] - 1
    assert sum(dp < 0 for dp, _ in rel) >= 2 and sum(dp >= 0 for dp, _ in rel) >= 2


def _check_asym(h, b):
    assert b.diagonal().sum() > 10 and (~b.diagonal()).sum() > 10
    assert not b[:, NO_IN].any() and not b[NO_OUT].any() and b[:, NO_OUT].sum() >= 3 and b[NO_IN].any()
    assert b[LONG_ROW].sum() > 2 * CHUNK and b[:, LONG_COL].sum() > 2 * CHUNK
    off = b & ~np.eye(h.n, dtype=bool)
    assert (off & ~off.T).sum() > 1000 and (off & off.T).sum() >= 20        # one-way pairs; pairs stored both ways


@functools.lru_cache(maxsize=None)
def host_graph(pattern, with_val, with_scale) -> G.HostCSR:
    b = {"lanes": _lanes_pattern, "asymdiag": _asym_pattern}[pattern]()
    n = b.shape[0]
    rng = np.random.RandomState(33 + 2 * with_val + with_scale)
    rowptr = np.concatenate([[0], np.cumsum(b.sum(1))]).astype(np.int32)
    col = np.nonzero(b)[1].astype(np.int32)
    val = None
    if with_val:
        # drawn per entry, so Ahat[v, u] and Ahat[u, v] are different numbers wherever both are stored: val_t and val are
        # then different arrays on 'lanes' too, whose HostCSR is therefore not marked symmetric
        m = np.where(b, rng.randint(1, 4, (n, n)), 0)
        same = np.triu(b & b.T & (m == m.T), 1)
        m[same] = m[same] % 3 + 1
        both = b & b.T & ~np.eye(n, dtype=bool)
        assert both.sum() >= 20 and (m[both] != m.T[both]).all()
        val = m[b].astype(np.float32)
        assert set(np.unique(val)) == {1.0, 2.0, 3.0}
    scale = SCALES[rng.randint(0, 4, n)] if with_scale else None
    h = G.HostCSR(n=n, rowptr=rowptr, col=col, val=val, row_scale=scale, symmetric=pattern == "lanes" and not with_val)
    if pattern == "lanes":
        _check_lanes(h)
    else:
        _check_asym(h, b)
    return h


# ---- the restatements -----------------------------------------------------------------------------------------------------
WRONG_RULES = ("no_shift", "inverse_ge", "val_for_val_t", "scale_u", "drop_lane63", "drop_last_partial", "skip_after_empty",
               "ignore_offsets0", "strand0_alt", "nodiag_update")


def _in_edges(h):
    """per window u the list of (v, q) with col[q] == u in stored row v, in ascending v: the stored A[v, u]"""
    inn = [[] for _ in range(h.n)]
    for v in range(h.n):
        for q in range(h.rowptr[v], h.rowptr[v + 1]):
            inn[h.col[q]].append((v, q))
    return inn


def _instances(inn_u, u, wrong=None):
    """[(v, q, j)] of window u: the instance's window, the storage index of Ahat[v, u] in (col, val) and its position among
    the in-edges of u (both -1 for instance 0 without a stored diagonal)"""
    own = [(v, q, j) for j, (v, q) in enumerate(inn_u) if v == u]
    rest = [(v, q, j) for j, (v, q) in enumerate(inn_u) if v != u]
    if wrong == "no_shift":          # instance k > 0 taken for in-edge k - 1 although the diagonal sits before it
        rest = [(inn_u[k][0], inn_u[k][1], k) for k in range(len(rest))]
    return (own or [(u, -1, -1)]) + rest


def _fields(h):
    val = np.ones(h.nnz) if h.val is None else h.val.astype(np.float64)
    scale = np.ones(h.n) if h.row_scale is None else h.row_scale.astype(np.float64)
    return val, scale


def plan_host(h, windows):
    """(counts int32 [M]: instances per variant, diag_pos int32 [M]: position of u among its in-edges, -1 without one)"""
    inn = _in_edges(h)
    counts, diag = [], []
    for u in windows:
        counts.append(len(_instances(inn[u], u)))
        diag.append(next((j for j, (v, _) in enumerate(inn[u]) if v == u), -1))
    return np.asarray(counts, np.int32), np.asarray(diag, np.int32)


def offsets_of(h, windows):
    return np.concatenate([[0], np.cumsum(plan_host(h, windows)[0], dtype=np.int64)])


def _rows1(h, X0, H1, windows, alt, own, wrong=None, absolute=False):
    val, scale = _fields(h)
    inn = _in_edges(h)
    start = np.concatenate([[0], np.cumsum([len(e) for e in inn])])         # where window u's in-edges start in transposed order
    X0, H1, alt = (np.asarray(a, np.float64) for a in (X0, H1, alt))
    rows, H, X = [], [], []
    for m, u in enumerate(windows):
        a = alt[m, [0, 0]] if wrong == "strand0_alt" else alt[m]
        inst = _instances(inn[u], u, wrong)
        for k, (v, q, j) in enumerate(inst[:1] if own else inst):
            coef = 0.0 if q < 0 else (scale[u] if wrong == "scale_u" else scale[v]) * val[q]
            if q >= 0 and wrong == "val_for_val_t":                          # the forward array read at the transposed index
                coef = scale[v] * val[start[u] + j]
            if q < 0 and wrong == "nodiag_update":
                coef = scale[u]
            rows.append(v)
            H.append(np.abs(H1[:, v]) + abs(coef) * np.abs(a - X0[:, u]) if absolute else H1[:, v] + coef * (a - X0[:, u]))
            X.append(a if k == 0 else X0[:, v])
    return np.asarray(rows, np.int32), np.stack(H, 1), np.stack(X, 1)


def rows1_host(h, X0, H1, windows, alt, own, wrong=None):
    """X0, H1 [S, n, d], alt [M, S, d] -> rows int32 [total], H_inst, X_inst float64 [S, total, d] (own: instance 0 alone)"""
    return _rows1(h, X0, H1, windows, alt, own, wrong)


def rows1_bound(h, X0, H1, windows, alt, own):
    """4u (|H1[v]| + |row_scale[v] Ahat[v, u]| |alt - X0[u]|): one rounding each of the coefficient, the difference and the
    fused multiply-add, first order, with one u to spare for the higher orders"""
    return 4 * U32 * _rows1(h, X0, H1, windows, alt, own, absolute=True)[1]


def _rows2(h, X1, H2, windows, X1_inst, own, wrong=None, absolute=False):
    val, scale = _fields(h)
    inn = _in_edges(h)
    X1, H2, X1_inst = (np.asarray(a, np.float64) for a in (X1, H2, X1_inst))
    H, R, K = [], [], []
    off = 0
    for u in windows:
        inst = _instances(inn[u], u)
        slot = {v: k for k, (v, _, _) in enumerate(inst)}
        if wrong == "inverse_ge":    # the instance of in-edge p as 1 + p - (p >= dp) for every p, the diagonal's own included
            dp = inst[0][2]
            slot = {v: 1 + p - int(0 <= dp <= p) for p, (v, _) in enumerate(inn[u])}
            slot.setdefault(u, 0)
        for k, (v, _, _) in enumerate(inst[:1] if own else inst):
            p0, p1 = h.rowptr[v], h.rowptr[v + 1]
            mem = [q for q in range(p0, p1) if h.col[q] in slot]             # ascending w: stored rows are sorted
            length = p1 - p0
            if wrong == "drop_lane63":
                mem = [q for q in mem if (q - p0) % CHUNK != CHUNK - 1]
            if wrong == "drop_last_partial" and length % CHUNK:
                mem = [q for q in mem if q - p0 < length - length % CHUNK]
            if wrong == "skip_after_empty":
                used = {(q - p0) // CHUNK for q in mem}
                first_empty = next((c for c in range(-(-length // CHUNK)) if c not in used), None)
                if first_empty is not None:
                    mem = [q for q in mem if (q - p0) // CHUNK < first_empty]
            acc = np.zeros_like(H2[:, 0])
            for q in mem:
                diff = X1_inst[:, off + slot[h.col[q]]] - X1[:, h.col[q]]
                acc += val[q] * (np.abs(diff) if absolute else diff)
            s = scale[u] if wrong == "scale_u" else scale[v]
            H.append(np.abs(H2[:, v]) + s * acc if absolute else H2[:, v] + s * acc)
            R.append(X1_inst[:, off + k])
            K.append(len(mem))
        off += len(inst)
    return np.stack(H, 1), np.stack(R, 1), np.asarray(K)


def rows2_host(h, X1, H2, windows, X1_inst, own, wrong=None):
    """X1, H2 [S, n, d], X1_inst [S, total, d] (every instance of every variant, own or not) -> H_out, X_res float64
    [S, total or M, d]"""
    return _rows2(h, X1, H2, windows, X1_inst, own, wrong)[:2]


def rows2_bound(h, X1, H2, windows, X1_inst, own):
    """(k + 4) u (|H2[v]| + row_scale[v] sum_w |Ahat[v, w]| |X1_inst[w] - X1[w]|), k members: the term added first passes
    k fused multiply-adds, its own difference and the final multiply-add (k + 2 roundings), two u to spare"""
    mag, _, k = _rows2(h, X1, H2, windows, X1_inst, own, absolute=True)
    return (k[None, :, None] + 4) * U32 * mag


def rows_ignoring_offsets0(offsets, m0, m1):
    """The wrong rule 'ignore_offsets0' for the batch of variants [m0, m1): row i of the batch's table taken for instance i
    of the whole list, not offsets[m0] + i.  Returns, per row, the global instance it computes, or -1 where that instance
    belongs to no variant of the batch (the row is never written)."""
    i = np.arange(int(offsets[m1] - offsets[m0]))
    return np.where((i >= offsets[m0]) & (i < offsets[m1]), i, -1)


# ---- the exact cases ------------------------------------------------------------------------------------------------------
def code(g, d):
    """[S, len(g), d] integers in [-16, 16]: three base-33 digits of the instance number spread over the columns, so that
    two instances below 33^3 never share a code"""
    g = np.asarray(g, np.int64)[None, :, None]
    c = np.arange(d)[None, None, :]
    s = np.arange(S)[:, None, None]
    return ((g // 33 ** (c % 3)) + c + 5 * s) % 33 - 16


def batches_of(n_var):
    return [(0, n_var // 3), (n_var // 3, 2 * n_var // 3), (2 * n_var // 3, n_var)]


@functools.lru_cache(maxsize=None)
def exact_case(pattern, with_val, with_scale, d):
    """Integer tables on a planted graph, every window a variant, and the restatement's answers as float32 (exactly)"""
    h = host_graph(pattern, with_val, with_scale)
    n = h.n
    rng = np.random.RandomState(1000 + d + 7 * PATTERNS.index(pattern) + 2 * with_val + with_scale)
    X0, H1, X1, H2 = (rng.randint(-8, 9, (S, n, d)).astype(np.float32) for _ in range(4))
    windows = np.arange(n, dtype=np.int32)
    alt = rng.randint(-8, 9, (n, S, d)).astype(np.float32)
    assert (alt[:, 0] != alt[:, 1]).any(1).all()
    offsets = offsets_of(h, windows)
    total = int(offsets[-1])
    assert total < 33 ** 3
    want = {}
    for own in (0, 1):
        rows, Hi, Xi = rows1_host(h, X0, H1, windows, alt, own)
        want["rows1", own] = (rows, Hi, Xi)
    rows = want["rows1", 0][0]
    X1_inst = (X1[:, rows] + code(np.arange(total), d)).astype(np.float32)
    for m in range(n):
        seg = X1_inst[:, offsets[m]:offsets[m + 1]] - X1[:, rows[offsets[m]:offsets[m + 1]]]
        assert np.unique(seg[0], axis=0).shape[0] == seg.shape[1]             # the codes of one variant all differ
    for own in (0, 1):
        want["rows2", own] = rows2_host(h, X1, H2, windows, X1_inst, own)
    # every partial sum is an integer multiple of 1/4 (the smallest row scale): exact in float32 while 4 x its size < 2^24
    val, scale = _fields(h)
    rowsum = np.add.reduceat(np.append(val, 0.0), h.rowptr[:-1].astype(np.int64)) * (np.diff(h.rowptr) > 0)
    largest = max(8 + scale.max() * rowsum.max() * 32, 8 + scale.max() * val.max() * 16)
    assert 4 * largest < 2 ** 24
    out = dict(h=h, windows=windows, X0=X0, H1=H1, X1=X1, H2=H2, alt=alt, offsets=offsets, X1_inst=X1_inst, largest=largest)
    for key, arrs in want.items():
        f32 = tuple(a if a.dtype == np.int32 else a.astype(np.float32) for a in arrs)
        assert all(np.array_equal(a, b) for a, b in zip(f32, arrs))         # nothing was rounded
        out[key] = f32
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


# ---- the float cases ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def float_case(kind, d):
    """Standard-normal tables on a graph of effects_cases (real row scales and values), its variant list, the float64
    restatement of both kernels and their derived bounds (rows1_bound, rows2_bound)"""
    import torch

    import effects_cases as EC
    h = EC.host_graph(kind)
    n = h.n
    seed = 70 + EC.GRAPH_KINDS.index(kind) + d
    g = torch.Generator().manual_seed(seed)
    X0, H1, X1, H2 = (torch.randn(S, n, d, generator=g).numpy() for _ in range(4))
    win, alt_f, alt_r = EC.variants(kind, n, d, torch.from_numpy(X0[0]), torch.from_numpy(X0[1]), seed)
    windows = win.astype(np.int32)
    alt = np.ascontiguousarray(torch.stack([alt_f, alt_r], 1).numpy())
    offsets = offsets_of(h, windows)
    rows, Hi, Xi = rows1_host(h, X0, H1, windows, alt, 0)
    X1_inst = (X1[:, rows] + torch.randn(S, rows.shape[0], d, generator=g).numpy()).astype(np.float32)
    Ho, _ = rows2_host(h, X1, H2, windows, X1_inst, 0)
    out = dict(h=h, windows=windows, X0=X0, H1=H1, X1=X1, H2=H2, alt=alt, offsets=offsets, rows=rows, X1_inst=X1_inst,
               H_inst=Hi, H_out=Ho, bound1=rows1_bound(h, X0, H1, windows, alt, 0),
               bound2=rows2_bound(h, X1, H2, windows, X1_inst, 0))
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out
