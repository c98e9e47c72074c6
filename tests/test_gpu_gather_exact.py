"""Every aggregation route held to exact integer sums on planted rows (tests/gather_cases.py).

The tables hold small integers, so every row sum is exact in fp32 in any order and the expected output is known as numbers
from an int64 CSR x dense product on the host (gather_cases.aggregate_ref / bwd_gather_ref).  The rule of every test: the
output buffer is prefilled with NaN and sits between two 4 096-byte guards of a fixed byte pattern; afterwards the result
EQUALS the reference element for element, holds no NaN, and the guards are untouched.  On failure the message names the
first wrong (strand, row, column) and that row's length and label.  No tolerance is chosen anywhere in this file."""
import ctypes
import functools
import time

import numpy as np
import pytest
import torch

import dropout_ref
import gather_cases as GC
from chromegcn_amd import _lib, graph as G

pytestmark = pytest.mark.gpu
DEV = "cuda"
P = _lib.ptr
GUARD = 4096
GUARD_BYTE = 0xA5
SD = GC.SD


# ---- buffers, graphs, comparison -----------------------------------------------------------------------------------------
class Guarded:
    """a float32 tensor prefilled with NaN between two guards"""

    def __init__(self, *shape):
        nbytes = 4 * int(np.prod(shape))
        self.raw = torch.full((nbytes + 2 * GUARD,), GUARD_BYTE, dtype=torch.uint8, device=DEV)
        self.t = self.raw[GUARD:GUARD + nbytes].view(torch.float32).view(*shape)
        self.t.fill_(float("nan"))
        assert self.t.data_ptr() % 16 == 0

    def guards_intact(self):
        return bool((self.raw[:GUARD] == GUARD_BYTE).all()) and bool((self.raw[-GUARD:] == GUARD_BYTE).all())


def dev(a, dtype=None):
    """device copy of a numpy array (the shared references are read-only: copied before torch sees them)"""
    return None if a is None else torch.from_numpy(np.array(a, order="C")).to(DEV, dtype=dtype)


class DevCsr:
    def __init__(self, rowptr, col, val=None, row_scale=None):
        self.rowptr, self.col, self.val, self.rs = dev(rowptr, torch.int32), dev(col, torch.int32), dev(val, torch.float32), dev(row_scale, torch.float32)
        if self.col.numel() == 0:
            self.col = torch.zeros(1, dtype=torch.int32, device=DEV)     # (a valid address for an empty list)
        self.n = int(self.rowptr.numel()) - 1

    @classmethod
    def of(cls, g, val=True):
        """the arrays of a ChromGraph"""
        self = cls.__new__(cls)
        self.rowptr, self.col, self.val, self.rs, self.n = g.rowptr, g.col, g.val if val else None, g.row_scale, g.n
        return self


def hand_aux(col=None, order=None, max_row_len=0, sixteen=False):
    """a cgcn_graph_aux built by hand -> (struct, tensors to keep alive)"""
    c16 = col.to(torch.int16) if sixteen else None
    return G.GraphAux(P(c16), P(order), max_row_len, 0), (c16, order)


def engine_graph(c, rs):
    """the case as the engine holds it: a ChromGraph, whose creation registers the 16-bit copy, tile_sorted_rows and
    max_row_len (and, with values of the 'both' form, the band-plus decomposition)"""
    d = DevCsr(c.rowptr, c.col, c.val, rs)
    return G.ChromGraph(n=d.n, nnz=int(c.col.size), rowptr=d.rowptr, col=d.col, val=d.val, row_scale=d.rs, rowptr_t=d.rowptr, col_t=d.col,
                        val_t=d.val, symmetric=True)


def assert_exact(got, want, deg, label, what, named_rows=()):
    """got: device tensor [S, n, d]; want: numpy of the same shape"""
    g = got.detach().cpu().numpy()
    bad = ~(g == want)                       # NaN compares unequal: an element never written is wrong
    if bad.any():
        s, i, c = (int(v) for v in np.argwhere(bad)[0])
        rows = np.unique(np.argwhere(bad)[:, 1])
        extra = ""
        if len(named_rows):
            extra = "; wrong rows among the strand ends %s: %s" % (list(named_rows), sorted(set(rows.tolist()) & set(named_rows)))
        raise AssertionError("%s: %d wrong elements in %d rows; first at (strand %d, row %d, column %d): got %r, want %r; that row has "
                             "%d entries and is: %s%s" % (what, int(bad.sum()), len(rows), s, i, c, g[s, i, c], want[s, i, c],
                                                          int(deg[i]), label(i), extra))
    assert not np.isnan(g).any(), what


@pytest.fixture
def lib():
    lb = _lib.load()
    try:
        yield lb
    finally:
        lb.cgcn_debug_set_fwd_split_bytes(-1)


def spmm(lb, csr, S, d, x, aux=None, n_cols=None, split=None):
    """cgcn_spmm into a guarded buffer; split: None = built-in threshold, 0 = sliced route forced, 1 << 40 = never by size"""
    y = Guarded(S, csr.n, d)
    lb.cgcn_debug_set_fwd_split_bytes(-1 if split is None else split)
    try:
        _lib.check(lb.cgcn_spmm(_lib.stream_ptr(), csr.n, csr.n if n_cols is None else n_cols, S, d, P(csr.rowptr), P(csr.col), P(csr.val),
                                P(csr.rs), P(x), P(y.t), aux), "cgcn_spmm")
        torch.cuda.synchronize()
    finally:
        lb.cgcn_debug_set_fwd_split_bytes(-1)
    return y


@functools.lru_cache(maxsize=None)
def reference(case_key, S, d):
    """(table, row scale, expected) of a square case, computed once and shared (never modified)"""
    c = CASES[case_key]()
    X = GC.int_table(S, c.n_cols, d, 1000 + 10 * S + d)
    rs = GC.inv_len_scale(c.rowptr)
    want = GC.aggregate_ref(c.rowptr, c.col, c.val, rs, X)
    for a in (X, rs, want):
        a.setflags(write=False)
    return c, X, rs, want


CASES = {"planted": lambda: GC.planted_graph(None), "planted_small": lambda: GC.planted_graph("small"),
         "whole": lambda: GC.whole_row_case(None), "whole_small": lambda: GC.whole_row_case("small"),
         "fused": lambda: GC.fused_case(None), "fused_small": lambda: GC.fused_case("small"),
         "iw65536": lambda: GC.index_width_case(65536), "iw65537": lambda: GC.index_width_case(65537)}
for _n in GC.SMALL_N:
    CASES["small%d" % _n] = functools.partial(GC.small_case, _n, None)
    CASES["small%d_small" % _n] = functools.partial(GC.small_case, _n, "small")


# ---- cgcn_spmm: the sliced routes ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,d", SD)
def test_sliced_aggregation_on_the_planted_graph(lib, S, d):
    """k_aggregate_sliced on the planted 2 113-row graph: int32 and 16-bit indices, without and with the registered row
    order, forced by the hook and routed by max_row_len alone (the 2 049-entry row), implicit and stored values"""
    c, X, rs, want = reference("planted", S, d)
    x, csr = dev(X), DevCsr(c.rowptr, c.col, None, rs)
    a32, k32 = hand_aux()
    a16, k16 = hand_aux(csr.col, sixteen=True)
    hub, kh = hand_aux(max_row_len=int(c.deg.max()))
    eg = engine_graph(c, rs)
    assert G.row_order(eg.col) is not None and G.col16_ptr(eg.col) is not None and G.max_row_len(eg.col) == 2049
    order = G.row_order(eg.col)
    ao, ko = hand_aux(order=order)
    for what, aux, split in (("int32, no order, hook", ctypes.addressof(a32), 0), ("no aux, hook", None, 0),
                             ("16-bit, no order, hook", ctypes.addressof(a16), 0),
                             ("int32, row order, hook", ctypes.addressof(ao), 0),
                             ("max_row_len alone, no hook", ctypes.addressof(hub), 1 << 40),
                             ("engine aux (16-bit, row order, max_row_len), no hook", G.aux_ptr(eg.col), 1 << 40)):
        y = spmm(lib, DevCsr.of(eg) if aux == G.aux_ptr(eg.col) else csr, S, d, x, aux, split=split)
        assert_exact(y.t, want, c.deg, c.label, "sliced aggregation, %s, S=%d d=%d" % (what, S, d))
        assert y.guards_intact(), what
    # stored values from {1, 2, 3}: the HAS_VAL instance (int32 indices)
    cv, Xv, rsv, wantv = reference("planted_small", S, d)
    y = spmm(lib, DevCsr(cv.rowptr, cv.col, cv.val, rsv), S, d, dev(Xv), None, split=0)
    assert_exact(y.t, wantv, cv.deg, cv.label, "sliced aggregation, stored values, S=%d d=%d" % (S, d))
    assert y.guards_intact()
    # the row order deals the rows to other waves than the planted ones: both walks still occur under it
    o = order.cpu().numpy()
    assert sorted(o.tolist()) == list(range(c.n_rows))
    walks = {GC.walk_of_wave(c.deg[o[p:p + 8]]) for p in range(0, c.n_rows - 7, 8)}
    assert walks == {"per-row", "cooperative"}


@pytest.mark.parametrize("S,d", SD)
def test_sliced_aggregation_on_graphs_of_one_tile_or_less(lib, S, d):
    for n in GC.SMALL_N:
        for key, sixteen in (("small%d" % n, False), ("small%d" % n, True), ("small%d_small" % n, False)):
            c, X, rs, want = reference(key, S, d)
            csr = DevCsr(c.rowptr, c.col, c.val, rs)
            aux, keep = hand_aux(csr.col, sixteen=sixteen)
            y = spmm(lib, csr, S, d, dev(X), ctypes.addressof(aux), split=0)
            assert_exact(y.t, want, c.deg, c.label, "sliced aggregation, %s, 16-bit=%s, S=%d d=%d" % (c.name, sixteen, S, d))
            assert y.guards_intact()


def test_sixteen_bit_indices_at_their_edge(lib):
    """n = 65 536 (column 65 535 is the int16 copy's -1, 32 768 its most negative number): the 16-bit instance against the
    integers, and the int32 instance on the same graph; n = 65 537: no copy is registered and the int32 instance runs"""
    S, d = 1, 128
    c, X, rs, want = reference("iw65536", S, d)
    eg = engine_graph(c, rs)
    assert G.col16_ptr(eg.col) is not None
    x = dev(X)
    use = DevCsr.of(eg)
    a32, _ = hand_aux()
    for what, aux in (("16-bit copy, row order", G.aux_ptr(eg.col)), ("int32", ctypes.addressof(a32))):
        y = spmm(lib, use, S, d, x, aux, split=0)
        assert_exact(y.t, want, c.deg, c.label, "n = 65 536, %s" % what)
        assert y.guards_intact()
    del x, eg, use
    c, X, rs, want = reference("iw65537", S, d)
    eg = engine_graph(c, rs)
    assert G.col16_ptr(eg.col) is None and G.aux_ptr(eg.col) is not None
    use = DevCsr.of(eg)
    y = spmm(lib, use, S, d, dev(X), G.aux_ptr(eg.col), split=0)
    assert_exact(y.t, want, c.deg, c.label, "n = 65 537, engine aux without a 16-bit copy")
    assert y.guards_intact()


# ---- band-plus and band --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def both_reference(n, S, d):
    h = GC.bandplus_host(n)[0]
    X = GC.int_table(S, n, d, 2000 + n + S + d)
    want = GC.aggregate_ref(h.rowptr, h.col, h.val, h.row_scale, X)
    for a in (X, want):
        a.setflags(write=False)
    return h, X, want


@pytest.mark.parametrize("S,d", SD)
def test_band_plus_aggregation(lib, S, d):
    """k_aggregate_sliced<BP>: the unit-entry list plus the +-7 window from LDS.  With S = 2 a window that ran past row n - 1
    of strand 0 would read strand 1 (and one before row 0 of strand 1 the end of strand 0): the rows at the strand ends
    are named in the message."""
    for n in GC.BANDPLUS_SMALL_N + (GC.PLANTED_N,):
        h, X, want = both_reference(n, S, d)
        if h.val is None:
            continue
        g = G.upload(h, DEV)
        assert G.has_band_plus(g.col) and (n < 128) == (G.row_order(g.col) is None)
        use = DevCsr.of(g)
        deg = np.diff(h.rowptr)
        label = lambda i: "row of the 'both' graph (merged length counted)"
        y = spmm(lib, use, S, d, dev(X), G.aux_ptr(g.col))
        assert_exact(y.t, want, deg, label, "band-plus, n=%d S=%d d=%d" % (n, S, d), GC.edge_rows(n))
        assert y.guards_intact()
        # the same decomposition by hand: int32 indices, no row order
        rp, cb = G.band_plus_part(g.rowptr, g.col, g.val, n)
        if cb.numel() == 0:
            cb = torch.zeros(1, dtype=torch.int32, device=DEV)
        aux = G.GraphAux(None, None, 0, 0, P(rp), P(cb), None, None)
        y = spmm(lib, use, S, d, dev(X), ctypes.addressof(aux))
        assert_exact(y.t, want, deg, label, "band-plus by hand (int32, no order), n=%d S=%d d=%d" % (n, S, d), GC.edge_rows(n))
        assert y.guards_intact()
    # no Hi-C entry at all, explicit unit values: an empty unit-entry list behind the registered dummy index array
    for n in (1, 7, 65):
        rowptr, col, val, rs = GC.bandplus_no_hic(n)
        X = GC.int_table(S, n, d, 77 + n)
        want = GC.aggregate_ref(rowptr, col, val, rs, X)
        csr = DevCsr(rowptr, col, val, rs)
        g = G.ChromGraph(n=n, nnz=int(col.size), rowptr=csr.rowptr, col=csr.col, val=csr.val, row_scale=csr.rs, rowptr_t=csr.rowptr,
                         col_t=csr.col, val_t=csr.val, symmetric=True)
        assert G.has_band_plus(g.col)
        y = spmm(lib, csr, S, d, dev(X), G.aux_ptr(g.col))
        assert_exact(y.t, want, np.diff(rowptr), lambda i: "band row, no Hi-C entry", "band-plus without Hi-C, n=%d S=%d d=%d" % (n, S, d),
                     GC.edge_rows(n))
        assert y.guards_intact()


@pytest.mark.parametrize("S,d", SD)
def test_band_aggregation(lib, S, d):
    for n in GC.BAND_N:
        h = GC.band_host(n)
        X = GC.int_table(S, n, d, 3000 + n)
        want = GC.aggregate_ref(h.rowptr, h.col, None, h.row_scale, X)
        g = G.upload(h, DEV)
        assert G.is_band(g.col)
        use = DevCsr.of(g)
        y = spmm(lib, use, S, d, dev(X), G.aux_ptr(g.col))
        assert_exact(y.t, want, np.diff(h.rowptr), lambda i: "band row", "band, n=%d S=%d d=%d" % (n, S, d), GC.edge_rows(n))
        assert y.guards_intact()


# ---- the whole-row kernels -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,d", SD + ((1, 36), (2, 36), (2, 4)))
def test_whole_row_aggregation(lib, S, d):
    """k_spmm (square, small table, hint withheld) and k_spmm_any (any width): tails around each instance's batch and
    around the 64-entry chunk, implicit and stored values, with and without a row scale"""
    for key in ("whole", "whole_small"):
        c = CASES[key]()
        X = GC.int_table(S, c.n_cols, d, 4000 + d)
        csr = DevCsr(c.rowptr, c.col, c.val, GC.inv_len_scale(c.rowptr))
        for rs in (GC.inv_len_scale(c.rowptr), None):
            csr.rs = dev(rs)
            y = spmm(lib, csr, S, d, dev(X), None)
            assert_exact(y.t, GC.aggregate_ref(c.rowptr, c.col, c.val, rs, X), c.deg, c.label,
                         "whole-row aggregation, %s, scale=%s, S=%d d=%d" % (c.name, rs is not None, S, d))
            assert y.guards_intact()


@pytest.mark.parametrize("S,d", ((2, 128), (1, 256), (2, 256), (1, 36), (2, 36)))
@pytest.mark.parametrize("shape", GC.RECT_SHAPES, ids=lambda s: "%dx%d" % s)
def test_rectangular_operators_through_the_registered_op(lib, shape, S, d):
    """torch.ops.chromegcn.spmm with n_rows != n_cols (20 000 rows: the second grid-stride trip of k_spmm's 4 096 workgroups
    of 4 waves), and its autograd backward on the transposed lists"""
    from chromegcn_amd import torch_ops  # noqa: F401  (registers the operators)
    n_rows, n_cols = shape
    for values in (None, "small"):
        c = GC.rect_case(n_rows, n_cols, values)
        X = GC.int_table(S, n_cols, d, 5000 + d)
        rt, ct, vt = GC.transpose_csr(c.rowptr, c.col, c.val, n_cols)
        a, b = DevCsr(c.rowptr, c.col, c.val), DevCsr(rt, ct, vt)
        for rs in (GC.inv_len_scale(c.rowptr), None):
            want = GC.aggregate_ref(c.rowptr, c.col, c.val, rs, X)
            y = torch.ops.chromegcn.spmm(dev(X), a.rowptr, a.col, a.val, dev(rs), b.rowptr, b.col, b.val)
            assert tuple(y.shape) == (S, n_rows, d)
            assert_exact(y, want, c.deg, c.label, "rectangular %s, scale=%s, S=%d d=%d" % (c.name, rs is not None, S, d))
            # (the operator allocates its own output: the same call through the C ABI, between guards)
            a.rs = dev(rs)
            yg = spmm(lib, a, S, d, dev(X), None, n_cols=n_cols)
            assert_exact(yg.t, want, c.deg, c.label, "rectangular %s through cgcn_spmm, scale=%s, S=%d d=%d" % (c.name, rs is not None, S, d))
            assert yg.guards_intact()
        # backward: dX = Ahat^T (diag(rs) dY); a power-of-two scale keeps the products (formed before the sums) exact
        rs2 = GC.pow2_scale(n_rows, 3)
        dY = GC.int_table(S, n_rows, d, 6000 + d)
        x = dev(X).requires_grad_(True)
        y = torch.ops.chromegcn.spmm(x, a.rowptr, a.col, a.val, dev(rs2), b.rowptr, b.col, b.val)
        y.backward(dev(dY))
        scaled = dY * rs2[None, :, None]
        want = np.stack([np.asarray(GC._int_csr(rt, ct, vt, n_rows).astype(np.float64) @ scaled[s].astype(np.float64)) for s in range(S)])
        assert np.abs(want).max() < GC.EXACT_BOUND / 4 and np.array_equal(want * 4, np.round(want * 4))   # multiples of 1/4: exact in fp32
        assert_exact(x.grad, want.astype(np.float32), np.diff(rt), lambda i: "row of the transposed list",
                     "autograd backward of rectangular %s, S=%d d=%d" % (c.name, S, d))


# ---- H of cgcn_layer_fwd -------------------------------------------------------------------------------------------------
def layer_fwd_H(lb, csr, S, d, x, aux, split):
    n = csr.n
    gen = torch.Generator(device=DEV).manual_seed(1)
    W, b = torch.randn(d, d, device=DEV, generator=gen) / d ** 0.5, torch.zeros(d, device=DEV)
    wg, cg = torch.randn(d, device=DEV, generator=gen) / d ** 0.5, torch.zeros(1, device=DEV)
    xn, z, gate = torch.empty_like(x), torch.empty_like(x), torch.empty(S, n, device=DEV)
    h = Guarded(S, n, d)
    lb.cgcn_debug_set_fwd_split_bytes(split)
    try:
        _lib.check(lb.cgcn_layer_fwd(_lib.stream_ptr(), n, S, d, P(csr.rowptr), P(csr.col), P(csr.val), P(csr.rs), P(x), P(W), P(b), P(wg), P(cg),
                                     P(xn), P(z), P(h.t), P(gate), 0.0, None, 0, None, None, 0, aux), "cgcn_layer_fwd")
        torch.cuda.synchronize()
    finally:
        lb.cgcn_debug_set_fwd_split_bytes(-1)
    assert bool(torch.isfinite(xn).all()) and bool(torch.isfinite(gate).all())
    return h


@pytest.mark.parametrize("S,d", SD)
def test_H_of_the_layer_forward_on_both_routes(lib, S, d):
    """fused route (k_layer_fwd's gather_tile: rows of 512 / 513, of 513 + 64 NW +- 1, two long rows in one tile of 16 / S
    nodes, a long row last in a partial tile): H is exact whatever the parameters.  Two-launch route: H is
    k_aggregate_sliced's own output."""
    plain, _ = hand_aux()
    for key in ("fused", "fused_small", "whole", "planted"):
        c, X, rs, want = reference(key, S, d)
        csr = DevCsr(c.rowptr, c.col, c.val, rs)
        routes = (("fused", 1 << 40), ("two-launch", 0)) if key != "planted" else (("two-launch", 0),)
        for what, split in routes:
            lib.cgcn_debug_set_fwd_split_bytes(split)
            assert lib.cgcn_debug_layer_fwd_route(c.n_rows, S, d, ctypes.addressof(plain), 0) == (0 if what == "fused" else 1)
            h = layer_fwd_H(lib, csr, S, d, dev(X), ctypes.addressof(plain), split)
            assert_exact(h.t, want, c.deg, c.label, "H of cgcn_layer_fwd, %s route, %s, S=%d d=%d" % (what, c.name, S, d))
            assert h.guards_intact()


# ---- the backward gather alone -------------------------------------------------------------------------------------------
SEED, CTR, STREAM = 99, 5, 1


def bwd_gather(lb, csr, S, d, dHs, dXn, gate, p, aux, co=None):
    """phase 2 of cgcn_layer_bwd alone (cgcn_debug_layer_bwd_phases): caller-filled dHs / dXn / gate, a zero-filled partial
    workspace (the riders then write zeros into the parameter gradients)"""
    n = csr.n
    z = torch.zeros(S, n, d, device=DEV)
    W, wg = torch.zeros(d, d, device=DEV), torch.zeros(d, device=DEV)
    dW, db, dwg, dcg = torch.ones(d, d, device=DEV), torch.ones(d, device=DEV), torch.ones(d, device=DEV), torch.ones(1, device=DEV)
    wsb = lb.cgcn_layer_bwd_workspace_bytes(n, S, d)
    ws = torch.zeros(wsb, dtype=torch.uint8, device=DEV)
    rng = torch.tensor([SEED, CTR], dtype=torch.int64, device=DEV)
    dx = Guarded(S, n, d)
    rc = lb.cgcn_debug_layer_bwd_phases(_lib.stream_ptr(), n, S, d, P(csr.rowptr), P(csr.col), P(csr.val), P(csr.rs), P(z), P(z), P(z), P(gate),
                                        P(W), P(wg), P(dXn), None, P(dx.t), P(dHs), P(dW), P(db), P(dwg), P(dcg), 0, p, P(rng) if p else None,
                                        STREAM, None, P(ws), wsb, 2, aux)
    _lib.check(rc, "cgcn_debug_layer_bwd_phases")
    torch.cuda.synchronize()
    for t in (dW, db, dwg, dcg):
        assert not bool(t.any())             # the second-stage sums of an all-zero workspace
    return dx


def bwd_inputs(S, n, d, seed):
    return GC.int_table(S, n, d, seed), GC.int_table(S, n, d, seed + 1, even=True), GC.gate_table(S, n, seed + 2)


def keep_mask(S, n, d, p):
    return None if p == 0 else dropout_ref.mask(SEED, CTR, STREAM, (S, n, d), p)


def check_bwd(lb, what, rowptr, col, val, S, d, p, aux_of, label, named=()):
    """run the backward gather over the list (rowptr, col, val) and compare with the integers"""
    n = len(rowptr) - 1
    dHs, dXn, gate = bwd_inputs(S, n, d, 7000 + n + d)
    keep = keep_mask(S, n, d, p)
    want = GC.bwd_gather_ref(rowptr, col, val, dHs, dXn, gate, keep, dropout_ref.keep_scale(p))
    csr = DevCsr(rowptr, col, val)
    aux, alive = aux_of(csr)
    dx = bwd_gather(lb, csr, S, d, dev(dHs), dev(dXn), dev(gate), p, aux)
    deg = np.diff(np.asarray(rowptr, np.int64))
    assert_exact(dx.t, want, deg, label, "backward gather, %s, S=%d d=%d p=%g" % (what, S, d, p), named)
    assert dx.guards_intact(), what
    if keep is not None:                      # dropped elements are exactly the reference's
        assert np.array_equal(dx.t.cpu().numpy()[~keep], np.zeros(int((~keep).sum()), np.float32))


@pytest.mark.parametrize("p", (0.0, 0.5))
@pytest.mark.parametrize("S,d", SD)
def test_backward_gather_alone_on_planted_rows(lib, S, d, p):
    """k_bwd_sliced: plain (int32), 16-bit and valued instances on the planted graph and on the small n; dXn even
    integers, gate in {0, 0.5, 1}, p = 0.5 (keep_scale 2, threshold 2^31): dX is exact"""
    def plain(csr):
        a, k = hand_aux()
        return ctypes.addressof(a), (a, k)

    def sixteen(csr):
        a, k = hand_aux(csr.col, sixteen=True)
        return ctypes.addressof(a), (a, k)
    for key, aux_of, what in (("planted", plain, "int32"), ("planted", sixteen, "16-bit"), ("planted_small", plain, "stored values")):
        c = CASES[key]()
        check_bwd(lib, "%s, %s" % (c.name, what), c.rowptr, c.col, c.val, S, d, p, aux_of, c.label)
    for n in GC.SMALL_N:
        for values, aux_of in ((None, sixteen), ("small", plain)):
            c = GC.small_case(n, values)
            check_bwd(lib, c.name, c.rowptr, c.col, c.val, S, d, p, aux_of, c.label)


@pytest.mark.parametrize("p", (0.0, 0.5))
@pytest.mark.parametrize("S,d", SD)
def test_backward_gather_alone_on_band_plus_and_band_graphs(lib, S, d, p):
    """k_bwd_sliced<BP> (the engine's registered decomposition) and k_bwd_band"""
    alive = []

    def registered(host):
        def f(csr):
            g = G.ChromGraph(n=csr.n, nnz=host.nnz, rowptr=csr.rowptr, col=csr.col, val=csr.val, row_scale=None, rowptr_t=csr.rowptr,
                             col_t=csr.col, val_t=csr.val, symmetric=True)
            alive.append(g)
            return G.aux_ptr(g.col), g
        return f
    for n in (7, 8, 15, 65, GC.PLANTED_N):
        h = GC.bandplus_host(n)[0]
        assert h.val is not None
        check_bwd(lib, "band-plus n=%d" % n, h.rowptr, h.col, h.val, S, d, p, registered(h), lambda i: "row of the 'both' graph",
                  GC.edge_rows(n))
        assert G.has_band_plus(alive[-1].col)
    for n in (1, 7, 33, 65, 257):
        h = GC.band_host(n)
        check_bwd(lib, "band n=%d" % n, h.rowptr, h.col, None, S, d, p, registered(h), lambda i: "band row", GC.edge_rows(n))
        assert G.is_band(alive[-1].col)


# ---- the companion range -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,d,n_main", ((1, 128, 130), (2, 128, 200), (1, 256, 130)))
def test_companion_range_of_the_backward_gather_is_exact(lib, S, d, n_main):
    """cgcn_layer_bwd_co with the planted graph (super rows, a partial last tile) as the companion; S = 1, d = 128 with a
    main problem of 3 tiles: 12 gather workgroups, so the companion range starts after 4 padding workgroups.  The companion's
    H is exact whatever the main problem's floating-point inputs."""
    assert S * d // 32 <= 8
    c, X, rs, want = reference("planted", S, d)
    co = engine_graph(c, rs)
    rowptr, col, _ = GC.planted_csr(n_main, n_main, {3: 70}, 5)
    a = GC._int_csr(rowptr, col, None, n_main)
    a = ((a + a.T) > 0).astype(np.float64)
    gm = G.upload(G.normalize_graph("hic", a, n_main), DEV)
    blocks = (S * d // 32) * ((n_main + 63) // 64)
    assert (blocks % 8 != 0) == (S == 1 and d == 128)
    gen = torch.Generator(device=DEV).manual_seed(3)
    rnd = lambda *sh: torch.randn(*sh, device=DEV, generator=gen)
    x, z, h, dxn = rnd(S, n_main, d), torch.tanh(rnd(S, n_main, d)), rnd(S, n_main, d), rnd(S, n_main, d)
    gate, W, wg = torch.rand(S, n_main, device=DEV, generator=gen), rnd(d, d) / d ** 0.5, rnd(d)
    dx, dhs = torch.empty_like(x), torch.empty_like(x)
    dW, db, dwg, dcg = torch.empty(d, d, device=DEV), torch.empty(d, device=DEV), torch.empty(d, device=DEV), torch.empty(1, device=DEV)
    wsb = lib.cgcn_layer_bwd_workspace_bytes(n_main, S, d)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    xc, H = dev(X), Guarded(S, c.n_rows, d)
    job = _lib.SpmmJob(co.n, S, d, P(co.rowptr), P(co.col), None, P(co.row_scale), P(xc), P(H.t), G.aux_ptr(co.col))
    # (the 2 049-entry row makes cgcn_spmm take the sliced route for the companion by max_row_len alone: no hook)
    assert lib.cgcn_debug_layer_bwd_co_route(n_main, S, d, P(gm.rowptr_t), P(gm.col_t), None, 1, G.aux_ptr(gm.col_t), ctypes.byref(job)) == 1
    _lib.check(lib.cgcn_layer_bwd_co(_lib.stream_ptr(), n_main, S, d, P(gm.rowptr_t), P(gm.col_t), None, P(gm.row_scale), P(x), P(z), P(h), P(gate),
                                     P(W), P(wg), P(dxn), None, P(dx), P(dhs), P(dW), P(db), P(dwg), P(dcg), 0, 0.0, None, 0, None, P(ws), wsb,
                                     None, None, G.aux_ptr(gm.col_t), ctypes.byref(job)), "cgcn_layer_bwd_co")
    torch.cuda.synchronize()
    assert_exact(H.t, want, c.deg, c.label, "companion H, S=%d d=%d" % (S, d))
    assert H.guards_intact()
    assert bool(torch.isfinite(dx).all()) and bool(torch.isfinite(dW).all())


# ---- the largest admitted table ------------------------------------------------------------------------------------------
def test_largest_admitted_table_on_the_sliced_route(lib):
    """S = 2, d = 256, n = 2^21 - 1: the table is 2^32 - 2 048 bytes, the largest spmm_check / check_shape admit
    ("32-bit byte offsets").  The addressing of every kernel on this route (cgcn_spmm -> launch_aggregate_sliced ->
    k_aggregate_sliced<2, 256, false, int, false>), read before this case was first run; the largest byte offset each forms:

      sliced_block<16>       b < 16 * 32 768 = 2^19 workgroups; per = 8 * tiles = 2^18; all int, far below 2^31.
      sliced_tile            order[r], rowptr[row], rowptr[row + 1]: int element indices < 2^21 + 1 off 64-bit pointers.
      aggregate_sliced_tile  slice_el = (slice / 8) * n * D + (slice % 8) * 32 in size_t: <= (2^21 - 1) * 256 + 224 elements.
                             lane_el = slice_el + (lane & 7) * 4 <= 2^29 - 4 elements.
                             lane_off = (unsigned)(lane_el * 4) <= 2^31 - 1 024 + 896 + 112 = 2^31 - 16 bytes: fits 32 bits.
      sliced_walk            col[kk], val[kk]: int index < nnz (about 3.2 million).
      SlicedBcast            off = ((unsigned)col << 10) + lane_off, col <= n - 1 = 2^21 - 2:
                             <= (2^31 - 2 048) + (2^31 - 16) = 2^32 - 2 064; the 16-byte load ends at 2^32 - 2 048, which
                             is the table's size exactly.  No wrap: the sum stays below 2^32 by 2 064.  The address is
                             base + (size_t)off.
      rs[i]                  int index < n.
      H store                &H[lane_el + (size_t)i * D]: size_t, <= 2^30 - 512 - 4 elements.
    n > 65 536, so no 16-bit copy can be in play (use_col16), and without stored values neither BP nor HAS_VAL.  Nothing on
    the route forms an offset that does not fit, so the limit in spmm_check is right as it stands.

    Expected values: int64 torch operations on the device for 4 096 sampled rows plus the planted ones (the last 8 rows: a
    super row, a cooperative-length row and short rows, all holding columns 0 and n - 1); every other element must at least
    not be NaN.  The table never visits the host."""
    S, d, n = 2, 256, (1 << 21) - 1
    t0 = time.time()
    gen = torch.Generator(device=DEV).manual_seed(11)
    ri = lambda lo, hi, sh, dt=torch.int64: torch.randint(lo, hi, sh, device=DEV, generator=gen, dtype=dt)
    planted = (800, 300, 3, 2, 64, 65, 9, 2)
    nreg = n - len(planted)
    deg = ri(0, 4, (nreg,))
    c0 = ri(0, n // 4, (nreg,))
    c1 = c0 + 1 + ri(0, n // 4, (nreg,))
    c2 = c1 + 1 + ri(0, n // 4, (nreg,))
    cand = torch.stack([c0, c1, c2], 1)
    cols = [cand[torch.arange(3, device=DEV)[None, :] < deg[:, None]]]
    for k, ln in enumerate(planted):         # sorted, unique, first column 0 and last column n - 1
        mid = torch.sort(torch.randperm(n - 2, device=DEV, generator=gen)[:ln - 2] + 1).values
        cols.append(torch.cat([torch.zeros(1, dtype=torch.int64, device=DEV), mid, torch.full((1,), n - 1, dtype=torch.int64, device=DEV)]))
    col64 = torch.cat(cols)
    deg_all = torch.cat([deg, torch.tensor(planted, device=DEV)])
    rowptr64 = torch.zeros(n + 1, dtype=torch.int64, device=DEV)
    rowptr64[1:] = torch.cumsum(deg_all, 0)
    assert int(rowptr64[-1]) == col64.numel() and int(col64.max()) == n - 1
    rowptr, col = rowptr64.to(torch.int32), col64.to(torch.int32)
    rs = (1.0 / deg_all.clamp(min=1).to(torch.float32)) * 0.75
    x = ri(-7, 8, (S, n, d), torch.int8).to(torch.float32)
    assert x.numel() * 4 == (1 << 32) - 2048
    y = Guarded(S, n, d)
    assert lib.cgcn_spmm(_lib.stream_ptr(), n + 1, n + 1, S, d, P(rowptr), P(col), None, P(rs), P(x), P(y.t), None) != 0   # one row more: refused
    torch.cuda.synchronize()
    t1 = time.time()
    _lib.check(lib.cgcn_spmm(_lib.stream_ptr(), n, n, S, d, P(rowptr), P(col), None, P(rs), P(x), P(y.t), None), "cgcn_spmm")
    torch.cuda.synchronize()
    t2 = time.time()
    assert y.guards_intact()
    assert not bool(torch.isnan(y.t).any())
    rows = torch.cat([torch.sort(torch.randperm(nreg, device=DEV, generator=gen)[:4096]).values, torch.arange(nreg, n, device=DEV)])
    lens = deg_all[rows]
    seg = torch.repeat_interleave(torch.arange(rows.numel(), device=DEV), lens)
    start = torch.repeat_interleave(rowptr64[rows], lens)
    within = torch.arange(seg.numel(), device=DEV) - torch.repeat_interleave(torch.cumsum(lens, 0) - lens, lens)
    nb = col64[start + within]
    for s in range(S):
        sums = torch.zeros(rows.numel(), d, dtype=torch.int64, device=DEV).index_add_(0, seg, x[s, nb].to(torch.int64))
        assert int(sums.abs().max()) < GC.EXACT_BOUND
        want = sums.to(torch.float32) * rs[rows, None]
        got = y.t[s, rows]
        bad = ~(got == want)
        if bool(bad.any()):
            i, c = (int(v) for v in torch.nonzero(bad)[0])
            raise AssertionError("largest table: %d wrong elements; first at (strand %d, row %d, column %d): got %r, want %r; the row has %d "
                                 "entries" % (int(bad.sum()), s, int(rows[i]), c, float(got[i, c]), float(want[i, c]), int(lens[i])))
    print("largest admitted table: cgcn_spmm %.3f s, whole test %.1f s" % (t2 - t1, time.time() - t0))
