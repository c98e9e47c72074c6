"""The feature-sliced gathers with first-touch warming (sliced_warm, cgcn_kernels.hip).

The first SLICED_WARM_WGS = 8 workgroups of every column slice touch one word of every line of the slice before their own
tile.  The values are discarded, so the results may not change by a bit.  So: the planted integer tables and the int64
reference of tests/gather_cases.py, outputs prefilled with NaN between guard bytes, comparison by equality (the helpers of
tests/test_gpu_gather_exact.py), at the smallest shapes where the new code takes another path:

  n = 1, 63, 64, 65, 129      one to three tiles: fewer tiles than warming workgroups (the slice is dealt over the tiles there
                              are), ragged last tile
  n = 577  = 64 * 9 + 1       ten tiles per slice: warming (tile < 8) and later workgroups both occur, ragged last tile
  n = 2113 = 64 * 33 + 1      34 tiles per slice: the planted graph of gather_cases.py, whose tiles 2-4 and 33 hold super rows
                              (> 768 entries)
  n = 4097                    the warming loop's second trip (512 threads x 8 workgroups = 4 096 nodes per trip), taken by
                              one thread
  S in {1, 2} x d in {128, 256}: 4, 8, 8 and 16 slices; 16 slices run two passes, and the second pass warms its own slice
  row_order: none, the engine's (tile_sorted_rows), and p -> (37 p + 11) mod n, which moves rows across the 64-row groups
  int32 and 16-bit indices, stored values, the band-plus instance, the backward gather alone, and a backward gather with
  riders and a companion of another n (129 / 65) against the two separate launches, bit for bit."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import gather_cases as GC
import test_gpu_bwd_companion as CO
import test_gpu_gather_exact as E
from chromegcn_amd import _lib, graph as G

pytestmark = pytest.mark.gpu
DEV = "cuda"
P = _lib.ptr
SD = GC.SD
SMALL_NS = (1, 63, 64, 65, 129, 64 * 9 + 1)
WARM_WGS = 8                 # SLICED_WARM_WGS of cgcn_kernels.hip
assert (SMALL_NS[-1] + 63) // 64 > WARM_WGS
SECOND_TRIP_N = 512 * WARM_WGS + 1


@pytest.fixture
def lib():
    lb = _lib.load()
    try:
        yield lb
    finally:
        lb.cgcn_debug_set_fwd_split_bytes(-1)


@functools.lru_cache(maxsize=None)
def cold_case(n, values=None):
    """a long first row (a cooperative walk from n = 65 on), an empty last row, a 9-entry row in the middle, the rest 0-5"""
    L = {0: min(n, 70), n - 1: 0, n // 2: min(n, 9)} if n > 2 else {0: n}
    return GC.Case("cold_n%d_%s" % (n, values or "ones"), n, n, L, 300 + n, values)


@functools.lru_cache(maxsize=None)
def cold_reference(n, S, d, values=None):
    c = cold_case(n, values)
    X = GC.int_table(S, n, d, 3000 + n + 10 * S + d)
    rs = GC.inv_len_scale(c.rowptr)
    want = GC.aggregate_ref(c.rowptr, c.col, c.val, rs, X)
    for a in (X, rs, want):
        a.setflags(write=False)
    return c, X, rs, want


def orders(c):
    """(name, row_order tensor or None): natural, the engine's, and one that moves rows across the 64-row groups"""
    n = c.n_rows
    cross = (37 * np.arange(n, dtype=np.int64) + 11) % n
    assert sorted(cross.tolist()) == list(range(n))
    if n > 64:
        assert (cross // 64 != np.arange(n) // 64).any()
    return (("natural", None), ("engine", G.tile_sorted_rows(E.dev(c.deg.astype(np.int32)))),
            ("across groups", E.dev(cross.astype(np.int32))))


def aggregation_variants(lb, c, X, rs, want, S, d):
    x, csr = E.dev(X), E.DevCsr(c.rowptr, c.col, c.val, rs)
    for oname, order in orders(c):
        for sixteen in ((False,) if c.val is not None else (False, True)):
            aux, keep = E.hand_aux(csr.col, order=order, sixteen=sixteen)
            y = E.spmm(lb, csr, S, d, x, ctypes.addressof(aux), split=0)
            what = "%s, %s order, %s indices, S=%d d=%d" % (c.name, oname, "16-bit" if sixteen else "int32", S, d)
            E.assert_exact(y.t, want, c.deg, c.label, what)
            assert y.guards_intact(), what


@pytest.mark.parametrize("S,d", SD)
def test_aggregation_with_fewer_tiles_than_warming_workgroups(lib, S, d):
    for n in SMALL_NS:
        aggregation_variants(lib, *cold_reference(n, S, d), S, d)
    for n in (1, 65, 64 * 9 + 1):       # stored values: the HAS_VAL instance
        aggregation_variants(lib, *cold_reference(n, S, d, "small"), S, d)


@pytest.mark.parametrize("S,d", SD)
def test_aggregation_with_a_second_trip_of_the_warming_loop(lib, S, d):
    aggregation_variants(lib, *cold_reference(SECOND_TRIP_N, S, d), S, d)


@pytest.mark.parametrize("S,d", SD)
def test_aggregation_with_warming_and_later_workgroups_and_super_rows(lib, S, d):
    aggregation_variants(lib, *E.reference("planted", S, d), S, d)
    aggregation_variants(lib, *E.reference("planted_small", S, d), S, d)


@pytest.mark.parametrize("S,d", SD)
def test_band_plus_aggregation(lib, S, d):
    """k_aggregate_sliced<BP> through the engine's registered decomposition: n = 65 (two tiles, no row order) and n = 2 113
    (34 tiles, row order, unit lists of 885 and 985 entries: super rows)"""
    for n in (65, GC.PLANTED_N):
        h, X, want = E.both_reference(n, S, d)
        g = G.upload(h, DEV)
        assert G.has_band_plus(g.col)
        y = E.spmm(lib, E.DevCsr.of(g), S, d, E.dev(X), G.aux_ptr(g.col))
        E.assert_exact(y.t, want, np.diff(h.rowptr), lambda i: "row of the 'both' graph", "band-plus, n=%d S=%d d=%d" % (n, S, d),
                       GC.edge_rows(n))
        assert y.guards_intact()


@pytest.mark.parametrize("S,d", SD)
def test_backward_gather_alone(lib, S, d):
    """k_bwd_sliced (the riders sum an all-zero workspace): every n and order with 16-bit indices, stored values and dropout
    on the two sizes that have warming-only and warming-and-later workgroups"""
    def aux_of(order, sixteen):
        def f(csr):
            a, k = E.hand_aux(csr.col, order=order, sixteen=sixteen)
            return ctypes.addressof(a), (a, k)
        return f
    for c in [cold_case(n) for n in SMALL_NS] + [GC.planted_graph(None)]:
        for oname, order in orders(c):
            E.check_bwd(lib, "%s, %s order, 16-bit" % (c.name, oname), c.rowptr, c.col, c.val, S, d, 0.0, aux_of(order, True), c.label)
    for c in (cold_case(64 * 9 + 1, "small"), GC.planted_graph("small"), GC.planted_graph(None)):
        E.check_bwd(lib, "%s, engine order, int32, p = 0.5" % c.name, c.rowptr, c.col, c.val, S, d, 0.5, aux_of(orders(c)[1][1], False), c.label)
    h = GC.bandplus_host(GC.PLANTED_N)[0]
    alive = []

    def registered(csr):
        g = G.ChromGraph(n=csr.n, nnz=h.nnz, rowptr=csr.rowptr, col=csr.col, val=csr.val, row_scale=None, rowptr_t=csr.rowptr,
                         col_t=csr.col, val_t=csr.val, symmetric=True)
        alive.append(g)
        return G.aux_ptr(g.col), g
    E.check_bwd(lib, "band-plus n=%d" % GC.PLANTED_N, h.rowptr, h.col, h.val, S, d, 0.0, registered, lambda i: "row of the 'both' graph",
                GC.edge_rows(GC.PLANTED_N))
    assert G.has_band_plus(alive[-1].col)


@pytest.mark.parametrize("S,d", ((2, 128), (1, 128), (1, 256)))
def test_backward_gather_with_riders_and_a_companion_of_another_size(lib, S, d):
    """cgcn_layer_bwd_co, n_main = 129 (three tiles), n_co = 65 (two), the fused SGD step and the second-stage sums riding:
    dX, dHs, the gradient, parameter and momentum arenas, the dropout counter and H equal the two separate launches bit for
    bit; and on an integer table the companion's H equals the int64 reference"""
    lib.cgcn_debug_set_fwd_split_bytes(0)
    gm, gc = CO.hic_graph(129, 91), CO.hic_graph(65, 92)
    pr = CO.Problem(gm, S, gc, S, d=d, seed=9)
    CO.check_equal(lib, pr, rides=True)
    X = GC.int_table(S, 65, d, 93)
    pr.xc = E.dev(X)
    rc, out = pr.run(lib, True)
    assert rc == CO.OK
    rowptr, col = gc.rowptr.cpu().numpy(), gc.col.cpu().numpy()
    want = GC.aggregate_ref(rowptr, col, None, gc.row_scale.cpu().numpy(), X)
    E.assert_exact(out[6], want, np.diff(rowptr), lambda i: "row of the companion graph", "companion H, S=%d d=%d" % (S, d))
