"""The planted gather cases themselves (tests/gather_cases.py), without a GPU: every planted row has the stated length, every
labelled wave is what the restated rule says, every partial sum stays below 2^24 (so that fp32 is exact in any order), and
the integer reference agrees with a float64 scipy product and with a plain Python loop."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import dropout_ref
import gather_cases as GC
from chromegcn_amd import graph as G


def _square_cases():
    cs = [GC.planted_graph(None), GC.planted_graph("small"), GC.whole_row_case(None), GC.whole_row_case("small"),
          GC.fused_case(None), GC.fused_case("small")]
    cs += [GC.small_case(n, v) for n in GC.SMALL_N for v in (None, "small")]
    return cs


def _all_cases():
    return _square_cases() + [GC.index_width_case(n) for n in (65536, 65537)] + \
        [GC.rect_case(r, c, v) for r, c in GC.RECT_SHAPES for v in (None, "small")]


def _merged_both(n):
    h = GC.bandplus_host(n)[0]
    return h.rowptr, h.col, h.val, n


def _csr_lists():
    out = [(c.name, c.rowptr, c.col, c.val, c.n_cols) for c in _all_cases()]
    out += [("band_n%d" % n,) + (lambda h: (h.rowptr, h.col, h.val, n))(GC.band_host(n)) for n in GC.BAND_N]
    out += [("both_n%d" % n,) + _merged_both(n) for n in GC.BANDPLUS_SMALL_N + (GC.PLANTED_N,)]
    return out


def test_every_planted_row_has_its_length_and_the_lists_are_canonical():
    for c in _all_cases():
        deg = c.deg
        assert c.rowptr.dtype == np.int32 and c.col.dtype == np.int32 and c.rowptr[0] == 0 and c.rowptr[-1] == c.col.size
        for r, ln in c.lengths.items():
            assert deg[r] == ln, (c.name, r)
        rest = np.ones(c.n_rows, bool)
        rest[list(c.lengths)] = False
        assert deg[rest].size == 0 or deg[rest].max() <= 5, c.name
        assert c.col.min(initial=0) >= 0 and c.col.max(initial=0) < c.n_cols
        inc = np.diff(c.col.astype(np.int64)) > 0
        starts = np.zeros(c.col.size, bool)
        starts[c.rowptr[1:-1][c.rowptr[1:-1] < c.col.size]] = True
        assert np.all(inc | starts[1:]), c.name                      # strictly increasing inside every row
        for r, cols in c.forced.items():
            assert set(cols) <= set(c.col[c.rowptr[r]:c.rowptr[r + 1]].tolist()), (c.name, r)
        if c.values == "small":
            assert set(np.unique(c.val).tolist()) <= {1.0, 2.0, 3.0}
        else:
            assert c.val is None
    g = GC.planted_graph(None)
    for ln in GC.PER_ROW_LENGTHS + GC.SUPER_LENGTHS + GC.NOT_SUPER_LENGTHS + (32, 33, 96, 97, 127, 128, 129, 200):
        assert ln in g.lengths.values(), ln
    assert GC.PLANTED_N % 64 == 1 and g.lengths[GC.PLANTED_N - 1] > GC.SLICED_SUPER
    assert g.deg.max() == 2049 > GC.FWD_HUB_ROW
    f = GC.fused_case(None)
    for ln in (512, 513, 1024, 1025, 1026):
        assert ln in f.lengths.values()
    assert f.lengths[0] > GC.LONG_ROW and f.lengths[1] > GC.LONG_ROW                  # two long rows in the first tile of 8 or 16 nodes
    assert GC.FUSED_N % 16 and GC.FUSED_N % 8 and f.lengths[GC.FUSED_N - 1] > GC.LONG_ROW


def test_labelled_waves_and_super_lengths_follow_the_restated_rules():
    """If SLICED_COOP_OVERHEAD or SLICED_SUPER is retuned (and gather_cases' copies with them), this says which planted waves
    no longer take the walk they are named for."""
    for values in (None, "small"):
        c = GC.planted_graph(values)
        deg = c.deg
        seen = set()
        for r0, walk in c.waves:
            assert r0 % 8 == 0
            assert GC.walk_of_wave(deg[r0:r0 + 8]) == walk, (c.name, r0, deg[r0:r0 + 8].tolist())
            seen.add(walk)
        assert seen == {"per-row", "cooperative"}
        # the placements of the super rows
        sup = np.flatnonzero(deg > GC.SLICED_SUPER)
        tiles = sup // 64
        assert np.bincount(tiles).max() >= 2                                             # two in one tile
        assert any(r % 64 == 0 for r in sup) and any(r % 64 == 63 for r in sup)          # tile positions 0 and 63
        assert sup[-1] == GC.PLANTED_N - 1 and (GC.PLANTED_N - 1) % 64 == 0              # alone in the last, partial tile
        w = deg[64 * 4 + 16:64 * 4 + 24]
        assert GC.is_super(w[0]) and w[1] > 192 and 0 in w.tolist() and GC.walk_of_wave(w) == "cooperative"
    for ln in GC.SUPER_LENGTHS:
        assert GC.is_super(ln)
    for ln in GC.NOT_SUPER_LENGTHS + GC.PER_ROW_LENGTHS:
        assert not GC.is_super(ln)
    # the edges as derived from the rule: sm + 3 >= ceil(mx / 8)
    assert GC.walk_of_wave([0] * 7 + [32]) == "per-row" and GC.walk_of_wave([0] * 7 + [33]) == "cooperative"
    assert GC.walk_of_wave([1] * 7 + [96]) == "per-row" and GC.walk_of_wave([1] * 7 + [97]) == "cooperative"
    assert all(GC.walk_of_wave([ln] * 8) == "per-row" for ln in (200, 768))
    # the eighths of a super row: seg = ceil(ceil(len / 8) / 64) * 64 entries per wave
    eighths = lambda ln: [max(0, min(ln, (w + 1) * (-(-(-(-ln // 8)) // 64) * 64)) - w * (-(-(-(-ln // 8)) // 64) * 64)) for w in range(8)]
    assert eighths(769) == [128] * 6 + [1, 0]
    assert eighths(1024) == [128] * 8
    assert eighths(1025) == [192] * 5 + [65, 0, 0]
    assert eighths(1800) == [256] * 7 + [8]


def test_every_partial_sum_of_every_case_is_below_two_to_the_24():
    """cumulative sums of |terms| along each row's list: the last one bounds every partial sum in every order"""
    for name, rowptr, col, val, n_cols in _csr_lists():
        absval = np.ones(col.size) if val is None else np.abs(val.astype(np.float64))
        x = np.abs(GC.int_table(2, n_cols, 4, 3))            # the tables' law is per element: 4 columns of it stand for all
        assert x.max() <= 7
        cum = np.cumsum(absval * 7.0)
        start = np.concatenate([[0.0], cum])[np.asarray(rowptr[:-1], np.int64)]
        last = np.concatenate([[0.0], cum])[np.asarray(rowptr[1:], np.int64)] - start
        assert last.max() + 15 * 7 + 6 < GC.EXACT_BOUND, name
        a = sp.csr_matrix((absval, col, rowptr), shape=(len(rowptr) - 1, n_cols))
        assert (a @ x[0].astype(np.float64)).max(initial=0) <= last.max()
    assert 2049 * 7 * 3 + 15 * 7 < GC.EXACT_BOUND


def test_aggregate_ref_equals_a_float64_product_to_zero():
    for c in _all_cases():
        S, d = 2, 8
        X = GC.int_table(S, c.n_cols, d, 5)
        rs = GC.inv_len_scale(c.rowptr)
        got = GC.aggregate_ref(c.rowptr, c.col, c.val, rs, X)
        a = sp.csr_matrix((np.ones(c.col.size) if c.val is None else c.val.astype(np.float64), c.col, c.rowptr), shape=(c.n_rows, c.n_cols))
        for s in range(S):
            want64 = a @ X[s].astype(np.float64)
            assert np.array_equal(GC.int_sums(c.rowptr, c.col, c.val, X)[s].astype(np.float64), want64), c.name
            want = want64.astype(np.float32) * rs[:, None]                       # exact sum, one fp32 product
            assert np.array_equal(got[s], want), c.name
            assert np.abs(got[s].astype(np.float64) - want64 * rs.astype(np.float64)[:, None]).max(initial=0) <= \
                2.0 ** -24 * np.abs(want64 * rs.astype(np.float64)[:, None]).max(initial=0) + 1e-300
        assert got.dtype == np.float32 and not np.isnan(got).any()
    assert np.array_equal(GC.aggregate_ref(c.rowptr, c.col, c.val, None, X), GC.int_sums(c.rowptr, c.col, c.val, X).astype(np.float32))


def test_bwd_gather_ref_equals_a_plain_loop_on_forty_rows():
    n, S, d, p = 40, 2, 8, 0.5
    rowptr, col, val = GC.planted_csr(n, n, {3: 17, 20: 40, 39: 0}, 9, "small")
    dHs, dXn, gate = GC.int_table(S, n, d, 1), GC.int_table(S, n, d, 2, even=True), GC.gate_table(S, n, 3)
    assert set(np.unique(gate).tolist()) == {0.0, 0.5, 1.0} and np.all(dXn % 2 == 0) and np.abs(dXn).max() == 6
    assert dropout_ref.dropout_threshold(p) == 1 << 31 and dropout_ref.keep_scale(p) == 2.0
    keep = dropout_ref.mask(99, 5, 1, (S, n, d), p)
    for kp in (None, keep):
        got = GC.bwd_gather_ref(rowptr, col, val, dHs, dXn, gate, kp, dropout_ref.keep_scale(p))
        for s in range(S):
            for i in range(n):
                for c in range(d):
                    acc = 0
                    for k in range(rowptr[i], rowptr[i + 1]):
                        acc += int(val[k]) * int(dHs[s, col[k], c])
                    want = (1.0 - float(gate[s, i])) * float(dXn[s, i, c]) + acc
                    if kp is not None:
                        want = want * 2.0 if kp[s, i, c] else 0.0
                    assert got[s, i, c] == want
    assert 0 < keep.sum() < keep.size


def test_band_and_band_plus_cases_are_what_they_are_named():
    for n in GC.BAND_N:
        h = GC.band_host(n)
        assert G.band_halfwidth(torch.from_numpy(h.rowptr), torch.from_numpy(h.col), None, n) == GC.BAND
    empty_unit_rows = 0
    for n in GC.BANDPLUS_SMALL_N + (GC.PLANTED_N,):
        h, hubs = GC.bandplus_host(n)
        assert h.symmetric
        if h.val is None:            # (no contact at all fell outside the diagonal: the graph is the band)
            assert n == 1
            continue
        bp = G.band_plus_part(torch.from_numpy(h.rowptr), torch.from_numpy(h.col), torch.from_numpy(h.val), n)
        assert bp is not None, n
        rp, cb = bp[0].numpy().astype(np.int64), bp[1].numpy().astype(np.int64)
        # the decomposition restated: unit entries + the band window = the merged row
        a = sp.csr_matrix((h.val.astype(np.float64), h.col, h.rowptr), shape=(n, n))
        unit = sp.csr_matrix((np.ones(cb.size), cb, rp), shape=(n, n))
        band = sp.csr_matrix(G._band(n) + sp.identity(n))
        assert abs(a - unit - band).sum() == 0
        empty_unit_rows += int((np.diff(rp) == 0).sum())
        if n == GC.PLANTED_N:
            deg = np.diff(h.rowptr)
            assert tuple(int(deg[r]) for r in hubs) == GC.BANDPLUS_HUBS
            assert np.diff(rp).max() > GC.SLICED_SUPER - 2 * GC.BAND - 1
    assert empty_unit_rows > 0                                   # a row whose unit-entry list is empty
    for n in (1, 7, 65):
        rowptr, col, val, _ = GC.bandplus_no_hic(n)
        bp = G.band_plus_part(torch.from_numpy(rowptr), torch.from_numpy(col), torch.from_numpy(val), n)
        assert bp is not None and bp[1].numel() == 0 and int(bp[0].abs().sum()) == 0
    assert GC.edge_rows(8) == list(range(8)) and GC.edge_rows(100) == list(range(7)) + list(range(93, 100))


def test_tables_are_small_integers():
    t = GC.int_table(2, 500, 128, 1)
    assert t.dtype == np.float32 and t.min() == -7 and t.max() == 7 and np.array_equal(t, np.round(t))
    assert abs(float(t.mean())) < 0.05 and not np.array_equal(t[0], t[1])
    s = GC.pow2_scale(1000, 1)
    assert set(np.unique(s).tolist()) == {0.25, 0.5, 1.0, 2.0}
    r = GC.inv_len_scale(np.array([0, 0, 3, 4], np.int32))
    assert r.tolist() == [0.0, np.float32(1 / 3), 1.0]
