"""tests/ablation_ref.py -- the host statement of the label-pair ablation (scripts/visualize.py:79-119) -- pinned: the matrix
composed from the per-entry-point restatements equals the dense method, the case builders deliver the rows and counts they
promise, the committed seeds keep the entries large against the comparison's tolerance, and the float32 error of one layer is
measured (the yardstick of the layer bound in tests/test_gpu_ablation_cases.py).  No GPU."""
import numpy as np
import pytest
import torch

import ablation_ref as R

# Both sides are float64 statements of the same operation; they differ in the order of their sums (ulps of the O(1) row
# aggregates and means).  M = (base - abl) / base cancels two O(1) means, which leaves an absolute floor of a few hundred
# ulps whatever the entry's size: the relative bound alone cannot hold for an entry of 1e-9.
DENSE_TOL = dict(rtol=1e-10, atol=1e-13)
PLANTED_ROWS = (R.L_HUB, R.L_U0, R.L_V0, R.L_EMPTY, R.L_ZERO_I)
PLANTED_COLS = (R.L_ALL_NB, R.L_BUT_ONE, R.L_U0, R.L_V0, R.L_EMPTY, R.L_EVERY, R.L_ZERO_J)


def _setup(kind, layers, d=128):
    seed = 40 + 2 * R.GRAPH_KINDS.index(kind) + layers
    orc = R.make_oracle(d, R.C_FULL, layers, seed).double()
    x = R.features(R.N, d, seed)
    t, planted = R.case_targets(kind)
    g = R.graph_arrays(R.host_graph(kind), exact=True)
    return orc, x, t, planted, g


def _both(kind, layers, rows, cols):
    orc, x, t, _planted, g = _setup(kind, layers)
    want = R.reference_matrix(orc, R.dense_of(g), x[0], x[1], t, rows=rows, cols=cols)
    got, _base = R.restricted_matrix_ref(R.model_params(orc), g, x.numpy(), t.numpy(), rows=rows, cols=cols)
    removes = R.removes_something(R.host_graph(kind), R.positives(t.numpy()))
    return got, want, removes


@pytest.mark.parametrize("layers", [1, 2])
@pytest.mark.parametrize("kind", R.GRAPH_KINDS)
def test_composed_pieces_equal_the_dense_method(kind, layers):
    assert len(set(R.SUBSET_COLS)) == 40 and min(R.SUBSET_COLS) == 0 and max(R.SUBSET_COLS) == 102
    assert sorted({c >> 5 for c in R.ROW_LABELS}) == [0, 1, 2, 3]
    got, want, removes = _both(kind, layers, R.ROW_LABELS, R.SUBSET_COLS)
    np.testing.assert_allclose(got, want, **DENSE_TOL)
    block = np.zeros_like(removes)
    block[np.ix_(R.ROW_LABELS, R.SUBSET_COLS)] = True
    assert np.all(got[block & ~removes] == 0.0)
    assert np.count_nonzero(got[block & removes]) > 100


@pytest.mark.parametrize("kind", R.GRAPH_KINDS)
def test_planted_pairs_equal_the_dense_method(kind):
    """a row that loses every entry, one that keeps exactly one, pairs that remove nothing, an empty row label (NaN), an empty
    column label (0), a column label positive everywhere, and on 'coo' a row that keeps stored zeros only"""
    got, want, removes = _both(kind, 2, PLANTED_ROWS, PLANTED_COLS)
    np.testing.assert_allclose(got, want, **DENSE_TOL)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.all(np.isnan(got[R.L_EMPTY, [c for c in PLANTED_COLS if c != R.L_EMPTY]])) and got[R.L_EMPTY, R.L_EMPTY] == 0
    assert np.all(got[:, R.L_EMPTY] == 0)
    assert got[R.L_U0, R.L_V0] == 0 and got[R.L_V0, R.L_U0] == 0 and not removes[R.L_U0, R.L_V0] and not removes[R.L_V0, R.L_U0]
    assert abs(got[R.L_HUB, R.L_ALL_NB]) > 1e-4 and abs(got[R.L_HUB, R.L_BUT_ONE]) > 1e-4
    assert got[R.L_HUB, R.L_ALL_NB] != got[R.L_HUB, R.L_BUT_ONE]
    if kind == "coo":
        assert np.isfinite(got[R.L_ZERO_I, R.L_ZERO_J]) and abs(got[R.L_ZERO_I, R.L_ZERO_J]) > 1e-4


@pytest.mark.parametrize("kind", R.GRAPH_KINDS)
def test_mask_then_dense_forward_equals_the_dense_method(kind):
    orc, x, t, _planted, g = _setup(kind, 2)
    pos = R.positives(t.numpy())
    prep = R.prepare_ref(t.numpy())
    pairs = [(3, 64), (33, 102), (64, 0), (102, 33), (R.L_HUB, R.L_ALL_NB), (R.L_HUB, R.L_BUT_ONE), (R.L_U0, R.L_V0)]
    if kind == "coo":
        pairs.append((R.L_ZERO_I, R.L_ZERO_J))
    A = R.dense_of(g)
    xf, xr = x[0].double(), x[1].double()
    with torch.no_grad():
        base = R.reduce_ref(torch.stack([R._dense_forward(orc, A, xf), R._dense_forward(orc, A, xr)]).numpy(), prep)
        for i, j in pairs:
            val_out, rs_out, removed = R.mask_ref(g, pos, i, j, dtype=np.float64)
            A2 = R.masked_dense(g, val_out, rs_out)
            logits = torch.stack([R._dense_forward(orc, A2, xf), R._dense_forward(orc, A2, xr)]).numpy()
            got = R.reduce_ref(logits, prep, i, j, removed, base)
            want = R.reference_matrix(orc, A, x[0], x[1], t, rows=[i], cols=[j])[i, j]
            np.testing.assert_allclose(got, want, err_msg=str((i, j)), **DENSE_TOL)
            assert (got == 0) == (removed == 0)


# ---- the builders ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.GRAPH_KINDS)
def test_graphs_and_targets_deliver_what_they_promise(kind):
    h = R.host_graph(kind)
    t, pl = R.case_targets(kind)
    pos = R.positives(t.numpy())
    assert t.shape == (R.N, R.C_FULL) and (h.val is not None) == (kind in ("both", "coo")) and (h.row_scale is None) == (kind == "coo")
    lens = np.diff(h.rowptr)
    if kind in ("hub", "coo"):
        assert lens.max() == 200 and np.count_nonzero(lens == 0) == 1          # a long row; a row with no stored entry
    if kind == "coo":
        assert not h.symmetric and lens[R.COO_EMPTY_ROW] == 0
        z = slice(h.rowptr[R.COO_ZERO_ROW], h.rowptr[R.COO_ZERO_ROW + 1])
        assert np.count_nonzero(h.val[z] == 0) == 3 and np.count_nonzero(h.val[z]) == 3 and h.val.min() >= 0
        assert pos[:, R.L_ZERO_I].sum() == 1 and np.array_equal(pos[h.col[z], R.L_ZERO_J], h.val[z] != 0)
        np.testing.assert_allclose(np.bincount(np.repeat(np.arange(h.n), lens), h.val, h.n)[lens > 0], 1.0, rtol=1e-6)
    nb = h.col[h.rowptr[pl.hub]:h.rowptr[pl.hub + 1]]
    assert lens[pl.hub] == lens.max() and np.flatnonzero(pos[:, R.L_HUB]).tolist() == [pl.hub]
    assert pos[nb, R.L_ALL_NB].all() and pos[:, R.L_ALL_NB].sum() == len(nb)           # the hub row loses every entry
    assert np.count_nonzero(~pos[nb, R.L_BUT_ONE]) == 1 and not pos[pl.keep_one, R.L_BUT_ONE]   # ... keeps exactly one
    removes = R.removes_something(h, pos)
    assert not removes[R.L_U0, R.L_V0] and not removes[R.L_V0, R.L_U0] and removes[R.L_HUB, R.L_ALL_NB]
    assert pos[:, R.L_EMPTY].sum() == 0 and pos[:, R.L_EVERY].all()
    counts = pos.sum(0)
    assert all(counts[i] >= 2 for i in R.ROW_LABELS)
    # the restricted-route shape of the issue: 102 column labels = six blocks of 16 and one of 6; four words of bits
    assert R.prepare_ref(t.numpy()).bits.shape == (R.N, 4)
    for i in R.ROW_LABELS:
        assert len(R.layer_cols(i, 102)) == 102 and i not in R.layer_cols(i, 102)
        assert {c >> 5 for c in R.layer_cols(i, 15)} == {0, 1, 2, 3}


def test_count_builders():
    t = R.count_targets(R.N, R.HEAD_COUNTS, 1)
    assert tuple(int(c) for c in R.prepare_ref(t).counts) == (1, 2, 3, 4, 5, 8, 9, 300)
    t = R.count_targets(R.N, R.REDUCE_COUNTS, 2)
    assert tuple(int(c) for c in R.prepare_ref(t).counts) == (1, 255, 256, 257, 300)
    assert R.PREPARE_N == (1, 255, 256, 257, 300) and R.PREPARE_C == (1, 31, 32, 33, 64, 65, 103)
    p = R.prepare_ref(R.prepare_targets(257, 65))
    assert p.bits.shape == (257, 3) and p.lists.shape == (65, 257)
    for c in (0, 31, 32, 64):
        k = p.counts[c]
        assert np.all(np.diff(p.lists[c, :k]) > 0) and np.array_equal(p.ranks[c, p.lists[c, :k]], np.arange(k))
        assert np.count_nonzero(p.ranks[c] >= 0) == k
    raw = np.array([[-0.0, -1.0, 2.5, np.nan, 1e-45, 0.0]], np.float32)
    assert raw[0, 4] != 0 and R.prepare_ref(raw).bits[0, 0] == 0b011110


# ---- the tolerance cannot hide a failure ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.MATRIX_KINDS)
def test_entries_are_large_against_the_tolerance(kind):
    """the whole-matrix comparison allows atol 1e-5: at least half of the defined off-diagonal pairs that remove an entry are
    100x that, and no base_i is saturated -- by the float64 reference alone"""
    c = R.matrix_case(kind)
    pos = R.positives(c["targets"].numpy())
    counts = pos.sum(0)
    defined = (counts > 0)[:, None] & (counts > 0)[None, :] & ~np.eye(R.C_FULL, dtype=bool)
    sel = defined & R.removes_something(R.host_graph(kind), pos)
    assert sel.sum() > 9000
    assert np.mean(np.abs(c["M"][sel]) >= 1e-3) >= 0.5
    assert np.all(c["M"][defined & ~sel] == 0)
    used = c["base"][counts > 0]
    assert np.isnan(c["base"][R.L_EMPTY]) and used.min() >= 0.05 and used.max() <= 0.95


def test_bases_of_the_head_and_reduce_cases_are_not_saturated():
    for d in (128, 256):
        hc = R.head_case(d)
        assert tuple(int(k) for k in hc["prep"].counts[:9]) == R.HEAD_COUNTS + (0,)
        assert np.isnan(hc["base"][8]) and hc["base"][:8].min() >= 0.05 and hc["base"][:8].max() <= 0.95
    rc = R.reduce_case()
    assert np.isnan(rc["base"][5]) and rc["base"][:5].min() >= 0.05 and rc["base"][:5].max() <= 0.95
    for i in range(5):       # the pair entries of the reduction test are 100x the tolerance
        assert abs(R.reduce_ref(rc["logits2"], rc["prep"], i, (i + 1) % 5, 3, rc["base"])) >= 1e-3


@pytest.mark.parametrize("kind", R.GRAPH_KINDS)
def test_subset_entries_are_large_against_the_tolerance(kind):
    """the same for the composed route's pair subset"""
    got, _want, removes = _both(kind, 2, R.ROW_LABELS, R.SUBSET_COLS)
    block = np.zeros_like(removes)
    block[np.ix_(R.ROW_LABELS, R.SUBSET_COLS)] = True
    sel = block & removes & ~np.eye(R.C_FULL, dtype=bool) & np.isfinite(got)
    assert np.mean(np.abs(got[sel]) >= 1e-3) >= 0.5


# ---- what float32 alone does to a layer ------------------------------------------------------------------------------------
def test_float32_yardstick_of_the_layer():
    """layer_ref with every array and operation in float32, against float64, over every case of the GPU layer test, both
    layers.  The figure is committed as LAYER_F32_YARDSTICK; a host whose float32 BLAS sums in another order moves the maximum
    by a rounding or two, so the measurement is held to [0.5, 1.5] x the committed figure -- the bound derived from it stays"""
    worst = 0.0
    for kind, n_cols, d in R.LAYER_CASES:
        c = R.layer_case(kind, n_cols, d)
        for i, (pl, cols, inst1, _removed, inst1_f32, inst2) in c["per_label"].items():
            f1, _ = R.layer_ref(c["g"], c["x1"], c["params"][0], c["pos"], pl, cols, dtype=np.float32)
            f2, _ = R.layer_ref(c["g"], c["x2"], c["params"][1], c["pos"], pl, cols, X_inst=inst1_f32, dtype=np.float32)
            assert f1.dtype == np.float32 and f2.dtype == np.float32
            worst = max(worst, float(np.abs(f1 - inst1).max()), float(np.abs(f2 - inst2).max()))
    print("max |f32 - f64| over the instance rows: %.3e" % worst)
    assert 0.5 * R.LAYER_F32_YARDSTICK <= worst <= 1.5 * R.LAYER_F32_YARDSTICK
