"""Every kernel of csrc/cgcn_ablation.hip alone, and label_pair_ablation at the workload's label count, against the float64
statements of tests/ablation_ref.py (pinned on the host by tests/test_ablation_ref_host.py): the set-up at the edges of its
256-row chunks and 32-label words, the layer kernel at every column-block count of C = 103 on implicit, explicit, hub and
explicit-value / no-row-scale graphs, the head at wave-uneven |P_i|, the mask and the reduction of the composed route, and the
whole 103 x 103 matrix.  Integer outputs are compared exactly."""
import numpy as np
import pytest
import torch

import ablation_ref as R
import chromegcn_amd as C
from chromegcn_amd import ops
from chromegcn_amd.ablation import label_pair_ablation
from chromegcn_amd.graph import as_graph

pytestmark = pytest.mark.gpu
DEV = "cuda"
M_TOL = dict(atol=1e-5, rtol=1e-4)             # the project's bound for M (tests/test_gpu_ablation.py::_check)
# Instance rows of k_abl_layer against layer_ref: 4 x the float32 yardstick -- layer_ref evaluated in float32 differs from
# float64 by at most R.LAYER_F32_YARDSTICK = 8.62e-07 over these very cases (measured by tests/test_ablation_ref_host.py);
# the factor 4 allows for FMA contraction and the kernel's own summation order.  Bound: 3.448e-06, absolute, on rows of O(1).
LAYER_TOL = 4 * R.LAYER_F32_YARDSTICK
SENTINEL = -12345.5


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _graph(kind):
    """the device graph of R.host_graph(kind), built the way a caller builds it: process_graph, or -- 'coo' -- as_graph of a
    torch sparse COO tensor (explicit values, no row scale, stored zeros kept); the same arrays as the host statement's"""
    h = R.host_graph(kind)
    if kind == "coo":
        g = as_graph(R.coo_tensor().to(DEV), DEV)
        assert g.val is not None and g.row_scale is None
    else:
        g = C.process_graph("both" if kind == "both" else "hic", {"c": R.raw_hic(kind)}, R.N, "c", device=DEV)
        np.testing.assert_array_equal(g.row_scale.cpu().numpy(), h.row_scale)
    np.testing.assert_array_equal(g.rowptr.cpu().numpy(), h.rowptr)
    np.testing.assert_array_equal(g.col.cpu().numpy(), h.col)
    assert (g.val is None) == (h.val is None)
    if h.val is not None:
        np.testing.assert_array_equal(g.val.cpu().numpy(), h.val)
    return g


def _prepare(targets):
    return ops.ablation_prepare(_dev(np.asarray(targets, np.float32)))


# ---- cgcn_ablation_prepare -------------------------------------------------------------------------------------------------
def _check_prepare(t):
    n, c = t.shape
    bits, lists, ranks, counts = (a.cpu().numpy() for a in _prepare(t))
    want = R.prepare_ref(t)
    np.testing.assert_array_equal(counts, want.counts)
    np.testing.assert_array_equal(bits.view(np.uint32), want.bits)
    np.testing.assert_array_equal(ranks, want.ranks)
    for lab in range(c):
        np.testing.assert_array_equal(lists[lab, :counts[lab]], want.lists[lab, :counts[lab]])
    return want


@pytest.mark.parametrize("c", R.PREPARE_C)
@pytest.mark.parametrize("n", R.PREPARE_N)
def test_prepare(n, c):
    want = _check_prepare(R.prepare_targets(n, c))
    assert n == 1 or want.counts.max() > 0


def test_prepare_full_empty_and_end_rows():
    n, c = 257, 65
    t = R.prepare_targets(n, c)
    t[:, 33] = 1                               # every row
    t[:, 64] = 0                               # none
    t[:, 31] = 0
    t[0, 31] = 1                               # only row 0
    t[:, 32] = 0
    t[n - 1, 32] = 1                           # only row n - 1
    want = _check_prepare(t)
    assert want.counts[[33, 64, 31, 32]].tolist() == [n, 0, 1, 1] and want.lists[32, 0] == n - 1


def test_prepare_raw_values():
    """a target is positive iff it is != 0: -0.0 is not, NaN and the smallest denormal are"""
    row = np.array([-0.0, -1.0, 2.5, np.nan, 1e-45, 0.0], np.float32)
    assert row[4] != 0 and row[4].view(np.uint32) == 1
    t = np.zeros((40, 70), np.float32)
    t[3, :6], t[39, 32:38], t[20, 64:70] = row, row, row
    want = _check_prepare(t)
    assert want.counts[:6].tolist() == [0, 1, 1, 1, 1, 0] and want.counts[36] == 1 and want.counts[68] == 1


# ---- cgcn_ablation_layer ---------------------------------------------------------------------------------------------------
def _dev_params(p):
    return (_dev(p.W, torch.float32), _dev(p.b, torch.float32), _dev(p.wg, torch.float32),
            torch.tensor([p.cg], dtype=torch.float32, device=DEV))


@pytest.mark.parametrize("kind,n_cols,d", R.LAYER_CASES)
def test_layer(kind, n_cols, d):
    """layer 1 from X alone and layer 2 reading layer-1 instances for the neighbours in P_i and for the row itself, for a row
    label of every word of the bitmask; the removed counts exactly; the slots of the last block past n_cols untouched"""
    c = R.layer_case(kind, n_cols, d)
    g = _graph(kind)
    bits, lists, ranks, counts = _prepare(c["pos"])
    x1, x2 = _dev(c["x1"]), _dev(c["x2"])
    p1, p2 = (_dev_params(p) for p in c["params"])
    slots = (n_cols + 15) // 16 * 16
    for i, (pl, cols, inst1, removed, inst1_f32, inst2) in c["per_label"].items():
        n_pos = len(pl)
        assert n_pos == int(counts[i]) and n_pos >= 2
        cols_t = torch.tensor(cols, dtype=torch.int32, device=DEV)
        out1 = torch.full((slots, n_pos, 2, d), SENTINEL, device=DEV)
        out2 = torch.full((slots, n_pos, 2, d), SENTINEL, device=DEV)
        rem = torch.full((slots, n_pos), -7, dtype=torch.int32, device=DEV)
        ops.ablation_layer(g, x1, None, p1, bits, R.C_FULL, lists[i], ranks[i], n_pos, cols_t, n_cols, out1, rem)
        x_inst = _dev(inst1_f32)
        ops.ablation_layer(g, x2, x_inst, p2, bits, R.C_FULL, lists[i], ranks[i], n_pos, cols_t, n_cols, out2, None)
        np.testing.assert_array_equal(rem[:n_cols].cpu().numpy(), removed)
        assert bool((rem[n_cols:] == -7).all())
        for got, want, what in ((out1, inst1, "layer 1"), (out2, inst2, "layer 2")):
            assert bool((got[n_cols:] == SENTINEL).all()), what
            err = np.abs(got[:n_cols].cpu().numpy().astype(np.float64) - want).max()
            print("%s %s n_cols=%d d=%d label %d: max error %.3e (bound %.3e)" % (what, kind, n_cols, d, i, err, LAYER_TOL))
            assert err <= LAYER_TOL, what
        assert removed.sum() > 0 or n_cols == 1
        assert np.abs(inst2 - inst1).max() > 0.1       # the layers differ: a swap of their inputs cannot pass
        if n_cols > 16:                                  # ... and so do the instances 16 slots apart: the block offset shows
            assert np.abs(inst1_f32[16:] - inst1_f32[:n_cols - 16]).max() > 0.1


# ---- cgcn_ablation_head ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_cols", [1, 17])
@pytest.mark.parametrize("d", [128, 256])
def test_head(d, n_cols):
    """base mode on unablated rows and pair mode on float32 instance rows from layer_ref, |P_i| = 1 .. 9 and 300: waves
    without a position, uneven trips"""
    hc = R.head_case(d)
    c = len(R.HEAD_LABELS)
    t, prep, hp, x, want_base = hc["targets"], hc["prep"], hc["hp"], hc["x"], hc["base"]
    pos = R.positives(t)
    model = C.ChromeGCN(d, d, c, 0.0, True, 1)
    model.load_state_dict(hc["orc"].state_dict())
    model = model.to(DEV).eval()
    bits, lists, ranks, counts = _prepare(t)
    base = torch.full((c,), SENTINEL, device=DEV)
    with torch.no_grad():
        ops.ablation_head(_dev(x), None, model.batch_norm, model.out, lists, counts, -1, 0, None, 0, None, base, None, d)
    np.testing.assert_allclose(base.cpu().numpy(), want_base, equal_nan=True, **M_TOL)
    assert np.isnan(base.cpu().numpy()[8])
    base32 = np.where(np.isnan(want_base), 1.0, want_base).astype(np.float32)       # the head alone: its base is an input
    base_d = _dev(base32)
    g = R.graph_arrays(R.host_graph("hic"))
    lp = R.layer_params(d, 62)[0]
    M = torch.zeros((c, c), device=DEV)
    want = np.zeros((c, c))
    for i in range(8):
        cols = [j for j in range(c) if j != i][8:9] if n_cols == 1 else [j for j in range(c) if j != i][:n_cols]
        pl = prep.lists[i, :prep.counts[i]]
        inst, removed = R.layer_ref(g, x, lp, pos, pl, cols)
        inst32 = inst.astype(np.float32)
        with torch.no_grad():
            ops.ablation_head(None, _dev(inst32), model.batch_norm, model.out, lists, None, i, len(pl),
                              torch.tensor(cols, dtype=torch.int32, device=DEV), n_cols, _dev(removed), base_d, M, d)
        want[i] = R.head_ref(hp, prep, i, inst=inst32, removed=removed, cols=cols, base=base32.astype(np.float64))
        if n_cols == 17:
            assert removed[cols.index(8)].sum() == 0          # the empty label removes nothing
    got = M.cpu().numpy()
    np.testing.assert_allclose(got, want, **M_TOL)
    assert np.all(got[want == 0] == 0.0) and np.count_nonzero(want) >= 8 * (n_cols > 1)
    assert np.abs(want).max() > 1e-3


# ---- cgcn_ablation_mask ----------------------------------------------------------------------------------------------------
MASK_PAIRS = ((3, 64), (33, 102), (64, 0), (102, 33), (R.L_HUB, R.L_ALL_NB), (R.L_HUB, R.L_BUT_ONE), (R.L_U0, R.L_V0),
              (R.L_EVERY, R.L_EVERY), (3, R.L_EMPTY))


@pytest.mark.parametrize("kind", ["hic", "both", "coo"])
def test_mask(kind):
    h = R.host_graph(kind)
    ga = R.graph_arrays(h)
    g = _graph(kind)
    t, planted = R.case_targets(kind)
    pos = R.positives(t.numpy())
    bits = _prepare(t.numpy())[0]
    val = torch.full((h.nnz,), SENTINEL, device=DEV)
    rs = torch.full((h.n,), SENTINEL, device=DEV)
    removed = torch.full((1,), 99, dtype=torch.int32, device=DEV)      # every call resets it
    rs_in = np.ones(h.n, np.float32) if h.row_scale is None else h.row_scale
    lens = np.diff(h.rowptr)
    rows = R.S.rows_of(h.rowptr)
    seen = set()
    for i, j in MASK_PAIRS + (((R.L_ZERO_I, R.L_ZERO_J),) if kind == "coo" else ()):
        ops.ablation_mask(g, bits, R.C_FULL, i, j, val, rs, removed)
        want_val, want_rs, want_removed = R.mask_ref(ga, pos, i, j)
        assert int(removed.item()) == want_removed
        np.testing.assert_array_equal(val.cpu().numpy(), want_val)
        got_rs = rs.cpu().numpy()
        drop = pos[rows, i] & pos[h.col, j]
        lost = np.bincount(rows[drop], minlength=h.n)
        untouched, emptied = lost == 0, (lost > 0) & (lost == lens)
        np.testing.assert_array_equal(got_rs[untouched].view(np.uint32), rs_in[untouched].view(np.uint32))
        assert np.all(got_rs[emptied] == 0.0)
        for u in np.flatnonzero(~untouched & ~emptied):
            np.testing.assert_allclose(got_rs[u], want_rs[u], rtol=(lens[u] + 2) * 2.0 ** -24, atol=0)
        seen |= {"nothing"} if want_removed == 0 else set()
        seen |= {"emptied"} if emptied.any() else set()
        seen |= {"partial"} if (~untouched & ~emptied).any() else set()
    assert seen == {"nothing", "emptied", "partial"}
    assert lost[R.COO_ZERO_ROW] == 3 if kind == "coo" else True


# ---- cgcn_ablation_reduce --------------------------------------------------------------------------------------------------
def test_reduce():
    rc = R.reduce_case()
    labels, t, prep, logits, logits2, want_base = R.REDUCE_LABELS, rc["targets"], rc["prep"], rc["logits"], rc["logits2"], rc["base"]
    c = len(labels)
    _bits, lists, _ranks, counts = _prepare(t)
    lg = _dev(logits)
    base = torch.full((c,), SENTINEL, device=DEV)
    ops.ablation_reduce(lg, lists, counts, -1, 0, None, base, None)
    np.testing.assert_allclose(base.cpu().numpy(), want_base, equal_nan=True, **M_TOL)
    assert np.isnan(base.cpu().numpy()[5])
    # pair mode: the mean over P_i of other logits, against a base that is an input
    lg2 = _dev(logits2)
    base32 = np.where(np.isnan(want_base), 1.0, want_base).astype(np.float32)
    base_d = _dev(base32)
    M = torch.full((c, c), SENTINEL, device=DEV)
    for i in range(5):
        j, j0 = (i + 1) % 5, (i + 2) % 5
        ops.ablation_reduce(lg2, lists, counts, i, j, torch.tensor([3], dtype=torch.int32, device=DEV), base_d, M)
        ops.ablation_reduce(lg2, lists, counts, i, j0, torch.tensor([0], dtype=torch.int32, device=DEV), base_d, M)
        got = M.cpu().numpy()
        want = R.reduce_ref(logits2, prep, i, j, 3, base32.astype(np.float64))
        assert abs(want) > 1e-3
        np.testing.assert_allclose(got[i, j], want, err_msg="|P_i| = %d" % labels[i], **M_TOL)
        assert got[i, j0] == 0.0
    assert np.count_nonzero(M.cpu().numpy() == SENTINEL) == c * c - 10


# ---- the whole matrix at the workload's label count ----------------------------------------------------------------------
def _check(got, want):
    np.testing.assert_allclose(got, want, **M_TOL)
    assert np.array_equal(np.isnan(got), np.isnan(want))


def _matrix_setup(kind):
    c = R.matrix_case(kind)
    model = C.ChromeGCN(R.MATRIX_D, R.MATRIX_D, R.C_FULL, 0.0, True, R.MATRIX_LAYERS)
    model.load_state_dict(c["orc"].state_dict())
    adj = R.coo_tensor().to(DEV) if kind == "coo" else _graph(kind)
    return c, model.to(DEV).eval(), c["x"][0].to(DEV), c["x"][1].to(DEV), adj, c["targets"].to(DEV)


@pytest.mark.parametrize("kind", R.MATRIX_KINDS)
def test_whole_matrix_restricted(kind):
    """C = 103, n = 300, rate 0.05, L = 2, d = 128, all 10 506 pairs: n_cols = 102 per row label (seven column blocks, the
    last of 6), four words of bits; 'coo': the torch sparse COO tensor a reference caller passes, stored zeros included"""
    c, model, x_f, x_r, adj, tg = _matrix_setup(kind)
    M, base = label_pair_ablation(model, x_f, x_r, adj, tg, route="restricted", return_base=True)
    _check(M.cpu().numpy(), c["M"])
    np.testing.assert_allclose(base.cpu().numpy(), c["base"], equal_nan=True, **M_TOL)
    assert np.array_equal(np.isnan(base.cpu().numpy()), np.isnan(c["base"]))
    if kind == "coo":
        assert np.isfinite(c["M"][R.L_ZERO_I, R.L_ZERO_J]) and abs(c["M"][R.L_ZERO_I, R.L_ZERO_J]) > 1e-4


@pytest.mark.parametrize("kind", R.MATRIX_KINDS)
def test_pair_subset_composed(kind):
    """the composed route (one forward per pair) on row labels of every word x 40 column labels, and on the planted pairs:
    a row that loses everything, one that keeps one entry, pairs that remove nothing, 'coo': a row that keeps stored zeros"""
    c, model, x_f, x_r, adj, tg = _matrix_setup(kind)
    for rows, cols in ((R.ROW_LABELS, R.SUBSET_COLS),
                       ((R.L_HUB, R.L_U0, R.L_ZERO_I, R.L_EMPTY), (R.L_ALL_NB, R.L_BUT_ONE, R.L_V0, R.L_ZERO_J))):
        M, base = label_pair_ablation(model, x_f, x_r, adj, tg, rows=rows, cols=cols, route="composed", return_base=True)
        want = np.zeros_like(c["M"])
        want[np.ix_(rows, cols)] = c["M"][np.ix_(rows, cols)]
        _check(M.cpu().numpy(), want)
        np.testing.assert_allclose(base.cpu().numpy(), c["base"], equal_nan=True, **M_TOL)
    assert M[R.L_U0, R.L_V0].item() == 0.0 and abs(want[R.L_HUB, R.L_ALL_NB]) > 1e-4
