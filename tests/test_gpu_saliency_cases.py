"""k_sddmm, k_saliency_rows and chromegcn_amd.saliency.adjacency_saliency against the float64 statements of
tests/saliency_ref.py (pinned on the host by tests/test_saliency_ref_host.py): every (S, d) instance of the product at planted
row lengths, past the launch's grid cap and on the transposed lists; the row normalisation with and without explicit values
on rows built for its branches; the whole saliency on all four adjacency types, the reference's own 'both' COO tensor and
asymmetric operators, at d = 128 / 256, one to four layers, on the fused and on the feature-sliced forward route."""
import types

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import chromegcn_amd as C
import saliency_ref as R
from chromegcn_amd import graph as G
from chromegcn_amd import ops
from chromegcn_amd.saliency import adjacency_saliency
from oracle import chromegcn_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
INSTANCES = [(1, 128), (2, 128), (1, 256), (2, 256)]
SDDMM_TOL = dict(atol=1e-4, rtol=1e-4)       # N(0,1) operands: sums of S * d <= 512 products, |out| ~ 20
NORM_TOL = dict(rtol=2e-6, atol=1e-7)        # only the order of the row sum differs from the reference
GRID_N = 16385 + 64                          # 4096 blocks x 4 waves = 16 384 rows per sweep of k_sddmm / k_saliency_rows


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _operands(S, n, d, seed):
    rng = np.random.RandomState(seed)
    return rng.randn(S, n, d).astype(np.float32), rng.randn(S, n, d).astype(np.float32)


def _host(g, transposed=False):
    rp, col = (g.rowptr_t, g.col_t) if transposed else (g.rowptr, g.col)
    return rp.cpu().numpy(), col.cpu().numpy()


# ---- k_sddmm ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,d", INSTANCES)
def test_sddmm_at_planted_row_lengths(S, d):
    """rows of exactly 1 .. 200 entries: both sides of the 8-row batch and of the 64-entry chunk, the clamped tail
    min(j + u, cnt - 1) at every remainder, the first and the last column of B"""
    a, rows = R.planted_pattern()
    n = R.PLANTED_N
    g = G.upload(G.normalize_graph("hic", a, n), DEV)
    rowptr, col = _host(g)
    lens = R.row_lengths(rowptr)
    assert tuple(int(lens[r]) for r in rows) == R.PLANTED_LENGTHS
    assert any(col[rowptr[i + 1] - 1] == n - 1 for i in range(n - 1)) and any(col[rowptr[i]] == 0 for i in range(1, n))
    A, B = _operands(S, n, d, 1)
    out = ops.sddmm(_dev(A), _dev(B), g).cpu().numpy()
    np.testing.assert_allclose(out, R.sddmm_ref(rowptr, col, A, B), **SDDMM_TOL)


@pytest.mark.parametrize("S,d", INSTANCES)
def test_sddmm_past_the_grid_cap_and_accumulating(S, d):
    """n = 16 449 rows on the +-7 band: the waves of the capped launch take a second row; every row is checked.  out= given:
    the product is added, bit for bit out + out"""
    h = G.normalize_graph("constant", None, GRID_N)
    g = G.upload(h, DEV)
    A, B = _operands(S, GRID_N, d, 2)
    At, Bt = _dev(A), _dev(B)
    out = ops.sddmm(At, Bt, g)
    out2 = ops.sddmm(At, Bt, g, out=out.clone())
    out, out2 = out.cpu().numpy(), out2.cpu().numpy()
    np.testing.assert_allclose(out, R.sddmm_ref(h.rowptr, h.col, A, B), **SDDMM_TOL)
    np.testing.assert_array_equal(out2, out + out)


@pytest.mark.parametrize("S,d", INSTANCES)
def test_sddmm_on_the_transposed_lists(S, d):
    n = 150
    g = G.upload(G.normalize_graph("hic", R.asymmetric_binary(n, 0.06, 3), n), DEV)
    assert not g.symmetric and g.col_t is not g.col
    A, B = _operands(S, n, d, 3)
    At, Bt = _dev(A), _dev(B)
    fwd, tr = ops.sddmm(At, Bt, g).cpu().numpy(), ops.sddmm(At, Bt, g, transposed=True).cpu().numpy()
    np.testing.assert_allclose(tr, R.sddmm_ref(*_host(g, True), A, B), **SDDMM_TOL)
    np.testing.assert_allclose(fwd, R.sddmm_ref(*_host(g), A, B), **SDDMM_TOL)
    assert fwd.shape == tr.shape and not np.array_equal(_host(g)[1], _host(g, True)[1])
    assert not np.allclose(fwd, tr, **SDDMM_TOL)


@pytest.mark.parametrize("S,d", INSTANCES)
def test_sddmm_single_row(S, d):
    g = G.upload(G.normalize_graph("hic", sp.csr_matrix((1, 1)), 1), DEV)
    A, B = _operands(S, 1, d, 4)
    out = ops.sddmm(_dev(A), _dev(B), g).cpu().numpy()
    assert out.shape == (1,)
    np.testing.assert_allclose(out, R.sddmm_ref([0, 1], [0], A, B), **SDDMM_TOL)


# ---- k_saliency_rows -------------------------------------------------------------------------------------------------------
def _hic_with_an_empty_row():
    """the planted pattern (rows of 1, 64, 65, 129 ... entries) with row 100 emptied: hic_ii = -1 cancels the identity"""
    a = R.planted_pattern()[0].tolil()
    assert 100 not in R.planted_pattern()[1]
    a[100, :] = 0
    a[100, 100] = -1.0
    return G.normalize_graph("hic", sp.csr_matrix(a), R.PLANTED_N)


def _norm_graphs():
    both = G.normalize_graph("both", R.hub_hic(300, "both", lengths=(64, 65, 129), empty_row=False)[0], 300)
    valued = G.host_csr_from_matrix(R.asymmetric_valued(200, 0.03, 4, lengths=(1, 64, 65, 129), empty_row=9))
    return {"hic": (_hic_with_an_empty_row(), True, True), "both": (both, False, False), "valued": (valued, True, True)}


def _check_normalised(rowptr, val, raw, roles=None):
    n = rowptr.shape[0] - 1
    graph = types.SimpleNamespace(n=n, rowptr=_dev(rowptr), val=None if val is None else _dev(val))
    rawt = _dev(raw)
    keep = rawt.clone()
    got_t = ops.saliency_normalize(rawt, graph)
    again = ops.saliency_normalize(rawt, graph)
    assert torch.equal(rawt, keep) and torch.equal(got_t, again)      # input untouched, same bits on a second call
    got = got_t.cpu().numpy()
    np.testing.assert_allclose(got, R.normalize_ref(rowptr, val, raw), **NORM_TOL)
    rows = R.rows_of(rowptr)
    rowmax = np.zeros(n, np.float32); np.maximum.at(rowmax, rows, got)
    assert np.all((rowmax == 1.0) | (rowmax == 0.0))
    assert got.size == 0 or (got.min() >= 0.0 and got.max() <= 1.0)
    if roles is not None:
        z = roles["zero"]
        assert rowptr[z + 1] - rowptr[z] >= 3 and np.all(got[rowptr[z]:rowptr[z + 1]] == 0.0) and rowmax[z] == 0.0
        if "single" in roles:
            assert got[rowptr[roles["single"]]] == 1.0
        for i in roles["last"]:
            assert got[rowptr[i + 1] - 1] == 1.0 and np.all(got[rowptr[i]:rowptr[i + 1] - 1] < 1.0)
        i, p, q = roles["tie"]
        assert got[p] == 1.0 and got[q] == 1.0 and np.sum(got[rowptr[i]:rowptr[i + 1]] == 1.0) == 2
        assert np.all(rowmax[np.setdiff1d(np.arange(n), roles["empty"] + [z])] == 1.0)


@pytest.mark.parametrize("explicit", [False, True], ids=["ones", "values"])
@pytest.mark.parametrize("name", ["hic", "both", "valued"])
def test_saliency_rows_on_rows_built_for_every_branch(name, explicit):
    """an empty row, a row of zero products (exactly 0), a one-entry row (exactly 1), rows of 64 / 65 / 129 entries whose
    largest product is the last one, two equal maxima -- with the graph's own values ('both': 1 and 2 with a row scale;
    'valued': negative and fractional) and with val == NULL on the same pattern; raw of both signs"""
    h, has_empty, single = _norm_graphs()[name]
    if explicit and h.val is None:            # the 'hic' pattern with values: the 'valued' set spread over it
        val = R.VALUE_SET[np.random.RandomState(6).randint(0, len(R.VALUE_SET), h.nnz)].astype(np.float32)
    else:
        val = h.val if explicit else None
    raw, roles = R.craft_raw(h.rowptr, val, 7, single=single)
    assert bool(roles["empty"]) == has_empty and (raw > 0).any() and (raw < 0).any()
    assert val is None or ((val != 1).any() and (name == "both" or (val < 0).any()))
    _check_normalised(h.rowptr, val, raw, roles)


@pytest.mark.parametrize("explicit", [False, True], ids=["ones", "values"])
def test_saliency_rows_past_the_grid_cap(explicit):
    if explicit:
        h = G.normalize_graph("both", O.random_symmetric_graph(GRID_N, 30000, 2, hic_like=True), GRID_N)
        assert h.val is not None and (h.val == 2).any()
    else:
        h = G.normalize_graph("constant", None, GRID_N)
    raw = np.random.RandomState(8).randn(h.nnz).astype(np.float32)
    _check_normalised(h.rowptr, h.val, raw)


# ---- adjacency_saliency end to end -----------------------------------------------------------------------------------------
# Scaled error max |got - want| / max |want| of the device against the float64 dense method (the device's own ReLU mask
# handed to it) over every case below -- four types + the 'both' COO + the asymmetric operators, four models, four sizes,
# normalised and not, both forward routes: 336 comparisons -- measured on an MI355X: worst 5.0e-6 ('constant', d = 128,
# three layers, n = 1, not normalised: one number, a cancelling sum), worst normalised 3.7e-6 (asymmetric valued, d = 256,
# four layers), no ReLU input on the other side of zero in any case.  The float32 dense method on the host reaches 3.1e-6.
# Not below 2.5e-6, so the bound stays the project's: atol 1e-4 * max |want|, rtol 1e-4.


@pytest.fixture
def split_forward(request):
    """route of cgcn_layer_fwd: 'fused' = built-in choice, 'split' = forced feature-sliced route (k_aggregate_sliced into H,
    then k_layer_dense), which full-size chromosomes take by default (tests/test_gpu_parity.py)"""
    from chromegcn_amd import _lib
    lib = _lib.load()
    lib.cgcn_debug_set_fwd_split_bytes(0 if request.param == "split" else -1)
    yield request.param
    lib.cgcn_debug_set_fwd_split_bytes(-1)


def _model_of(orc32, d, layers):
    model = C.ChromeGCN(d, d, R.E2E_C, 0.0, True, layers)
    model.load_state_dict(orc32.state_dict())
    return model.to(DEV).eval()


def _device_saliency(model, inputs, adj, normalize):
    """(graph, saliency, (mask of the forward strand, mask of the reverse strand)): the masks are what the torch head's
    BatchNorm was given, relu(h) > 0, forward strand first"""
    masks = []
    hook = model.batch_norm.register_forward_pre_hook(lambda mod, inp: masks.append((inp[0] > 0).cpu().numpy()))
    try:
        g, sal = adjacency_saliency(model, inputs[0].to(DEV), inputs[1].to(DEV), adj, inputs[2].to(DEV), normalize=normalize)
    finally:
        hook.remove()
    assert len(masks) == 2 and ops._saliency_tap is None
    return g, sal, tuple(masks)


def _compare(tag, model, orc64, A, inputs, adj, layers):
    """both normalize settings of one case against the float64 dense method; returns (graph, normalised saliency)"""
    x_f, x_r, t = inputs
    h64 = R.hidden_pair(orc64, A, x_f, x_r, layers)
    keep = None
    for normalize in (True, False):
        g, sal, masks = _device_saliency(model, inputs, adj, normalize)
        flips = R.check_relu_mask(masks, h64, tag)
        dense = R.dense_saliency(orc64, A, x_f, x_r, t, layers, relu_mask=masks, normalize=normalize)
        rowptr, col = _host(g)
        rows = R.rows_of(rowptr)
        want, got = dense[rows, col], sal.cpu().numpy()
        assert got.shape == want.shape == (g.nnz,)
        outside = np.ones(dense.shape, bool); outside[rows, col] = False
        assert np.all(dense[outside] == 0)                               # nothing outside the pattern
        err = R.scaled_error(got, want)
        print("E2E-ERR %s normalize=%d err=%.3e flips=%d" % (tag, normalize, err, flips))
        scale = float(np.abs(want).max()) if want.size else 0.0
        np.testing.assert_allclose(got, want, atol=1e-4 * scale, rtol=1e-4, err_msg=tag)
        if normalize:
            assert got.min() >= 0.0 and got.max() <= 1.0
            keep = (g, sal)
    return keep


E2E_KINDS = R.ADJ_TYPES + ("both_coo",)      # 'both_coo': the reference's own call, process_graph('both').cuda()


@pytest.mark.parametrize("split_forward", ["fused", "split"], indirect=True)
@pytest.mark.parametrize("d,layers", R.E2E_MODELS)
@pytest.mark.parametrize("kind", E2E_KINDS)
def test_adjacency_saliency_matches_the_float64_dense_method(kind, d, layers, split_forward):
    adj_type = "both" if kind == "both_coo" else kind
    for n in R.E2E_N:
        c = R.e2e_case(adj_type, d, layers, n)
        model = _model_of(c["orc"], d, layers)
        orc64 = c["orc"].double()
        tag = "%s d=%d L=%d n=%d %s" % (kind, d, layers, n, split_forward)
        coo = O.process_graph(adj_type, {"c": c["hic"]}, n, "c").to(DEV)
        adj = coo if kind == "both_coo" else C.process_graph(adj_type, {"c": c["hic"]}, n, "c", device=DEV)
        g, sal = _compare(tag, model, orc64, c["A"], c["inputs"], adj, layers)
        lens = R.row_lengths(_host(g)[0])
        if n == 300 and adj_type in ("hic", "both"):
            hubs, empty = R.hub_hic(300, adj_type, empty_row=(adj_type == "hic"))[1:]
            assert tuple(int(lens[r]) for r in hubs) == R.HUB_LENGTHS
            assert empty is None or lens[empty] == 0
        if kind == "both" and n >= 97:       # explicit values 1 / 2: band-plus form at n = 300, not at n = 97 (a diagonal is missing)
            assert g.val is not None and G.has_band_plus(g.col) == (n == 300)
        if kind == "both_coo" and n >= 97:   # row-normalised values, no row scale, A != A^T: the operator the guard used to refuse
            assert g.val is not None and g.row_scale is None and not g.symmetric and g.val_t is not g.val
        if kind == "constant" and n >= 97:
            assert G.is_band(g.col)
        # the torch sparse COO a reference caller hands over is recognised: same graph, same bits
        if kind in ("constant", "none") or (kind == "hic" and n != 300):
            g2, sal2, _ = _device_saliency(model, c["inputs"], coo, True)
            assert g2.val is None and torch.equal(g2.col, g.col) and torch.equal(g2.rowptr, g.rowptr)
            assert torch.equal(sal2, sal), tag


@pytest.mark.parametrize("d,layers", R.E2E_MODELS)
@pytest.mark.parametrize("kind", R.ASYM_KINDS)
def test_adjacency_saliency_on_asymmetric_operators(kind, d, layers):
    """dL/dA_ij = <dHs_i, X_j> holds for any A: the backward walks val_t, the product walks the forward pattern.
    'binary': A = diag(row_scale) pattern with pattern != pattern^T; 'valued': explicit negative and fractional values"""
    c = R.asym_case(kind, d, layers)
    model = _model_of(c["orc"], d, layers)
    g = G.upload(c["host"], DEV)
    assert not g.symmetric and (g.val is None) == (kind == "binary")
    _compare("asymmetric %s d=%d L=%d" % (kind, d, layers), model, c["orc"].double(), c["A"], c["inputs"], g, layers)


def test_saliency_tap_state():
    """two calls give the same bits; the tap is off afterwards, also after a call that raises before or inside the traced
    forward / backward"""
    d, layers, n = 128, 3, 97
    c = R.e2e_case("hic", d, layers, n)
    model = _model_of(c["orc"], d, layers)
    g = C.process_graph("hic", {"c": c["hic"]}, n, "c", device=DEV)
    x_f, x_r, t = (v.to(DEV) for v in c["inputs"])
    _, s1 = adjacency_saliency(model, x_f, x_r, g, t)
    assert ops._saliency_tap is None
    _, s2 = adjacency_saliency(model, x_f, x_r, g, t)
    assert torch.equal(s1, s2) and ops._saliency_tap is None
    with pytest.raises(RuntimeError):
        adjacency_saliency(model, x_f.cpu(), x_r.cpu(), g, t)         # features on the host: refused by the kernels' binding
    assert ops._saliency_tap is None
    with pytest.raises(RuntimeError):
        adjacency_saliency(model, x_f, x_r, g, t.cpu())               # targets on the host: the backward raises mid-way
    assert ops._saliency_tap is None
    _, s3 = adjacency_saliency(model, x_f, x_r, g, t)
    assert torch.equal(s1, s3)
