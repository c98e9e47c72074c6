"""tests/saliency_ref.py -- the host statement of the adjacency saliency (scripts/visualize.py:29-55) -- pinned piece against
piece, its graph builders held to the row lengths they promise, and the committed seeds of the end-to-end table checked for
what float32 alone does to the classifier head's ReLU mask.  No GPU: tests/test_gpu_saliency_cases.py holds the kernels to the
same functions."""
import numpy as np
import pytest
import torch

import saliency_ref as R
from chromegcn_amd import graph as G


def _gather(dense, rowptr, col):
    return dense[R.rows_of(rowptr), np.asarray(col, np.int64)]


def _outside_is_zero(dense, rowptr, col):
    mask = np.zeros(dense.shape, bool)
    mask[R.rows_of(rowptr), np.asarray(col, np.int64)] = True
    return bool(np.all(dense[~mask] == 0))


def _pieces_agree(A, pattern, orc32, inputs, layers):
    orc = orc32.double()
    x_f, x_r, t = inputs
    rowptr, col = pattern
    norm = R.dense_saliency(orc, A, x_f, x_r, t, layers)
    raw = R.dense_saliency(orc, A, x_f, x_r, t, layers, normalize=False)
    assert _outside_is_zero(norm, rowptr, col) and _outside_is_zero(raw, rowptr, col)
    # |adj * adj.grad| already holds the values: the pattern's normalisation of it takes val = None
    np.testing.assert_allclose(_gather(norm, rowptr, col), R.normalize_ref(rowptr, None, _gather(raw, rowptr, col)),
                               rtol=1e-12, atol=0)
    return raw


@pytest.mark.parametrize("adj_type,n", [("hic", 97), ("both", 97), ("hic", 300), ("constant", 5), ("none", 1)])
def test_dense_method_on_the_pattern_is_the_pattern_normalisation(adj_type, n):
    d, layers = 128, 3
    c = R.e2e_case(adj_type, d, layers, n)
    h = G.normalize_graph(adj_type, c["hic"], n)
    raw = _pieces_agree(c["A"], (h.rowptr, h.col), c["orc"], c["inputs"], layers)
    assert np.abs(raw).max() > 0


@pytest.mark.parametrize("kind", R.ASYM_KINDS)
def test_dense_method_on_asymmetric_operators(kind):
    c = R.asym_case(kind, 128, 1)
    h = c["host"]
    _pieces_agree(c["A"], (h.rowptr, h.col), c["orc"], c["inputs"], 1)


def test_sddmm_ref_is_the_gathered_dense_product():
    a, _ = R.planted_pattern()
    h = G.normalize_graph("hic", a, R.PLANTED_N)
    rng = np.random.RandomState(0)
    A, B = rng.randn(2, h.n, 12), rng.randn(2, h.n, 12)
    dense = A[0] @ B[0].T + A[1] @ B[1].T
    np.testing.assert_allclose(R.sddmm_ref(h.rowptr, h.col, A, B, chunk=1000), _gather(dense, h.rowptr, h.col), rtol=1e-12, atol=1e-13)


def test_normalize_ref_is_the_dense_normalisation():
    """visualize.py:49-55 on a dense matrix of |val * raw| against the pattern form, values of both signs, an empty row"""
    m = R.asymmetric_valued(60, 0.1, 3, lengths=(5,), empty_row=7)
    h = G.host_csr_from_matrix(m)
    raw = np.random.RandomState(1).randn(h.nnz)
    dense = np.zeros((60, 60))
    dense[R.rows_of(h.rowptr), h.col] = np.abs(h.val.astype(np.float64) * raw)
    adj_grad = torch.from_numpy(dense)
    s = adj_grad.sum(1); s[s == 0] = 1
    adj_grad = adj_grad / s.view(-1, 1)
    mx, _ = torch.max(adj_grad, 1); mx[mx == 0] = 1
    adj_grad = adj_grad / mx.view(-1, 1)
    np.testing.assert_allclose(R.normalize_ref(h.rowptr, h.val, raw), _gather(adj_grad.numpy(), h.rowptr, h.col), rtol=1e-14, atol=0)
    assert h.rowptr[7] == h.rowptr[8]


def test_planted_pattern_has_its_row_lengths_and_edge_columns():
    a, rows = R.planted_pattern()
    n = R.PLANTED_N
    h = G.normalize_graph("hic", a, n)
    lens = R.row_lengths(h.rowptr)
    assert tuple(int(lens[r]) for r in rows) == R.PLANTED_LENGTHS
    assert not h.symmetric and h.val is None
    assert lens.min() >= 1                                   # (every row has its diagonal)
    assert any(h.col[h.rowptr[i + 1] - 1] == n - 1 for i in range(n - 1))   # a row other than the last ends at column n - 1
    assert any(h.col[h.rowptr[i]] == 0 for i in range(1, n))                # a row other than the first points at column 0


@pytest.mark.parametrize("adj_type", ["hic", "both"])
def test_hub_graph_has_its_row_lengths(adj_type):
    hic, hubs, empty = R.hub_hic(300, adj_type, empty_row=(adj_type == "hic"))
    h = G.normalize_graph(adj_type, hic, 300)
    lens = R.row_lengths(h.rowptr)
    assert tuple(int(lens[r]) for r in hubs) == R.HUB_LENGTHS and h.symmetric
    if adj_type == "hic":
        assert lens[empty] == 0 and h.row_scale[empty] == 0 and h.val is None
    else:
        assert h.val is not None and set(np.unique(h.val)) == {1.0, 2.0}
        bp = G.band_plus_part(torch.from_numpy(h.rowptr), torch.from_numpy(h.col), torch.from_numpy(h.val), 300)
        assert bp is not None                               # the 'both' graph the feature-sliced kernels decompose
    h97 = G.normalize_graph("both", R.e2e_hic("both", 97), 97)
    assert G.band_plus_part(torch.from_numpy(h97.rowptr), torch.from_numpy(h97.col), torch.from_numpy(h97.val), 97) is None


def test_crafted_rows_have_their_roles():
    m = R.asymmetric_valued(200, 0.03, 4, lengths=(1, 64, 65, 129), empty_row=9)
    h = G.host_csr_from_matrix(m)
    raw, roles = R.craft_raw(h.rowptr, h.val, 2)
    want = R.normalize_ref(h.rowptr, h.val, raw)
    rp = h.rowptr
    assert roles["empty"] == [9]
    assert np.all(want[rp[roles["zero"]]:rp[roles["zero"] + 1]] == 0)
    assert rp[roles["single"] + 1] - rp[roles["single"]] == 1 and want[rp[roles["single"]]] == 1.0
    for i in roles["last"]:
        assert int(np.argmax(want[rp[i]:rp[i + 1]])) == rp[i + 1] - rp[i] - 1
    i, p, q = roles["tie"]
    assert want[p] == want[q] == 1.0 and p != q
    assert (raw > 0).any() and (raw < 0).any() and (h.val < 0).any()


def _flips_of_float32(c, layers):
    x_f, x_r, _ = c["inputs"]
    h32 = R.hidden_pair(c["orc"], c["A"].astype(np.float32), x_f, x_r, layers)
    h64 = R.hidden_pair(c["orc"].double(), c["A"], x_f, x_r, layers)   # (.double() converts in place: float32 runs first)
    return tuple(h > 0 for h in h32), h64


@pytest.mark.parametrize("d,layers", R.E2E_MODELS)
@pytest.mark.parametrize("adj_type", R.ADJ_TYPES)
def test_float32_alone_keeps_the_relu_mask_within_the_cap(adj_type, d, layers):
    """The committed seeds: the dense method in float32 on the host flips at most RELU_FLIPS_MAX ReLU inputs per case against
    float64, each closer to zero than RELU_MARGIN -- so a device mask that fails check_relu_mask is a wrong forward, not
    rounding.  With float32's mask handed over, float64 reproduces the float32 map within the project's bound."""
    for n in R.E2E_N:
        c = R.e2e_case(adj_type, d, layers, n)
        x_f, x_r, t = c["inputs"]
        want32 = R.dense_saliency(c["orc"], c["A"].astype(np.float32), x_f, x_r, t, layers)
        mask, h64 = _flips_of_float32(c, layers)
        R.check_relu_mask(mask, h64, "%s d=%d L=%d n=%d (float32 on the host)" % (adj_type, d, layers, n))
        want64 = R.dense_saliency(c["orc"], c["A"], x_f, x_r, t, layers, relu_mask=mask)
        np.testing.assert_allclose(want32, want64, atol=1e-4 * np.abs(want64).max(), rtol=1e-4)


@pytest.mark.parametrize("kind", R.ASYM_KINDS)
def test_float32_alone_keeps_the_relu_mask_within_the_cap_on_asymmetric_operators(kind):
    for d, layers in R.E2E_MODELS:
        c = R.asym_case(kind, d, layers)
        mask, h64 = _flips_of_float32(c, layers)
        R.check_relu_mask(mask, h64, "asymmetric %s d=%d L=%d (float32 on the host)" % (kind, d, layers))


def test_check_relu_mask_refuses_a_wrong_forward():
    h = (np.array([[0.5, -0.5, 2e-6]]), np.array([[1.0, -1.0, -3e-6]]))
    ok = (h[0] > 0, h[1] > 0)
    assert R.check_relu_mask(ok, h, "x") == 0
    near = (np.array([[True, False, False]]), np.array([[True, False, True]]))
    assert R.check_relu_mask(near, h, "x") == 2
    with pytest.raises(AssertionError, match="FORWARD"):
        R.check_relu_mask((np.array([[False, False, True]]), ok[1]), h, "x")
    many = (np.full((1, 20), 1e-7), np.full((1, 20), 1e-7))
    with pytest.raises(AssertionError, match="FORWARD"):
        R.check_relu_mask((np.zeros((1, 20), bool), many[1] > 0), many, "x")
