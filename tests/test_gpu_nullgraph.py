"""cgcn_null_graph against the host restatement (chromegcn_amd/nullgraph.py), bit for bit: rowptr, col, the entry count
and every counter, for the three models, four seeds and every case of tests/nullgraph_cases.py; then the layers above it:
null_chrom_graph, null_graph_test and the -hic_null training run."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import nullgraph_cases as K
from chromegcn_amd import ChromeGCN
from chromegcn_amd import graph as G
from chromegcn_amd import metrics as M
from chromegcn_amd import nullgraph as NG
from chromegcn_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda"


def check(out, want, info_want, model, rounds=NG.DEFAULT_ROUNDS):
    rowptr, col, sizes = out[:3]
    info = NG.info_from_sizes(sizes, rounds, model)
    nnz = int(sizes[0].item())
    assert rowptr.dtype == torch.int32 and col.dtype == torch.int32 and col.numel() >= max(nnz, 1)
    assert nnz == want.nnz == int(rowptr[-1].item())
    np.testing.assert_array_equal(rowptr.cpu().numpy(), want.indptr)
    np.testing.assert_array_equal(col[:nnz].cpu().numpy(), want.indices)
    assert not col[nnz:].any().item()
    assert info == info_want
    if len(out) == 4:
        assert out[3] == info_want


@pytest.mark.parametrize("name,model", K.CASES)
def test_bit_equal_to_the_restatement(name, model):
    g = K.graph(name)
    for seed in K.SEEDS:
        want, info = K.host(name, model, seed)
        check(NG.null_graph(g, model, seed, device=DEV, return_info=True), want, info, model)


@pytest.mark.parametrize("name,model,rounds", [("crowded", "distance", 1), ("crowded", "distance", 3), ("hic300_a", "distance", 1),
                                               ("hic300_b", "distance", 2), ("sparse300", "uniform", 1), ("big5000", "uniform", 1),
                                               ("big5000", "distance", 1)])
def test_few_rounds_leave_tokens_unplaced(name, model, rounds):
    want, info = K.host(name, model, 1, rounds)
    assert info["unplaced"] > 0
    check(NG.null_graph(K.graph(name), model, 1, rounds=rounds, device=DEV), want, info, model, rounds)


def test_pinned_known_answer_on_the_device():
    for model in K.MODELS:
        edges, info = K.PINNED[model]
        rowptr, col, sizes, got = NG.null_graph(K.graph("pinned8"), model, K.PINNED_SEED, device=DEV, return_info=True)
        a = sp.csr_matrix((np.ones(int(sizes[0])), col[:int(sizes[0])].cpu().numpy(), rowptr.cpu().numpy()), shape=(8, 8))
        assert K.upper_list(a) == edges and got == info


@pytest.mark.parametrize("model", K.MODELS)
def test_input_forms_and_streams(model):
    g = K.graph("hic300_a")
    want, info = K.host("hic300_a", model, 1)
    chrom = G.normalize_graph_device("hic", g, 300, DEV)
    assert chrom.nnz == g.nnz + 300                                      # the stored diagonal is ignored
    rp = torch.from_numpy(g.indptr.astype(np.int32)).to(DEV)
    ci = torch.from_numpy(g.indices.astype(np.int32)).to(DEV)
    longer = torch.cat([ci, torch.full((37,), 5, dtype=torch.int32, device=DEV)])   # col may be longer than rowptr[n]
    upper = sp.csr_matrix(sp.triu(g, 1))
    for form in (g, G.normalize_graph("hic", g, 300), chrom, (rp, ci), (rp, longer), upper):
        check(NG.null_graph(form, model, 1, device=DEV), want, info, model)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out = NG.null_graph((rp, ci), model, 1, device=DEV)
    side.synchronize()
    check(out, want, info, model)


def test_what_the_device_rejects():
    n2 = K.graph("n2")
    with pytest.raises(ValueError):
        NG.null_graph(n2, "uniform", device=DEV)                         # a host input: before anything is launched
    rp = torch.tensor([0, 1, 2], dtype=torch.int32, device=DEV)
    ci = torch.tensor([1, 0], dtype=torch.int32, device=DEV)
    rowptr, col, sizes = NG.null_graph((rp, ci), "uniform", device=DEV)   # a device input: flagged, the graph is empty
    assert int(sizes[0]) == 0 and int(sizes[9]) == NG.FLAG_UNSUPPORTED and rowptr.tolist() == [0, 0, 0]
    with pytest.raises(ValueError):
        NG.null_graph((rp, ci), "uniform", device=DEV, return_info=True)
    bad = torch.tensor([1, 7], dtype=torch.int32, device=DEV)            # a column outside the matrix is skipped and flagged
    rowptr, col, sizes = NG.null_graph((rp, bad), "distance", device=DEV)
    assert int(sizes[9]) == NG.FLAG_BAD_INDEX and int(sizes[1]) == 1 and rowptr.tolist() == [0, 1, 2]
    with pytest.raises(ValueError):
        NG.null_graph(K.graph("pinned8"), "random", device=DEV)
    with pytest.raises(ValueError):
        NG.null_chrom_graph(K.graph("pinned8"), "constant", device=DEV)


def same_graph(g, h):
    assert g.n == h.n and g.nnz == h.nnz and g.symmetric == h.symmetric
    np.testing.assert_array_equal(g.rowptr.cpu().numpy(), h.rowptr)
    np.testing.assert_array_equal(g.col.cpu().numpy(), h.col)
    np.testing.assert_array_equal(g.row_scale.cpu().numpy(), h.row_scale)
    assert (g.val is None) == (h.val is None)
    if h.val is not None:
        np.testing.assert_array_equal(g.val.cpu().numpy(), h.val)


@pytest.mark.parametrize("adj_type", ["hic", "both"])
@pytest.mark.parametrize("model", K.MODELS)
def test_null_chrom_graph_is_the_normalised_null_graph(adj_type, model):
    for name, seed in (("hic300_a", 2 ** 32 + 5), ("isolated", 0), ("band40", 1)):
        g = K.graph(name)
        want = G.normalize_graph(adj_type, K.host(name, model, seed)[0], g.shape[0])
        same_graph(NG.null_chrom_graph(g, adj_type, model, seed, device=DEV), want)


# ---- null_graph_test --------------------------------------------------------------------------------------------------
N, C, D, N_NULL = 300, 7, 128, 8


@pytest.fixture(scope="module")
def setup():
    torch.manual_seed(11)
    model = ChromeGCN(D, D, C, 0.2, True, 2).to(DEV)
    with torch.no_grad():
        model.batch_norm.running_mean.normal_(0.0, 0.1)
        model.batch_norm.running_var.uniform_(0.5, 1.5)
    chroms = []
    for name, seed in (("hic300_a", 5), ("hic300_b", 6)):
        f = synth.chrom_features(N, D, C, seed, positive_rate=0.2)
        assert f["target"].sum(0).min() > 0
        chroms.append((f["forward"].to(DEV), f["backward"].to(DEV), K.graph(name), f["target"].to(DEV)))
    return model, chroms


def by_hand(model, chroms, graphs):
    model.eval()
    with torch.no_grad():
        p = torch.cat([NG.strand_probs(model, torch.stack([xf, xr], 0), g) for (xf, xr, _, _), g in zip(chroms, graphs)], 0)
        m = M.multilabel_metrics(p, torch.cat([c[3] for c in chroms], 0))
    return {k: v.cpu().numpy().astype(np.float64) for k, v in m.items()}


@pytest.mark.parametrize("null_model,adj_type", [("distance", "hic"), ("degree", "both"), ("uniform", "hic")])
def test_null_graph_test_equals_the_steps_by_hand(setup, null_model, adj_type):
    model, chroms = setup
    xf, xr, hic, t = chroms[0]
    model.train()
    res = NG.null_graph_test(model, xf, xr, hic, t, null_model=null_model, n_null=N_NULL, seed=40, adj_type=adj_type, keep_null=True)
    assert model.training                                                 # the flag is restored
    assert isinstance(res, NG.NullGraphTest) and set(res.observed) == set(NG.METRICS) and res.n_null == N_NULL
    obs = by_hand(model, chroms[:1], [G.normalize_graph_device(adj_type, hic, N, DEV)])
    for k in NG.METRICS:
        np.testing.assert_array_equal(res.observed[k], obs[k])
        assert res.null[k].shape == (N_NULL, C) and res.observed[k].shape == (C,)
    for r in range(N_NULL):
        got = by_hand(model, chroms[:1], [NG.null_chrom_graph(hic, adj_type, null_model, 40 + r, device=DEV)])
        for k in NG.METRICS:
            np.testing.assert_array_equal(res.null[k][r], got[k])
    for k in NG.METRICS:
        st = NG.null_statistics(res.observed[k], res.null[k])
        for f in ("null_mean", "null_std", "z", "p"):
            np.testing.assert_array_equal(getattr(res, f)[k], st[f])
    assert np.any(res.null_std["auroc"] > 0)
    assert NG.null_graph_test(model, xf, xr, hic, t, null_model=null_model, n_null=2, seed=40, adj_type=adj_type).null is None


def test_a_full_band_is_its_own_null(setup):
    model, chroms = setup
    xf, xr, _, t = chroms[0]
    res = NG.null_graph_test(model, xf, xr, K.band(N), t, null_model="distance", n_null=N_NULL, seed=3, keep_null=True)
    for k in NG.METRICS:
        assert np.all(np.isfinite(res.observed[k]))
        np.testing.assert_array_equal(res.null[k], np.broadcast_to(res.observed[k], (N_NULL, C)))
        assert not res.null_std[k].any() and np.all(np.isnan(res.z[k])) and np.all(res.p[k] == 1.0)


def test_pooled_chromosomes_use_the_stated_seeds(setup):
    model, chroms = setup
    res = NG.null_graph_test(model, [c[0] for c in chroms], [c[1] for c in chroms], [c[2] for c in chroms],
                             [c[3] for c in chroms], null_model="distance", n_null=3, seed=100, keep_null=True)
    obs = by_hand(model, chroms, [G.normalize_graph_device("hic", c[2], N, DEV) for c in chroms])
    for r in range(3):
        graphs = [NG.null_chrom_graph(c[2], "hic", "distance", 100 + r * 2 + ci, device=DEV) for ci, c in enumerate(chroms)]
        got = by_hand(model, chroms, graphs)
        for k in NG.METRICS:
            np.testing.assert_array_equal(res.null[k][r], got[k])
    for k in NG.METRICS:
        np.testing.assert_array_equal(res.observed[k], obs[k])
    with pytest.raises(ValueError):
        NG.null_graph_test(model, [chroms[0][0]], [chroms[0][1]], [chroms[0][2], chroms[1][2]], [chroms[0][3]])


# ---- the training run -------------------------------------------------------------------------------------------------
def test_training_run_on_null_graphs(tmp_path):
    from chromegcn_amd import train
    argv = ["-synthetic", "-synthetic_chroms", "chr21,chr22", "-epochs", "1", "-hic_null", "distance", "-hic_null_seed", "9",
            "-model_name", str(tmp_path / "run")]
    opt = train.parse(argv)
    assert opt.hic_null == "distance" and opt.hic_null_seed == 9 and train.parse(["-synthetic"]).hic_null is None
    assert opt.adj_type == "hic"
    with pytest.raises(SystemExit):
        train.parse(["-synthetic", "-adj_type", "random"])              # -adj_type keeps its four choices
    plain = train.parse(argv[:5])
    _, raw = train.load_inputs(plain)
    _, graphs = train.load_inputs(opt)
    seen = 0
    for sp_ in ("train", "valid", "test"):
        assert list(graphs[sp_]) == list(raw[sp_])
        for c, (chrom, a) in enumerate(raw[sp_].items()):
            assert sp.issparse(a)
            want = G.normalize_graph("hic", NG.null_graph_host(a, "distance", 9 + c), a.shape[0])
            same_graph(graphs[sp_][chrom], want)
            assert graphs[sp_][chrom].nnz == G.normalize_graph("hic", a, a.shape[0]).nnz   # same edge count, other edges
            assert not np.array_equal(graphs[sp_][chrom].col.cpu().numpy(), G.normalize_graph("hic", a, a.shape[0]).col)
            seen += 1
    assert seen == 2
    hist = train.main(argv)
    assert len(hist) == 1 and np.isfinite(hist[0]["test"]["loss"])
