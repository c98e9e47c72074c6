"""Label statistics on the GPU (cgcn_labelstats_windows / cgcn_labelstats_graph) against the numpy / scipy restatement: counts
are exact integers, so every array is compared for equality -- nothing is excluded and there is no tolerance."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import ablation_ref as R
import labelstats_cases as LC
import chromegcn_amd as C
from chromegcn_amd import graph as G
from chromegcn_amd import metrics, train
from chromegcn_amd.labelstats import label_stats, label_stats_host, label_stats_split

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0") if torch.cuda.is_available() else None
INT_FIELDS = ("label_count", "labels_hist", "cooccurrence", "n_entries", "degree_sum", "contact_pairs")
CASES = LC.all_cases()


def _dev(t):
    return torch.from_numpy(np.ascontiguousarray(t)).to(DEV)


def _assert_equal(got, want):
    assert (got.n_windows, got.C, got.has_graph) == (want.n_windows, want.C, want.has_graph)
    for k in INT_FIELDS:
        w = getattr(want, k)
        if w is None:
            assert getattr(got, k) is None, k
            continue
        g = getattr(got, k)
        assert g.is_cuda and g.dtype == torch.int64 and tuple(g.shape) == w.shape, k
        assert torch.equal(g.cpu(), torch.from_numpy(w)), k
    h = got.host()
    assert all(np.array_equal(getattr(h, k), getattr(want, k)) for k in INT_FIELDS if getattr(want, k) is not None)


@pytest.mark.parametrize("name,targets,graph", CASES, ids=[c[0] for c in CASES])
def test_device_equals_host(name, targets, graph):
    _assert_equal(label_stats(_dev(targets), graph), label_stats_host(targets, graph))


def test_two_runs_give_the_same_arrays():
    _, t, g = next(c for c in CASES if c[0] == "hub_rows")
    td = _dev(t)
    a, b = label_stats(td, g), label_stats(td, g)
    for k in INT_FIELDS:
        assert torch.equal(getattr(a, k), getattr(b, k)), k


def test_accumulate_pools_three_chromosomes():
    cases = [c for c in CASES if c[0] in ("raw_scipy", "non_symmetric", "explicit_values")]
    ts, gs = [_dev(t) for _, t, _ in cases], [g for _, _, g in cases]
    singles = [label_stats(t, g) for t, g in zip(ts, gs)]
    pooled = label_stats_split(ts, gs)
    summed = singles[0] + singles[1] + singles[2]
    assert pooled.n_windows == summed.n_windows == 600
    for k in INT_FIELDS:
        assert torch.equal(getattr(pooled, k), getattr(summed, k)), k
        assert torch.equal(getattr(pooled, k), sum(getattr(s, k) for s in singles)), k
    by_name = label_stats_split({c[0]: t for c, t in zip(cases, ts)}, {c[0]: c[2] for c in cases})
    assert all(torch.equal(getattr(pooled, k), getattr(by_name, k)) for k in INT_FIELDS)
    windows_only = label_stats_split(ts)
    assert not windows_only.has_graph and torch.equal(windows_only.cooccurrence, pooled.cooccurrence)


@pytest.mark.parametrize("adj_type", ["hic", "both"])
def test_chrom_graph_equals_its_scipy_matrix(adj_type):
    _, t, raw = next(c for c in CASES if c[0] == "raw_scipy")
    td = _dev(t)
    from_raw = label_stats(td, raw)
    for cg in (G.upload(G.normalize_graph(adj_type, raw, raw.shape[0]), DEV), G.process_graph(adj_type, {"c": raw}, raw.shape[0], "c", DEV)):
        got = label_stats(td, cg)
        if adj_type == "hic":                      # the self loop process_graph adds is not counted
            for k in INT_FIELDS:
                assert torch.equal(getattr(got, k), getattr(from_raw, k)), k
        else:                                      # the band's entries are edges of that graph
            band = sp.csr_matrix(raw + G._band(raw.shape[0]))
            band.data[:] = 1.0
            _assert_equal(got, label_stats_host(t, band))


def test_contact_pairs_equal_the_ablations_removed_entries():
    """the entries the label-pair ablation removes for (i, j) on a 'hic' graph are the neighbour entries from P_i to P_j and
    the self loops of the windows in both: removed = contact_pairs[i, j] + |P_i and P_j|"""
    h = R.host_graph("hic")
    targets, _ = R.case_targets("hic")
    pos = R.positives(targets.numpy())
    s = label_stats(targets.to(DEV), G.upload(h, DEV)).host()
    ga = R.graph_arrays(h)
    for i in R.ROW_LABELS + (R.L_HUB, R.L_EVERY):
        for j in (0, R.L_ALL_NB, R.L_BUT_ONE, R.L_EMPTY, R.L_EVERY, 102):
            _, _, removed = R.mask_ref(ga, pos, i, j)
            assert s.contact_pairs[i, j] == removed - s.cooccurrence[i, j], (i, j)


def test_per_chromosome_metrics_equal_the_slices():
    torch.manual_seed(3)
    lengths, names = [300, 211, 64], ["chr3", "chr8", "chr21"]
    n, c = sum(lengths), 9
    probs = torch.rand(n, c, device=DEV)
    targets = (torch.rand(n, c, device=DEV) < 0.3).float()
    got = metrics.per_chromosome_metrics(probs, targets, lengths, names)
    assert list(got) == names
    at = 0
    for name, k in zip(names, lengths):
        want = metrics.compute_metrics(probs[at:at + k].clone(), targets[at:at + k].clone(), 0.0)
        for key, v in want.items():
            if key != "time":
                assert np.array_equal(np.asarray(got[name][key]), np.asarray(v), equal_nan=True), (name, key)
        at += k
    whole = metrics.compute_metrics(probs, targets, 0.0)
    assert got["chr3"]["meanAUC"] != whole["meanAUC"]          # not the reference's unsliced call
    with pytest.raises(ValueError):
        metrics.per_chromosome_metrics(probs, targets, [300, 211], ["a", "b"])


def test_cpu_tensors_and_bad_shapes_are_refused():
    t = torch.zeros(10, 5)
    with pytest.raises(RuntimeError, match="GPU"):
        label_stats(t)
    with pytest.raises(RuntimeError, match="GPU"):
        label_stats_split([t.to(DEV), t])
    with pytest.raises(RuntimeError, match="GPU"):
        label_stats(t.numpy())
    with pytest.raises(RuntimeError, match="unsupported"):
        label_stats(torch.zeros(4, 257, device=DEV))
    with pytest.raises(ValueError, match="nodes"):
        label_stats(t.to(DEV), sp.identity(11, format="csr"))
    with pytest.raises(TypeError):
        label_stats(t.to(DEV), np.eye(10))
    with pytest.raises(ValueError, match="column"):
        label_stats(t.to(DEV), C.HostCSR(n=10, rowptr=np.arange(11, dtype=np.int32), col=np.full(10, 10, np.int32), val=None,
                                         row_scale=None, symmetric=False))


def test_bool_and_integer_targets_and_empty_input():
    t = LC.bernoulli_targets(65, 70, 3, 0.2)
    want = label_stats_host(t)
    for dt in (torch.bool, torch.int32, torch.uint8, torch.float64):
        _assert_equal(label_stats(_dev(t).to(dt)), want)
    stale = label_stats(_dev(t))                    # n = 0 launches nothing and still zeroes fresh outputs
    empty = label_stats(torch.zeros(0, 70, device=DEV), sp.csr_matrix((0, 0)))
    assert stale.label_count.sum() > 0 and empty.n_windows == 0
    for k in INT_FIELDS:
        assert not getattr(empty, k).any(), k


def test_workload_shape():
    t, a = LC.workload_case()
    _assert_equal(label_stats(_dev(t), a), label_stats_host(t, a))


def test_summarize_data_prints_the_six_numbers():
    import io
    ts = {sp_: {"c%d" % i: {"target": torch.from_numpy(LC.bernoulli_targets(n, 12, 31 + n, 0.25))} for i, n in enumerate(ns)}
          for sp_, ns in (("train", (130, 65)), ("valid", (70,)), ("test", (999,)))}
    buf = io.StringIO()
    stats = train.summarize_data(ts, DEV, out=buf)
    both = torch.cat([f["target"] for sp_ in ("train", "valid") for f in ts[sp_].values()])      # the test split is not counted
    assert stats.n_windows == 265
    want = [both.sum(1).mean(), torch.median(both.sum(1)), both.sum(1).max(), both.sum(0).mean(), torch.median(both.sum(0)),
            both.sum(0).max()]
    lines = buf.getvalue().splitlines()
    assert [ln.split(":")[0] for ln in lines] == ["Mean Labels Per Sample", "Median Labels Per Sample", "Max Labels Per Sample",
                                                  "Mean Samples Per Label", "Median Samples Per Label", "Max Samples Per Label"]
    for ln, w in zip(lines, want):
        # four printed decimals (5e-5) and torch's float32 mean of values below 128 (2^-24 * 128 < 1e-5)
        assert abs(float(ln.split(":")[1]) - float(w)) <= 6e-5


def test_analyze_results_tool_writes_the_per_label_table(tmp_path):
    """tools/analyze_results.py in this process: two prediction sets, a graph pickle and the lengths give the figure's table"""
    import csv
    import importlib.util
    import json
    import os
    import pickle
    from chromegcn_amd.compare import compare_labels
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "analyze_results.py")
    spec = importlib.util.spec_from_file_location("analyze_results_tool", path)
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    lengths = {"chr8": 200, "chr21": 130}
    graphs = {"chr8": LC.random_symmetric(200, 900, 2), "chr21": LC.random_symmetric(130, 600, 10), "chrX": None}
    rng = np.random.RandomState(5)
    t = LC.bernoulli_targets(330, 12, 6, 0.3)
    t[:, 11] = 0                                                   # a label without a window: dropped, NaN in the table
    pa = np.clip(0.5 * t + 0.6 * rng.rand(330, 12), 0, 1).astype(np.float32)
    pb = np.clip(0.7 * t + 0.5 * rng.rand(330, 12), 0, 1).astype(np.float32)
    torch.save(torch.from_numpy(pa), tmp_path / "a.pt")
    np.savez(tmp_path / "b.npz", test_preds=pb, other=pa)
    np.save(tmp_path / "t.npy", t)
    (tmp_path / "lengths.json").write_text(json.dumps(lengths))
    (tmp_path / "groups.json").write_text(json.dumps({"tfbs": list(range(8)), "hm": [8, 9, 10, 11]}))
    with open(tmp_path / "graphs.pkl", "wb") as f:
        pickle.dump(graphs, f)
    tool.main(["--preds-a", str(tmp_path / "a.pt"), "--preds-b", str(tmp_path / "b.npz") + "::test_preds", "--targets",
               str(tmp_path / "t.npy"), "--lengths", str(tmp_path / "lengths.json"), "--graphs", str(tmp_path / "graphs.pkl"),
               "--groups", str(tmp_path / "groups.json"), "--out", str(tmp_path / "o" / "table.npz"), "--csv",
               str(tmp_path / "o" / "table.csv")])
    z = np.load(tmp_path / "o" / "table.npz")
    want = label_stats_host(t[:200], graphs["chr8"]) + label_stats_host(t[200:], graphs["chr21"])
    assert all(np.array_equal(z[k], getattr(want, k)) for k in INT_FIELDS)
    assert np.array_equal(z["average_degree"], want.average_degree(), equal_nan=True) and np.isnan(z["average_degree"][11])
    ma = {k: v.double().cpu().numpy() for k, v in metrics.multilabel_metrics(_dev(pa), _dev(t)).items()}
    mb = {k: v.double().cpu().numpy() for k, v in metrics.multilabel_metrics(_dev(pb), _dev(t)).items()}
    for m in ("auroc", "aupr", "recall_at_fdr"):
        r = compare_labels(ma[m], mb[m], want.average_degree())
        assert np.array_equal(z[m + "_diff"], r["diff"]) and z[m + "_dropped"].tolist() == [11]
        for k in ("t", "p", "slope", "intercept", "r", "p_regress", "stderr"):
            assert np.array_equal(float(z["%s_%s" % (m, k)]), r[k], equal_nan=True), (m, k)   # NaN: every difference equal
    assert float(z["auroc_t"]) < 0                                 # b is the better model: a - b is negative
    with open(tmp_path / "o" / "table.csv") as f:
        rows = list(csv.reader(f))
    assert rows[0][:3] == ["label", "windows", "average_degree"] and len(rows) == 13
    assert int(rows[4][1]) == int(want.label_count[3]) and float(rows[4][2]) == want.average_degree()[3]
    assert float(rows[4][5]) == mb["auroc"][3] - ma["auroc"][3]
