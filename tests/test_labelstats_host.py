"""Label statistics without a GPU: the numpy / scipy restatement against the definitions in plain loops, the derived numbers
against numpy, torch and scipy, the golden of the reference's summarize_data and label weights, compare_labels, the train flag
and the argument checks of the C ABI (which answer before any launch)."""
import os

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.stats
import torch

import labelstats_cases as LC
from chromegcn_amd import _build, _lib, train
from chromegcn_amd.compare import compare_labels
from chromegcn_amd.graph import HostCSR
from chromegcn_amd.labelstats import label_stats_host, label_stats_split_host

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g14_labelstats.npz")
INT_FIELDS = ("label_count", "labels_hist", "cooccurrence", "n_entries", "degree_sum", "contact_pairs")
CASES = LC.all_cases()


def _is_symmetric(graph):
    if isinstance(graph, HostCSR):
        return graph.symmetric
    return (abs(sp.csr_matrix(graph) - sp.csr_matrix(graph).T)).nnz == 0


@pytest.mark.parametrize("name,targets,graph", CASES, ids=[c[0] for c in CASES])
def test_host_restatement_equals_the_definitions(name, targets, graph):
    got = label_stats_host(targets, graph)
    want = LC.brute_force(targets, graph)
    n, C = targets.shape
    assert (got.n_windows, got.C, got.has_graph) == (n, C, graph is not None)
    for k in INT_FIELDS:
        if k in want:
            a = getattr(got, k)
            assert a.dtype == np.int64 and np.array_equal(a, want[k]), k
        else:
            assert getattr(got, k) is None
    # identities
    assert int((np.arange(C + 1) * got.labels_hist).sum()) == int(got.label_count.sum())
    assert int(got.labels_hist.sum()) == n
    assert np.array_equal(np.diag(got.cooccurrence), got.label_count)
    assert np.array_equal(got.cooccurrence, got.cooccurrence.T)
    if graph is not None and _is_symmetric(graph):
        assert np.array_equal(got.contact_pairs, got.contact_pairs.T)


def test_the_cases_hold_what_they_promise():
    by = {c[0]: c for c in CASES}
    assert len(LC.shape_cases()) == len(LC.CS) * len(LC.NS)
    _, t, _ = by["raw_scipy"]
    pos = t != 0
    assert pos[3].sum() == 0 and pos[4].sum() == pos[199].sum() == 102 and pos[:, 50].sum() == 0
    assert (by["all_ones"][1] != 0).all()              # windows with all C labels
    s = label_stats_host(*by["all_ones"][1:])
    assert s.n_entries[0] > 0 and np.all(s.contact_pairs == s.n_entries[0])
    odd = by["raw_values"][1]
    assert np.isnan(odd).any() and (odd == 0.5).any() and (odd == -1).any() and np.signbit(odd[odd == 0]).any()
    s = label_stats_host(*by["identity_only"][1:])
    assert s.n_entries[0] == 0 and not s.contact_pairs.any() and not s.degree_sum.any()
    g = by["explicit_values"][2]
    assert (g.val == 0).any() and (g.val == 2).any() and (g.val < 0).any()
    hub = sp.csr_matrix(by["hub_rows"][2])
    assert sorted(np.diff(hub.indptr).tolist())[-3:] == [64, 65, 3000]
    last = sp.csr_matrix(by["all_in_last_row"][2])
    assert np.diff(last.indptr)[:-1].sum() == 0 and last.nnz == 60
    # 'hic' adds the self loop and 'both' the band: neither self loop counts, the band's entries do
    raw, hic, both = (label_stats_host(t, by[k][2]) for k in ("raw_scipy", "normalize_hic", "normalize_both"))
    assert np.array_equal(raw.contact_pairs, hic.contact_pairs) and raw.n_entries[0] == hic.n_entries[0]
    assert both.n_entries[0] > raw.n_entries[0]


def test_pearson_equals_corrcoef():
    """the closed form on the integers against np.corrcoef of the {0, 1} matrix: within 1e-12 absolute (the closed form's worst
    difference measured on the CPU was 1.4e-15 over five cases up to n = 345 726, C = 103), NaN where it is NaN"""
    for n, C, rate, seed in ((1000, 103, 0.05, 1), (257, 12, 0.4, 2), (5000, 64, 0.01, 3)):
        t = LC.bernoulli_targets(n, C, seed, rate)
        t[:, 0] = 0                                  # a constant column: NaN row and column
        t[:, C - 1] = 1
        with np.errstate(invalid="ignore", divide="ignore"):
            want = np.corrcoef(t.astype(np.float64).T)
        got = label_stats_host(t).pearson()
        assert np.array_equal(np.isnan(got), np.isnan(want))
        assert np.isnan(got[0]).all() and np.isnan(got[:, C - 1]).all()
        ok = ~np.isnan(want)
        assert np.abs(got[ok] - want[ok]).max() <= 1e-12


def test_medians_equal_torch_median():
    for n, C, seed in ((64, 7, 1), (65, 8, 2), (1000, 103, 3), (2, 2, 4)):    # even and odd counts: the lower middle value
        t = LC.bernoulli_targets(n, C, seed, 0.3)
        s = label_stats_host(t)
        tt = torch.from_numpy(t)
        lw, sl = s.labels_per_window(), s.samples_per_label()
        assert lw["median"] == float(torch.median(tt.sum(1))) and sl["median"] == float(torch.median(tt.sum(0)))
        assert lw["max"] == float(tt.sum(1).max()) and sl["max"] == float(tt.sum(0).max())
        assert lw["mean"] == pytest.approx(float(tt.double().sum(1).mean()), rel=1e-15)
        assert sl["mean"] == pytest.approx(float(tt.double().sum(0).mean()), rel=1e-15)


def test_average_degree_and_enrichment():
    _, t, g = next(c for c in CASES if c[0] == "raw_scipy")
    s = label_stats_host(t, g)
    deg = np.asarray(sp.csr_matrix(g).sum(axis=1)).ravel()
    pos = t != 0
    avg = s.average_degree()
    assert np.isnan(avg[50]) and np.isnan(s.contact_enrichment()[50]).all() and np.isnan(s.contact_enrichment()[:, 50]).all()
    for c in (0, 7, 102):
        assert avg[c] == pytest.approx(deg[pos[:, c]].mean(), rel=1e-14)
    e = s.contact_enrichment()
    a, b = 1, 60
    assert e[a, b] == pytest.approx(s.contact_pairs[a, b] * s.n_entries[0] / (s.degree_sum[a] * s.degree_sum[b]), rel=1e-14)
    with pytest.raises(ValueError, match="graph"):
        label_stats_host(t).average_degree()


def test_add_pools():
    cases = [c for c in CASES if c[0] in ("raw_scipy", "non_symmetric", "explicit_values")]
    parts = [label_stats_host(t, g) for _, t, g in cases]
    total = parts[0] + parts[1] + parts[2]
    assert total.n_windows == 600 and total.C == 103
    for k in INT_FIELDS:
        assert np.array_equal(getattr(total, k), sum(getattr(p, k) for p in parts)), k
    pooled = label_stats_split_host([t for _, t, _ in cases], [g for _, _, g in cases])
    assert all(np.array_equal(getattr(total, k), getattr(pooled, k)) for k in INT_FIELDS)
    by_name = label_stats_split_host({c[0]: c[1] for c in cases}, {c[0]: c[2] for c in cases})
    assert all(np.array_equal(getattr(total, k), getattr(by_name, k)) for k in INT_FIELDS)
    with pytest.raises(ValueError, match="labels"):
        parts[0] + label_stats_host(np.ones((3, 5), np.float32))
    with pytest.raises(ValueError, match="graph"):
        parts[0] + label_stats_host(cases[0][1])


def test_golden_of_the_reference():
    z = np.load(GOLDEN)
    targets, lengths = z["targets"], z["lengths"].tolist()
    assert targets.shape == (300, 12) and sum(lengths) == 300 and os.path.getsize(GOLDEN) < 200 * 1024
    at, ts, gs = 0, [], []
    for i, k in enumerate(lengths):
        ts.append(targets[at:at + k])
        gs.append(sp.csr_matrix((z["val_%d" % i], z["col_%d" % i], z["rowptr_%d" % i]), shape=(k, k)))
        at += k
    assert any((g.data == 2).any() for g in gs)          # values above 1: clipped there, one entry here
    # summarize_data counts train + valid, here all three chromosomes.  The reference prints float32 tensors with four
    # decimals: half a unit of the last printed digit, 5e-5, plus the float32 rounding of its means (values below 2^7: under
    # 4e-6) bounds the difference; medians and maxima are whole numbers and exact.
    s = label_stats_split_host(ts)
    lw, sl = s.labels_per_window(), s.samples_per_label()
    got = np.array([lw["mean"], lw["median"], lw["max"], sl["mean"], sl["median"], sl["max"]])
    assert np.abs(got - z["summary"]).max() <= 5.4e-5
    assert np.array_equal(got[[1, 2, 4, 5]], z["summary"][[1, 2, 4, 5]])
    # the correlation matrix is formed from the train rows alone (util_methods.py:46-48)
    train_rows = label_stats_split_host(ts[:2])
    assert np.abs(train_rows.pearson() - z["pearson"]).max() <= 1e-12
    # the label weights over the three chromosomes: float32 sums of whole numbers below 2^24 are exact, the quotient is
    # rounded to float32 once (relative 2^-24)
    w = label_stats_split_host(ts, gs)
    assert np.array_equal(w.degree_sum, z["label_neighbor_count"].astype(np.int64))
    assert np.array_equal(w.label_count, z["label_count"].astype(np.int64))
    assert np.abs(w.average_degree() / z["label_weights"] - 1).max() <= 2.0 ** -24


def test_compare_labels_equals_scipy():
    rng = np.random.RandomState(0)
    C = 40
    a, b, w = rng.rand(C), rng.rand(C) + 0.05, rng.rand(C) * 30
    w[10] = w[11]                                         # equal weights: the stable order keeps 10 before 11
    a[3], b[7], w[20] = np.nan, np.nan, np.nan
    groups = {"tfbs": range(0, 25), "hm": range(25, 36), "dnase": range(36, 40)}
    r = compare_labels(a, b, w, groups)
    keep = np.array([i for i in range(C) if i not in (3, 7, 20)])
    assert r["dropped"].tolist() == [3, 7, 20] and np.array_equal(r["kept"], keep)
    assert np.array_equal(r["diff"], b[keep] - a[keep])
    t, p = scipy.stats.ttest_rel(a[keep], b[keep])
    assert (r["t"], r["p"]) == (float(t), float(p))
    order = keep[np.argsort(w[keep], kind="stable")]
    assert np.array_equal(r["order"], order) and list(order).index(10) + 1 == list(order).index(11)
    assert np.array_equal(r["weights_sorted"], w[order]) and np.array_equal(r["diff_sorted"], (b - a)[order])
    lr = scipy.stats.linregress(w[keep], (b - a)[keep])
    assert (r["slope"], r["intercept"], r["r"], r["p_regress"], r["stderr"]) == tuple(float(v) for v in lr[:5])
    for name, idx in groups.items():
        d = np.array([(b - a)[i] for i in idx if i in set(keep.tolist())])
        assert r["groups"][name] == {"improved": int((d >= 0).sum()), "worse": int((d < 0).sum())}
    # without weights a NaN weight drops nothing, and there is no regression
    r2 = compare_labels(a, b)
    assert r2["dropped"].tolist() == [3, 7] and "slope" not in r2 and "groups" not in r2
    r3 = compare_labels([0.5, np.nan], [0.6, 0.7], [1.0, 2.0])
    assert np.isnan(r3["t"]) and np.isnan(r3["slope"]) and r3["diff"].tolist() == pytest.approx([0.1])
    with pytest.raises(ValueError):
        compare_labels(a, b[:-1])


def test_summarize_data_flag():
    assert train.parse(["-feat_dir", "f", "-summarize_data"]).summarize_data is True
    assert train.parse(["-feat_dir", "f"]).summarize_data is False


def test_argument_checks_answer_without_launching():
    _build.build_library()
    lib = _lib.load()
    assert lib.cgcn_abi_version() == 26 == _lib.ABI_VERSION
    OK, BAD_ARG, UNSUPPORTED, WORKSPACE = 0, -1, -2, -4
    P = 0x10000                                           # never dereferenced: every call below returns before a launch
    q = lambda n, C: _lib.query("cgcn_labelstats_workspace_bytes", n=n, C=C)
    assert q(100, 103) == 100 * 2 * 8 + 192 and q(100, 64) == 1024 and q(1, 256) == 256 and q(0, 5) == 256
    assert q(10, 0) == 0 and q(10, 257) == 0 and q(-1, 5) == 0

    def windows(n=10, C=5, targets=P, workspace=P, workspace_bytes=1 << 20, label_count=P, labels_hist=P, cooccurrence=P):
        return _lib.query("cgcn_labelstats_windows", stream=None, n=n, C=C, targets=targets, workspace=workspace,
                          workspace_bytes=workspace_bytes, label_count=label_count, labels_hist=labels_hist,
                          cooccurrence=cooccurrence, accumulate=0)

    def graph(n=10, C=5, nnz=20, rowptr=P, col=P, label_bits=P, label_bits_bytes=1 << 20, degree_sum=P, contact_pairs=P,
              n_entries=P):
        return _lib.query("cgcn_labelstats_graph", stream=None, n=n, C=C, nnz=nnz, rowptr=rowptr, col=col, val=None,
                          label_bits=label_bits, label_bits_bytes=label_bits_bytes, degree_sum=degree_sum,
                          contact_pairs=contact_pairs, n_entries=n_entries, accumulate=0)

    for C in (0, 257, -3):                                # judged before any pointer
        assert windows(C=C, targets=None, label_count=None) == UNSUPPORTED
        assert graph(C=C, rowptr=None, degree_sum=None) == UNSUPPORTED
    assert graph(nnz=1 << 31, col=None) == UNSUPPORTED
    assert windows(n=-1) == BAD_ARG and graph(n=-1) == BAD_ARG and graph(nnz=-1) == BAD_ARG
    for k in ("targets", "workspace", "label_count", "labels_hist", "cooccurrence"):
        assert windows(**{k: None}) == BAD_ARG, k
    for k in ("rowptr", "col", "label_bits", "degree_sum", "contact_pairs", "n_entries"):
        assert graph(**{k: None}) == BAD_ARG, k
    assert windows(n=0, label_count=None) == BAD_ARG      # n = 0 still zeroes the outputs
    assert windows(workspace_bytes=255) == WORKSPACE and graph(label_bits_bytes=255) == WORKSPACE
    assert windows(n=100, C=103, workspace_bytes=100 * 2 * 8) == WORKSPACE
    assert OK == 0
