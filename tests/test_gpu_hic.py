"""The top-K Hi-C contact graph built on the device (csrc/cgcn_hic.hip, chromegcn_amd/hic.py) against the numpy restatement
build_hic_graph_host, which tests/test_hic_host.py ties to the reference's own step 7.  The graph is structure: every
comparison is exact (rowptr and col identical, row_scale bitwise equal to the device normaliser's on the host-built matrix)."""
import types

import numpy as np
import pytest
import torch

from chromegcn_amd import ChromeGCN, _lib, graph as G, hic, synth
from chromegcn_amd.finetune import finetune

from test_hic_host import golden_cases

pytestmark = pytest.mark.gpu
DEV = "cuda"
BAD_ARG, UNSUPPORTED, WORKSPACE = -1, -2, -4
ADJ_TYPES = ("hic", "constant", "both", "none")


def assert_same_graph(g, want, what):
    assert (g.n, g.nnz, g.symmetric) == (want.n, want.nnz, want.symmetric), what
    assert torch.equal(g.rowptr, want.rowptr) and torch.equal(g.col, want.col), what
    assert torch.equal(g.row_scale.view(torch.int32), want.row_scale.view(torch.int32)), what      # bitwise
    assert (g.val is None) == (want.val is None) and (g.val is None or torch.equal(g.val, want.val)), what


def check(args, adj_types=("hic",), contacts=None, what=""):
    """device build == host build for the arguments of build_hic_graph_host; returns the raw host matrix"""
    a = hic.build_hic_graph_host(**args)
    n = a.shape[0]
    src = contacts if contacts is not None else args["pos1"]
    g, raw = hic.build_hic_graph(src, args["pos2"], args["count"], args["norm"], args["resolution_bp"], args["window_start"],
                                 args["hic_edges"], adj_type=adj_types[0], device=DEV, return_raw=True)
    assert raw.shape == a.shape and np.array_equal(raw.indptr, a.indptr) and np.array_equal(raw.indices, a.indices), what
    assert raw.has_sorted_indices and np.all(raw.data == 1.0), what
    assert_same_graph(g, G.normalize_graph_device(adj_types[0], a, n, DEV), what)
    for t in adj_types[1:]:
        g = hic.build_hic_graph(src, args["pos2"], args["count"], args["norm"], args["resolution_bp"], args["window_start"],
                                args["hic_edges"], adj_type=t, device=DEV)
        assert_same_graph(g, G.normalize_graph_device(t, a, n, DEV), (what, t))
    return a


@pytest.mark.timeout(600)
def test_golden_cases_of_the_reference_for_every_adj_type(golden):
    for c, args, adj, tie in golden_cases(golden):
        a = check(args, ADJ_TYPES if args["window_start"].size >= 7 else ("hic", "none"), what="golden case %d" % c)
        assert np.array_equal(np.asarray(a.todense()), adj.astype(np.float64)), c


def _sized(chrom):
    r = synth.raw_contacts(chrom)
    return r, hic.HicContacts(r["pos1"], r["pos2"], r["count"], DEV)


def _args(r, norm, edges):
    return dict(pos1=r["pos1"], pos2=r["pos2"], count=r["count"], norm=r["norm"] if norm else None,
                resolution_bp=r["resolution_bp"], window_start=r["window_start"], hic_edges=edges)


@pytest.mark.timeout(900)
def test_chr21_size_contacts_norm_and_budgets():
    r, c = _sized("chr21")
    s = c.survivors(r["window_start"])
    assert s == hic.survivor_values(r["pos1"], r["pos2"], r["count"], None, 1000, r["window_start"])[3].size > 250000
    for norm in (False, True):
        for edges in (250000, 500000, 1000000, 2 * s + 2):             # the last: K larger than the survivor count
            check(_args(r, norm, edges), ADJ_TYPES if edges == 500000 else ("hic",), contacts=c,
                  what=("chr21", norm, edges))


@pytest.mark.timeout(1200)
def test_chr1_size_contacts_norm_and_budgets():
    r, c = _sized("chr1")
    assert c.survivors(r["window_start"]) > 500000
    for norm in (False, True):
        for edges in (250000, 500000, 1000000):
            check(_args(r, norm, edges), contacts=c, what=("chr1", norm, edges))


@pytest.mark.timeout(600)
def test_two_builds_are_bitwise_equal_and_a_sweep_equals_fresh_builds():
    r, c = _sized("chr21")
    graphs = {}
    for edges in (250000, 500000, 1000000):
        g = c.build(r["norm"], 1000, r["window_start"], edges)
        again = c.build(r["norm"], 1000, r["window_start"], edges)
        fresh = hic.build_hic_graph(r["pos1"], r["pos2"], r["count"], r["norm"], 1000, r["window_start"], edges, device=DEV)
        assert_same_graph(again, g, edges)
        assert_same_graph(fresh, g, edges)
        graphs[edges] = g
    def pairs(g):
        rows = torch.repeat_interleave(torch.arange(g.n, device=DEV), (g.rowptr[1:] - g.rowptr[:-1]).long())
        return set((rows * g.n + g.col.long()).tolist())
    small, big = pairs(graphs[250000]), pairs(graphs[500000])
    assert small < big and len(big) > len(small) > graphs[250000].n


@pytest.mark.timeout(600)
def test_degenerate_inputs():
    r = synth.raw_contacts("chr21")
    ws, e = r["window_start"], np.zeros(0, np.int32)
    few = slice(0, 5000)
    base = dict(norm=r["norm"], resolution_bp=1000, hic_edges=1000)
    # M = 0
    check(dict(pos1=e, pos2=e, count=np.zeros(0), window_start=ws, **base), ADJ_TYPES, what="M = 0")
    # zero survivors: windows that no record touches; no window at all; only pos1 == pos2 records
    off = (ws[:50] + 1).astype(np.int32)
    check(dict(pos1=r["pos1"][few], pos2=r["pos2"][few], count=r["count"][few], window_start=off, **base), ADJ_TYPES,
          what="no survivor")
    check(dict(pos1=r["pos1"][few], pos2=r["pos2"][few], count=r["count"][few], window_start=e, **base), ("hic",), what="N = 0")
    check(dict(pos1=ws[:300], pos2=ws[:300], count=np.ones(300), window_start=ws, **base), ("hic",), what="diagonal only")
    # a budget of one record and of none; float32 counts are widened
    a = dict(pos1=r["pos1"], pos2=r["pos2"], count=r["count"].astype(np.float32), window_start=ws, norm=None, resolution_bp=1000)
    check(dict(hic_edges=2, **a), what="K = 1")
    check(dict(hic_edges=1, **a), what="K = 0")
    check(dict(hic_edges=3001, **a), what="float32 counts")


@pytest.mark.timeout(600)
def test_more_than_65536_windows():
    rng = np.random.RandomState(11)
    n, m = 70001, 600000
    ws = (np.sort(rng.choice(200000, n, replace=False)) * 500).astype(np.int32)
    i, j = rng.randint(0, n, m), rng.randint(0, n, m)
    i[:1000], j[:1000] = n - 1 - rng.randint(0, 50, 1000), rng.randint(0, 50, 1000)       # ranks beyond 16 bits on both sides
    _, first = np.unique(i.astype(np.int64) * n + j, return_index=True)
    first = first[rng.permutation(first.size)]
    pos1, pos2 = ws[i[first]].copy(), ws[j[first]].copy()
    miss = rng.random_sample(first.size) < 0.3
    pos1[miss] += 7                                                                       # not a window
    count = (1 + rng.poisson(1.5, first.size)).astype(np.float64)
    norm = 0.5 + rng.random_sample(200000)
    norm[rng.random_sample(norm.size) < 0.05] = np.nan
    for nv in (None, norm):
        a = check(dict(pos1=pos1, pos2=pos2, count=count, norm=nv, resolution_bp=500, window_start=ws, hic_edges=300000),
                  ("hic", "both"), what="N > 65536")
        assert a.nnz > 200000 and a[n - 40:, :60].nnz > 0


@pytest.mark.timeout(600)
def test_one_epoch_on_the_device_built_graph_equals_the_host_built_one():
    r = synth.raw_contacts("chr21", background_per_bin=8.0, peak_pairs_per_window=30.0)
    n, d, C = r["window_start"].size, 128, 12
    feats = {"chrT": synth.chrom_features(n, d, C, 77)}
    a = hic.build_hic_graph_host(r["pos1"], r["pos2"], r["count"], r["norm"], 1000, r["window_start"], 60000)
    assert a.nnz > 50000
    g_dev = hic.build_hic_graph(r["pos1"], r["pos2"], r["count"], r["norm"], 1000, r["window_start"], 60000, device=DEV)
    g_host = G.process_graph("hic", {"chrT": a}, n, "chrT", DEV)
    out = []
    for g in (g_dev, g_host):
        torch.manual_seed(5)
        model = ChromeGCN(d, d, C, 0.2, True, 2).to(DEV)
        opt = torch.optim.SGD(model.parameters(), lr=0.25, momentum=0.9, weight_decay=1e-6)
        o = types.SimpleNamespace(adj_type="hic", hip_graphs=True)
        torch.manual_seed(6)
        pred, targ, loss = finetune(None, model, feats, None, opt, 1, None, o, "train", split_adj_dict={"chrT": g})
        torch.cuda.synchronize()
        out.append((pred.clone(), float(loss), {k: v.detach().clone() for k, v in model.state_dict().items()}))
    assert torch.equal(out[0][0], out[1][0]) and out[0][1] == out[1][1]
    for k in out[0][2]:
        assert torch.equal(out[0][2][k], out[1][2][k]), k


@pytest.mark.timeout(300)
def test_bad_arguments_raise_with_the_librarys_message():
    r = synth.raw_contacts("chr21", background_per_bin=1.0, peak_pairs_per_window=5.0)
    c = hic.HicContacts(r["pos1"], r["pos2"], r["count"], DEV)
    ws = torch.from_numpy(r["window_start"]).to(DEV)
    n, cap = int(ws.numel()), c.survivors(r["window_start"])
    K = 1000
    need = _lib.query("cgcn_hic_workspace_bytes", M=c.M, N=n, capacity=cap, K=K)
    assert need > 0
    wsp = torch.empty(need, dtype=torch.uint8, device=DEV)
    rowptr = torch.full((n + 1,), -7, dtype=torch.int32, device=DEV)
    col = torch.full((2 * K,), -7, dtype=torch.int32, device=DEV)
    sizes = torch.full((2,), -7, dtype=torch.int64, device=DEV)
    norm = torch.from_numpy(r["norm"]).to(DEV)
    good = dict(M=c.M, pos1=c.pos1, pos2=c.pos2, count=c.count, norm=norm, n_bins=int(norm.numel()), resolution_bp=1000,
                window_start=ws, N=n, K=K, capacity=cap, workspace=wsp, workspace_bytes=need, rowptr_out=rowptr, col_out=col,
                nnz_out=sizes.data_ptr(), n_survivors=sizes.data_ptr() + 8)
    for over, code in ((dict(M=-1), BAD_ARG), (dict(N=-1), BAD_ARG), (dict(K=-1), BAD_ARG), (dict(pos1=None), BAD_ARG),
                       (dict(count=None), BAD_ARG), (dict(window_start=None), BAD_ARG), (dict(rowptr_out=None), BAD_ARG),
                       (dict(col_out=None), BAD_ARG), (dict(nnz_out=None), BAD_ARG), (dict(workspace=None), BAD_ARG),
                       (dict(resolution_bp=0), BAD_ARG), (dict(K=2 ** 30), UNSUPPORTED), (dict(capacity=2 ** 31), UNSUPPORTED),
                       (dict(workspace_bytes=need - 1), WORKSPACE)):
        assert _lib.query("cgcn_hic_build", **dict(good, **over)) == code, over
    with pytest.raises(RuntimeError, match=r"chromegcn_amd: cgcn_hic_build failed: bad argument.*\(code -1\)"):
        _lib.call("cgcn_hic_build", **dict(good, count=None))
    with pytest.raises(RuntimeError, match=r"chromegcn_amd: cgcn_hic_count failed: bad argument.*\(code -1\)"):
        _lib.call("cgcn_hic_count", M=c.M, pos1=c.pos1, pos2=None, window_start=ws, N=n, workspace=wsp, workspace_bytes=need,
                  n_survivors=sizes)
    torch.cuda.synchronize()
    assert bool((rowptr == -7).all()) and bool((col == -7).all()) and bool((sizes == -7).all())     # nothing was launched
    # a capacity below the survivor count: reported, nothing overrun
    small = cap // 2
    need2 = _lib.query("cgcn_hic_workspace_bytes", M=c.M, N=n, capacity=small, K=K)
    wsp2 = torch.empty(need2 + 4096, dtype=torch.uint8, device=DEV)
    wsp2[need2:] = 0x5A
    _lib.call("cgcn_hic_build", **dict(good, capacity=small, workspace=wsp2, workspace_bytes=need2))
    torch.cuda.synchronize()
    assert int(sizes[1]) == cap > small and bool((wsp2[need2:] == 0x5A).all())
    # python-side checks
    with pytest.raises(ValueError, match="strictly increasing"):
        c.build(None, 1000, r["window_start"][::-1].copy(), 1000)
    with pytest.raises(ValueError, match="bins"):
        c.build(r["norm"][:10], 1000, r["window_start"], 1000)
    with pytest.raises(ValueError, match="hic_edges"):
        c.build(None, 1000, r["window_start"], 2 ** 31)
