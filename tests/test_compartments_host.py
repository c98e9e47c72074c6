"""The numpy tier of the A/B compartment rule (chromegcn_amd/compartments.py): each restatement against literal double loops
on maps of at most 40 bins, the Pearson map against np.corrcoef, compartments_host against np.linalg.eigh of its own Pearson map
within the Davis-Kahan bound of the residual stop, 100 % recovery of the planted compartments, and everything around the
eigenvector: orientation, calls, domains, edge shares, stratified metrics, flat rows, too few and too many bins, the host builder
within compartments, tools/hic_compartments.py on the restatement, the train flags, the entry points' argument checks (no launch).
No GPU.

Bounds of this tier: two summation orders of the same K terms differ by at most 2 (K - 1) 2^-53 sum|terms| to first order
(each is within (K - 1) 2^-53 sum|terms| of the exact sum); a product of two m-term rows adds one rounding per product:
2 m 2^-53 (|Z| |Z|^T)."""
import math

import numpy as np
import pytest
import scipy.sparse as sp

from chromegcn_amd import bootstrap, build_hic_graph_host, hicmap, hicnorm, insulation
from chromegcn_amd import compartments as CP

import compartment_cases as CC

LOOP_CASES = [(1, False, False), (3, True, False), (5, True, True), (17, False, False), (17, True, True), (38, True, True)]


def literal(c):
    """rules 1 to 6 of the docstring as plain Python loops over lists: dict of B, dsum, cnt, K (terms per distance), e, M, mean, ss"""
    A = hicnorm.contact_matrix_host(c["pos1"], c["pos2"], c["count"], c["res"], c["n_bins"]).toarray()
    n = A.shape[0]
    nv = None if c["norm"] is None else hicnorm.clean_norm(c["norm"], n)
    keep = [b for b in range(n) if sum(A[b]) > 0 and (nv is None or math.isfinite(nv[b]))]
    m = len(keep)
    B = [[A[a, b] if nv is None else A[a, b] / (nv[a] * nv[b]) for b in keep] for a in keep]
    dsum, cnt = [0.0] * n, [0] * n
    for i in range(m):
        for j in range(i, m):
            dsum[keep[j] - keep[i]] += B[i][j]
            cnt[keep[j] - keep[i]] += 1
    return dict(keep=keep, B=np.array(B).reshape(m, m), dsum=np.array(dsum), cnt=np.array(cnt))


def literal_rows(B, keep, e, ignore):
    m = len(keep)
    M = [[B[i][j] / e[abs(keep[j] - keep[i])] if abs(keep[j] - keep[i]) >= ignore and e[abs(keep[j] - keep[i])] > 0 else 1.0
          for j in range(m)] for i in range(m)]
    mean = [sum(row) / m for row in M]
    return np.array(M).reshape(m, m), np.array(mean)


@pytest.mark.parametrize("case", LOOP_CASES, ids=CC.case_id)
def test_restatements_against_literal_loops(case):
    c = CC.kernel_case(*case)
    L = literal(c)
    keep, n, m = c["keep"], c["n_bins"], c["keep"].size
    assert L["keep"] == keep.tolist()
    A = hicnorm.contact_matrix_host(c["pos1"], c["pos2"], c["count"], c["res"], n)
    valid = hicmap.valid_bins(np.asarray(A.sum(axis=1)).ravel(), c["norm"])
    got_keep, rank = CP.kept_bins(valid, c["res"])
    assert np.array_equal(got_keep, keep) and np.array_equal(np.flatnonzero(rank >= 0), keep) and rank[keep].tolist() == list(range(m))
    B = CP.balanced_dense_host(A, c["norm"], keep)
    assert np.array_equal(B, L["B"]) and np.array_equal(B, B.T)
    assert np.array_equal(CP.pair_counts(valid), L["cnt"])
    dsum = CP.dist_sums_host(B, keep, n)
    assert np.all(np.abs(dsum - L["dsum"]) <= 2 * np.maximum(L["cnt"] - 1, 0) * CC.EPS * L["dsum"])
    if c["norm"] is None:
        assert np.array_equal(dsum, L["dsum"])                        # integer counts: exact in any order
    e = CP.expected_from_dist_sums(dsum, L["cnt"])
    assert np.array_equal(e, np.array([s / k if k else 0.0 for s, k in zip(dsum, L["cnt"])]))
    for ignore in (0, 2):
        M, mean, ss = CP.oe_rows_host(B, keep, e, ignore)
        LM, Lmean = literal_rows(B.tolist(), keep.tolist(), e.tolist(), ignore)
        assert np.array_equal(M, LM)
        assert np.all(np.abs(mean - Lmean) <= (2 * (m - 1) * CC.EPS * np.abs(M).sum(axis=1) + CC.EPS * np.abs(M.sum(axis=1))) / m)
        sq = [[(x - mu) * (x - mu) for x in row] for row, mu in zip(M.tolist(), mean.tolist())]
        assert np.all(np.abs(ss - np.array([sum(row) for row in sq])) <= 2 * (m - 1) * CC.EPS * np.array(sq).reshape(m, m).sum(axis=1))
        Z = CP.standardise_host(M, mean, ss)
        LZ = [[(x - mu) / math.sqrt(s) if s > 0 else 0.0 for x in row] for row, mu, s in zip(M.tolist(), mean.tolist(), ss.tolist())]
        assert np.array_equal(Z, np.array(LZ).reshape(m, m))
        C = CP.pearson_host(Z)
        LC = np.array([[sum(a * b for a, b in zip(zi, zj)) for zj in LZ] for zi in LZ]).reshape(m, m)
        assert np.array_equal(C, C.T) and np.all(np.abs(C - LC) <= 2 * m * CC.EPS * (np.abs(Z) @ np.abs(Z).T))
    if ignore == 2 and m >= 3:
        assert np.all(M[np.abs(keep[:, None] - keep[None, :]) < 2] == 1.0)


@pytest.mark.parametrize("case", [(5, True, True), (38, True, True)], ids=CC.case_id)
def test_power_step_against_literal_loops(case):
    c = CC.kernel_case(*case)
    r = CP.compartments_host(c["pos1"], c["pos2"], c["count"], c["norm"], c["res"], n_bins=c["n_bins"], n_eigs=3)
    C, m = r.pearson, r.keep.size
    prev = [r.E[k, r.keep] for k in range(2)]
    v = CP.start_vector(m)
    assert abs(float(v @ v) - 1.0) < 4 * CC.EPS and np.allclose(v * np.sqrt(np.sum((np.cos(0.7 * np.arange(m)) + 0.1) ** 2)),
                                                                 np.cos(0.7 * np.arange(m)) + 0.1, rtol=1e-15)
    for n_prev in (0, 1, 2):
        y, lam, nn, r2, dots, v_next = CP.power_step_host(C, v, prev[:n_prev])
        ly = [sum(C[i, j] * v[j] for j in range(m)) for i in range(m)]
        ldots = [sum(p[i] * ly[i] for i in range(m)) for p in prev[:n_prev]]
        ly = [ly[i] - sum(d * p[i] for d, p in zip(ldots, prev[:n_prev])) for i in range(m)]
        llam = sum(v[i] * ly[i] for i in range(m))
        bound_y = 2 * m * CC.EPS * (np.abs(C) @ np.abs(v)) * (1 + 2 * n_prev)
        assert np.all(np.abs(y - np.array(ly)) <= bound_y + 1e-300)
        assert abs(lam - llam) <= 2 * m * CC.EPS * float(np.abs(v) @ np.abs(y)) + float(np.abs(v) @ bound_y)
        assert abs(nn - sum(x * x for x in ly)) <= 1e-12 * nn
        assert abs(r2 - sum((ly[i] - llam * v[i]) ** 2 for i in range(m))) <= 1e-9 * max(r2, 1e-30) + 1e-24
        assert len(dots) == n_prev and np.allclose(v_next, np.array(ly) / math.sqrt(nn), rtol=1e-12, atol=1e-15)


@pytest.mark.parametrize("name", ["n40_a", "n130_b", "n600_a"])
def test_pearson_host_is_corrcoef(name):
    r = CC.planted_host(name)
    c = CC.planted_case(name)
    A = hicnorm.contact_matrix_host(c["pos1"], c["pos2"], c["count"], CC.RES, c["n_bins"])
    B = CP.balanced_dense_host(A, None, r.keep)
    M, mean, ss = CP.oe_rows_host(B, r.keep, r.expected)
    assert np.array_equal(CP.pearson_host(CP.standardise_host(M, mean, ss)), r.pearson)
    assert np.max(np.abs(r.pearson - np.corrcoef(M))) <= 1e-12
    assert np.max(np.abs(np.diag(r.pearson) - 1.0)) <= 1e-12


@pytest.mark.parametrize("name", sorted(CC.PLANTED))
def test_planted_recovery_and_eigh(name):
    c, r = CC.planted_case(name), CC.planted_host(name)
    m = r.keep.size
    assert m == c["n_bins"] - c["holes"].size and not np.isin(c["holes"], r.keep).any()
    lam, V = CC.eigh_desc(r.pearson)
    # the conditions the seeds were fixed for
    assert lam[1] / lam[0] <= 0.5 and lam[1] / lam[0] <= 0.28
    assert r.info["converged"] == [True] and 7 <= r.info["iterations"][0] <= 19
    assert r.info["residual"][0] <= CC.TOL * r.info["eigenvalue"][0] and r.info["flat_rows"] == 0
    v = r.E[0, r.keep]
    err = np.max(np.abs(v - CC.aligned(V[:, 0], v)))
    assert err <= 4e-11 and err <= CC.vector_bounds(lam, m, CC.TOL, 1)[0]
    assert abs(r.eigenvalues[0] - lam[0]) <= 1e-9 * lam[0]
    assert np.all(np.isnan(r.E[0, c["holes"]])) and not np.isnan(v).any()
    call = r.compartment_of_bin
    assert call.dtype == np.int8 and np.array_equal(call[r.keep], c["comp"][r.keep]) and np.all(call[c["holes"]] == 0)   # 100 %


@pytest.mark.parametrize("name", CC.THREE_VECTORS)
def test_three_vectors_against_eigh(name):
    r = CC.planted_host(name, 3)
    m = r.keep.size
    lam, V = CC.eigh_desc(r.pearson)
    bounds = CC.vector_bounds(lam, m, CC.TOL, 3)
    assert r.info["converged"] == [True] * 3
    for j in range(3):
        assert min(CC.gaps(lam, j)) >= 0.2
        v = r.E[j, r.keep]
        assert np.max(np.abs(v - CC.aligned(V[:, j], v))) <= bounds[j]
        assert abs(r.eigenvalues[j] - lam[j]) <= 1e-8 * lam[0]
    assert np.array_equal(r.E[0], CC.planted_host(name).E[0], equal_nan=True)                # the first vector does not depend on n_eigs
    G = r.E[:, r.keep] @ r.E[:, r.keep].T
    assert np.max(np.abs(G - np.eye(3))) <= 1e-8


def test_orientation_rule():
    c, r = CC.planted_case("n65_a"), CC.planted_host("n65_a")
    n = c["n_bins"]
    flipped = r.oriented(-c["comp"].astype(np.float64))
    assert np.array_equal(flipped.E, -r.E, equal_nan=True) and np.array_equal(flipped.compartment_of_bin, -r.compartment_of_bin)
    assert flipped.pearson is r.pearson
    for orient in (None, np.zeros(n), np.full(n, 3.0)):                       # the fallback: the largest |E| is positive
        f = r.oriented(orient)
        assert f.E[0, int(np.nanargmax(np.abs(f.E[0])))] > 0
        assert np.array_equal(np.abs(f.E), np.abs(r.E), equal_nan=True)
    tie = CP.Compartments(np.array([[np.nan, -0.5, 0.5, 0.1]]), np.ones(1), None, np.arange(1, 4), np.zeros(4), {}, CC.RES)
    assert tie.oriented(None).E[0].tolist()[1:] == [0.5, -0.5, -0.1]           # the lowest bin on ties
    only = np.zeros(n)
    only[r.keep[0]] = 1.0                                                      # one bin decides: its entry becomes positive
    assert r.oriented(only).E[0, r.keep[0]] > 0 and r.oriented(-only).E[0, r.keep[0]] < 0
    with pytest.raises(ValueError):
        r.oriented(np.zeros(n + 1))
    t = np.zeros((6, 3))
    t[[0, 1, 1, 5], [0, 0, 2, 1]] = 1
    ws = np.array([0, 1, 2, 3, 4, 9]) * CC.RES // 2                            # two windows per bin; the last beyond 2 bins
    assert CP.label_density(t, ws, CC.RES, 2).tolist() == [3.0, 0.0]
    assert CP.label_density(t[:, 0], ws, CC.RES, 5).tolist() == [2.0, 0.0, 0.0, 0.0, 0.0]


def test_calls_domains_and_edge_share():
    E = np.array([[0.3, -0.2, np.nan, 0.0, -0.1, 0.4]])
    r = CP.Compartments(E, np.ones(1), None, np.array([0, 1, 4, 5]), np.zeros(6), {}, 1000)
    assert r.compartment_of_bin.tolist() == [1, -1, 0, 0, -1, 1] and r.compartment_of_bin.dtype == np.int8
    dom = r.as_domains()
    assert dom.dtype == np.int32 and dom.tolist() == [0, 1, 4, 5, 1, 0]
    ws = np.array([0, 500, 1000, 2000, 4000, 5500, 6000, -5])
    comp = r.compartment_of_windows(ws)
    assert comp.dtype == np.int8 and comp.tolist() == [1, 1, -1, 0, -1, 1, 0, 0]
    assert r.a_share() == 0.5
    # 5 windows: A A B B none; entries (row -> cols)
    comp5 = np.array([1, 1, -1, -1, 0])
    g = sp.csr_matrix(np.array([[1, 1, 1, 0, 0],
                                [1, 0, 0, 1, 1],
                                [1, 0, 1, 1, 0],
                                [0, 1, 1, 0, 0],
                                [0, 1, 0, 0, 1]], dtype=np.float64))
    want = {"AA": 3, "BB": 3, "AB": 4, "uncalled": 3, "nnz": 13}
    assert CP.compartment_edge_share(g, comp5) == want
    assert CP.compartment_edge_share((g.indptr, np.concatenate([g.indices, [0, 0]])), comp5) == want
    assert sum(want[k] for k in ("AA", "BB", "AB", "uncalled")) == want["nnz"]
    with pytest.raises(ValueError):
        CP.compartment_edge_share(g, comp5[:4])


def test_compartment_metrics_are_weighted_metrics_of_the_two_rows():
    rng = np.random.default_rng(5)
    n, C = 300, 4
    targets = (rng.random((n, C)) < 0.3).astype(np.float32)
    probs = np.clip(0.5 * targets + rng.random((n, C)) * 0.7, 0, 1).astype(np.float32)
    comp = rng.choice([-1, 0, 1], n).astype(np.int8)
    got = CP.compartment_metrics(probs, targets, comp, 0.5, host=True)
    rows = np.zeros((2, n), np.int32)
    rows[0, np.flatnonzero(comp == 1)] = 1
    rows[1, np.flatnonzero(comp == -1)] = 1
    want = bootstrap.metrics_from_sums(bootstrap.weighted_sums_host(probs, targets, rows, 0.5))
    assert sorted(got) == ["A", "B"] and sorted(got["A"]) == sorted(bootstrap.METRICS)
    for k in bootstrap.METRICS:
        assert got["A"][k].shape == (C,) and np.array_equal(got["A"][k], want[k][0], equal_nan=True)
        assert np.array_equal(got["B"][k], want[k][1], equal_nan=True)
    sub = bootstrap.metrics_from_sums(bootstrap.weighted_sums_host(probs[comp == 1], targets[comp == 1], np.ones((1, int((comp == 1).sum())), np.int32), 0.5))
    assert np.array_equal(got["A"]["auroc"], sub["auroc"][0], equal_nan=True)   # a 0 / 1 row is the subset


def test_flat_rows_get_nan():
    n = 12
    a, b = np.triu_indices(n)
    count = np.where(b - a >= 2, 0.0, 5.0)          # nothing beyond the ignored diagonals: every O/E entry is 0 or the neutral 1
    count[(a == 0) & (b == 8)] = 3.0                # distance 8: the rows 0-3 and 8-11 have a partner there, the rows 4-7 are flat
    k = count > 0
    r = CP.compartments_host(a[k] * CC.RES, b[k] * CC.RES, count[k], None, CC.RES, n_bins=n)
    A = hicnorm.contact_matrix_host(a[k] * CC.RES, b[k] * CC.RES, count[k], CC.RES, n)
    M, mean, ss = CP.oe_rows_host(CP.balanced_dense_host(A, None, r.keep), r.keep, r.expected)
    flat = ss == 0
    assert r.info["flat_rows"] == 4 and np.flatnonzero(flat).tolist() == [4, 5, 6, 7]
    assert np.array_equal(np.isnan(r.E[0]), flat)
    Z = CP.standardise_host(M, mean, ss)
    assert np.all(Z[flat] == 0) and np.all(r.pearson[flat] == 0) and np.all(r.pearson[:, flat] == 0)
    assert np.all(r.compartment_of_bin[flat] == 0) and np.all(r.as_domains()[flat] == 2 + np.flatnonzero(flat))


@pytest.mark.parametrize("bins", [0, 1, 2])
def test_fewer_than_three_bins(bins):
    p = np.arange(bins, dtype=np.int64) * CC.RES
    r = CP.compartments_host(p, p, np.full(bins, 4.0), None, CC.RES, n_bins=5, n_eigs=2)
    assert r.E.shape == (2, 5) and np.isnan(r.E).all() and np.isnan(r.eigenvalues).all() and r.pearson is None
    assert r.info["converged"] == [False, False] and r.info["iterations"] == [0, 0] and r.keep.tolist() == list(range(bins))
    assert r.compartment_of_bin.tolist() == [0] * 5 and r.as_domains().tolist() == [2, 3, 4, 5, 6] and math.isnan(r.a_share())


def test_too_many_bins_is_refused_before_anything_dense():
    p = np.arange(CP.MAX_KEPT + 1, dtype=np.int64) * 1000
    with pytest.raises(ValueError, match=r"coarser resolution, 2000 bp"):
        CP.compartments_host(p, p, np.ones(p.size), None, 1000)          # diagonal records: a sparse matrix, 8193 kept bins
    with pytest.raises(ValueError, match="coarser"):
        CP.kept_bins(np.ones(3 * CP.MAX_KEPT, bool), 50000)
    assert CP.kept_bins(np.ones(CP.MAX_KEPT, bool), 1000)[0].size == CP.MAX_KEPT
    for bad in (dict(n_eigs=0), dict(n_eigs=4), dict(tol=0.0), dict(max_iter=0), dict(ignore_diags=-1)):
        with pytest.raises(ValueError):
            CP.compartments_host(p[:4], p[:4], np.ones(4), None, 1000, **bad)


def test_restricted_host_build_keeps_what_same_domain_says():
    c, r = CC.planted_case("n130_a"), CC.planted_host("n130_a")
    dom = r.as_domains()
    ws = (np.arange(c["n_bins"]) * CC.RES).astype(np.int32)
    keep = insulation.same_domain_host(c["pos1"], c["pos2"], dom, CC.RES)
    comp = r.compartment_of_bin
    b1, b2 = c["pos1"] // CC.RES, c["pos2"] // CC.RES
    assert np.array_equal(keep, (comp[b1] == comp[b2]) & (comp[b1] != 0) | (b1 == b2))
    assert 0 < keep.sum() < keep.size
    got = build_hic_graph_host(c["pos1"], c["pos2"], c["count"], None, CC.RES, ws, 2000, domains=(dom, CC.RES))
    want = build_hic_graph_host(c["pos1"][keep], c["pos2"][keep], c["count"][keep], None, CC.RES, ws, 2000)
    assert got.nnz == 2000 and np.array_equal(got.indptr, want.indptr) and np.array_equal(got.indices, want.indices)
    share = CP.compartment_edge_share(got, r.compartment_of_windows(ws))
    assert share["AB"] == 0 and share["uncalled"] == 0 and share["AA"] + share["BB"] == share["nnz"] == got.nnz
    free = CP.compartment_edge_share(build_hic_graph_host(c["pos1"], c["pos2"], c["count"], None, CC.RES, ws, 2000), r.compartment_of_windows(ws))
    assert free["AB"] > 0 and free["nnz"] == 2000


def test_hic_compartments_tool_writes_the_planted_calls(tmp_path, capsys):
    import importlib.util
    import os
    from chromegcn_amd import hic
    spec = importlib.util.spec_from_file_location("hic_compartments", os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "tools", "hic_compartments.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    c = CC.planted_case("n65_a")
    cache = str(tmp_path / "chrT.cghic")
    hic.save_contacts_cache(cache, hic.HostContacts(c["pos1"], c["pos2"], c["count"], {}, CC.RES, None))
    orient = tmp_path / "peaks.bedGraph"
    orient.write_text("".join("chrT\t%d\t%d\t%d\n" % (b * CC.RES, (b + 1) * CC.RES, 3 if c["comp"][b] > 0 else 1) for b in range(65))
                      + "chrU\t0\t100000\t99\n")
    prefix = str(tmp_path / "out" / "chrT")
    tool.main([cache, "--chrom", "chrT", "--res", str(CC.RES), "--norm", "RAW", "--host", "--pearson", "--orient", str(orient),
               "--out-prefix", prefix])
    rows = [ln.split("\t") for ln in open(prefix + ".E1.bedGraph").read().splitlines()]
    want = CC.planted_host("n65_a")
    assert [int(r[1]) // CC.RES for r in rows] == want.keep.tolist() and all(r[0] == "chrT" for r in rows)
    assert [1 if float(r[3]) > 0 else -1 for r in rows] == c["comp"][want.keep].tolist()
    assert np.allclose([float(r[3]) for r in rows], want.E[0, want.keep], rtol=1e-8)
    assert np.array_equal(np.load(prefix + ".pearson.npy"), want.pearson) and np.array_equal(np.load(prefix + ".keep.npy"), want.keep)
    assert "64 of 65 bins kept, 64 called" in capsys.readouterr().out


def test_train_arguments():
    from chromegcn_amd import train
    opt = train.parse(["-feat_dir", "f", "-hic_contacts", "caches"])
    assert (opt.hic_compartments, opt.hic_compartment_norm, opt.hic_compartment_restrict) == (0, "VC", False)
    opt = train.parse(["-feat_dir", "f", "-hic_contacts", "caches", "-hic_compartments", "100000", "-hic_compartment_norm", "KR",
                       "-hic_compartment_restrict"])
    assert (opt.hic_compartments, opt.hic_compartment_norm, opt.hic_compartment_restrict) == (100000, "KR", True)


def test_entry_point_argument_checks():
    from chromegcn_amd import _build, _lib
    _build.build_library()
    _lib.load()
    p = 0x10000   # never read: every call below returns before a launch

    def rc(fn, ok, **kw):
        return _lib.query(fn, **{**ok, **kw})

    dense = dict(stream=None, n=10, rowptr=p, col=p, val=p, norm=None, n_norm=0, rank=p, m=5, ld=6, B=p)
    dist = dict(stream=None, n=10, m=5, ld=6, B=p, keep=p, rank=p, dsum=p)
    rows = dict(stream=None, m=5, ld=6, B=p, keep=p, e=p, n_e=10, ignore_diags=2, stages=3, mean=p, ss=p)
    corr = dict(stream=None, m=5, ld=6, Z=p, C=p)
    step = dict(stream=None, m=5, C=p, v=p, prev=None, n_prev=0, y=p + 64, v_next=p + 128, rec=p + 192)
    name = {"cgcn_hiccomp_dense": "B", "cgcn_hiccomp_dist_sums": "B", "cgcn_hiccomp_oe_rows": "B", "cgcn_hiccomp_corr": "Z"}
    for fn, ok in (("cgcn_hiccomp_dense", dense), ("cgcn_hiccomp_dist_sums", dist), ("cgcn_hiccomp_oe_rows", rows),
                   ("cgcn_hiccomp_corr", corr)):
        B = name[fn]
        assert rc(fn, ok, ld=5) == -1 and rc(fn, ok, ld=4) == -1 and rc(fn, ok, m=-1) == -1      # an odd ld, ld < m
        assert rc(fn, ok, **{B: p + 8}) == -1 and rc(fn, ok, **{B: None}) == -1                  # rows off 16 bytes
        assert rc(fn, ok, m=CP.MAX_KEPT + 1, ld=CP.MAX_KEPT + 2) == -2
    for ptr in ("rowptr", "col", "val", "rank"):
        assert rc("cgcn_hiccomp_dense", dense, **{ptr: None}) == -1
    assert rc("cgcn_hiccomp_dense", dense, n=-1) == -1 and rc("cgcn_hiccomp_dense", dense, norm=p, n_norm=0) == -1
    assert rc("cgcn_hiccomp_dense", dense, n=0, rowptr=None) == 0 and rc("cgcn_hiccomp_dense", dense, m=0, ld=0, B=None) == 0
    for ptr in ("keep", "rank", "dsum"):
        assert rc("cgcn_hiccomp_dist_sums", dist, **{ptr: None}) == -1
    assert rc("cgcn_hiccomp_dist_sums", dist, n=-1) == -1 and rc("cgcn_hiccomp_dist_sums", dist, n=0, dsum=None) == 0
    for ptr in ("keep", "e", "mean", "ss"):
        assert rc("cgcn_hiccomp_oe_rows", rows, **{ptr: None}) == -1
    assert rc("cgcn_hiccomp_oe_rows", rows, stages=0) == -1 and rc("cgcn_hiccomp_oe_rows", rows, stages=4) == -1
    assert rc("cgcn_hiccomp_oe_rows", rows, ignore_diags=-1) == -1 and rc("cgcn_hiccomp_oe_rows", rows, n_e=-1) == -1
    assert rc("cgcn_hiccomp_oe_rows", rows, m=0, ld=0, B=None) == 0
    assert rc("cgcn_hiccomp_corr", corr, C=None) == -1 and rc("cgcn_hiccomp_corr", corr, m=0, ld=0, Z=None, C=None) == 0
    for ptr in ("C", "v", "y", "v_next", "rec"):
        assert rc("cgcn_hiccomp_step", step, **{ptr: None}) == -1
    assert rc("cgcn_hiccomp_step", step, m=0) == -1 and rc("cgcn_hiccomp_step", step, n_prev=1) == -1      # prev is NULL
    assert rc("cgcn_hiccomp_step", step, v_next=p) == -1 and rc("cgcn_hiccomp_step", step, n_prev=-1) == -1
    assert rc("cgcn_hiccomp_step", step, prev=p, n_prev=3) == -2 and rc("cgcn_hiccomp_step", step, m=CP.MAX_KEPT + 1) == -2
    with pytest.raises(RuntimeError, match=r"cgcn_hiccomp_corr failed: bad argument.*\(code -1\)"):
        _lib.call("cgcn_hiccomp_corr", **{**corr, "ld": 5})
