"""The compartment kernels (csrc/cgcn_compartment.hip) one by one against their numpy restatements, each fed the DEVICE's own
upstream outputs read back, so that no comparison leans on the stage before it; then HicContacts.compartments against
compartments_host and np.linalg.eigh on planted maps, and the compartment-restricted device build against the host builder.
Sizes: m kept bins either side of the K step of 4, the MFMA tile of 16 and the workgroup tile of 64, one m = 1500 for many
workgroups and the mirrored store; with and without holes (m < n, distances skip), with and without a norm vector.  Every
kernel runs twice per case and must give the same bits.  A case's stages run once and are shared by its tests."""
import functools

import numpy as np
import pytest
import torch

from chromegcn_amd import HicContacts, bootstrap, build_hic_graph_host, hicmap
from chromegcn_amd import compartments as CP

import compartment_cases as CC

pytestmark = pytest.mark.gpu
DEV = "cuda"
cases = pytest.mark.parametrize("case", CC.KERNEL_CASES, ids=CC.case_id)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def twice(fn):
    a, b = fn().cpu().numpy(), fn().cpu().numpy()
    assert same_bits(a, b)                       # no order that scheduling could change
    return a


@functools.lru_cache(maxsize=None)
def stages(case):
    """every stage of one kernel case on the device, read back: dict of numpy arrays (B, M, Z are [m, m], the padding cut)"""
    c = CC.kernel_case(*case)
    keep, n, m = c["keep"], c["n_bins"], c["keep"].size
    hc = HicContacts(c["pos1"], c["pos2"], c["count"], DEV)
    A = hc.contact_matrix(CC.RES, n)
    nv = None if c["norm"] is None else torch.from_numpy(c["norm"]).to(DEV)
    valid = hicmap.valid_bins(A.vc.cpu().numpy(), c["norm"])
    assert np.array_equal(np.flatnonzero(valid), keep)
    Bd = CP.balanced_dense(A, nv, keep)
    B = twice(lambda: CP.balanced_dense(A, nv, keep))
    assert B.shape == (m, m + (m & 1)) and np.all(B[:, m:] == 0)
    dsum = twice(lambda: CP.dist_sums(Bd, keep, n))
    e = CP.expected_from_dist_sums(dsum, CP.pair_counts(valid))

    def stats():
        t = Bd.clone()
        mean, ss = CP.oe_rows(t, keep, e, 2, stages=1)
        return torch.cat([t.ravel(), mean, ss])
    packed = twice(stats)
    ld = m + (m & 1)
    M, mean, ss = packed[:m * ld].reshape(m, ld), packed[m * ld:m * ld + m], packed[m * ld + m:]
    Md, st = torch.from_numpy(M).to(DEV), (torch.from_numpy(mean).to(DEV), torch.from_numpy(ss).to(DEV))

    def z():
        t = Md.clone()
        CP.oe_rows(t, keep, e, 2, stages=2, stats=st)
        return t
    Z = twice(z)
    both = Bd.clone()
    mean3, ss3 = CP.oe_rows(both, keep, e, 2)                 # the two stages in one call: the same bits
    assert same_bits(both.cpu().numpy(), Z) and same_bits(mean3.cpu().numpy(), mean) and same_bits(ss3.cpu().numpy(), ss)
    assert np.all(M[:, m:] == 0) and np.all(Z[:, m:] == 0)    # the padding is never written
    Zd = torch.from_numpy(Z).to(DEV)
    C = twice(lambda: CP.pearson(Zd))
    return dict(c=c, host=A.to_host(), valid=valid, B=B[:, :m], dsum=dsum, e=e, M=M[:, :m], mean=mean, ss=ss, Z=Z[:, :m], C=C)


@cases
def test_dense_is_the_host_matrix_bit_for_bit(case):
    s = stages(case)
    assert same_bits(s["B"], CP.balanced_dense_host(s["host"], s["c"]["norm"], s["c"]["keep"]))
    assert np.array_equal(s["B"], s["B"].T) and (s["B"] > 0).any()


@cases
def test_dist_sums(case):
    s = stages(case)
    keep, n, m = s["c"]["keep"].astype(np.int64), s["c"]["n_bins"], s["c"]["keep"].size
    ref = CP.dist_sums_host(s["B"], keep, n)
    i, j = np.triu_indices(m)
    d, t = keep[j] - keep[i], s["B"][i, j]
    if s["c"]["norm"] is None:                               # integer counts, no vector: exact in any order
        assert same_bits(s["dsum"], ref) and np.array_equal(ref, np.bincount(d, weights=t, minlength=n))
    K = np.bincount(d, minlength=n)
    assert np.array_equal(K, CP.pair_counts(s["valid"]))
    assert np.all(np.abs(s["dsum"] - ref) <= np.maximum(K - 1, 0) * CC.EPS * np.bincount(d, weights=np.abs(t), minlength=n))
    assert np.all(s["dsum"][K == 0] == 0) and s["dsum"][0] > 0


@cases
def test_oe_rows(case):
    s = stages(case)
    keep, m = s["c"]["keep"], s["c"]["keep"].size
    M, mean, _ = CP.oe_rows_host(s["B"], keep, s["e"], 2)
    assert same_bits(s["M"], M)                                                    # given the same e
    assert np.all(np.abs(s["mean"] - mean) <= (CC.reordered_sum_bound(np.abs(M)) + CC.EPS * np.abs(M).sum(axis=1)) / m)
    t = s["M"] - s["mean"][:, None]                                                # ss against the host sum taken with the DEVICE's mean
    assert np.all(np.abs(s["ss"] - CP.wave_sum(t * t)) <= CC.reordered_sum_bound(t * t))
    assert same_bits(s["Z"], CP.standardise_host(s["M"], s["mean"], s["ss"]))      # elementwise from the device's mean and ss
    if m >= 3:
        assert np.all(s["M"][np.abs(keep[:, None] - keep[None, :]) < 2] == 1.0)


@cases
def test_pearson_map(case):
    s = stages(case)
    Z, C, m = s["Z"], s["C"], s["c"]["keep"].size
    assert C.shape == (m, m) and same_bits(C, np.ascontiguousarray(C.T))           # symmetric by construction
    assert np.all(np.abs(C - Z @ Z.T) <= 2 * m * CC.EPS * (np.abs(Z) @ np.abs(Z).T))
    flat = s["ss"] == 0
    assert np.all(np.abs(np.diag(C)[~flat] - 1.0) <= 4 * m * CC.EPS) and np.all(C[flat] == 0)


@cases
def test_power_step(case):
    s = stages(case)
    C, m = s["C"], s["c"]["keep"].size
    Cd = torch.from_numpy(C).to(DEV)
    _, V = CC.eigh_desc(C)
    v = CP.start_vector(m)
    vd = torch.from_numpy(v).to(DEV)
    u, mu = CC.EPS, m * CC.EPS
    for n_prev in range(min(3, m + 1)):
        prev = np.array(V[:, :n_prev].T, order="C", copy=True).reshape(n_prev, m) + 0.0
        pd = torch.from_numpy(prev).to(DEV) if n_prev else None
        got = twice(lambda: torch.cat(CP.power_step(Cd, vd, pd)))
        y, v_next, rec = got[:m], got[m:2 * m], got[2 * m:]
        hy, lam, nn, r2, dots, _ = CP.power_step_host(C, v, list(prev))
        # bounds of m-term sums taken in two orders, from absolute values, passed down the chain
        by = 2 * mu * (np.abs(C) @ np.abs(v))
        y0 = np.abs(C @ v)
        bd = [float(np.abs(p) @ by) + 2 * mu * float(np.abs(p) @ y0) for p in prev]
        by = by + sum((b * np.abs(p) + 4 * u * abs(dot) * np.abs(p) for b, dot, p in zip(bd, dots, prev)), np.zeros(m)) + 4 * u * y0
        assert np.all(np.abs(y - hy) <= by)
        assert all(abs(rec[3 + p] - dots[p]) <= bd[p] for p in range(n_prev)) and np.all(rec[3 + n_prev:] == 0)
        bl = float(np.abs(v) @ by) + 2 * mu * float(np.abs(v) @ np.abs(hy))
        assert abs(rec[0] - lam) <= bl
        assert abs(rec[1] - nn) <= 2 * np.sqrt(nn) * np.linalg.norm(by) + np.linalg.norm(by) ** 2 + 2 * mu * nn
        assert rec[1] >= 0 and rec[2] >= 0
        assert abs(np.sqrt(rec[2]) - np.sqrt(r2)) <= np.linalg.norm(by + bl * np.abs(v)) + 2 * mu * np.sqrt(r2)
        assert same_bits(v_next, y / np.sqrt(rec[1]) if rec[1] > 0 else y)


@pytest.mark.parametrize("name", CC.GPU_PLANTED)
def test_compartments_end_to_end_on_planted_maps(name):
    c, want = CC.planted_case(name), CC.planted_host(name)
    hc = HicContacts(c["pos1"], c["pos2"], c["count"], DEV)
    orient = c["comp"].astype(np.float64)
    got = hc.compartments(None, CC.RES, n_bins=c["n_bins"], tol=CC.TOL, orient=orient)
    assert got.pearson.is_cuda and np.array_equal(got.keep, want.keep) and got.info["converged"] == [True]
    assert got.info["flat_rows"] == 0 and got.info["iterations"][0] % CP.CHECK_EVERY == 0 and got.info["host_syncs"] >= 4
    assert np.allclose(got.expected, want.expected, rtol=1e-13, atol=0)
    C, m = got.pearson.cpu().numpy(), got.keep.size
    lam, V = CC.eigh_desc(C)
    bound = CC.vector_bounds(lam, m, CC.TOL, 1)[0]
    v = got.E[0, got.keep]
    assert np.max(np.abs(v - CC.aligned(V[:, 0], v))) <= bound                     # the host tier's bound with eigh of the device's C
    assert np.array_equal(np.isnan(got.E), np.isnan(want.E))
    sure = np.abs(np.nan_to_num(got.E[0])) > bound
    assert sure.sum() >= m - 2 and np.array_equal(np.sign(got.E[0][sure]), np.sign(want.E[0][sure]))
    assert np.array_equal(got.compartment_of_bin[sure], want.compartment_of_bin[sure])
    assert np.array_equal(got.compartment_of_bin[got.keep], c["comp"][got.keep])   # the planted calls, 100 %
    assert abs(got.eigenvalues[0] - lam[0]) <= 1e-9 * lam[0]
    base = hc.compartments(None, CC.RES, n_bins=c["n_bins"], tol=CC.TOL)
    assert hc.compartments(None, CC.RES, n_bins=c["n_bins"], tol=CC.TOL) is base    # kept per argument tuple
    assert base.pearson is got.pearson and np.array_equal(np.abs(base.E), np.abs(got.E), equal_nan=True)


def test_three_vectors_and_a_named_norm():
    name = "n257_b"
    c = CC.planted_case(name)
    hc = HicContacts(c["pos1"], c["pos2"], c["count"], DEV)
    got = hc.compartments(None, CC.RES, n_bins=c["n_bins"], tol=CC.TOL, n_eigs=3, check_every=1)
    want = CC.planted_host(name, 3)
    lam, V = CC.eigh_desc(got.pearson.cpu().numpy())
    bounds = CC.vector_bounds(lam, got.keep.size, CC.TOL, 3)
    assert got.info["converged"] == [True] * 3
    assert all(abs(a - b) <= 1 for a, b in zip(got.info["iterations"], want.info["iterations"]))   # check_every = 1: the host's stops
    for j in range(3):
        v = got.E[j, got.keep]
        assert np.max(np.abs(v - CC.aligned(V[:, j], v))) <= bounds[j]
    vc = hc.compartments("VC", CC.RES, n_bins=c["n_bins"], orient=c["comp"].astype(np.float64))
    vc_host = CP.compartments_host(c["pos1"], c["pos2"], c["count"], "VC", CC.RES, n_bins=c["n_bins"], orient=c["comp"].astype(np.float64))
    assert vc.info["converged"] == [True] and np.array_equal(vc.compartment_of_bin, vc_host.compartment_of_bin)
    assert np.array_equal(vc.compartment_of_bin[vc.keep], c["comp"][vc.keep])
    assert np.nanmax(np.abs(vc.E - vc_host.E)) <= 1e-8


def test_fewer_than_three_bins_and_bad_arguments():
    p = np.arange(2, dtype=np.int32) * CC.RES
    hc = HicContacts(p, p, np.full(2, 4.0), DEV)
    r = hc.compartments(None, CC.RES, n_bins=5, n_eigs=2)
    assert np.isnan(r.E).all() and r.E.shape == (2, 5) and r.info["converged"] == [False, False] and r.pearson is None
    with pytest.raises(ValueError):
        hc.compartments(None, CC.RES, n_eigs=4)
    with pytest.raises(TypeError):
        hc.compartments(None, CC.RES, window=3)
    s = stages((5, False, False))
    B = torch.from_numpy(np.ascontiguousarray(np.pad(s["B"], ((0, 0), (0, 1))))).to(DEV)
    with pytest.raises(ValueError):
        CP.dist_sums(B[:, :5], s["c"]["keep"], 5)              # not [m, m + (m & 1)] contiguous
    with pytest.raises(ValueError):
        CP.dist_sums(B, s["c"]["keep"], 4)                     # a kept bin beyond n
    with pytest.raises(ValueError):
        CP.oe_rows(B, s["c"]["keep"], s["e"], 2, stages=2)     # stage 2 alone needs the statistics


def test_restricted_device_build_and_stratified_metrics():
    name = "n130_a"
    c, want = CC.planted_case(name), CC.planted_host(name)
    hc = HicContacts(c["pos1"], c["pos2"], c["count"], DEV)
    comp = hc.compartments(None, CC.RES, n_bins=c["n_bins"], tol=CC.TOL, orient=c["comp"].astype(np.float64))
    dom = comp.as_domains()
    assert np.array_equal(dom, want.as_domains())
    ws = (np.arange(c["n_bins"]) * CC.RES).astype(np.int32)
    g, raw = hc.build(None, CC.RES, ws, 2000, return_raw=True, domains=(dom, CC.RES))
    host = build_hic_graph_host(c["pos1"], c["pos2"], c["count"], None, CC.RES, ws, 2000, domains=(dom, CC.RES))
    assert raw.nnz == 2000 and np.array_equal(raw.indptr, host.indptr) and np.array_equal(raw.indices, host.indices)
    cw = comp.compartment_of_windows(ws)
    share = CP.compartment_edge_share((g.rowptr, g.col, g.nnz), cw)
    assert share["AB"] == 0 and share["nnz"] == g.nnz and share == CP.compartment_edge_share(g, cw)
    rng = np.random.default_rng(3)
    targets = (rng.random((ws.size, 3)) < 0.3).astype(np.float32)
    probs = np.clip(0.4 * targets + 0.6 * rng.random((ws.size, 3)), 0, 1).astype(np.float32)
    pd, td = torch.from_numpy(probs).to(DEV), torch.from_numpy(targets).to(DEV)
    got = CP.compartment_metrics(pd, td, cw)
    rows = np.stack([cw > 0, cw < 0]).astype(np.int32)
    ref = bootstrap.weighted_metrics(pd, td, rows)
    host_m = CP.compartment_metrics(pd, td, cw, host=True)
    for k in bootstrap.METRICS:
        assert np.array_equal(got["A"][k], ref[k][0], equal_nan=True) and np.array_equal(got["B"][k], ref[k][1], equal_nan=True)
        assert np.allclose(got["A"][k], host_m["A"][k], rtol=1e-12, equal_nan=True)


def test_graphs_from_contact_caches_with_compartments(tmp_path, capsys):
    from chromegcn_amd import hic, train
    c = CC.planted_case("n130_a")
    n = c["n_bins"]
    ws = (np.arange(0, n) * CC.RES).astype(np.int32)
    hic.save_contacts_cache(hic.contact_cache_path(str(tmp_path), "chrT"), hic.HostContacts(c["pos1"], c["pos2"], c["count"], {}, CC.RES, ws))
    targets = np.zeros((n, 4), np.float32)
    targets[c["comp"] > 0, :2] = 1                 # the planted A side carries the peaks
    kw = dict(resolution_bp=CC.RES, norm=None, tol=CC.TOL, targets={"chrT": targets})
    report = {}
    free = hic.graphs_from_contact_caches(str(tmp_path), ["chrT"], 2000, "", compartments=kw, compartment_report=report)["chrT"]
    comp, cw, share = report["chrT"]
    assert np.array_equal(comp.compartment_of_bin[comp.keep], c["comp"][comp.keep]) and np.array_equal(cw, comp.compartment_of_bin)
    assert share == CP.compartment_edge_share(free, cw) and share["AB"] > 0 and share["nnz"] == free.nnz
    plain = hic.graphs_from_contact_caches(str(tmp_path), ["chrT"], 2000, "")["chrT"]          # the default: as it was
    assert plain.nnz == free.nnz and torch.equal(plain.col[:plain.nnz], free.col[:free.nnz])
    report2 = {}
    only = hic.graphs_from_contact_caches(str(tmp_path), ["chrT"], 2000, "", compartments=dict(kw, restrict=True),
                                          compartment_report=report2)["chrT"]
    want = HicContacts(c["pos1"], c["pos2"], c["count"], DEV).build(None, CC.RES, ws, 2000, domains=(comp.as_domains(), CC.RES))
    assert only.nnz == want.nnz and torch.equal(only.rowptr, want.rowptr) and torch.equal(only.col[:only.nnz], want.col[:want.nnz])
    assert report2["chrT"][2]["AB"] == 0 and report2["chrT"][2]["nnz"] == only.nnz
    with pytest.raises(ValueError):
        hic.graphs_from_contact_caches(str(tmp_path), ["chrT"], 2000, "", compartments=dict(kw, restrict=True),
                                       domains=dict(window_bp=10 * CC.RES, norm=None, resolution_bp=CC.RES))
    opt = train.parse(["-synthetic"])
    train.report_compartments(opt, "test", report)
    line = capsys.readouterr().out
    assert "[hic_compartments] test chrT: 127 of 130 bins called" in line and "AB %d" % share["AB"] in line
    assert np.array_equal(opt.compartment_of_window["test"], cw)


def test_run_model_reports_the_test_metrics_by_compartment(capsys):
    import types
    import chromegcn_amd as C
    from chromegcn_amd import runner, synth
    n = 300
    test = {"chr1": synth.chrom_features(n, 128, 9, 0, positive_rate=0.3)}
    graphs = {"test": {"chr1": synth.contact_graph(n, 6 * n, 0)}}
    torch.manual_seed(0)
    model = C.ChromeGCN(128, 128, 9, 0.2, True, 2).to(DEV)
    comp = np.where(np.arange(n) < 200, 1, -1).astype(np.int8)
    hist = {}
    for name, cw in (("split", comp), ("all_a", np.ones(n, np.int8)), ("off", None)):
        opt = types.SimpleNamespace(epochs=1, adj_type="hic", model_name=None, lr_decay2=0, load_gcn=True, test_only=True)
        if cw is not None:
            opt.compartment_of_window = {"test": cw}
        optim = torch.optim.SGD(model.parameters(), lr=0.25, momentum=0.9, weight_decay=1e-6)
        hist[name] = runner.run_model(None, model, {}, {}, test, None, optim, None, opt, None, graphs=graphs,
                                      verbose=name == "split")[0]["test"]
    out = capsys.readouterr().out
    assert "test, compartment A (200 windows):" in out and "test, compartment B (100 windows):" in out
    assert "compartments" not in hist["off"]
    by = hist["split"]["compartments"]
    assert sorted(by) == ["A", "B"] and sorted(by["A"]) == sorted(bootstrap.METRICS) and by["A"] != by["B"]
    assert all(0 <= v <= 1 for m in by.values() for v in m.values())
    whole = hist["all_a"]["compartments"]                      # every window in A: the split's own float64 point estimate
    assert abs(whole["A"]["auroc"] - hist["all_a"]["meanAUC"]) < 1e-4 and abs(whole["A"]["aupr"] - hist["all_a"]["meanAUPR"]) < 1e-4
    assert all(np.isnan(v) for v in whole["B"].values())
