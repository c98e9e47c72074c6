"""Distance sums, the expected vector and the distance-aware graph builds on the device (csrc/cgcn_hicdist.hip, the *_dist
variants of csrc/cgcn_hic.hip) against the numpy restatement that tests/test_hic_distance_host.py ties to the definitions.
Integer sums are compared bit for bit, fractional ones within the bound of a reordered sum of non-negative terms, graphs
exactly (indptr and indices).  Sizes: the distance-sum passes work on 64-record wavefront tiles in workgroups of 256, and
the fold of one distance takes 64 tiles per trip, so the record counts sit on both sides of 64 and 256, one distance spans
more than 64 tiles, and one case has more than 65 535 distances."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from chromegcn_amd import HicNormError, _lib, build_hic_graph, build_hic_graph_host, hic, hic_expected_vector, hicdist, hicnorm, synth  # noqa: F401

import hicnorm_cases as HC
from test_hic_distance_host import graph_records

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -53
BAD_ARG, UNSUPPORTED, WORKSPACE = -1, -2, -4


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def head(c, m):
    return dict(c, pos1=c["pos1"][:m], pos2=c["pos2"][:m], count=c["count"][:m])


def one_distance(m=10000, n_bins=300, d=5, seed=3):
    """m records, all of them d bins apart, fractional counts: 157 tiles of one run"""
    rng = np.random.default_rng(seed)
    i = rng.integers(0, n_bins - d, m)
    swap = rng.random(m) < 0.5
    p1, p2 = i * HC.RES + rng.integers(0, HC.RES, m), (i + d) * HC.RES + rng.integers(0, HC.RES, m)
    return dict(pos1=np.where(swap, p2, p1).astype(np.int32), pos2=np.where(swap, p1, p2).astype(np.int32),
                count=rng.uniform(0.5, 30.0, m), res=HC.RES, n_bins=n_bins)


def noisy_norm(n_bins, seed, inf=False):
    rng = np.random.default_rng(seed)
    nv = rng.lognormal(0.0, 0.5, n_bins)
    if n_bins > 8:
        bad = rng.choice(n_bins, 4, replace=False)
        nv[bad] = [np.nan, 0.0, np.nan, 0.0]
        if inf:
            nv[np.setdiff1d(np.arange(n_bins), bad)[0]] = np.inf
    return nv


SUM_CASES = {
    "n1": lambda: HC.case("n1"),
    "m63": lambda: head(HC.case("n65"), 63), "m64": lambda: head(HC.case("n65"), 64), "m65": lambda: head(HC.case("n65"), 65),
    "m255": lambda: head(HC.case("n65"), 255), "m256": lambda: head(HC.case("n65"), 256), "m257": lambda: head(HC.case("n65"), 257),
    "n257_frac": lambda: HC.case("n257_frac"),
    "m70k_n257": lambda: HC.hic_like(257, 200000, 17, dup_share=1.7, n_empty=3),     # every short distance spans many tiles
    "one_distance": one_distance,
    "n70001": lambda: HC.case("n70001"),                                            # distances beyond 65 535
}


@functools.lru_cache(maxsize=None)
def sum_case(name):
    return SUM_CASES[name]()


def check_sums(c, norm, what, n_bins="given"):
    n_bins = c["n_bins"] if n_bins == "given" else n_bins
    raw_h, act_h = hicdist.distance_sums_host(c["pos1"], c["pos2"], c["count"], norm, c["res"], n_bins)
    dev = hic.HicContacts(c["pos1"], c["pos2"], c["count"], DEV)
    raw_d, act_d = (t.cpu().numpy() for t in dev.distance_sums(norm, c["res"], n_bins))
    dev._dist_sums.clear()   # the second call computes again
    raw_2, act_2 = (t.cpu().numpy() for t in dev.distance_sums(norm, c["res"], n_bins))
    assert same_bits(raw_d, raw_2) and same_bits(act_d, act_2), what
    d = np.abs(c["pos1"].astype(np.int64) // c["res"] - c["pos2"].astype(np.int64) // c["res"])
    k = np.bincount(d, minlength=raw_h.size)
    bound = 2.0 * np.maximum(k - 1, 0) * U
    if np.all(c["count"] == np.floor(c["count"])):
        assert same_bits(raw_d, raw_h), what
    for name, got, want in (("raw", raw_d, raw_h), ("act", act_d, act_h)):
        assert np.array_equal(got == 0, want == 0), (what, name)
        nz = want != 0
        err = np.abs(got[nz] / want[nz] - 1.0)
        worst = float((err / np.maximum(bound[nz], U)).max()) if nz.any() else 0.0
        print("%s %s: M=%d, n_bins=%d, most records at one distance %d, worst error / bound %.3g"
              % (what, name, c["pos1"].size, raw_h.size, int(k.max()) if k.size else 0, worst))
        assert np.all(err <= bound[nz]), (what, name)
    return dev


@pytest.mark.parametrize("name", list(SUM_CASES))
def test_distance_sums_equal_the_host(name):
    """raw bit-equal for integer counts; every raw[d], act[d] within 2 (k_d - 1) 2^-53 relative of np.bincount (two orders of
    k_d non-negative terms, each within (k_d - 1) 2^-53 of the exact sum); the same bits from a second call"""
    c = sum_case(name)
    check_sums(c, None, name + " RAW")
    check_sums(c, noisy_norm(c["n_bins"], 9), name + " vector")
    if name == "m65":   # n_bins left to the device, a vector shorter than the bins, and more bins than the records reach
        dev = check_sums(c, noisy_norm(20, 9), name + " short vector", n_bins=None)
        assert dev.distance_sums(None, c["res"])[0].numel() == int(max(c["pos1"].max(), c["pos2"].max())) // c["res"] + 1
        check_sums(c, None, name + " wide", n_bins=300)
    if name == "m70k_n257":   # NaN, 0 and +inf entries beside empty bins, n_bins no multiple of 64
        check_sums(c, noisy_norm(c["n_bins"], 9, inf=True), name + " vector with +inf")


def test_bad_records_are_refused():
    c = sum_case("m257")
    for over, match in ((dict(count=np.where(np.arange(257) == 200, np.nan, c["count"])), "finite"),
                        (dict(count=np.where(np.arange(257) == 3, -1.0, c["count"])), "finite"),
                        (dict(count=np.where(np.arange(257) == 70, np.inf, c["count"])), "finite"),
                        (dict(pos2=np.where(np.arange(257) == 256, -1, c["pos2"]).astype(np.int32)), "non-negative")):
        bad = dict(c, **over)
        for n_bins in (None, c["n_bins"]):
            with pytest.raises(ValueError, match=match):
                hic.HicContacts(bad["pos1"], bad["pos2"], bad["count"], DEV).distance_sums(None, c["res"], n_bins)
            with pytest.raises(ValueError, match=match):
                hicdist.distance_sums_host(bad["pos1"], bad["pos2"], bad["count"], None, c["res"], n_bins)
    with pytest.raises(ValueError, match="n_bins=10 but the records reach bin"):
        hic.HicContacts(c["pos1"], c["pos2"], c["count"], DEV).distance_sums(None, c["res"], 10)
    empty = hic.HicContacts(np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0), DEV)
    assert empty.distance_sums(None, 1000)[0].numel() == 0
    raw, act = empty.distance_sums(None, 1000, 5)
    assert raw.tolist() == [0.0] * 5 and act.tolist() == [0.0] * 5


@functools.lru_cache(maxsize=None)
def chr21():
    return synth.raw_contacts("chr21")


@pytest.mark.timeout(300)
def test_chr21_size():
    r = chr21()
    c = dict(pos1=r["pos1"], pos2=r["pos2"], count=r["count"], res=r["resolution_bp"], n_bins=None)
    check_sums(c, None, "chr21 RAW", n_bins=None)
    dev = check_sums(c, r["norm"], "chr21 vector", n_bins=None)
    ex, info = dev.expected_vector(None, c["res"], return_info=True)
    want, winfo = hicdist.expected_vector_host(c["pos1"], c["pos2"], c["count"], None, c["res"], return_info=True)
    print("chr21 expected: n_bins %d, w_max %d, whole range %d, host syncs %d" % (ex.numel(), info["w_max"], info["whole_range"],
                                                                                info["host_syncs"]))
    if np.all(c["count"] == np.floor(c["count"])):
        assert same_bits(ex.cpu().numpy(), want)
    assert info["w_max"] == winfo["w_max"] and info["whole_range"] == winfo["whole_range"] and info["host_syncs"] <= 3


@pytest.mark.parametrize("name", ["n1", "m65", "n257_frac", "m70k_n257"])
def test_expected_vector(name):
    """the device's vector IS expected_from_sums of the device's own sums; for RAW and integer counts it is the host's"""
    c = sum_case(name)
    dev = hic.HicContacts(c["pos1"], c["pos2"], c["count"], DEV)
    for norm in (None, noisy_norm(c["n_bins"], 4), "VC"):
        for min_count in (400, 50, 0):
            raw, act = (t.cpu().numpy() for t in dev.distance_sums(norm, c["res"], c["n_bins"]))
            ex, info = dev.expected_vector(norm, c["res"], c["n_bins"], min_count=min_count, return_info=True)
            want, winfo = hicdist.expected_from_sums(raw, act, min_count, return_info=True)
            assert ex.dtype == torch.float64 and ex.device.type == "cuda"
            assert same_bits(ex.cpu().numpy(), want), (name, min_count)
            assert (info["w_max"], info["whole_range"]) == (winfo["w_max"], winfo["whole_range"]) and 1 <= info["host_syncs"] <= 3
            if norm is None and np.all(c["count"] == np.floor(c["count"])):
                host = hicdist.expected_vector_host(c["pos1"], c["pos2"], c["count"], None, c["res"], c["n_bins"], min_count)
                assert same_bits(ex.cpu().numpy(), host), (name, min_count)
    again = dev.expected_vector("VC", c["res"], c["n_bins"], min_count=50)
    assert again is dev.expected_vector("VC", c["res"], c["n_bins"], min_count=50)        # kept per argument tuple
    top = hic_expected_vector(c["pos1"], c["pos2"], c["count"], None, c["res"], c["n_bins"], device=DEV)
    assert same_bits(top.cpu().numpy(), dev.expected_vector(None, c["res"], c["n_bins"]).cpu().numpy())


# ----------------------------------------------------------------------------------------------
# builds
# ----------------------------------------------------------------------------------------------
def assert_same_csr(raw, want, what):
    assert raw.shape == want.shape, what
    assert np.array_equal(raw.indptr, want.indptr) and np.array_equal(raw.indices, want.indices), what


def both_builds(c, ws, res, norm, edges, what, window_bp=None, **kw):
    dev = hic.HicContacts(c["pos1"], c["pos2"], c["count"], DEV)
    _, raw = dev.build(norm, res, ws, edges, return_raw=True, window_bp=window_bp, **kw)
    want = build_hic_graph_host(c["pos1"], c["pos2"], c["count"], norm, res, ws, edges, window_bp=window_bp, **kw)
    assert_same_csr(raw, want, what)
    return raw, dev


def bad_vector(c, res, keep=60):
    """an expected vector with NaN, 0, negative and inf entries, shorter than the largest distance"""
    ex = hicdist.expected_vector_host(c["pos1"], c["pos2"], c["count"], None, res, min_count=50)[:keep].copy()
    ex[[3, 7, 11, 15]] = [np.nan, 0.0, -1.0, np.inf]
    return ex


@pytest.mark.parametrize("up", [1, 5])
def test_builds_equal_the_host(up):
    c, ws, res = graph_records(up)
    wbp = res // up if up > 1 else None
    nv = hicnorm.hic_norm_vector_host(c["pos1"], c["pos2"], c["count"], "VC", res)[0]
    nv = hicnorm.pad_vector(nv, int(ws[-1]) // res + 1)
    ex_vc = hicdist.expected_vector_host(c["pos1"], c["pos2"], c["count"], nv, res, min_count=50)
    plain, dev = both_builds(c, ws, res, nv, HC.GRAPH_EDGES, "plain", wbp)
    s0 = dev.survivors(ws, res, wbp)
    for gap_in_res, few in ((0.5, False), (1, False), (80, True), (200, True)):
        gap = int(gap_in_res * res)
        for ex, label in ((None, "gap alone"), (ex_vc, "vector"), (bad_vector(c, res), "bad vector")):
            raw, dev = both_builds(c, ws, res, nv, HC.GRAPH_EDGES, "%s gap %d up %d" % (label, gap, up), wbp, min_distance_bp=gap,
                                   expected=ex)
            s = dev.survivors(ws, res, wbp, min_distance_bp=gap)
            assert s == hic.survivor_values(c["pos1"], c["pos2"], c["count"], None, res, ws, wbp, gap)[0].size
            assert (s < HC.GRAPH_EDGES // 2) == few and (raw.nnz == 0) == (gap_in_res == 200) and s <= s0
            if ex is None and gap_in_res <= 1 and up == 1:   # grid records that differ are at least res apart
                assert_same_csr(raw, plain, "a gap of res changes nothing")
                assert s == s0
    both_builds(c, ws, res, None, HC.GRAPH_EDGES, "no norm, a vector", wbp, expected=ex_vc)
    both_builds(c, ws, res, None, HC.GRAPH_EDGES, "no norm, an empty vector", wbp, expected=np.zeros(0))


@pytest.mark.parametrize("up", [1, 5])
def test_defaults_are_the_existing_entry_points(up):
    """min_distance_bp = 0 and expected = NULL through the *_dist entry points: the arrays of cgcn_hic_build / _build_up"""
    c, ws, res = graph_records(up)
    dev = hic.HicContacts(c["pos1"], c["pos2"], c["count"], DEV)
    wbp = res // up
    cap = dev.survivors(ws) if up == 1 else dev.survivors(ws, res, wbp)
    n, k = int(ws.size), HC.GRAPH_EDGES // 2
    nv = torch.from_numpy(hicnorm.pad_vector(hicnorm.hic_norm_vector_host(c["pos1"], c["pos2"], c["count"], "VC", res)[0],
                                             int(ws[-1]) // res + 1)).to(DEV)
    extra = {} if up == 1 else dict(resolution_bp=res, window_bp=wbp, n_window_bins=int(ws[-1]) // wbp + 1)
    fn = "cgcn_hic_build" if up == 1 else "cgcn_hic_build_up"
    need = _lib.query("cgcn_hic_workspace_bytes" if up == 1 else "cgcn_hic_up_workspace_bytes", M=dev.M, N=n, capacity=cap, K=k, **extra)
    outs = []
    for dist in ({}, dict(min_distance_bp=0, expected=None, n_expected=0)):
        wsp = torch.empty(need, dtype=torch.uint8, device=DEV)
        rowptr = torch.full((n + 1,), -7, dtype=torch.int32, device=DEV)
        col = torch.full((2 * min(k, cap),), -7, dtype=torch.int32, device=DEV)
        sizes = torch.zeros(2, dtype=torch.int64, device=DEV)
        args = dict(M=dev.M, pos1=dev.pos1, pos2=dev.pos2, count=dev.count, norm=nv, n_bins=int(nv.numel()), resolution_bp=res,
                    window_start=dev._ws_dev, N=n, K=k, capacity=cap, workspace=wsp, workspace_bytes=need, rowptr_out=rowptr,
                    col_out=col, nnz_out=sizes.data_ptr(), n_survivors=sizes.data_ptr() + 8)
        _lib.call(fn + ("_dist" if dist else ""), **dict(args, **extra, **dist))
        outs.append((rowptr.cpu().numpy(), col.cpu().numpy(), sizes.cpu().numpy()))
    assert all(np.array_equal(a, b) for a, b in zip(*outs)) and outs[0][2][0] > 0 and outs[0][2][1] == cap
    count = torch.zeros(2, dtype=torch.int64, device=DEV)
    need0 = _lib.query("cgcn_hic_workspace_bytes" if up == 1 else "cgcn_hic_up_workspace_bytes", M=dev.M, N=n, capacity=0, K=0, **extra)
    _lib.call("cgcn_hic_count_dist" if up == 1 else "cgcn_hic_count_up_dist", M=dev.M, pos1=dev.pos1, pos2=dev.pos2,
              window_start=dev._ws_dev, N=n, min_distance_bp=0, workspace=torch.empty(need0, dtype=torch.uint8, device=DEV),
              workspace_bytes=need0, n_survivors=count, **extra)
    assert int(count[0]) == cap


def test_auto_raw_takes_the_tied_records_in_file_order():
    """expected="auto" without a norm: the vector is the host's bit for bit (integer counts), so the values are, and the
    K-th value is tied: the ordered tie take has to agree with the host's stable sort"""
    c, ws, res = graph_records(1)
    ex = hicdist.expected_vector_host(c["pos1"], c["pos2"], c["count"], None, res, min_count=400)
    v = np.sort(hic.survivor_values(c["pos1"], c["pos2"], c["count"], None, res, ws, expected=ex)[3])[::-1]
    k = HC.GRAPH_EDGES // 2
    assert v[k - 1] == v[k], "the case is meant to cut inside a run of equal values"
    for kw in ({}, dict(expected_args=dict(min_count=50)), dict(min_distance_bp=3000)):
        both_builds(c, ws, res, None, HC.GRAPH_EDGES, "auto RAW %r" % (kw,), expected="auto", **kw)
    c5, ws5, res5 = graph_records(5)
    both_builds(c5, ws5, res5, None, HC.GRAPH_EDGES, "auto RAW up 5", res5 // 5, expected="auto", min_distance_bp=res5)


@pytest.mark.parametrize("kind", ["VC", "KR"])
@pytest.mark.parametrize("min_count", [400, 50])
def test_auto_with_a_computed_norm_equals_the_host_graph_of_the_hosts_vectors(kind, min_count):
    """the device scores with ITS norm and expected vectors, the host with its own; they differ by roundings, and
    tests/test_hic_distance_host.py has checked that the K-th and the next value of this case are >= 1e-9 apart"""
    c, ws, res = graph_records(1)
    both_builds(c, ws, res, kind, HC.GRAPH_EDGES, "auto %s" % kind, expected="auto", expected_args=dict(min_count=min_count))


def test_graphs_from_contact_caches(tmp_path):
    for chrom, seed in (("chrA", 41), ("chrB", 42)):
        g, w = HC.graph_case(seed)
        hic.save_contacts_cache(hic.contact_cache_path(str(tmp_path), chrom), hic.HostContacts(g["pos1"], g["pos2"], g["count"], {}, g["res"], w))
    kw = dict(min_distance_bp=3000, expected="auto", expected_args=dict(min_count=50))
    graphs = hic.graphs_from_contact_caches(str(tmp_path), ["chrA", "chrB"], HC.GRAPH_EDGES, "", device=DEV, **kw)
    plain = hic.graphs_from_contact_caches(str(tmp_path), ["chrA", "chrB"], HC.GRAPH_EDGES, "", device=DEV)
    for chrom, seed in (("chrA", 41), ("chrB", 42)):
        g, w = HC.graph_case(seed)
        one, raw = build_hic_graph(g["pos1"], g["pos2"], g["count"], None, g["res"], w, HC.GRAPH_EDGES, device=DEV, return_raw=True, **kw)
        assert_same_csr(raw, build_hic_graph_host(g["pos1"], g["pos2"], g["count"], None, g["res"], w, HC.GRAPH_EDGES, **kw), chrom)
        got = graphs[chrom]
        assert got.n == one.n == 90 and got.nnz == one.nnz > 0
        assert torch.equal(got.rowptr, one.rowptr) and torch.equal(got.col[:got.nnz], one.col[:one.nnz])
        assert not (plain[chrom].nnz == got.nnz and torch.equal(plain[chrom].col[:got.nnz], got.col[:got.nnz]))   # it matters
    # a vector the cache stores under a name (tools/hic_ingest.py --compute-expected): the RAW one is the device's bit for bit
    for chrom, seed in (("chrA", 41), ("chrB", 42)):
        g, w = HC.graph_case(seed)
        stored = {"eRAW": hicdist.expected_vector_host(g["pos1"], g["pos2"], g["count"], None, g["res"], min_count=50)}
        hic.save_contacts_cache(hic.contact_cache_path(str(tmp_path), chrom), hic.HostContacts(g["pos1"], g["pos2"], g["count"], stored, g["res"], w))
    named = hic.graphs_from_contact_caches(str(tmp_path), ["chrA", "chrB"], HC.GRAPH_EDGES, "", device=DEV, min_distance_bp=3000, expected="eRAW")
    for chrom in ("chrA", "chrB"):
        assert named[chrom].nnz == graphs[chrom].nnz and torch.equal(named[chrom].col[:named[chrom].nnz], graphs[chrom].col[:graphs[chrom].nnz])
    with pytest.raises(ValueError, match="holds no 'eKR' vector"):
        hic.graphs_from_contact_caches(str(tmp_path), ["chrA"], HC.GRAPH_EDGES, "", device=DEV, expected="eKR")


def test_entry_points_reject_bad_arguments_before_any_launch():
    c, ws, res = graph_records(5)
    dev = hic.HicContacts(c["pos1"], c["pos2"], c["count"], DEV)
    wbp = res // 5
    cap = dev.survivors(ws, res, wbp)
    n, k, bins = int(ws.size), 400, int(ws[-1]) // wbp + 1
    ex = torch.ones(50, dtype=torch.float64, device=DEV)
    need = _lib.query("cgcn_hic_up_workspace_bytes", M=dev.M, N=n, capacity=cap, K=k, resolution_bp=res, window_bp=wbp, n_window_bins=bins)
    wsp = torch.empty(need, dtype=torch.uint8, device=DEV)
    rowptr = torch.full((n + 1,), -7, dtype=torch.int32, device=DEV)
    col = torch.full((2 * k,), -7, dtype=torch.int32, device=DEV)
    sizes = torch.full((2,), -7, dtype=torch.int64, device=DEV)
    direct = dict(M=dev.M, pos1=dev.pos1, pos2=dev.pos2, count=dev.count, norm=None, n_bins=0, resolution_bp=res, window_start=dev._ws_dev,
                  N=n, K=k, capacity=cap, min_distance_bp=1000, expected=ex, n_expected=50, workspace=wsp, workspace_bytes=need,
                  rowptr_out=rowptr, col_out=col, nnz_out=sizes.data_ptr(), n_survivors=sizes.data_ptr() + 8)
    upd = dict(direct, window_bp=wbp, n_window_bins=bins)
    for fn, good in (("cgcn_hic_build_dist", direct), ("cgcn_hic_build_up_dist", upd)):
        for over, code in ((dict(min_distance_bp=-1), BAD_ARG), (dict(n_expected=-1), BAD_ARG), (dict(n_expected=0), BAD_ARG),
                           (dict(resolution_bp=0), BAD_ARG), (dict(M=-1), BAD_ARG), (dict(pos1=None), BAD_ARG),
                           (dict(rowptr_out=None), BAD_ARG), (dict(workspace=None), BAD_ARG), (dict(K=2 ** 30), UNSUPPORTED),
                           (dict(workspace_bytes=256), WORKSPACE)):
            assert _lib.query(fn, **dict(good, **over)) == code, (fn, over)
    cnt = dict(M=dev.M, pos1=dev.pos1, pos2=dev.pos2, window_start=dev._ws_dev, N=n, min_distance_bp=1000, workspace=wsp,
               workspace_bytes=need, n_survivors=sizes.data_ptr() + 8)
    cnt_up = dict(cnt, resolution_bp=res, window_bp=wbp, n_window_bins=bins)
    for fn, good in (("cgcn_hic_count_dist", cnt), ("cgcn_hic_count_up_dist", cnt_up)):
        for over, code in ((dict(min_distance_bp=-5), BAD_ARG), (dict(M=-1), BAD_ARG), (dict(pos2=None), BAD_ARG),
                           (dict(n_survivors=None), BAD_ARG), (dict(workspace_bytes=16), WORKSPACE)):
            assert _lib.query(fn, **dict(good, **over)) == code, (fn, over)
    assert _lib.query("cgcn_hic_count_up_dist", **dict(cnt_up, window_bp=1500)) == BAD_ARG
    raw = torch.full((300,), -7.0, dtype=torch.float64, device=DEV)
    act = torch.full((300,), -7.0, dtype=torch.float64, device=DEV)
    need_d = _lib.query("cgcn_hicdist_workspace_bytes", M=dev.M, n_bins=300)
    assert need_d > 0
    sums = dict(M=dev.M, pos1=dev.pos1, pos2=dev.pos2, count=dev.count, norm=None, n_norm=0, resolution_bp=res, n_bins=300,
                workspace=torch.empty(need_d, dtype=torch.uint8, device=DEV), workspace_bytes=need_d, raw_out=raw, act_out=act,
                sizes=sizes)
    for over, code in ((dict(M=-1), BAD_ARG), (dict(n_bins=-1), BAD_ARG), (dict(n_norm=-1), BAD_ARG), (dict(resolution_bp=0), BAD_ARG),
                       (dict(count=None), BAD_ARG), (dict(raw_out=None), BAD_ARG), (dict(act_out=None), BAD_ARG),
                       (dict(sizes=None), BAD_ARG), (dict(workspace=None), BAD_ARG), (dict(norm=ex, n_norm=0), BAD_ARG),
                       (dict(M=2 ** 31), UNSUPPORTED), (dict(n_bins=2 ** 31 - 1), UNSUPPORTED), (dict(workspace_bytes=need_d - 1), WORKSPACE)):
        assert _lib.query("cgcn_hicdist_sums", **dict(sums, **over)) == code, over
    assert _lib.query("cgcn_hicdist_workspace_bytes", M=2 ** 31, n_bins=300) == 0
    assert _lib.query("cgcn_hicdist_workspace_bytes", M=-1, n_bins=300) == 0
    assert _lib.query("cgcn_hicdist_workspace_bytes", M=10, n_bins=2 ** 31 - 1) == 0
    torch.cuda.synchronize()
    assert bool((rowptr == -7).all()) and bool((col == -7).all()) and bool((sizes == -7).all())     # nothing was launched
    assert bool((raw == -7).all()) and bool((act == -7).all())
    # python-side checks
    with pytest.raises(ValueError, match="negative"):
        dev.build(None, res, ws, 800, window_bp=wbp, min_distance_bp=-1)
    with pytest.raises(ValueError, match="auto"):
        dev.build(None, res, ws, 800, window_bp=wbp, expected="juicer")
    with pytest.raises(ValueError, match="norm kind"):
        dev.expected_vector("ICE", res)


def test_hic_ingest_stores_expected_vectors_that_old_caches_do_not_need(tmp_path):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    try:
        import hic_ingest
    finally:
        sys.path.pop(0)
    g, w = HC.graph_case(41)
    d = hic_ingest.chrom_dir(str(tmp_path / "hic"), "GM12878", "1", "chrA")
    os.makedirs(d)
    with open(os.path.join(d, "chrA_1kb.RAWobserved"), "w") as f:
        f.write("".join("%d\t%d\t%.1f\n" % rec for rec in zip(g["pos1"].tolist(), g["pos2"].tolist(), g["count"].tolist())))
    (tmp_path / "windows.bed").write_text("".join("chrA\t%d\t%d\tpeak\n" % (s, s + 1000) for s in w.tolist()))
    out = str(tmp_path / "caches")
    lines = hic_ingest.main(["--hic-root", str(tmp_path / "hic"), "--cell", "GM12878", "--bed", str(tmp_path / "windows.bed"), "--chroms",
                             "chrA", "--out", out, "--compute-expected", "RAW,VC"])
    assert lines[0]["norms"] == ["eRAW", "eVC"]
    c = hic.load_contacts_cache(hic.contact_cache_path(out, "chrA"))
    assert same_bits(c.norms["eRAW"], hicdist.expected_vector_host(g["pos1"], g["pos2"], g["count"], None, g["res"]))
    assert c.norms["eVC"].shape == c.norms["eRAW"].shape and np.all(c.norms["eVC"][:3] > 0)
    named = hic.graphs_from_contact_caches(out, ["chrA"], HC.GRAPH_EDGES, "", device=DEV, expected="eRAW", min_distance_bp=2000)["chrA"]
    auto = hic.graphs_from_contact_caches(out, ["chrA"], HC.GRAPH_EDGES, "", device=DEV, expected="auto", min_distance_bp=2000)["chrA"]
    assert named.nnz == auto.nnz > 0 and torch.equal(named.rowptr, auto.rowptr) and torch.equal(named.col[:named.nnz], auto.col[:auto.nnz])
    with pytest.raises(SystemExit, match="--compute-expected takes a subset"):
        hic_ingest.main(["--hic-root", "x", "--cell", "y", "--bed", "z", "--chroms", "chrA", "--out", out, "--compute-expected", "ICE"])
