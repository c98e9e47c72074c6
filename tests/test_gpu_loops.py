"""The loop kernels (csrc/cgcn_loops.hip) against the numpy restatement of chromegcn_amd/loops.py, fed the device matrix read
back so that the comparison does not lean on the aggregation: the band bit for bit, the local expected values bit for bit with
the same NaN pattern, the histograms and the ordered pixel list exactly; HicContacts.loops against loops_host on planted maps;
the loop-restricted device build against the host builder (indptr and indices exactly).
Sizes: a tile is 8 rows x 32 distances with a halo of w rows and 2 w distances, so the bin counts sit either side of 8 and 64,
the distances either side of 32 and 64 and beyond n, and the half-widths run from (0, 1) to the largest (9, 10); 257 x 66 pixels
cross many tiles and many 256-pixel compaction tiles; 5 001 x 201 pixels are far more tiles than compute units."""
import functools

import numpy as np
import pytest
import torch

from chromegcn_amd import HicContacts, build_hic_graph_host, hicmap, loops

import loops_cases as LC

pytestmark = pytest.mark.gpu
DEV = "cuda"
PW = [(0, 1), (1, 3), (2, 5), (4, 7), (9, 10)]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


@functools.lru_cache(maxsize=None)
def device_case(name):
    """(the device matrix, the matrix read back) of a hicnorm case"""
    c = LC.case(name)
    A = HicContacts(c["pos1"], c["pos2"], c["count"], DEV).contact_matrix(c["res"], c["n_bins"])
    return A, A.to_host()


@functools.lru_cache(maxsize=None)
def device_map(n, seed=0, density=0.5, reach=None, top=40, empty=()):
    """(the device matrix, the matrix read back, its row sums) of a sparse integer map with n bins, the bins `empty` left out"""
    p1, p2, cnt = LC.records_of(LC.sparse_integer_map(n, n if reach is None else reach, 100 + n + seed, density=density, top=top))
    k = ~np.isin(p1 // LC.RES, empty) & ~np.isin(p2 // LC.RES, empty)
    A = HicContacts(p1[k], p2[k], cnt[k], DEV).contact_matrix(LC.RES, n)
    host = A.to_host()
    return A, host, np.asarray(host.sum(axis=1)).ravel()


def dev(v):
    return None if v is None else torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).to(DEV)


@pytest.mark.parametrize("name", ["n1", "n2", "n63", "n64", "n65", "fullrow", "n257_frac"])
def test_band(name):
    A, host = device_case(name)
    for width in (1, 63, 64, 65, 400):       # either side of a wavefront; 400 exceeds every n here
        got = hicmap.device_band(A, width).cpu().numpy()
        assert same_bits(got, hicmap.band_host(host, width)), width
    with pytest.raises(ValueError):
        hicmap.device_band(A, 0)


def d_values(n, md):
    return sorted({md, 60, 63, 64, 65, max(n - 1, 0), n + 10})


@pytest.mark.parametrize("with_norm", [False, True], ids=["raw", "noisy_norm"])
@pytest.mark.parametrize("n", [2, 15, 64, 65, 200, 257])
def test_lambda_bit_for_bit(n, with_norm):
    check_lambda(n, with_norm)


@pytest.mark.parametrize("with_norm", [False, True], ids=["raw", "noisy_norm"])
def test_lambda_bit_for_bit_beside_empty_bins(with_norm):
    """bins without a contact next to the vector's NaN, 0 and +inf bins and its missing last bin"""
    A, host, vc = device_map(130, empty=(7, 64, 129))
    assert np.all(vc[[7, 64, 129]] == 0)
    check_lambda(130, with_norm, empty=(7, 64, 129))


def check_lambda(n, with_norm, empty=()):
    A, host, vc = device_map(n, empty=empty)
    norm = LC.noisy_norm(n, 70 + n, inf=bool(empty)) if with_norm else None
    ex = np.random.default_rng(n).uniform(0.2, 3.0, n)
    candidates = 0
    for p, w in PW:
        for D in d_values(n, p + 3):
            r = loops.loop_rule(LC.RES, n, p=p, w=w, max_distance_bp=D * LC.RES)
            assert r.D == D and r.min_dist == p + 3
            want_lam, want_cand = loops.loop_lambdas_host(hicmap.band_host(host, r.width), vc, norm, ex, p, w, D)
            band = hicmap.device_band(A, r.width)
            hist, flags, lam = loops.loop_histograms(band, A.vc, dev(norm), dev(ex), r, want_lambda=True)
            hist2, flags2, lam2 = loops.loop_histograms(band, A.vc, dev(norm), dev(ex), r, want_lambda=True)
            lam, lam2 = lam.cpu().numpy(), lam2.cpu().numpy()
            assert same_bits(lam, want_lam), (p, w, D)                    # the NaN pattern included
            assert same_bits(lam, lam2) and torch.equal(hist, hist2) and torch.equal(flags, flags2)
            assert np.array_equal((flags.cpu().numpy() < 0), want_cand)   # bit 31: the candidate
            want_hist = loops.loop_histograms_host(hicmap.band_host(host, r.width), want_lam, want_cand)
            assert np.array_equal(hist.cpu().numpy(), want_hist)
            candidates += int(want_cand.sum())
    assert candidates > 0 or n < 15


def check_hist_and_pixels(A, host, vc, norm, ex, r, thresholds=("computed",)):
    hband = hicmap.band_host(host, r.width)
    t = loops.chunk_boundaries(r.K)
    want_lam, want_cand = loops.loop_lambdas_host(hband, vc, norm, ex, r.p, r.w, r.D, r.ignore_diags, r.min_dist)
    want_hist = loops.loop_histograms_host(hband, want_lam, want_cand, t, r.W - 1)
    band = hicmap.device_band(A, r.width)
    hist, flags, _ = loops.loop_histograms(band, A.vc, dev(norm), dev(ex), r, t)
    hist = hist.cpu().numpy()
    assert np.array_equal(hist, want_hist)
    assert np.all(hist.sum(axis=(1, 2)) == want_cand.sum())
    out = {}
    for kind in thresholds:
        thr = {"computed": lambda: loops.loop_thresholds(want_hist, r.fdr, t), "all_W": lambda: np.full((4, r.K), r.W, np.int32),
               "all_0": lambda: np.zeros((4, r.K), np.int32)}[kind]()
        want = loops.enriched_pixels_host(hband, want_lam, want_cand, thr, t, r.W - 1)
        got = loops.enriched_pixels(band, A.vc, dev(norm), dev(ex), r, flags, thr)
        assert np.array_equal(got.i, want.i) and np.array_equal(got.j, want.j), kind      # the same pixels in the same order
        assert same_bits(got.observed, want.observed) and same_bits(got.lam, want.lam), kind
        out[kind] = (want, int(want_cand.sum()))
    return out, want_hist


@pytest.mark.parametrize("with_norm", [False, True], ids=["raw", "noisy_norm"])
def test_histograms_and_pixels(with_norm):
    n, D = 257, 65
    A, host, vc = device_map(n)
    norm = LC.noisy_norm(n, 70 + n) if with_norm else None
    ex = np.random.default_rng(5).uniform(2.0, 30.0, n)
    r = loops.loop_rule(LC.RES, n, p=1, w=3, max_distance_bp=D * LC.RES, fdr=0.5)
    out, _ = check_hist_and_pixels(A, host, vc, norm, ex, r, ("computed", "all_W", "all_0"))
    assert out["all_W"][0].i.size == 0
    assert out["all_0"][0].i.size == out["all_0"][1] > 10000              # every candidate: the list crosses many tiles
    assert 0 < out["computed"][0].i.size < out["all_0"][1]


def test_histogram_contended_and_clipped():
    """a map that is zero but for a few pixels: every candidate but those lands on o = 0 of a handful of chunks; and counts above
    max_count, which clip to the last cell"""
    n, D = 200, 60
    A, host, vc = device_map(n, seed=1, density=0.002, reach=50, top=4000)
    assert 5 < host.nnz < 60
    vc_all = np.ones(n)                                                   # validity must not depend on the few pixels
    Adev = type(A)(A.n, A.nnz, A.rowptr, A.col, A.val, torch.ones(n, dtype=torch.float64, device=DEV), A.row_nnz)
    ex = np.full(n, 0.5)
    r = loops.loop_rule(LC.RES, n, p=1, w=3, max_distance_bp=D * LC.RES, max_count=20)
    out, hist = check_hist_and_pixels(Adev, host, vc_all, None, ex, r, ("computed", "all_0"))
    total = out["all_0"][1]
    assert total > 9000 and hist[0, :, 0].sum() > total - 60              # the contended cells
    assert hist[0, :, 20].sum() > 0 and hist[:, :, 1:20].sum() >= 0       # the clipped cell: counts up to 3 999 at max_count = 20
    assert hist[0, 0, 0] > total // 2                                     # lambda = 0 nearly everywhere: one word takes them all


def test_larger_grid():
    n, D = 5001, 200
    A, host, vc = device_map(n, density=0.05, reach=220)
    ex = 3.0 / (1.0 + np.arange(n))
    r = loops.loop_rule(10000, n)                                          # (2, 5), D = 200, W = 10 001, K = 40
    assert (r.p, r.w, r.D) == (2, 5, D)
    out, _ = check_hist_and_pixels(A, host, vc, None, ex, r)
    assert out["computed"][1] > 900000 and out["computed"][0].i.size > 0


def ulps(a, b):
    """the largest distance of two float64 arrays in units in the last place (same shape, no NaN)"""
    a, b = np.ascontiguousarray(a, dtype=np.float64).view(np.int64), np.ascontiguousarray(b, dtype=np.float64).view(np.int64)
    return int(np.max(np.abs(a - b))) if a.size else 0


def assert_same_loops(got, want):
    assert len(got) == len(want) > 0
    assert np.array_equal(got.peak_i, want.peak_i) and np.array_equal(got.peak_j, want.peak_j)
    assert np.array_equal(got.n_pixels, want.n_pixels) and same_bits(got.observed, want.observed)
    assert same_bits(got.centroid, want.centroid) and same_bits(got.radius, want.radius)
    assert np.array_equal(got.info["thresholds"], want.info["thresholds"])
    assert [got.info[k] for k in ("candidates", "enriched", "kept_after_ratios")] == \
           [want.info[k] for k in ("candidates", "enriched", "kept_after_ratios")]
    print("lambda: %d ulp apart at most" % ulps(got.lam, want.lam))
    assert same_bits(got.lam, want.lam) and np.array_equal(got.k, want.k)


@pytest.mark.parametrize("seed", [0, 1])
def test_end_to_end_on_planted_loops_explicit_vector(seed):
    c, want = LC.planted(seed), LC.planted_host(seed, "explicit")
    hc = HicContacts(c["pos1"], c["pos2"], c["count"], DEV)
    got = hc.loops("VC", c["res"], LC.planted_vectors(seed)[1], n_bins=c["n_bins"], **LC.P_RULE)
    assert_same_loops(got, want)
    assert got.info["host_syncs"] == 3 and LC.matched(got, c["plants"]) == (LC.P_BLOBS, 0)
    with pytest.raises(ValueError):
        hc.loops("VC", c["res"], "auto", p=2, w=11)
    with pytest.raises(ValueError):
        hc.loops("VC", 20000)


@pytest.mark.parametrize("seed", [0, 1])
def test_end_to_end_on_planted_loops_auto_vector(seed):
    """HicContacts.loops(expected="auto") against loops_host(expected="auto"): identical loops, bit-equal lambda.  Every lambda
    is a multiple of ex[d], so this holds only because loops_host forms its "auto" vector from the distance sums in the DEVICE's
    summation order (hicdist.distance_sums_device_order_host; test_distance_sums_in_device_order pins that restatement).  With
    np.bincount's record order the two vectors were up to 90 ulp apart on seed 1 and lambda up to 77 ulp; that distance is
    printed here for the record."""
    c, want = LC.planted(seed), LC.planted_host(seed, "auto")
    hc = HicContacts(c["pos1"], c["pos2"], c["count"], DEV)
    got = hc.loops("VC", c["res"], "auto", n_bins=c["n_bins"], **LC.P_RULE)
    assert hc.loops("VC", c["res"], "auto", n_bins=c["n_bins"], **LC.P_RULE) is got          # kept per argument tuple
    from chromegcn_amd import hicdist
    ex_dev = hc.expected_vector("VC", c["res"], n_bins=c["n_bins"]).cpu().numpy()
    ex_host = hicdist.expected_vector_host(c["pos1"], c["pos2"], c["count"], "VC", c["res"], n_bins=c["n_bins"])
    print("seed %d: the device's vector is %d ulp from the record-order vector at most" % (seed, ulps(ex_dev, ex_host)))
    sums = hicdist.distance_sums_device_order_host(c["pos1"], c["pos2"], c["count"], "VC", c["res"], c["n_bins"])
    assert same_bits(ex_dev, hicdist.expected_from_sums(*sums))
    assert_same_loops(got, want)


def many_tiles_records(seed=3, n=300, m=20000):
    """fractional counts at three distances only: some 6 700 records = 105 tiles of 64 per distance, so that a lane of the fold
    adds more than one partial"""
    rng = np.random.default_rng(seed)
    i = rng.integers(0, n - 2, m)
    j = i + rng.integers(0, 3, m)
    sw = rng.random(m) < 0.3
    return (np.where(sw, j, i) * LC.RES).astype(np.int32), (np.where(sw, i, j) * LC.RES).astype(np.int32), rng.uniform(0.1, 9.0, m), n


@pytest.mark.parametrize("name", ["planted1", "n63", "n64", "n65", "n257_frac", "many_tiles"])
def test_distance_sums_in_device_order(name):
    """hicdist.distance_sums_device_order_host IS cgcn_hicdist_sums: the same bits without a vector, with a noisy vector and
    with the records' VC vector (read back from the device), where np.bincount's record order differs in the last places"""
    from chromegcn_amd import hicdist
    if name == "planted1":
        c = LC.planted(1)
        p1, p2, cnt, n, res = c["pos1"], c["pos2"], c["count"], c["n_bins"], c["res"]
    elif name == "many_tiles":
        p1, p2, cnt, n = many_tiles_records()
        res = LC.RES
    else:
        c = LC.case(name)
        p1, p2, cnt, n, res = c["pos1"], c["pos2"], c["count"], c["n_bins"], c["res"]
    hc = HicContacts(p1, p2, cnt, DEV)
    differs = False
    for norm in (None, LC.noisy_norm(n, 4), "VC"):
        raw, act = hc.distance_sums(norm, res, n)
        # the VC vector of fractional counts has a summation order of its own: the host is fed the device's vector read back
        nv = hc.norm_vector("VC", res, n).cpu().numpy() if isinstance(norm, str) else norm
        want_raw, want_act = hicdist.distance_sums_device_order_host(p1, p2, cnt, nv, res, n)
        assert same_bits(raw.cpu().numpy(), want_raw) and same_bits(act.cpu().numpy(), want_act), (name, type(norm))
        differs = differs or not np.array_equal(want_act, hicdist.distance_sums_host(p1, p2, cnt, nv, res, n)[1])
    if name in ("n257_frac", "many_tiles"):
        assert differs                                  # the case does tell the two orders apart


@pytest.mark.parametrize("seed", [0, 1])
def test_auto_is_the_device_vector(seed):
    """expected = "auto" is HicContacts.expected_vector with the call's norm: the host restatement fed that vector read back
    gives the same loops and the same bits"""
    c = LC.planted(seed)
    hc = HicContacts(c["pos1"], c["pos2"], c["count"], DEV)
    got = hc.loops("VC", c["res"], "auto", n_bins=c["n_bins"], **LC.P_RULE)
    ex = hc.expected_vector("VC", c["res"], n_bins=c["n_bins"]).cpu().numpy()
    want = loops.loops_host(c["pos1"], c["pos2"], c["count"], "VC", c["res"], ex, n_bins=c["n_bins"], **LC.P_RULE)
    assert_same_loops(got, want)


def test_within_loops_and_the_restricted_build():
    from test_insulation_host import DOMAIN_BP, DOMAINS
    c, ws = LC.graph_case()
    hc = HicContacts(c["pos1"], c["pos2"], c["count"], DEV)
    found = loops.Loops(5 * c["res"], 24, np.array([1, 8, 12]), np.array([3, 14, 15]), np.zeros((3, 2)), np.zeros(3),
                        np.ones(3, np.int64), np.ones(3), np.ones((3, 4)), np.zeros((3, 4), np.int64))
    for pad in (0, 1, 2):
        keep = loops.same_loop_host(c["pos1"], c["pos2"], found, pad)
        sel = hc.within_loops(found, pad)
        assert 0 < sel.M == int(keep.sum()) < hc.M
        assert np.array_equal(sel.pos1.cpu().numpy(), c["pos1"][keep]) and np.array_equal(sel.pos2.cpu().numpy(), c["pos2"][keep])
        assert np.array_equal(sel.count.cpu().numpy(), c["count"][keep])                    # file order
    for norm, ex in ((None, None), ("VC", "auto")):
        kw = dict(min_distance_bp=2000, expected=ex)
        want = build_hic_graph_host(c["pos1"], c["pos2"], c["count"], norm, c["res"], ws, LC.GRAPH_EDGES, loops=(found, 1), **kw)
        _, raw = hc.build(norm, c["res"], ws, LC.GRAPH_EDGES, return_raw=True, loops=(found, 1), **kw)
        assert raw.nnz > 0 and np.array_equal(raw.indptr, want.indptr) and np.array_equal(raw.indices, want.indices)
        assert loops.loop_edge_share(raw, found, ws, 1) == (raw.nnz, raw.nnz)
        want = build_hic_graph_host(c["pos1"], c["pos2"], c["count"], norm, c["res"], ws, LC.GRAPH_EDGES, loops=(found, 1),
                                    domains=(DOMAINS, DOMAIN_BP), **kw)
        _, both = hc.build(norm, c["res"], ws, LC.GRAPH_EDGES, return_raw=True, loops=(found, 1), domains=(DOMAINS, DOMAIN_BP), **kw)
        assert 0 < both.nnz < raw.nnz and np.array_equal(both.indptr, want.indptr) and np.array_equal(both.indices, want.indices)
        plain = hc.build(norm, c["res"], ws, LC.GRAPH_EDGES, **kw)
        none = hc.build(norm, c["res"], ws, LC.GRAPH_EDGES, loops=None, **kw)
        assert plain.nnz == none.nnz and torch.equal(plain.rowptr, none.rowptr) and torch.equal(plain.col[:plain.nnz], none.col[:none.nnz])
        inside, nnz = loops.loop_edge_share(plain, found, ws, 1)
        assert 0 < inside < nnz == plain.nnz
    empty = loops.Loops(5 * c["res"], 24, np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros((0, 2)), np.zeros(0),
                        np.zeros(0, np.int64), np.zeros(0), np.zeros((0, 4)), np.zeros((0, 4), np.int64))
    assert hc.within_loops(empty).M == 0


def test_graphs_from_contact_caches_with_loops(tmp_path):
    from chromegcn_amd import hic
    c = LC.planted(1)
    ws = (np.arange(0, LC.P_N) * LC.P_RES).astype(np.int32)
    hic.save_contacts_cache(hic.contact_cache_path(str(tmp_path), "chrT"), hic.HostContacts(c["pos1"], c["pos2"], c["count"], {}, LC.P_RES, ws))
    kw = dict(norm="VC", resolution_bp=LC.P_RES, expected=LC.planted_vectors(1)[1], n_bins=LC.P_N, **LC.P_RULE)
    report = {}
    g = hic.graphs_from_contact_caches(str(tmp_path), ["chrT"], 4000, "", loops=dict(kw, restrict=True, pad_bins=1),
                                       loop_report=report)["chrT"]
    found = LC.planted_host(1)
    want = build_hic_graph_host(c["pos1"], c["pos2"], c["count"], None, LC.P_RES, ws, 4000, loops=(found, 1))
    free = build_hic_graph_host(c["pos1"], c["pos2"], c["count"], None, LC.P_RES, ws, 4000)
    assert g.nnz == want.nnz + ws.size                                     # the normaliser's self loops
    called, inside, nnz = report["chrT"]
    assert np.array_equal(called.peak_i, found.peak_i) and (inside, nnz) == loops.loop_edge_share(free, found, ws, 1)
    plain = hic.graphs_from_contact_caches(str(tmp_path), ["chrT"], 4000, "")["chrT"]       # the default: as it was
    assert plain.nnz == free.nnz + ws.size
