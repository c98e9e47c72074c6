"""The loop rule on the host (chromegcn_amd/loops.py; no GPU): the offset lists, the band-shaped restatement against a literal
loop over pixels and cells, an exact plant whose local expected values equal the counts bit for bit, loop_thresholds against its
definition, loops_from_pixels on hand-made pixel lists, recovery of planted loops, the guards, and the loop restriction of the
host graph builder."""
import numpy as np
import pytest
from scipy.stats import poisson

from chromegcn_amd import build_hic_graph_host, hicmap, hicnorm, loops

import loops_cases as LC


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def literal_pixels(A, norm, ex, p, w, D, ignore_diags=2, min_dist=None):
    """rules 1 to 6, one pixel and one cell after the other from the dense matrix: (lam [4, n, D + 1], cand [n, D + 1])"""
    n = A.shape[0]
    md = p + ignore_diags + 1 if min_dist is None else min_dist
    valid = hicmap.valid_bins(A.sum(axis=1), norm)
    nv = np.ones(n) if norm is None else hicnorm.clean_norm(norm, n)
    offs = [o.tolist() for o in loops.neighbourhood_offsets(p, w)]
    lam, cand = np.full((4, n, D + 1), np.nan), np.zeros((n, D + 1), bool)
    for i in range(n):
        for d in range(md, D + 1):
            j = i + d
            if j >= n or not (valid[i] and valid[j]):
                continue
            res = []
            for lst in offs:
                S, T, C = 0.0, 0.0, 0
                for da, db in lst:
                    a, b = i + da, j + db
                    if a < 0 or b >= n or b - a < ignore_diags or not (valid[a] and valid[b]):
                        continue
                    S += A[a, b] / (nv[a] * nv[b])
                    T += ex[b - a] if b - a < len(ex) else 0.0
                    C += 1
                res.append((S, T, C, len(lst)))
            if all(T > 0 and 2 * C >= full for _, T, C, full in res):
                cand[i, d] = True
                for x, (S, T, _, _) in enumerate(res):
                    lam[x, i, d] = ((S / T) * ex[d]) * (nv[i] * nv[j])
    return lam, cand


def test_offset_lists_sizes_order_and_the_peak_box():
    for (p, w), sizes in {(1, 3): (32, 8, 12, 12), (2, 5): (84, 21, 18, 18), (4, 7): (132, 33, 18, 18)}.items():
        lists = loops.neighbourhood_offsets(p, w)
        assert tuple(o.shape[0] for o in lists) == sizes == (4 * (w * w - p * p), w * w - p * p, 6 * (w - p), 6 * (w - p))
        for o in lists:
            rows = [tuple(r) for r in o.tolist()]
            assert rows == sorted(set(rows))                                        # row-major, no repeats
            assert not any(abs(da) <= p and abs(db) <= p for da, db in rows)        # disjoint from the peak box
            assert all(abs(da) <= w and abs(db) <= w for da, db in rows)
        donut, ll, h, v = [set(map(tuple, o.tolist())) for o in lists]
        assert ll < donut and all(da >= 1 and db <= -1 for da, db in ll)
        assert all(da != 0 and db != 0 for da, db in donut)
        assert all(abs(da) <= 1 and p < abs(db) for da, db in h) and v == {(db, da) for da, db in h}
    assert loops.neighbourhood_offsets(0, 1)[0].tolist() == [[-1, -1], [-1, 1], [1, -1], [1, 1]]
    for bad in [(3, 3), (-1, 2), (2, 11)]:
        with pytest.raises(ValueError):
            loops.neighbourhood_offsets(*bad)


def test_chunk_boundaries_and_the_chunk_index():
    t = loops.chunk_boundaries()
    assert t.size == 39 and t[0] == 1.0 and t[3] == 2.0 and np.all(np.diff(t) > 0)
    assert same_bits(t, np.power(2.0, np.arange(39) / 3.0))


@pytest.mark.parametrize("p,w,D,with_norm", [(1, 3, 12, False), (1, 3, 30, True), (0, 1, 5, True), (2, 5, 9, False)])
def test_the_band_restatement_equals_the_literal_loop(p, w, D, with_norm):
    n = 23
    A = LC.sparse_integer_map(n, 20, 5 + D, density=0.6).toarray()
    A[7, :] = A[:, 7] = 0.0                                       # an empty bin
    norm = LC.noisy_norm(n, 9) if with_norm else None
    ex = np.random.default_rng(2).uniform(0.5, 3.0, n)
    want_lam, want_cand = literal_pixels(A, norm, ex, p, w, D)
    lam, cand = loops.loop_lambdas_host(hicmap.band_host(A, D + 2 * w + 1), A.sum(axis=1), norm, ex, p, w, D)
    assert np.array_equal(cand, want_cand) and cand.sum() > 0
    assert same_bits(lam, want_lam)


def test_exact_plant_lambda_equals_the_count_bit_for_bit():
    n, D, p, w = 40, 25, 1, 3
    g = np.round(300.0 / (1.0 + np.arange(n))) + 1.0              # integer counts falling with distance
    A = LC.constant_map(n, g)
    A[18, :] = A[:, 18] = 0.0                                     # an empty bin: not valid
    band = hicmap.band_host(A, D + 2 * w + 1)
    lam, cand = loops.loop_lambdas_host(band, A.sum(axis=1), None, g, p, w, D)
    i, d = np.nonzero(cand)
    for x in range(4):
        assert same_bits(lam[x][cand], A[i, i + d])               # S and T are the same terms in the same order
        assert np.all(np.isnan(lam[x][~cand]))
    # rule 5 by hand: the cells of a neighbourhood that lie inside the matrix, off the empty bin and at a distance >= 2
    offs = loops.neighbourhood_offsets(p, w)
    want = np.zeros_like(cand)
    for i in range(n):
        for d in range(p + 2 + 1, D + 1):
            j = i + d
            if j >= n or 18 in (i, j):
                continue
            ok = True
            for o in offs:
                a, b = i + o[:, 0], j + o[:, 1]
                c = int(np.sum((a >= 0) & (b < n) & (b - a >= 2) & (a != 18) & (b != 18)))
                ok = ok and 2 * c >= o.shape[0]
            want[i, d] = ok
    assert np.array_equal(cand, want)
    assert cand[0, 10] and not cand[0, 3]                         # the corner keeps half a donut; d < min_dist
    assert cand[17, 10] and not cand[18, 10] and not cand[8, 10]  # beside the empty bin; on it (as i and as j)
    assert not cand[n - 5, 10] and cand[n - 11, 10] and not cand[:, :4].any()
    # with every bin valid the top corner is cut twice: (0, d) loses the rows above, (n - 1 - d, d) the columns beyond
    hist = loops.loop_histograms_host(band, lam, cand)
    assert hist.shape == (4, 40, 10001) and np.all(hist.sum(axis=(1, 2)) == cand.sum())


def direct_threshold(h, lam, fdr):
    """rule 9 for one chunk, evaluated as it reads"""
    W, N = len(h), int(sum(h))
    for o in range(W):
        obs = int(sum(h[o:]))
        if obs > 0 and N * poisson.sf(o - 1, lam) <= fdr * obs:
            return o
    return W


def test_loop_thresholds_against_the_definition():
    rng = np.random.default_rng(4)
    K, W = 6, 30
    t = loops.chunk_boundaries(K)
    hist = np.zeros((4, K, W), np.int32)
    for x in range(4):
        for k in (0, 1, 3, 5):
            lam = t[min(k, K - 2)]
            c = np.minimum(rng.poisson(0.8 * lam, 400), W - 1)
            c[:3 + x] = np.minimum(rng.integers(12, 29, 3 + x), W - 1)       # a few enriched pixels
            hist[x, k] = np.bincount(c, minlength=W)
    thr = loops.loop_thresholds(hist, 0.1, t)
    assert thr.shape == (4, K) and thr.dtype == np.int32
    for x in range(4):
        for k in range(K):
            assert thr[x, k] == direct_threshold(hist[x, k].tolist(), t[min(k, K - 2)], 0.1), (x, k)
    assert np.all(thr[:, [2, 4]] == W)                                      # an empty chunk
    assert np.all(thr[:, [0, 1, 3, 5]] < W) and np.all(thr[:, [0, 1, 3, 5]] > 0)
    last = thr
    for fdr in (0.2, 0.5, 1.0):                                             # a larger fdr never raises a threshold
        nxt = loops.loop_thresholds(hist, fdr, t)
        assert np.all(nxt <= last)
        last = nxt
    with pytest.raises(ValueError):
        loops.loop_thresholds(hist, 0.1, t[:-1])


def pixels(rows):
    """Pixels from (i, j, observed[, lambda]) rows in (i, j) order; lambda = 1 for all four unless given"""
    rows = sorted(rows)
    lam = np.array([[r[3] if len(r) > 3 else 1.0] * 4 for r in rows], dtype=np.float64).reshape(-1, 4)
    return loops.Pixels(np.array([r[0] for r in rows]), np.array([r[1] for r in rows]), np.array([float(r[2]) for r in rows]), lam)


def test_clusters_two_blobs_a_chain_ties_and_strict_ratios():
    res = 10000                                                     # radius_bins = 2
    two = loops.loops_from_pixels(pixels([(10, 30, 50), (11, 30, 40), (10, 31, 30), (15, 35, 60), (16, 35, 20)]), res, 100)
    assert list(zip(two.peak_i.tolist(), two.peak_j.tolist())) == [(15, 35), (10, 30)] and two.n_pixels.tolist() == [2, 3]
    assert two.observed.tolist() == [60.0, 50.0] and two.info["kept_after_ratios"] == 5
    assert np.allclose(two.centroid, [[15.5, 35.0], [31.0 / 3, 91.0 / 3]]) and np.allclose(two.radius, [0.5, 2.0 / 3])
    # a chain along i: (24, 50) is 4 bins from the peak and comes in only as the centroid moves (20 -> 21 -> 21.67 -> 22); (27, 50)
    # stays out
    chain = loops.loops_from_pixels(pixels([(20, 50, 90), (22, 50, 80), (23, 50, 70), (23, 51, 60), (24, 50, 50), (27, 50, 10)]),
                                    res, 100)
    assert chain.n_pixels.tolist() == [5, 1] and chain.peak_i.tolist() == [20, 27]
    assert np.allclose(chain.centroid[0], [22.4, 50.2]) and np.isclose(chain.radius[0], 2.4)
    # the far end first in sorted order: it is reached by the RESCAN, after the centroid has moved
    rescan = loops.loops_from_pixels(pixels([(20, 50, 90), (23, 50, 85), (22, 50, 80)]), res, 100)
    assert rescan.n_pixels.tolist() == [3]
    apart = loops.loops_from_pixels(pixels([(20, 50, 90), (23, 50, 85)]), res, 100)
    assert apart.n_pixels.tolist() == [1, 1]
    # ties in the count resolve by (i, j)
    tie = loops.loops_from_pixels(pixels([(31, 60, 7), (30, 61, 7), (30, 60, 7), (50, 90, 7)]), res, 100)
    assert list(zip(tie.peak_i.tolist(), tie.peak_j.tolist())) == [(30, 60), (50, 90)]
    # a ratio exactly at the limit is dropped: strict >
    edge = loops.loops_from_pixels(pixels([(10, 30, 7.0, 4.0), (40, 70, 7.0, 3.999), (60, 90, 6.0, 4.0)]), res, 100)
    assert list(zip(edge.peak_i.tolist(), edge.peak_j.tolist())) == [(40, 70)] and edge.info["kept_after_ratios"] == 1
    lam = np.array([[4.0, 1.0, 4.0, 4.0]])                          # 1.5 x 4 = 6 passes h and v, 1.75 x 4 = 7 does not pass the donut
    one = loops.Pixels(np.array([10]), np.array([30]), np.array([6.5]), lam)
    assert len(loops.loops_from_pixels(one, res, 100)) == 0
    assert len(loops.loops_from_pixels(one, res, 100, ratios=(1.5, 1.75, 1.5, 1.5))) == 1
    assert loops.loops_from_pixels(one, res, 100, ratios=(1.5,) * 4).k.tolist() == [[7, 1, 7, 7]]   # t_6 = 4 <= 4; t_0 = 1 <= 1
    small = loops.loops_from_pixels(pixels([(10, 30, 50), (11, 30, 40), (50, 90, 9)]), res, 100, min_cluster_pixels=2)
    assert small.peak_i.tolist() == [10]
    none = loops.loops_from_pixels(pixels([]), res, 100)
    assert len(none) == 0 and none.centroid.shape == (0, 2) and none.lam.shape == (0, 4) and none.to_bedpe("chr1") == ""


@pytest.mark.parametrize("seed", LC.SEEDS)
def test_planted_loops_are_recovered(seed):
    """Every plant is matched by a loop within one bin and there is no other loop: at most zero plants may be missed."""
    c, found = LC.planted(seed), LC.planted_host(seed)
    hit, extra = LC.matched(found, c["plants"])
    print("seed %d: %d loops, %d of %d plants matched, %d other loops, candidates %d, enriched %d, kept %d"
          % (seed, len(found), hit, len(c["plants"]), extra, found.info["candidates"], found.info["enriched"],
             found.info["kept_after_ratios"]))
    assert len(c["plants"]) - hit <= 0
    assert extra == 0 and len(found) == len(c["plants"])
    assert np.all(found.peak_i < found.peak_j) and np.all(found.n_pixels >= 1)
    assert np.array_equal(found.k, np.searchsorted(loops.chunk_boundaries(), found.lam, side="right"))
    lines = found.to_bedpe("chr9").splitlines()
    assert len(lines) == len(found) and lines[0].split("\t")[:6] == [
        "chr9", str(found.peak_i[0] * LC.P_RES), str((found.peak_i[0] + 1) * LC.P_RES), "chr9", str(found.peak_j[0] * LC.P_RES),
        str((found.peak_j[0] + 1) * LC.P_RES)]
    assert set(found.anchors().tolist()) == set(found.peak_i.tolist()) | set(found.peak_j.tolist())


def test_guards_and_argument_errors():
    with pytest.raises(ValueError, match="resolution_bp or a smaller max_distance_bp"):
        loops.loop_rule(10000, 2 ** 21, max_distance_bp=2000000)          # 2^21 x 201 > 2^28
    assert loops.loop_rule(10000, 2 ** 20).D == 200
    for bad in (dict(p=2, w=11), dict(n_chunks=65), dict(max_count=65536), dict(p=3, w=3), dict(p=-1, w=3), dict(fdr=0.0),
                dict(ignore_diags=-1), dict(min_dist=-1), dict(ratios=(1.5, 1.5))):
        with pytest.raises(ValueError):
            loops.loop_rule(10000, 100, **bad)
    with pytest.raises(ValueError, match="give p and w"):
        loops.loop_rule(20000, 100)
    with pytest.raises(TypeError):
        loops.loop_rule(10000, 100, window=3)
    assert [loops.loop_rule(r)[1:3] for r in (5000, 10000, 25000)] == [(4, 7), (2, 5), (1, 3)]
    r = loops.loop_rule(10000, 100)
    assert (r.D, r.ignore_diags, r.min_dist, r.K, r.W, r.radius_bins, r.width) == (200, 2, 5, 40, 10001, 2, 211)
    c = LC.planted(0)
    with pytest.raises(ValueError):   # the guard comes before the matrix: nothing is aggregated for a rule that cannot run
        loops.loops_host(c["pos1"], c["pos2"], c["count"], "VC", c["res"], p=2, w=11)
    with pytest.raises(ValueError):
        loops.loops_host(c["pos1"], c["pos2"], c["count"], "VC", c["res"], "juicer", **LC.P_RULE)
    with pytest.raises(ValueError):   # an expected vector that ends before the pixels' distances
        loops.loops_host(c["pos1"], c["pos2"], c["count"], "VC", c["res"], np.ones(30), **LC.P_RULE)
    band = np.zeros((10, 9))
    with pytest.raises(ValueError):
        loops.loop_lambdas_host(band, np.ones(10), None, np.ones(10), 1, 3, 5)   # 5 + 6 + 1 = 12 wide


def test_same_loop_host_and_footprints():
    found = loops.Loops(1000, 50, np.array([10, 0]), np.array([30, 49]), np.zeros((2, 2)), np.zeros(2), np.ones(2, np.int64),
                        np.ones(2), np.ones((2, 4)), np.zeros((2, 4), np.int64))
    keys = found.footprint_keys(1)
    assert keys.size == 9 + 4 and np.all(np.diff(keys) > 0)          # the corner loop keeps a in {0, 1}, b in {48, 49}
    assert found.footprint_keys(0).size == 2
    p1 = np.array([9000, 11999, 12000, 30500, 8999, 10000, 0, 999, 49000, 10000, 50000, -1])
    p2 = np.array([29000, 31999, 30000, 10500, 30000, 32000, 49999, 50000, 0, 10000, 0, 30000])
    want = [True, True, False, True, False, False, True, False, True, False, False, False]
    #       corner  corner  i + 2  swapped i - 2  j + 2  (0, 49) beyond the matrix (0, 49) swapped  the diagonal  beyond  negative
    assert loops.same_loop_host(p1, p2, found, 1).tolist() == want
    assert loops.same_loop_host(p1, p2, found, 2).tolist()[:6] == [True, True, True, True, True, True]
    assert loops.same_loop_host(p1, p2, found, 0).tolist() == [False, False, False, True, False, False, True, False, True, False,
                                                                False, False]
    for bad in (found.peak_i, (found, 1, 2), (found, -1)):
        with pytest.raises(ValueError):
            loops.check_loops(bad)


def test_host_builder_with_loops():
    c, ws = LC.graph_case()
    plain = build_hic_graph_host(c["pos1"], c["pos2"], c["count"], None, c["res"], ws, LC.GRAPH_EDGES)
    none = build_hic_graph_host(c["pos1"], c["pos2"], c["count"], None, c["res"], ws, LC.GRAPH_EDGES, loops=None)
    assert np.array_equal(plain.indptr, none.indptr) and np.array_equal(plain.indices, none.indices)
    found = loops.Loops(5 * c["res"], 24, np.array([1, 8, 12]), np.array([3, 14, 15]), np.zeros((3, 2)), np.zeros(3),
                        np.ones(3, np.int64), np.ones(3), np.ones((3, 4)), np.zeros((3, 4), np.int64))
    keep = loops.same_loop_host(c["pos1"], c["pos2"], found, 1)
    assert 0 < keep.sum() < keep.size
    got = build_hic_graph_host(c["pos1"], c["pos2"], c["count"], "VC", c["res"], ws, LC.GRAPH_EDGES, expected="auto",
                               loops=(found, 1))
    vc, _ = hicnorm.hic_norm_vector_host(c["pos1"], c["pos2"], c["count"], "VC", c["res"])
    from chromegcn_amd import hicdist
    ex = hicdist.expected_vector_host(c["pos1"], c["pos2"], c["count"], vc, c["res"])
    pre = build_hic_graph_host(c["pos1"][keep], c["pos2"][keep], c["count"][keep], hicnorm.pad_vector(vc, int(ws[-1]) // c["res"] + 1),
                               c["res"], ws, LC.GRAPH_EDGES, expected=ex)      # the vectors come from ALL records
    assert got.nnz > 0 and np.array_equal(got.indptr, pre.indptr) and np.array_equal(got.indices, pre.indices)
    assert loops.loop_edge_share(got, found, ws, 1) == (got.nnz, got.nnz)
    inside, nnz = loops.loop_edge_share(plain, found, ws, 1)
    assert 0 < inside < nnz == plain.nnz
    alone = build_hic_graph_host(c["pos1"], c["pos2"], c["count"], None, c["res"], ws, LC.GRAPH_EDGES, loops=found)   # pad_bins = 1
    pair = build_hic_graph_host(c["pos1"], c["pos2"], c["count"], None, c["res"], ws, LC.GRAPH_EDGES, loops=(found, 1))
    assert np.array_equal(alone.indptr, pair.indptr) and np.array_equal(alone.indices, pair.indices)
    from test_insulation_host import DOMAIN_BP, DOMAINS
    from chromegcn_amd import insulation
    both = build_hic_graph_host(c["pos1"], c["pos2"], c["count"], None, c["res"], ws, LC.GRAPH_EDGES, domains=(DOMAINS, DOMAIN_BP),
                                loops=(found, 1))
    k2 = keep & insulation.same_domain_host(c["pos1"], c["pos2"], DOMAINS, DOMAIN_BP)
    pre2 = build_hic_graph_host(c["pos1"][k2], c["pos2"][k2], c["count"][k2], None, c["res"], ws, LC.GRAPH_EDGES)
    assert 0 < k2.sum() < keep.sum() and np.array_equal(both.indptr, pre2.indptr) and np.array_equal(both.indices, pre2.indices)


def test_loops_from_the_records_as_a_dict():
    c = LC.planted(1)
    ws = (np.arange(0, LC.P_N) * LC.P_RES).astype(np.int32)
    kw = dict(norm="VC", resolution_bp=c["res"], expected=LC.planted_vectors(1)[1], n_bins=c["n_bins"], pad_bins=1, **LC.P_RULE)
    got = build_hic_graph_host(c["pos1"], c["pos2"], c["count"], None, c["res"], ws, 4000, loops=kw)
    want = build_hic_graph_host(c["pos1"], c["pos2"], c["count"], None, c["res"], ws, 4000, loops=(LC.planted_host(1), 1))
    assert got.nnz == 2 * 9 * 6 and np.array_equal(got.indptr, want.indptr) and np.array_equal(got.indices, want.indices)


def test_hic_loops_tool_writes_the_host_loops(tmp_path, capsys):
    import importlib.util
    import os
    from chromegcn_amd import hic
    spec = importlib.util.spec_from_file_location("hic_loops", os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "tools", "hic_loops.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    c = LC.planted(2)
    cache = str(tmp_path / "chrT.cghic")
    hic.save_contacts_cache(cache, hic.HostContacts(c["pos1"], c["pos2"], c["count"], {}, LC.P_RES, None))
    out = str(tmp_path / "out" / "chrT.bedpe")
    tool.main([cache, "--chrom", "chrT", "--res", str(LC.P_RES), "--peak", "1", "--window", "3", "--max-distance",
               str(LC.P_D * LC.P_RES), "--host", "--out", out])
    want = loops.loops_host(c["pos1"], c["pos2"], c["count"], "VC", LC.P_RES, "auto", **LC.P_RULE)
    assert open(out).read() == want.to_bedpe("chrT") and len(want) > 0
    rows = [ln.split("\t") for ln in open(out).read().splitlines()]
    assert all(len(r) == 15 and r[0] == r[3] == "chrT" for r in rows)
    assert [int(r[1]) // LC.P_RES for r in rows] == want.peak_i.tolist() and [int(r[4]) // LC.P_RES for r in rows] == want.peak_j.tolist()
    assert "%d loops from" % len(want) in capsys.readouterr().out


def test_train_arguments():
    from chromegcn_amd import train
    opt = train.parse(["-feat_dir", "f", "-hic_contacts", "caches"])
    assert (opt.hic_loops, opt.hic_loop_norm, opt.hic_loop_fdr, opt.hic_loop_pad, opt.hic_loop_restrict) == (0, "VC", 0.1, 1, False)
    opt = train.parse(["-feat_dir", "f", "-hic_contacts", "caches", "-hic_loops", "10000", "-hic_loop_norm", "KR", "-hic_loop_fdr",
                       "0.05", "-hic_loop_pad", "2", "-hic_loop_restrict"])
    assert (opt.hic_loops, opt.hic_loop_norm, opt.hic_loop_fdr, opt.hic_loop_pad, opt.hic_loop_restrict) == (10000, "KR", 0.05, 2, True)


def test_entry_point_argument_checks():
    from chromegcn_amd import _build, _lib
    _build.build_library()
    _lib.load()
    q = 0x10000   # never read: every call below returns before a launch

    def rc(fn, ok, **kw):
        return _lib.query(fn, **{**ok, **kw})

    band = dict(stream=None, n=10, rowptr=q, col=q, val=q, width=5, band=q)
    for ptr in ("rowptr", "col", "val", "band"):
        assert rc("cgcn_hicloops_band", band, **{ptr: None}) == -1
    assert rc("cgcn_hicloops_band", band, width=0) == -1 and rc("cgcn_hicloops_band", band, n=-1) == -1
    assert rc("cgcn_hicloops_band", band, n=0, col=None, val=None, band=None) == 0
    stencil = dict(n=10, D=20, width=27, band=q, vc=q, norm=None, n_norm=0, expected=q, n_expected=10, p=1, w=3, ignore_diags=2)
    one = dict(stream=None, min_dist=4, bounds=q, n_chunks=40, W=10001, hist=q, flags=q, lambda_out=None, **stencil)
    wsp = _lib.query("cgcn_hicloops_workspace_bytes", n=10, D=20)
    assert wsp > 0 and _lib.query("cgcn_hicloops_workspace_bytes", n=2 ** 21, D=200) == 0 and \
        _lib.query("cgcn_hicloops_workspace_bytes", n=-1, D=20) == 0
    two = dict(stream=None, flags=q, thr=q, n_chunks=40, W=10001, capacity=5, workspace=q, workspace_bytes=wsp, pix_ij=q, pix_val=q,
               **stencil)
    for fn, ok in (("cgcn_hicloops_pass1", one), ("cgcn_hicloops_write", two)):
        assert rc(fn, ok, w=11, width=43) == -2 and rc(fn, ok, n_chunks=65) == -2 and rc(fn, ok, W=65537) == -2   # rule 13
        assert rc(fn, ok, n=2 ** 21, D=200, width=207) == -2
        assert rc(fn, ok, p=3) == -1 and rc(fn, ok, p=-1) == -1 and rc(fn, ok, w=0, p=0) == -1 and rc(fn, ok, ignore_diags=-1) == -1
        assert rc(fn, ok, width=26) == -1                       # the band must reach D + 2 w
        assert rc(fn, ok, n_expected=9) == -1                   # the vector must reach min(n, D + 1)
        assert rc(fn, ok, norm=q, n_norm=0) == -1 and rc(fn, ok, n_chunks=1) == -1 and rc(fn, ok, W=0) == -1
        for ptr in ("band", "vc", "expected", "flags"):
            assert rc(fn, ok, **{ptr: None}) == -1, (fn, ptr)
    assert rc("cgcn_hicloops_pass1", one, min_dist=-1) == -1 and rc("cgcn_hicloops_pass1", one, bounds=None) == -1
    assert rc("cgcn_hicloops_pass1", one, hist=None) == -1
    assert rc("cgcn_hicloops_pass1", one, n=0, band=None, vc=None, expected=None, flags=None, n_expected=0) == 0
    assert rc("cgcn_hicloops_write", two, workspace_bytes=wsp - 1) == -4 and rc("cgcn_hicloops_write", two, thr=None) == -1
    assert rc("cgcn_hicloops_write", two, pix_ij=None) == -1 and rc("cgcn_hicloops_write", two, capacity=-1) == -1
    assert rc("cgcn_hicloops_write", two, capacity=0, pix_ij=None, pix_val=None) == 0       # nothing to write: no launch
    count = dict(stream=None, n=10, D=20, width=27, band=q, flags=q, thr=q, n_chunks=40, W=10001, workspace=q, workspace_bytes=wsp,
                 total=q)
    for ptr in ("band", "flags", "thr", "workspace", "total"):
        assert rc("cgcn_hicloops_count", count, **{ptr: None}) == -1
    assert rc("cgcn_hicloops_count", count, workspace_bytes=wsp - 1) == -4 and rc("cgcn_hicloops_count", count, width=20) == -1
    assert rc("cgcn_hicloops_count", count, n_chunks=65) == -2 and rc("cgcn_hicloops_count", count, W=65537) == -2
    with pytest.raises(RuntimeError, match=r"cgcn_hicloops_pass1 failed: unsupported.*\(code -2\)"):
        _lib.call("cgcn_hicloops_pass1", **{**one, "w": 11, "width": 43})


def test_device_order_distance_sums_are_the_same_sums():
    """another order of the same terms: equal for integer counts, within the bound of a reordered sum otherwise; empty distances
    stay 0; more than 64 tiles at one distance"""
    from chromegcn_amd import hicdist
    rng = np.random.default_rng(8)
    for m, frac in ((0, False), (1, False), (64, True), (65, True), (30000, True), (30000, False)):
        i = rng.integers(0, 98, m)
        j = i + rng.integers(0, 3, m)
        c = rng.uniform(0.1, 9.0, m) if frac else rng.integers(1, 50, m).astype(np.float64)
        for norm in (None, LC.noisy_norm(100, 4)):
            raw, act = hicdist.distance_sums_host(i * 1000, j * 1000, c, norm, 1000, 100)
            raw2, act2 = hicdist.distance_sums_device_order_host(i * 1000, j * 1000, c, norm, 1000, 100)
            assert raw2.shape == act2.shape == (100,) and np.all(raw2[3:] == 0) and np.all(act2[3:] == 0)
            if not frac:
                assert np.array_equal(raw, raw2)
            k = np.bincount(np.abs(i - j), minlength=100)
            assert np.all(np.abs(raw - raw2) <= 2.0 * np.maximum(k - 1, 0) * 2.0 ** -53 * np.abs(raw))
            assert np.all(np.abs(act - act2) <= 2.0 * np.maximum(k - 1, 0) * 2.0 ** -53 * np.abs(act))
    with pytest.raises(ValueError):
        hicdist.distance_sums_device_order_host([0], [5000], [-1.0], None, 1000)
