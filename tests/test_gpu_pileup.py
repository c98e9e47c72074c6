"""The pile-up kernels (csrc/cgcn_pileup.hip) against the numpy restatement of chromegcn_amd/pileup.py, fed the device matrix
read back so that the comparison does not lean on the aggregation: the value band bit for bit with the same NaN pattern, and P, N,
kept and skipped exactly; every case is run twice and must give the same bits.
Sizes: a slice is 256 centres and a team S^2 = (2 w + 1)^2 threads, 8 teams per workgroup from w = 3 down, 4 at w = 5 and 1 at
w = 10, so M runs either side of one slice and up to five, w over every team shape, n from the smallest map with one legal centre
to 257 bins, and G over one group, three with an empty one and 64, the groups interleaved in the input."""
import functools

import numpy as np
import pytest
import torch

from chromegcn_amd import HicContacts, hicmap, pileup

import pileup_cases as PC
from pileup_cases import LC

pytestmark = pytest.mark.gpu
DEV = "cuda"


@functools.lru_cache(maxsize=None)
def device_map(n, empty=()):
    """(the device matrix, the matrix read back, its row sums) of a sparse integer map with n bins, the bins `empty` left out"""
    p1, p2, cnt = PC.integer_map(n)[1]
    k = ~np.isin(p1 // PC.RES, empty) & ~np.isin(p2 // PC.RES, empty)
    A = HicContacts(p1[k], p2[k], cnt[k], DEV).contact_matrix(PC.RES, n)
    host = A.to_host()
    return A, host, np.asarray(host.sum(axis=1)).ravel()


def dev(v):
    return None if v is None else torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).to(DEV)


@functools.lru_cache(maxsize=None)
def bands(n, w, value, norm_kind="noisy", empty=()):
    """(the rule, the device value band, the restatement's) of a map; the expected vector stops short of the band and has a zero"""
    A, host, vc = device_map(n, empty)
    r = PC.rule_for(n, w, value)
    norm = {"none": None, "noisy": PC.noisy_norm(n, 70 + n), "noisy_inf": PC.noisy_norm(n, 70 + n, inf=True)}[norm_kind]
    ex = np.random.default_rng(n + w).uniform(0.2, 3.0, r.max_dist + 1)       # min(n, max_dist + 1) at least; the band is wider
    ex[r.min_dist + 1] = 0.0
    want = pileup.value_band_host(hicmap.band_host(host, r.width), vc, norm, ex, r)
    got = pileup.value_band(hicmap.device_band(A, r.width), A.vc, dev(norm), dev(ex) if value == "oe" else None, r)
    return r, got, want


@pytest.mark.parametrize("norm_kind", ["none", "noisy"])
@pytest.mark.parametrize("value", pileup.VALUES)
def test_value_band_bit_for_bit(value, norm_kind):
    for n, w, empty in ((7, 1, ()), (64, 2, (20,)), (257, 10, (3, 100)), (65, 5, ())):
        r, got, want = bands(n, w, value, norm_kind, empty)
        assert r.max_dist + 1 < r.width and PC.same_bits(got.cpu().numpy(), want), (n, w)       # the NaN pattern included
        again = bands.__wrapped__(n, w, value, norm_kind, empty)[1]
        assert torch.equal(got.view(torch.int64), again.view(torch.int64))
        took = np.isfinite(want)
        assert took.any() and not took.all()
        if empty:
            assert not took[empty[0]].any() and not took[empty[0] - 1, 1].any()
        if value == "oe":
            assert not took[:, r.min_dist + 1].any() and not took[:, r.max_dist + 1:].any()


@pytest.mark.parametrize("value", pileup.VALUES)
def test_value_band_with_every_kind_of_bad_norm_entry(value):
    """257 bins, two of them empty; the vector is a bin short and holds NaN, 0 and +inf"""
    r, got, want = bands(257, 10, value, "noisy_inf", (3, 100))
    assert PC.same_bits(got.cpu().numpy(), want) and np.isfinite(want).any()


def run_twice(vb, ci, cj, g, G, r):
    got = pileup.pileup_sums(vb, ci, cj, g, G, r)
    again = pileup.pileup_sums(vb, torch.from_numpy(ci).to(DEV), torch.from_numpy(cj).to(DEV),
                               None if g is None else torch.from_numpy(g).to(DEV), G, r)          # device tensors: the same
    PC.assert_same_pileup(again, got)
    return got


@pytest.mark.parametrize("w", PC.W_ALL)
@pytest.mark.parametrize("nkind", ["smallest", "n64", "n257"])
def test_sums_bit_for_bit(nkind, w):
    n = {"smallest": PC.smallest_n(w), "n64": 64, "n257": 257}[nkind]
    r, vb, want_vb = bands(n, w, "oe")
    kept_total = 0
    for M in PC.M_ALL:
        for G in PC.G_ALL:
            ci, cj, g = PC.centres(n, r, M, G, seed=1000 * w + M + G)
            got = run_twice(vb, ci, cj, g, G, r)
            want = pileup.pileup_sums_host(want_vb, ci, cj, g, G, r)
            PC.assert_same_pileup(got, want)
            assert int(got.kept.sum()) + sum(got.skipped.values()) == M
            if G == 3:
                assert got.kept[1] == 0 and not got.count[1].any()
            kept_total += int(got.kept.sum())
    assert kept_total > 2000
    if nkind == "smallest":                        # exactly one legal centre
        got = run_twice(vb, np.array([w, w + 1, w - 1]), np.array([w + r.min_dist, w + 1 + r.min_dist, w - 1 + r.min_dist]), None, 1, r)
        assert got.kept.tolist() == [1] and got.skipped == {"group": 0, "edge": 2, "near": 0, "far": 0}


def test_limits_duplicates_and_nothing_kept():
    n, w = 64, 2
    r, vb, want_vb = bands(n, w, "balanced")
    lo, hi = r.min_dist, r.max_dist
    # one bin inside and one bin outside each of the four limits, then a group outside its range at either end
    ci = np.array([w, w - 1, n - 1 - w - lo, n - w - lo, 10, 10, 10, 10, 10, 10])
    cj = np.array([w + lo, w - 1 + lo, n - 1 - w, n - w, 10 + lo, 9 + lo, 10 + hi, 11 + hi, 10 + lo, 10 + lo])
    g = np.array([0, 0, 0, 0, 0, 0, 0, 0, -1, 2])
    got = run_twice(vb, ci, cj, g, 2, r)
    PC.assert_same_pileup(got, pileup.pileup_sums_host(want_vb, ci, cj, g, 2, r))
    assert got.kept.tolist() == [4, 0] and got.skipped == {"group": 2, "edge": 2, "near": 1, "far": 1}
    # heavy duplicates of one centre, five slices of them, the larger bin first
    ci, cj = np.full(1200, 30), np.full(1200, 12)
    got = run_twice(vb, ci, cj, None, 1, r)
    PC.assert_same_pileup(got, pileup.pileup_sums_host(want_vb, ci, cj, None, 1, r))
    assert got.kept.tolist() == [1200] and got.count.max() == 1200
    # nothing kept: zeros and NaN means
    for ci, cj, g in ((np.array([0, 1]), np.array([1, 63]), None), (np.array([10, 10]), np.array([30, 30]), np.array([5, -3])),
                      (np.zeros(0, np.int64), np.zeros(0, np.int64), None)):
        got = run_twice(vb, ci, cj, g, 3, r)
        assert not got.kept.any() and not got.sum.any() and not got.count.any() and np.isnan(got.mean).all()
        assert sum(got.skipped.values()) == ci.size
    with pytest.raises(ValueError, match="different lengths"):
        pileup.pileup_sums(vb, np.array([1, 2]), np.array([30]), None, 1, r)
    with pytest.raises(ValueError):
        pileup.pileup_sums(vb, np.array([10]), np.array([30]), None, 65537, r)
    with pytest.raises(ValueError):
        pileup.pileup_sums(vb[:, :-1].contiguous(), np.array([10]), np.array([30]), None, 1, r)


def test_integer_counts_are_exact():
    n = 257
    A, host, vc = device_map(n)
    for w in (2, 10):
        r = PC.rule_for(n, w, "observed")
        vb = pileup.value_band(hicmap.device_band(A, r.width), A.vc, None, None, r)
        ci, cj, g = PC.centres(n, r, 3000, 3, seed=11 + w)
        got = run_twice(vb, ci, cj, g, 3, r)
        want, cnt = PC.integer_reference(host, ci, cj, g, 3, r)
        assert np.array_equal(got.sum, want.astype(np.float64)) and np.array_equal(got.count, cnt) and want.max() > 1000


def test_max_dist_at_the_guards_edge():
    """n = 7 bins at w = 1: the band may be 2^28 // 7 wide.  One distance more is refused before anything is allocated."""
    n, w = 7, 1
    A, host, vc = device_map(n)
    width = pileup.MAX_ELEMS // n
    kw = dict(value="observed", w=w, max_distance_bp=(width - 2 * w - 1) * PC.RES)
    r = pileup.pileup_rule(PC.RES, n, **kw)
    assert r.width == width and n * width <= pileup.MAX_ELEMS < n * (width + 1)
    ci, cj = np.array([1, 1, 2, 1, 0]), np.array([4, 5, 5, 3, 4])
    got = pileup.pileup_of_matrix(A, None, None, (ci, cj), resolution_bp=PC.RES, **kw)
    want = pileup.pileup_sums_host(pileup.value_band_host(hicmap.band_host(host, width), vc, None, None, r), ci, cj, None, 1, r)
    PC.assert_same_pileup(got, want)
    assert got.kept.tolist() == [3] and got.skipped == {"group": 0, "edge": 1, "near": 1, "far": 0}
    before = torch.cuda.memory_allocated()
    with pytest.raises(ValueError, match="2\\^28"):
        pileup.pileup_of_matrix(A, None, None, (ci, cj), resolution_bp=PC.RES, **{**kw, "max_distance_bp": (width - 2 * w) * PC.RES})
    assert torch.cuda.memory_allocated() == before


def test_graphs_from_contact_caches_with_apa(tmp_path, capsys):
    """what `train -hic_apa` prints: the edges of the unrestricted graph, their control shifted by 3 w and the loops, and the
    graphs themselves as without it"""
    from chromegcn_amd import build_hic_graph_host, hic, train
    c = LC.planted(1)
    ws = (np.arange(0, LC.P_N) * LC.P_RES).astype(np.int32)
    hic.save_contacts_cache(hic.contact_cache_path(str(tmp_path), "chrT"), hic.HostContacts(c["pos1"], c["pos2"], c["count"], {}, LC.P_RES, ws))
    apa = dict(w=3, resolution_bp=LC.P_RES, max_distance_bp=LC.P_D * LC.P_RES, min_dist=6)
    report = {}
    g = hic.graphs_from_contact_caches(str(tmp_path), ["chrT"], 12000, "", apa=apa, apa_report=report,
                                       loops=dict(norm="VC", resolution_bp=LC.P_RES, n_bins=LC.P_N, **LC.P_RULE))["chrT"]
    plain = hic.graphs_from_contact_caches(str(tmp_path), ["chrT"], 12000, "")["chrT"]
    assert g.nnz == plain.nnz and torch.equal(g.rowptr, plain.rowptr) and torch.equal(g.col[:g.nnz], plain.col[:plain.nnz])
    free = build_hic_graph_host(c["pos1"], c["pos2"], c["count"], None, LC.P_RES, ws, 12000)
    i, j, _ = pileup.centres_of_graph(free, ws, LC.P_RES)
    rec = (c["pos1"], c["pos2"], c["count"])
    piles = report["chrT"]
    assert sorted(piles) == ["control", "edges", "loops"]
    PC.assert_same_pileup(piles["edges"], pileup.pileup_host(*rec, (i, j), **apa))
    PC.assert_same_pileup(piles["control"], pileup.pileup_host(*rec, pileup.shifted_centres(i, j, 9), **apa))
    found = LC.planted_host(1, "auto")
    PC.assert_same_pileup(piles["loops"], pileup.pileup_host(*rec, found, **apa))
    assert piles["edges"].kept[0] > 3000 and piles["loops"].scores()["P2LL"][0] > 2.0
    capsys.readouterr()
    train.report_apa("train", report)
    out = capsys.readouterr().out.splitlines()
    assert [ln.split()[3] for ln in out] == ["edges:", "control:", "loops:"] and all(ln.startswith("[hic_apa] train chrT ") for ln in out)


@pytest.mark.parametrize("seed", [1])
def test_hic_contacts_pileup_on_loops_and_graph_edges(seed):
    c = LC.planted(seed)
    hc = HicContacts(c["pos1"], c["pos2"], c["count"], DEV)
    kw = dict(norm="VC", resolution_bp=c["res"], expected="auto", n_bins=c["n_bins"], w=3, max_distance_bp=LC.P_D * LC.P_RES)
    rec = (c["pos1"], c["pos2"], c["count"])
    found = hc.loops("VC", c["res"], "auto", n_bins=c["n_bins"], **LC.P_RULE)
    got = hc.pileup(found, **kw)
    PC.assert_same_pileup(got, pileup.pileup_host(*rec, found, **kw))
    assert got.kept.tolist() == [len(found)] and got.scores()["P2LL"][0] > 2.0
    ws = (np.arange(0, LC.P_N) * LC.P_RES).astype(np.int32)
    _, raw = hc.build(None, c["res"], ws, 12000, return_raw=True)          # 6 000 records: edges at every distance up to 60
    i, j, entry = pileup.centres_of_graph(raw, ws, c["res"])
    edges = [6, 12, 24, 61]
    g = pileup.distance_groups(i, j, edges)
    assert entry.size == raw.nnz // 2 > 1000 and set(g.tolist()) == {-1, 0, 1, 2}
    for value in pileup.VALUES:
        more = {**kw, "value": value, "min_dist": 6}
        got = hc.pileup((i, j), g, 3, **more)
        PC.assert_same_pileup(got, pileup.pileup_host(*rec, (i, j), g, 3, **more))
        assert got.kept.min() > 500 and got.skipped["group"] > 500            # the edges nearer than 6 bins have no group
        ti, tj = torch.from_numpy(i).to(DEV), torch.from_numpy(j).to(DEV)
        PC.assert_same_pileup(hc.pileup((ti, tj), pileup.distance_groups(ti, tj, edges), 3, **more), got)
    assert len(hc._pileup_bands) == 1 and len(hc._pileup_values) == 3              # one raw band, one value band per kind
    control = hc.pileup(pileup.shifted_centres(found.peak_i, found.peak_j, 9), **kw)
    assert hc.pileup(found, **kw).scores()["P2LL"][0] > control.scores()["P2LL"][0]
    with pytest.raises(ValueError):
        hc.pileup(found, **{**kw, "w": 11})
    with pytest.raises(ValueError):
        hc.pileup(found, **{**kw, "min_dist": 5})
    with pytest.raises(ValueError):
        hc.pileup((i, j[:-1]), **kw)
