"""The map comparison's rule on the host (chromegcn_amd/mapcompare.py; no GPU): the smoothing against scipy's uniform filter and
against the literal loop of rule 3, the strata's correlations against np.corrcoef over a literal selection of rule 4's cells, the
properties a similarity score must have, the ordering of replicates and different maps on planted domains, graph_edge_overlap,
tools/hic_compare.py on the restatement, the train flags, the entry points' argument checks (no launch)."""
import importlib.util
import os

import numpy as np
import pytest
import scipy.ndimage as ndi
import scipy.sparse as sp

from chromegcn_amd import hic, hicmap, hicnorm, mapcompare as MC

import mapcompare_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


def literal_smooth(dense, nv, h, D):
    """rule 3 as it is written: four loops, S[i, d] for the cells inside the matrix"""
    n = dense.shape[0]

    def V(p, q):
        if not (0 <= p < n and 0 <= q < n):
            return 0.0
        lo, hi = min(p, q), max(p, q)
        return dense[lo, hi] if nv is None else dense[lo, hi] / (nv[lo] * nv[hi])

    S = np.zeros((D + 1, MC.leading_dim(n)))
    for d in range(min(D, n - 1) + 1):
        for i in range(n - d):
            s = 0.0
            for da in range(-h, h + 1):
                r = 0.0
                for db in range(-h, h + 1):
                    r = r + V(i + da, i + d + db)
                s = s + r
            S[d, i] = s
    return S


@pytest.mark.parametrize("h", [0, 1, 2, 5, 20])
@pytest.mark.parametrize("n", [1, 2, 7, 41, 64, 257])
def test_smoothing_is_the_uniform_filter_times_its_size(n, h):
    A = C.sparse_integer_map(n, max(n // 2, 1), 100 * n + h)
    for D in sorted({0, min(9, n - 1), n - 1, n + 3}):          # D >= n: the strata beyond the matrix are zeros
        S = MC.smooth_strata_host(hicmap.band_host(A, D + 2 * h + 1), None, h, D)
        assert S.shape == (D + 1, MC.leading_dim(n))
        F = np.rint(ndi.uniform_filter(A.toarray(), 2 * h + 1, mode="constant") * (2 * h + 1) ** 2)
        want = np.zeros_like(S)
        for d in range(min(D, n - 1) + 1):
            want[d, :n - d] = np.diagonal(F, d)
        assert np.array_equal(S, want), (n, h, D)
    if n <= 41:
        D = n + 1
        band = hicmap.band_host(A, D + 2 * h + 3)               # a wider band than the rule needs reads the same
        assert same_bits(MC.smooth_strata_host(band, None, h, D), literal_smooth(A.toarray(), None, h, D))


@pytest.mark.parametrize("n,h", [(7, 1), (41, 2), (41, 5), (23, 20)])
def test_smoothing_with_a_norm_vector_is_the_literal_loop(n, h):
    A = C.sparse_integer_map(n, n // 2, 7 * n + h)
    for norm in (C.noisy_norm(n, 3), C.noisy_norm(n, 4)[:n - 1], C.noisy_norm(n + 5, 5)):
        nv = hicnorm.clean_norm(norm, n)
        D = n - 1
        with np.errstate(all="ignore"):
            want = literal_smooth(A.toarray(), nv, h, D)
        got = MC.smooth_strata_host(hicmap.band_host(A, D + 2 * h + 1), norm, h, D)
        assert same_bits(got, want) and np.isfinite(got).all()
    # the two-level order is what makes the separable form and the direct one the same bits: float values, not integers
    B = sp.csr_matrix(A.multiply(1.0 / 3.0))
    assert same_bits(MC.smooth_strata_host(hicmap.band_host(B, n + 2 * h), None, h, n - 1), literal_smooth(B.toarray(), None, h, n - 1))


def literal_cells(Sa, Sb, valid, n, d):
    """rule 4's cells of stratum d, one by one"""
    xs, ys = [], []
    for i in range(n - d):
        if valid[i] and valid[i + d] and (Sa[d, i] != 0 or Sb[d, i] != 0):
            xs.append(Sa[d, i])
            ys.append(Sb[d, i])
    return np.array(xs), np.array(ys)


def pair_41():
    """two maps of 41 bins with holes at different bins, dense enough that every compared stratum has a spread"""
    a = C.with_holes(C.sparse_integer_map(41, 30, 11, density=0.9), [5])
    b = C.with_holes(C.sparse_integer_map(41, 30, 12, density=0.9), [17, 30])
    return a, b


@pytest.mark.parametrize("norm", [None, "VC"])
@pytest.mark.parametrize("h", [0, 2])
def test_rho_is_np_corrcoef_over_the_literal_selection(h, norm):
    a, b = pair_41()
    D = 25
    got = MC.map_scc_host(C.records_of(a), C.records_of(b), norm=norm, resolution_bp=C.RES, h=h, max_distance_bp=D * C.RES)
    assert got.rule == MC.SccRule(C.RES, h, 1, D) and got.rho.shape == got.cells.shape == got.weights.shape == (D + 1,)
    nvs = [None if norm is None else hicnorm.hic_norm_vector_host(*C.records_of(m), norm, C.RES, 41)[0] for m in (a, b)]
    valid = hicmap.valid_bins(np.asarray(a.sum(axis=1)).ravel(), nvs[0]) & hicmap.valid_bins(np.asarray(b.sum(axis=1)).ravel(), nvs[1])
    assert np.array_equal(got.valid, valid) and not valid[[5, 17, 30]].any() and valid.sum() == 38
    Sa, Sb = (MC.smooth_strata_host(hicmap.band_host(m, D + 2 * h + 1), nv, h, D) for m, nv in zip((a, b), nvs))
    assert np.isnan(got.rho[0]) and got.cells[0] == 0                      # below min_dist
    num = den = 0.0
    for d in range(1, D + 1):
        x, y = literal_cells(Sa, Sb, valid, 41, d)
        assert got.cells[d] == x.size >= 3 and x.std() > 0 and y.std() > 0
        assert abs(got.rho[d] - np.corrcoef(x, y)[0, 1]) <= 1e-12
        assert got.weights[d] == (x.size + 1) / 12.0
        num, den = num + got.weights[d] * got.rho[d], den + got.weights[d]
    assert got.scc == num / den and got.n_strata == D
    # min_dist = 0 adds the diagonal's stratum
    with0 = MC.map_scc_host(C.records_of(a), C.records_of(b), norm=norm, resolution_bp=C.RES, h=h, max_distance_bp=D * C.RES, min_dist=0)
    x, y = literal_cells(Sa, Sb, valid, 41, 0)
    assert with0.cells[0] == x.size and abs(with0.rho[0] - np.corrcoef(x, y)[0, 1]) <= 1e-12
    assert same_bits(with0.rho[1:], got.rho[1:])


def test_sums_follow_the_rules_order():
    """rule 5 on a stratum of more than one chunk against its literal restatement: lanes, butterfly, chunks"""
    n, rng = 4100, np.random.default_rng(5)
    Sa, Sb = rng.uniform(0, 3, (2, MC.leading_dim(n))), rng.uniform(0, 3, (2, MC.leading_dim(n)))
    Sa[:, rng.integers(0, n, 400)] = 0.0
    valid = rng.random(n) > 0.1
    got = MC.stratum_sums_host(Sa, Sb, valid, n, min_dist=1)
    d = 1
    part = valid[:n - d] & valid[d:] & ((Sa[d, :n - d] != 0) | (Sb[d, :n - d] != 0))

    def literal(t):
        total = 0.0
        for c0 in range(0, n - d, MC.CHUNK):
            lanes = np.zeros(64)
            for i in range(c0, min(c0 + MC.CHUNK, n - d)):
                if part[i]:
                    lanes[(i - c0) % 64] += t[i]
            for o in (32, 16, 8, 4, 2, 1):
                lanes = lanes + lanes[np.arange(64) ^ o]
            total = total + lanes[0]
        return total
    x, y = Sa[d, :n - d], Sb[d, :n - d]
    assert got.cells[d] == part.sum() and got.cells[0] == 0
    assert got.sx[d] == literal(x) and got.sy[d] == literal(y)
    mx, my = got.sx[d] / part.sum(), got.sy[d] / part.sum()
    assert got.mx[d] == mx and got.my[d] == my
    assert got.sxx[d] == literal((x - mx) * (x - mx)) and got.syy[d] == literal((y - my) * (y - my))
    assert got.sxy[d] == literal((x - mx) * (y - my))


def test_properties():
    a, b = pair_41()
    ra, rb = C.records_of(a), C.records_of(b)
    kw = dict(resolution_bp=C.RES, h=2, max_distance_bp=25 * C.RES)
    own = MC.map_scc_host(ra, ra, **kw)
    assert abs(own.scc - 1.0) <= 1e-12 and np.all(np.abs(own.rho[1:] - 1.0) <= 1e-12)
    base = MC.map_scc_host(ra, rb, **kw)
    assert -1.0 < base.scc < 1.0
    doubled = MC.map_scc_host(ra, (rb[0], rb[1], 2.0 * rb[2]), **kw)       # a power of two: every product scales exactly
    assert same_bits(doubled.rho, base.rho) and doubled.scc == base.scc and np.array_equal(doubled.cells, base.cells)
    swapped = MC.map_scc_host(rb, ra, **kw)
    assert np.array_equal(swapped.cells, base.cells) and np.allclose(swapped.rho, base.rho, rtol=0, atol=1e-12, equal_nan=True)
    # a hole in either map removes exactly its cells
    whole = MC.map_scc_host(C.records_of(C.sparse_integer_map(41, 30, 11, density=0.9)), ra, **kw)
    v = whole.valid
    assert not v[5] and v.sum() == 40
    for d in range(1, 26):
        assert whole.cells[d] == int(np.dot(v[:41 - d].astype(int), v[d:].astype(int)))   # dense maps: no cell is zero in both
    # padding with zeros changes nothing: the shorter map, n_bins beyond both
    short = with_bins = C.records_of(C.sparse_integer_map(30, 20, 13, density=0.9))
    pair = MC.map_scc_host(ra, short, **kw)
    assert pair.valid.size == 41 and not pair.valid[30:].any() and same_bits(MC.map_scc_host(short, ra, **kw).cells, pair.cells)
    padded = MC.map_scc_host(ra, with_bins, n_bins=50, **kw)
    assert padded.valid.size == 50 and same_bits(padded.rho, pair.rho) and padded.scc == pair.scc
    # a sweep over h is the single calls
    sweep = MC.map_scc_host(ra, rb, resolution_bp=C.RES, h=[0, 2], max_distance_bp=25 * C.RES)
    assert isinstance(sweep, list) and same_bits(sweep[1].rho, base.rho) and sweep[0].rule.h == 0
    # a pair of norms: one entry per map
    vec = C.noisy_norm(41, 9)
    mixed = MC.map_scc_host(ra, rb, norm=(None, vec), **kw)
    assert not mixed.valid[[1, 3, 4]].any() and mixed.valid[6]
    with pytest.raises(ValueError, match="a pair with one entry per map"):
        MC.map_scc_host(ra, rb, norm=(None, vec, vec), **kw)


def test_empty_and_nan_outcomes(tmp_path):
    none = (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0))
    one = (np.array([0], np.int32), np.array([0], np.int32), np.array([3.0]))
    ra = C.records_of(pair_41()[0])
    kw = dict(resolution_bp=C.RES, h=1)
    r = MC.map_scc_host(none, none, **kw)
    assert np.isnan(r.scc) and r.rho.size == 0 and r.valid.size == 0 and r.rule.max_dist == -1
    r = MC.map_scc_host(one, one, **kw)                                       # n = 1: the diagonal alone
    assert np.isnan(r.scc) and r.rho.shape == (1,) and r.cells.tolist() == [0]
    r = MC.map_scc_host(ra, none, **kw)                                       # nothing is valid in both
    assert np.isnan(r.scc) and not r.valid.any() and r.cells.sum() == 0 and r.rho.shape == (41,)
    two = (np.array([0, 0, 1000], np.int32), np.array([0, 1000, 1000], np.int32), np.array([3.0, 1.0, 2.0]))
    r = MC.map_scc_host(two, two, **kw)                                       # one cell per stratum: N < 3
    assert np.isnan(r.scc) and r.cells.tolist() == [0, 1] and np.isnan(r.rho).all()
    flat = C.records_of(sp.csr_matrix(np.ones((12, 12))))                     # constant strata away from the edges: no spread
    r = MC.map_scc_host(flat, flat, resolution_bp=C.RES, h=0)
    assert np.isnan(r.scc) and (r.cells[1:10] >= 3).all() and (r.sums.sxx == 0).all()
    r.save(str(tmp_path / "flat.npz"))
    z = np.load(str(tmp_path / "flat.npz"))
    assert np.isnan(float(z["scc"])) and z["cells"].tolist() == r.cells.tolist() and int(z["h"]) == 0 and int(z["max_dist"]) == 11
    assert MC.scc_from_sums(MC._empty_sums(-1))[1].size == 0


def test_guards():
    ra = C.records_of(pair_41()[0])
    with pytest.raises(ValueError, match="h=21: more than 20"):
        MC.scc_rule(C.RES, 10, h=21)
    with pytest.raises(ValueError, match="h must not be negative"):
        MC.scc_rule(C.RES, 10, h=-1)
    with pytest.raises(ValueError, match="min_dist must not be negative"):
        MC.map_scc_host(ra, ra, resolution_bp=C.RES, min_dist=-1)
    with pytest.raises(ValueError, match="different resolutions"):
        MC.map_scc_host(ra, ra, resolution_bp=(1000, 5000))
    assert MC.scc_rule((1000, 1000), 41, 5).res == 1000
    with pytest.raises(ValueError, match="2\\^28 band elements: take a coarser resolution_bp or a shorter max_distance_bp"):
        MC.scc_rule(1000, 250000, h=5, max_distance_bp=5_000_000)
    assert MC.scc_rule(40000, 6200, h=5) == MC.SccRule(40000, 5, 1, 125) and MC.scc_rule(40000, 6200, h=5).width == 136
    assert MC.scc_rule(1000, 30, h=3, max_distance_bp=10 ** 9).max_dist == 29 and MC.scc_rule(1000, 0).max_dist == -1
    with pytest.raises(ValueError, match="h=21"):                             # before anything is read
        MC.map_scc_host(None, None, resolution_bp=C.RES, h=[1, 21])
    with pytest.raises(ValueError, match="the band is 5 wide but D=3 and h=2 need 8"):
        MC.smooth_strata_host(np.zeros((4, 5)), None, 2, 3)
    with pytest.raises(ValueError, match="one validity entry per bin"):
        MC.stratum_sums_host(np.zeros((2, 4)), np.zeros((2, 4)), np.ones(3, bool), 4)


# a replicate (the same intensity, another draw) against a map with other domains, on the restatement: rule and seeds fixed
# first, the assertion after.  Measured on the restatement: replicate 0.29 .. 0.70, other -0.04 .. 0.13, shallow replicate 0.25 .. 0.59.
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_a_replicate_scores_above_a_map_with_other_domains(seed):
    a = C.planted_draw(200, 20, 200, 10 + seed)
    rep = C.planted_draw(200, 20, 200, 20 + seed)
    other = C.planted_draw(200, 33, 200, 30 + seed)
    shallow = C.planted_draw(200, 20, 50, 40 + seed)
    kw = dict(resolution_bp=C.RES, h=[0, 1, 3], max_distance_bp=60 * C.RES)
    for r, o, s in zip(MC.map_scc_host(a, rep, **kw), MC.map_scc_host(a, other, **kw), MC.map_scc_host(a, shallow, **kw)):
        assert r.rule.max_dist == 60 and r.n_strata == 60
        assert r.scc >= o.scc + 0.2, (r.rule.h, r.scc, o.scc)
        assert s.scc > o.scc, (r.rule.h, s.scc, o.scc)


def test_graph_edge_overlap():
    rng = np.random.default_rng(8)
    n = 30
    ga = sp.csr_matrix((rng.random((n, n)) < 0.2).astype(np.float64))
    gb = sp.csr_matrix((rng.random((n, n)) < 0.2).astype(np.float64))
    sa, sb = set(zip(*ga.nonzero())), set(zip(*gb.nonzero()))
    got = MC.graph_edge_overlap(ga, gb)
    assert (got["shared"], got["only_a"], got["only_b"]) == (len(sa & sb), len(sa - sb), len(sb - sa))
    assert got["jaccard"] == len(sa & sb) / len(sa | sb) and "by_group" not in got
    edges = [0, 1, 5, 12]
    by = MC.graph_edge_overlap((ga.indptr, ga.indices), gb, groups=edges)["by_group"]
    for g in range(3):
        def sel(s):
            return {(i, j) for i, j in s if edges[g] <= abs(j - i) < edges[g + 1]}
        assert (by["shared"][g], by["only_a"][g], by["only_b"][g]) == (len(sel(sa & sb)), len(sel(sa - sb)), len(sel(sb - sa)))
        assert by["jaccard"][g] == len(sel(sa & sb)) / len(sel(sa | sb))
    assert MC.graph_edge_overlap(ga, ga)["jaccard"] == 1.0
    empty = MC.graph_edge_overlap(sp.csr_matrix((4, 4)), sp.csr_matrix((4, 4)))
    assert empty["shared"] == 0 and np.isnan(empty["jaccard"])
    with pytest.raises(ValueError, match="the graph has 29 windows"):
        MC.graph_edge_overlap(ga, gb[:29, :29])
    with pytest.raises(ValueError, match="ascending"):
        MC.graph_edge_overlap(ga, gb, groups=[3, 3])


def test_hic_compare_tool_on_a_tiny_fixture(tmp_path, capsys):
    spec = importlib.util.spec_from_file_location("hic_compare", os.path.join(ROOT, "tools", "hic_compare.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    a, b = pair_41()
    paths = []
    for name, m in (("a", a), ("b", b)):
        paths.append(str(tmp_path / (name + ".cghic")))
        hic.save_contacts_cache(paths[-1], hic.HostContacts(*C.records_of(m), {}, C.RES, None))
    out = str(tmp_path / "out" / "chrT.scc")
    tool.main(paths + ["--chrom", "chrT", "--res", str(C.RES), "--h", "0,2", "--max-distance", str(25 * C.RES), "--host", "--out", out])
    want = MC.map_scc_host(C.records_of(a), C.records_of(b), resolution_bp=C.RES, h=[0, 2], max_distance_bp=25 * C.RES)
    for h, w in zip((0, 2), want):
        z = np.load("%s.h%d.npz" % (out, h))
        assert float(z["scc"]) == w.scc and same_bits(z["rho"], w.rho) and np.array_equal(z["cells"], w.cells) and int(z["h"]) == h
    table = np.loadtxt(out + ".txt")
    assert table.shape == (26, 5) and np.array_equal(table[:, 0], np.arange(26)) and np.array_equal(table[:, 3], want[1].cells)
    assert np.allclose(table[1:, 4], want[1].rho[1:], rtol=1e-9) and np.isnan(table[0, 2])
    assert "chrT h=2: SCC %.6f over 25 strata" % want[1].scc in capsys.readouterr().out
    with pytest.raises(SystemExit):
        tool.main(paths + ["--chrom", "chrT", "--h", "21", "--host", "--out", out])
    with pytest.raises(SystemExit):
        tool.main(paths + ["--chrom", "chrT", "--norm", "XX", "--host", "--out", out])


def test_train_arguments(capsys):
    from chromegcn_amd import train
    opt = train.parse(["-feat_dir", "f", "-hic_contacts", "caches"])
    assert (opt.hic_compare, opt.hic_compare_res, opt.hic_compare_h, opt.hic_compare_norm) == (None, 40000, 5, "NONE")
    opt = train.parse(["-feat_dir", "f", "-hic_contacts", "caches", "-hic_compare", "other", "-hic_compare_res", "10000",
                       "-hic_compare_h", "20", "-hic_compare_norm", "VC"])
    assert (opt.hic_compare, opt.hic_compare_res, opt.hic_compare_h, opt.hic_compare_norm) == ("other", 10000, 20, "VC")
    for bad in (["-hic_compare", "other"], ["-hic_contacts", "c", "-hic_compare", "o", "-hic_compare_h", "21"],
                ["-hic_contacts", "c", "-hic_compare", "o", "-hic_compare_res", "0"],
                ["-hic_contacts", "c", "-hic_compare", "o", "-hic_compare_norm", "XX"]):
        with pytest.raises(SystemExit):
            train.parse(["-feat_dir", "f"] + bad)
    assert "-hic_compare needs -hic_contacts" in capsys.readouterr().err
    a, b = pair_41()
    cmp = MC.map_scc_host(C.records_of(a), C.records_of(b), resolution_bp=C.RES, h=2, max_distance_bp=25 * C.RES)
    train.report_compare("valid", {"chrT": (cmp, MC.graph_edge_overlap(a, b))})
    ov = MC.graph_edge_overlap(a, b)
    assert capsys.readouterr().out == ("[hic_compare] valid chrT: SCC %.4f, N strata 25, edges shared/only/only %d/%d/%d, Jaccard %.4f\n"
                                       % (cmp.scc, ov["shared"], ov["only_a"], ov["only_b"], ov["jaccard"]))


def test_entry_point_argument_checks():
    from chromegcn_amd import _build, _lib
    _build.build_library()
    _lib.load()
    q = 0x10000   # never read: every call below returns before a launch

    def rc(fn, ok, **kw):
        return _lib.query(fn, **{**ok, **kw})
    sm = dict(stream=None, n=10, D=4, h=2, width=9, band=q, norm=None, n_norm=0, ld=10, S=q)
    for ptr in ("band", "S"):
        assert rc("cgcn_mapcmp_smooth", sm, **{ptr: None}) == -1
    assert rc("cgcn_mapcmp_smooth", sm, width=8) == -1 and rc("cgcn_mapcmp_smooth", sm, h=-1) == -1
    assert rc("cgcn_mapcmp_smooth", sm, ld=9) == -1 and rc("cgcn_mapcmp_smooth", sm, norm=q, n_norm=0) == -1
    assert rc("cgcn_mapcmp_smooth", sm, n=-1) == -1 and rc("cgcn_mapcmp_smooth", sm, D=-1) == -1
    assert rc("cgcn_mapcmp_smooth", sm, h=21, width=47) == -2
    assert rc("cgcn_mapcmp_smooth", sm, n=2 ** 21, ld=2 ** 21, width=129) == -2
    assert rc("cgcn_mapcmp_smooth", sm, n=0, ld=0, band=None, S=None) == 0
    wsp = _lib.query("cgcn_mapcmp_workspace_bytes", n=4100, D=4)
    assert wsp >= 5 * 3 * 28 and _lib.query("cgcn_mapcmp_workspace_bytes", n=-1, D=4) == 0
    assert _lib.query("cgcn_mapcmp_workspace_bytes", n=2 ** 20, D=2 ** 9) == 0 and _lib.query("cgcn_mapcmp_workspace_bytes", n=0, D=0) > 0
    su = dict(stream=None, n=4100, D=4, ld=4100, Sa=q, Sb=q, valid=q, min_dist=1, pass_no=1, workspace=q, workspace_bytes=wsp,
              cells=q, stats=q)
    for ptr in ("Sa", "Sb", "valid", "workspace", "cells", "stats"):
        assert rc("cgcn_mapcmp_sums", su, **{ptr: None}) == -1
    assert rc("cgcn_mapcmp_sums", su, pass_no=0) == -1 and rc("cgcn_mapcmp_sums", su, pass_no=3) == -1
    assert rc("cgcn_mapcmp_sums", su, min_dist=-1) == -1 and rc("cgcn_mapcmp_sums", su, ld=4099) == -1
    assert rc("cgcn_mapcmp_sums", su, workspace_bytes=wsp - 1) == -4
    assert rc("cgcn_mapcmp_sums", su, n=2 ** 20, ld=2 ** 20, D=2 ** 9) == -2
