"""Insulation scores, boundaries, domains and the domain-restricted graph on the host (chromegcn_amd/insulation.py, the
`domains` argument of chromegcn_amd/hic.py's host builder): the diamond sums against the literal double loop over the dense
matrix, the rule behind the sums against hand-written profiles and a loop restatement written for this file, the recovery of
planted domain starts, the argument checks of the C entry point (no launch, no GPU), tools/hic_domains.py on the restatement
and the defaults of the train flags."""
import ctypes
import math

import numpy as np
import pytest

import insulation_cases as IC
from chromegcn_amd import _build, _lib, hic, hicdist, hicnorm, insulation

SUM_CASES = ("n1", "n2", "n63", "n65_nodiag", "n257_frac", "fullrow")


# ----------------------------------------------------------------------------------------------
# rule 2: the sums
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_norm", [False, True])
@pytest.mark.parametrize("name", SUM_CASES)
def test_diamond_sums_equal_the_double_loop(name, with_norm):
    c = IC.case(name)
    a = IC.dense(c)
    norm = IC.noisy_norm(c["n_bins"], 40 + c["n_bins"]) if with_norm else None
    want, K = IC.loop_sums(a, norm, IC.SUM_WINDOWS)
    got = insulation.diamond_sums_host(hicnorm.contact_matrix_host(c["pos1"], c["pos2"], c["count"], c["res"], c["n_bins"]),
                                       norm, IC.SUM_WINDOWS)
    integer = bool(np.all(c["count"] == np.floor(c["count"])))
    IC.assert_sums_close(got, want, K, exact=integer and not with_norm)
    assert np.all(got[:, 0] == 0)
    assert np.array_equal(K, IC.term_counts(a, norm, IC.SUM_WINDOWS))   # the counter the GPU tests bound their error with
    if with_norm and c["n_bins"] > 4:
        assert np.any((want == 0) & (IC.loop_sums(a, None, IC.SUM_WINDOWS)[0] > 0))   # the NaN / 0 bins empty some diamonds


def test_diamond_sums_in_chunks_equal_one_pass(monkeypatch):
    c = IC.planted_case("n257")
    A = hicnorm.contact_matrix_host(c["pos1"], c["pos2"], c["count"], c["res"], c["n_bins"])
    want = insulation.diamond_sums_host(A, None, (3, 25))
    monkeypatch.setattr(insulation, "_CHUNK", 1000)
    assert np.array_equal(insulation.diamond_sums_host(A, None, (3, 25)), want)   # integer counts: exact in every order


def test_windows_are_checked():
    A = np.ones((4, 4))
    for bad in ([], [0], [2, 2], [3, 2], list(range(1, 10))):
        with pytest.raises(ValueError):
            insulation.diamond_sums_host(A, None, bad)
    with pytest.raises(ValueError):
        insulation.windows_in_bins([1500], 1000)
    assert insulation.windows_in_bins([2000, 5000], 1000) == (2, 5)


# ----------------------------------------------------------------------------------------------
# rules 3 - 6: hand-written profiles.  One window of 1 bin, every bin valid: npix = 1 from bin 1 on, so score = S and
# L = log2(S / mean); S = 2^p makes the differences of L whole numbers up to the rounding of the quotient and the logarithm.
# ----------------------------------------------------------------------------------------------
def profile(p, span, min_strength=0.9, **kw):
    S = np.array([0.0 if x is None else 2.0 ** x for x in p])[None, :]
    return insulation.insulation_from_sums(S, np.ones(len(p), bool), (1,), span=span, min_strength=min_strength, **kw)


def test_the_leftmost_of_equal_minima_wins():
    r = profile([None, 3, 3, 1, 1, 3, 3], span=2)
    assert r.boundaries[0].tolist() == [3] and r.strength[0].tolist() == pytest.approx([2.0], abs=1e-12)
    assert not r.defined[0, 0] and r.defined[0, 1:].all() and np.isnan(r.log2[0, 0])
    r = profile([None, 3, 3, 1, 2, 1, 3, 3], span=1)   # span 1: two separate minima
    assert r.boundaries[0].tolist() == [3, 5] and r.strength[0].tolist() == pytest.approx([1.0, 1.0], abs=1e-12)
    assert profile([None, 3, 3, 1, 2, 1, 3, 3], span=2).boundaries[0].tolist() == [3]


def test_no_boundary_without_a_defined_neighbour_on_each_side():
    assert profile([None, 0, 3, 3, 3], span=2).boundaries[0].size == 0            # nothing defined to the left of bin 1
    assert profile([None, 3, 3, 3, 0], span=2).boundaries[0].size == 0            # nothing to the right of the last bin
    p = [None, 3, 3, None, None, 1, None, None, 3, 3]
    assert profile(p, span=2).boundaries[0].size == 0                             # both neighbourhoods undefined (S = 0)
    r = profile(p, span=4)
    assert r.boundaries[0].tolist() == [5] and r.strength[0].tolist() == pytest.approx([2.0], abs=1e-12)
    assert profile(p, span=4, min_strength=2.5).boundaries[0].size == 0           # the strength threshold
    assert profile([None, 3, 3, None, 1, 3, 3], span=1).boundaries[0].size == 0   # left neighbour undefined at span 1


def test_the_npix_threshold():
    valid = np.ones(8, bool)
    valid[3] = False
    S = np.ones((1, 8))
    r = insulation.insulation_from_sums(S, valid, (2,))                        # ceil(0.66 * 4) = 3
    assert r.npix[0].tolist() == [0, 2, 2, 2, 2, 2, 4, 2]
    assert r.defined[0].tolist() == [False] * 6 + [True, False]
    r = insulation.insulation_from_sums(S, valid, (2,), min_valid_share=0.5)   # ceil(0.5 * 4) = 2
    assert r.defined[0].tolist() == [False, True, True, False, True, True, True, True]
    assert np.array_equal(r.score[0][r.defined[0]], np.array([0.5, 0.5, 0.5, 0.5, 0.25, 0.5]))


def test_domain_of_bin():
    d = insulation.domains_from_boundaries([3, 7], 10)
    assert d.dtype == np.int32 and d.tolist() == [0, 0, 0, 1, 1, 1, 1, 2, 2, 2]
    assert insulation.domains_from_boundaries([], 4).tolist() == [0, 0, 0, 0]
    assert insulation.domains_from_boundaries([0], 3).tolist() == [1, 1, 1]


def brute_rule(S, valid, w, share, s, min_strength):
    """rules 3 to 5 for one window, one bin after the other: (defined, L, boundaries, strengths)"""
    n = len(valid)
    defined, score = np.zeros(n, bool), np.full(n, np.nan)
    for i in range(n):
        up = sum(bool(valid[j]) for j in range(max(i - w, 0), i))
        dn = sum(bool(valid[j]) for j in range(i, min(i + w, n)))
        defined[i] = bool(valid[i]) and up * dn >= math.ceil(share * (w * w)) and S[i] > 0
        if defined[i]:
            score[i] = S[i] / (up * dn)
    L = np.full(n, np.nan)
    if defined.any():
        L[defined] = np.log2(score[defined] / np.mean(score[defined]))
    bounds, strengths = [], []
    for i in range(n):
        if not defined[i]:
            continue
        left = [L[j] for j in range(max(i - s, 0), i) if defined[j]]
        right = [L[j] for j in range(i + 1, min(i + s, n - 1) + 1) if defined[j]]
        if left and right and all(L[i] < x for x in left) and all(L[i] <= x for x in right):
            st = min(max(left), max(right)) - L[i]
            if st >= min_strength:
                bounds.append(i)
                strengths.append(st)
    return defined, L, bounds, strengths


@pytest.mark.parametrize("name", ["n257", "n400_empty"])
def test_the_rule_equals_its_loop_restatement(name):
    ins = IC.planted_host(name)
    for span, strength, share in ((None, 0.2, 0.66), (7, 0.0, 0.9)):
        got = insulation.insulation_from_sums(ins.sums, ins.valid, ins.windows, min_valid_share=share, span=span, min_strength=strength)
        for k, w in enumerate(ins.windows):
            defined, L, bounds, strengths = brute_rule(ins.sums[k], ins.valid, w, share, w if span is None else span, strength)
            assert np.array_equal(got.defined[k], defined) and np.array_equal(got.log2[k], L, equal_nan=True)
            assert got.boundaries[k].tolist() == bounds and got.strength[k].tolist() == strengths
            assert len(bounds) >= 3   # the planted starts at least


@pytest.mark.parametrize("seed", IC.SEEDS)
@pytest.mark.parametrize("name", sorted(IC.PLANTED))
def test_planted_starts_are_recovered(name, seed):
    c, ins = IC.planted_case(name, seed), IC.planted_host(name, seed)
    for k in range(len(IC.RECOVERY_WINDOWS)):
        assert ins.boundaries[k].tolist() == c["starts"].tolist()
        assert np.all(ins.strength[k] >= IC.RECOVERY_STRENGTH)
        assert np.array_equal(ins.domain_of_bin(k), np.searchsorted(c["starts"], np.arange(c["n_bins"]), side="right"))
    assert not ins.valid[c["empty"]].any() and ins.valid.sum() == c["n_bins"] - c["empty"].size


def test_named_norm_and_domains_host():
    c = IC.planted_case("n400")
    vc, _ = hicnorm.hic_norm_vector_host(c["pos1"], c["pos2"], c["count"], "VC", IC.RES, c["n_bins"])
    a = insulation.insulation_host(c["pos1"], c["pos2"], c["count"], "VC", IC.RES, [10 * IC.RES], n_bins=c["n_bins"], min_strength=1.0)
    b = insulation.insulation_host(c["pos1"], c["pos2"], c["count"], vc, IC.RES, [10 * IC.RES], n_bins=c["n_bins"], min_strength=1.0)
    assert np.array_equal(a.sums, b.sums) and a.boundaries[0].tolist() == b.boundaries[0].tolist() == c["starts"].tolist()
    dom, bp = insulation.domains_host(c["pos1"], c["pos2"], c["count"], 10 * IC.RES, norm="VC", resolution_bp=IC.RES,
                                      n_bins=c["n_bins"], min_strength=1.0)
    assert bp == IC.RES and np.array_equal(dom, a.domain_of_bin(0))
    with pytest.raises(TypeError):
        insulation.insulation_host(c["pos1"], c["pos2"], c["count"], None, IC.RES, [10 * IC.RES], strength=1.0)


# ----------------------------------------------------------------------------------------------
# rule 7: the host builder
# ----------------------------------------------------------------------------------------------
DOMAIN_BP = 5 * IC.RES
DOMAINS = np.searchsorted([5, 11, 17], np.arange(22), side="right").astype(np.int32)   # 22 of the 24 bins: the rest never match


def explicit_vectors(c):
    """the VC vector and the "auto" expected vector of ALL records, as the builder computes them"""
    vc, _ = hicnorm.hic_norm_vector_host(c["pos1"], c["pos2"], c["count"], "VC", c["res"])
    return vc, hicdist.expected_vector_host(c["pos1"], c["pos2"], c["count"], vc, c["res"])


@pytest.mark.parametrize("gap", [0, 3000])
@pytest.mark.parametrize("scoring", ["raw", "vc_oe"])
def test_host_builder_within_domains(scoring, gap):
    c, ws = IC.graph_case()
    norm, ex = (None, None) if scoring == "raw" else ("VC", "auto")
    got = hic.build_hic_graph_host(c["pos1"], c["pos2"], c["count"], norm, c["res"], ws, IC.GRAPH_EDGES,
                                   min_distance_bp=gap, expected=ex, domains=(DOMAINS, DOMAIN_BP))
    dom = insulation.domain_of_windows(ws, DOMAINS, DOMAIN_BP)
    assert (dom < 0).any() and got.nnz > 100
    coo = got.tocoo()
    assert np.all(dom[coo.row] == dom[coo.col]) and np.all(dom[coo.row] >= 0)       # every edge joins two windows of one domain
    assert insulation.domain_edge_share(got, dom) == (got.nnz, got.nnz)
    keep = insulation.same_domain_host(c["pos1"], c["pos2"], DOMAINS, DOMAIN_BP)
    assert 0 < keep.sum() < keep.size
    nv, ev = (None, None) if scoring == "raw" else explicit_vectors(c)
    if nv is not None:
        nv = hicnorm.pad_vector(nv, int(ws[-1]) // c["res"] + 1)
    want = hic.build_hic_graph_host(c["pos1"][keep], c["pos2"][keep], c["count"][keep], nv, c["res"], ws, IC.GRAPH_EDGES,
                                    min_distance_bp=gap, expected=ev)
    assert np.array_equal(got.indptr, want.indptr) and np.array_equal(got.indices, want.indices)
    free = hic.build_hic_graph_host(c["pos1"], c["pos2"], c["count"], norm, c["res"], ws, IC.GRAPH_EDGES, min_distance_bp=gap, expected=ex)
    same, nnz = insulation.domain_edge_share(free, dom)
    assert 0 < same < nnz == free.nnz                                               # the unrestricted graph crosses boundaries


def test_domains_none_is_unchanged_and_arguments_are_checked():
    c, ws = IC.graph_case()
    base = hic.build_hic_graph_host(c["pos1"], c["pos2"], c["count"], "VC", c["res"], ws, IC.GRAPH_EDGES)
    for d in (None, (np.zeros(c["n_bins"], np.int32), c["res"])):   # one domain that holds every bin keeps every record
        g = hic.build_hic_graph_host(c["pos1"], c["pos2"], c["count"], "VC", c["res"], ws, IC.GRAPH_EDGES, domains=d)
        assert np.array_equal(g.indptr, base.indptr) and np.array_equal(g.indices, base.indices)
    a = hic.survivor_values(c["pos1"], c["pos2"], c["count"], None, c["res"], ws)
    b = hic.survivor_values(c["pos1"], c["pos2"], c["count"], None, c["res"], ws, domains=(DOMAINS, DOMAIN_BP))
    keep = insulation.same_domain_host(c["pos1"], c["pos2"], DOMAINS, DOMAIN_BP)
    assert np.array_equal(b[0], a[0][keep[a[0]]])   # the indices of the whole file, in file order
    with pytest.raises(ValueError):
        hic.build_hic_graph_host(c["pos1"], c["pos2"], c["count"], None, c["res"], ws, IC.GRAPH_EDGES, domains=(DOMAINS, 1500))
    with pytest.raises(ValueError):
        hic.build_hic_graph_host(c["pos1"], c["pos2"], c["count"], None, c["res"], ws, IC.GRAPH_EDGES, domains=DOMAINS)


def test_host_builder_takes_domains_computed_from_the_records():
    c = IC.planted_case("n257")
    ws = (np.arange(0, 257, 2) * IC.RES).astype(np.int32)
    kw = dict(window_bp=10 * IC.RES, norm=None, resolution_bp=IC.RES, min_strength=1.0)
    got = hic.build_hic_graph_host(c["pos1"], c["pos2"], c["count"], None, IC.RES, ws, 600, domains=kw)
    dom = np.searchsorted(c["starts"], np.arange(257), side="right").astype(np.int32)
    want = hic.build_hic_graph_host(c["pos1"], c["pos2"], c["count"], None, IC.RES, ws, 600, domains=(dom, IC.RES))
    assert got.nnz > 0 and np.array_equal(got.indptr, want.indptr) and np.array_equal(got.indices, want.indices)


# ----------------------------------------------------------------------------------------------
# the C entry point's argument checks: nothing is launched, the library loads without a GPU
# ----------------------------------------------------------------------------------------------
def test_entry_point_argument_checks():
    _build.build_library()
    _lib.load()
    p = 0x10000   # never read: every call below returns before a launch
    win = lambda *w: (ctypes.c_int32 * len(w))(*w)   # noqa: E731
    ok = dict(stream=None, n=10, rowptr=p, col=p, val=p, norm=None, n_norm=0, n_windows=2, windows=win(2, 5), out=p)

    def rc(**kw):
        return _lib.query("cgcn_hicinsul_sums", **{**ok, **kw})

    for name in ("rowptr", "col", "val", "out", "windows"):
        assert rc(**{name: None}) == -1
    assert rc(n=-1) == -1 and rc(n_windows=0) == -1 and rc(n_windows=-3) == -1
    assert rc(norm=p, n_norm=0) == -1 and rc(n_norm=-1) == -1
    assert rc(windows=win(0, 5)) == -1 and rc(windows=win(5, 5)) == -1 and rc(windows=win(5, 2)) == -1
    assert rc(n_windows=3, windows=win(1, 2, -4)) == -1
    assert rc(n_windows=9, windows=win(*range(1, 10))) == -2
    assert rc(n=0, col=None, val=None, out=None) == 0   # no bins: nothing to read, nothing launched
    with pytest.raises(RuntimeError, match=r"cgcn_hicinsul_sums failed: bad argument.*\(code -1\)"):
        _lib.call("cgcn_hicinsul_sums", **{**ok, "windows": win(3, 3)})


# ----------------------------------------------------------------------------------------------
# the command line and the train flags
# ----------------------------------------------------------------------------------------------
def test_hic_domains_tool_writes_the_planted_domains(tmp_path, capsys):
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("hic_domains", os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "tools", "hic_domains.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    c = IC.planted_case("n257")
    cache = str(tmp_path / "chrT.cghic")
    hic.save_contacts_cache(cache, hic.HostContacts(c["pos1"], c["pos2"], c["count"], {}, IC.RES, None))
    prefix = str(tmp_path / "out" / "chrT")
    tool.main([cache, "--chrom", "chrT", "--res", str(IC.RES), "--windows", "10000,25000", "--norm", "RAW", "--min-strength", "1.0",
               "--domain-window", "25000", "--out-prefix", prefix, "--host"])
    rows = [ln.split("\t") for ln in open(prefix + ".domains.bed").read().splitlines()]
    edges = [0] + (c["starts"] * IC.RES).tolist() + [257 * IC.RES]
    assert [(r[0], int(r[1]), int(r[2]), r[3]) for r in rows] == [("chrT", a, b, "domain%d" % k)
                                                                  for k, (a, b) in enumerate(zip(edges[:-1], edges[1:]))]
    ins = IC.planted_host("n257")
    assert [float(r[4]) for r in rows] == pytest.approx([0.0] + ins.strength[1].tolist(), abs=1e-6)
    graph = [ln.split("\t") for ln in open(prefix + ".w10000.log2.bedGraph").read().splitlines()]
    assert [int(r[1]) // IC.RES for r in graph] == np.flatnonzero(ins.defined[0]).tolist()
    assert [float(r[3]) for r in graph] == pytest.approx(ins.log2[0][ins.defined[0]].tolist(), abs=1e-6)
    assert "3 boundaries" in capsys.readouterr().out


def test_train_flags_default_to_off():
    from chromegcn_amd import train
    opt = train.parse(["-synthetic"])
    assert (opt.hic_domains, opt.hic_domain_res, opt.hic_domain_strength) == (0, 10000, 0.5)
    opt = train.parse(["-synthetic", "-hic_domains", "250000", "-hic_domain_res", "5000", "-hic_domain_strength", "0.8"])
    assert (opt.hic_domains, opt.hic_domain_res, opt.hic_domain_strength) == (250000, 5000, 0.8)
