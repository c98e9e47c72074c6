"""The pile-up rule (chromegcn_amd/pileup.py) on the host: the numpy restatement against the literal loop, the two-level
summation order pinned by a case that only that order answers, hand-written answers for a single planted pixel, exact integer
sums, the participation counts beside empty and unbalanced bins, every skip reason at and off its boundary, the scores on a
hand-written matrix, the centre-list helpers, the guards, the ordering of planted loops against their shifted control, the tool
and the train flag.  Nothing here needs a GPU."""
import importlib.util
import os

import numpy as np
import pytest
import scipy.sparse as sp

from chromegcn_amd import hic, hicmap, hicnorm, loops, pileup

import pileup_cases as PC
from pileup_cases import LC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host_band(A, norm, ex, r):
    A = sp.csr_matrix(A, dtype=np.float64)
    return pileup.value_band_host(hicmap.band_host(A, r.width), np.asarray(A.sum(axis=1)).ravel(), norm, ex, r)


@pytest.mark.parametrize("value", pileup.VALUES)
@pytest.mark.parametrize("w", [1, 2, 5])
def test_sums_against_the_literal_loop(w, value):
    n = 64
    A, _ = PC.integer_map(n)
    r = PC.rule_for(n, w, value)
    ex = np.random.default_rng(w).uniform(0.2, 3.0, r.max_dist + 3)         # shorter than the band: reads as 0 beyond
    vb = host_band(A, PC.noisy_norm(n, 7), ex, r)
    assert np.isnan(vb).any() and np.isfinite(vb).sum() > 200
    for M, G in ((600, 3), (257, 1), (40, 64)):
        ci, cj, g = PC.centres(n, r, M, G, seed=M + w)
        got = pileup.pileup_sums_host(vb, ci, cj, g, G, r)
        P, N, kept, skipped = PC.literal_sums(vb, ci, cj, g, G, r)
        assert PC.same_bits(got.sum, P) and np.array_equal(got.count, N)
        assert np.array_equal(got.kept, kept) and got.skipped == skipped
        assert kept.sum() > 0 and sum(skipped.values()) > 0                         # each reason: its own test below
        if G == 3:
            assert kept[1] == 0 and not got.count[1].any() and np.isnan(got.mean[1]).all()


def test_the_two_level_order_is_pinned():
    """601 centres whose centre cells hold 1e16, 255 x 1, 256 x 1, 88 x 1, 1e16.  Slice 0 is 1e16 then ones (every + 1 is
    rounded away: 1e16), slice 1 is 256, slice 2 is 88 then 1e16 (1e16 + 88, exact); folded in slice order: 1e16 + 256, then
    2e16 + 344, exact.  One flat sequential sum gives 2e16, a pairwise or an exact sum 2e16 + 600."""
    vals = np.array([1e16] + [1.0] * 255 + [1.0] * 256 + [1.0] * 88 + [1e16])
    M, d = vals.size, 5
    n = M + 10
    r = pileup.pileup_rule(PC.RES, n, value="observed", w=1, max_distance_bp=8 * PC.RES)
    vb = np.zeros((n, r.width))
    ci = 1 + np.arange(M)
    vb[ci, d] = vals
    got = pileup.pileup_sums_host(vb, ci, ci + d, None, 1, r)
    assert got.kept[0] == M == 601 and got.sum[0, 1, 1] == 2e16 + 344.0
    assert float(np.sum(vals)) != 2e16 + 344.0                               # pairwise: another answer
    flat = 0.0
    for v in vals:
        flat += v
    assert flat == 2e16                                                      # one level: another answer still
    P, _, _, _ = PC.literal_sums(vb, ci, ci + d, None, 1, r)
    assert PC.same_bits(got.sum, P)
    # the groups are summed apart: the same cells split over two interleaved groups
    g = np.arange(M) % 2
    two = pileup.pileup_sums_host(vb, ci, ci + d, g, 2, r)
    # group 0: 1e16 and 255 ones (1e16), then 44 ones and 1e16 (1e16 + 44); group 1: 256 ones, then 44
    assert two.kept.tolist() == [301, 300] and two.sum[0, 1, 1] == 2e16 + 44.0 and two.sum[1, 1, 1] == 300.0


def test_a_single_planted_pixel():
    """one contact of 7 between bins 20 and 40: the only cell with two valid bins.  Every centre sees it at the offset
    (20 - i, 40 - j) or not at all."""
    kw = dict(norm=None, resolution_bp=1000, n_bins=64, value="observed", w=2, min_dist=4, max_distance_bp=30000)
    rec = ([20000], [40000], [7.0])

    def run(centres, **more):
        return pileup.pileup_host(*rec, centres, **{**kw, **more})
    p = run(([20], [40]))
    want = np.zeros((5, 5))
    want[2, 2] = 7.0
    assert np.array_equal(p.sum[0], want) and np.array_equal(p.count[0], want == 7.0) and p.kept.tolist() == [1]
    assert p.mean[0, 2, 2] == 7.0 and np.isnan(p.mean[0]).sum() == 24
    p = run(([19], [41]))                       # the pixel lies one row below and one column left: towards the diagonal
    want = np.zeros((5, 5))
    want[3, 1] = 7.0
    assert np.array_equal(p.sum[0], want) and p.count[0].sum() == 1
    p = run(([22, 18, 20, 17], [38, 42, 43, 40]))     # offsets (-2, 2), (2, -2); (0, -3) and (3, 0) lie outside the window
    want = np.zeros((5, 5))
    want[0, 4] = want[4, 0] = 7.0
    assert np.array_equal(p.sum[0], want) and p.count[0].sum() == 2 and p.kept.tolist() == [4]
    p = run(([20, 20, 20], [40, 40, 40]))       # duplicates are kept
    assert p.sum[0, 2, 2] == 21.0 and p.count[0, 2, 2] == 3 and p.kept.tolist() == [3]
    p = run(([40, 20], [20, 40]), group=[1, 0], n_groups=3)     # a swapped centre; group 2 stays empty
    assert p.sum[:, 2, 2].tolist() == [7.0, 7.0, 0.0] and p.kept.tolist() == [1, 1, 0] and np.isnan(p.mean[2]).all()
    # balanced by a vector and over an explicit expected vector: the stated order of operations
    nv = np.full(64, 2.0)
    nv[40] = 3.0
    p = run(([20], [40]), norm=nv, value="balanced")
    assert p.sum[0, 2, 2] == 7.0 / (2.0 * 3.0)
    ex = np.full(31, 0.7)
    p = run(([20], [40]), norm=nv, value="oe", expected=ex)
    assert p.sum[0, 2, 2] == (7.0 / (2.0 * 3.0)) / 0.7
    ex[20] = 0.0                                # no expected value at the pixel's distance: the cell takes no part
    p = run(([20], [40]), norm=nv, value="oe", expected=ex)
    assert p.count.sum() == 0 and p.kept.tolist() == [1]
    with pytest.raises(ValueError):
        run(([20], [40]), norm=nv, value="oe", expected=np.ones(30))         # must reach min(n, max_dist + 1) = 31


def test_integer_counts_are_exact():
    n = 257
    A, _ = PC.integer_map(n)
    r = PC.rule_for(n, 2, "observed")
    ci, cj, g = PC.centres(n, r, 3000, 3, seed=11)
    got = pileup.pileup_sums_host(host_band(A, None, None, r), ci, cj, g, 3, r)
    want, cnt = PC.integer_reference(A, ci, cj, g, 3, r)
    assert got.kept.sum() > 1500 and np.array_equal(got.count, cnt)
    assert np.array_equal(got.sum, want.astype(np.float64)) and want.max() > 1000


def test_counts_beside_empty_and_unbalanced_bins():
    n = 40
    dense = np.ones((n, n))
    dense[12, :] = dense[:, 12] = 0.0                                       # an empty bin
    norm = np.ones(n)
    norm[25], norm[27] = np.nan, 0.0
    r = pileup.pileup_rule(PC.RES, n, value="balanced", w=1, max_distance_bp=30 * PC.RES)
    vb = host_band(dense, norm, None, r)
    p = pileup.pileup_sums_host(vb, [11, 5, 5, 5], [20, 24, 26, 15], None, 1, r)
    # (11, 20): row da = +1 is bin 12; (5, 24): column db = +1 is bin 25; (5, 26): columns -1 and +1 are 25 and 27; (5, 15): whole
    want = np.array([[3, 4, 2], [3, 4, 2], [2, 3, 1]])
    assert np.array_equal(p.count[0], want) and np.array_equal(p.sum[0], want.astype(np.float64))
    raw = pileup.pileup_sums_host(host_band(dense, None, None, r._replace(value="observed")), [11, 5, 5, 5], [20, 24, 26, 15], None, 1,
                                  r._replace(value="observed"))
    assert np.array_equal(raw.count[0], np.array([[4, 4, 4], [4, 4, 4], [3, 3, 3]]))        # without a vector only bin 12 is out


def test_every_skip_reason_at_its_boundary():
    n, w = 50, 2
    r = pileup.pileup_rule(PC.RES, n, value="observed", w=w, min_dist=6, max_distance_bp=20 * PC.RES)
    vb = np.ones((n, r.width))

    def run(i, j, g=0, G=2):
        p = pileup.pileup_sums_host(vb, [i], [j], [g], G, r)
        return int(p.kept.sum()), p.skipped
    none = dict.fromkeys(pileup.REASONS, 0)
    assert run(10, 20, 0) == (1, none) and run(10, 20, 1) == (1, none)
    assert run(10, 20, 2) == (0, {**none, "group": 1}) and run(10, 20, -1) == (0, {**none, "group": 1})
    assert run(2, 12) == (1, none) and run(1, 11) == (0, {**none, "edge": 1})                # i - w >= 0
    assert run(30, 47) == (1, none) and run(31, 48) == (0, {**none, "edge": 1})              # j + w <= n - 1
    assert run(10, 16) == (1, none) and run(10, 15) == (0, {**none, "near": 1})              # min_dist <= j - i
    assert run(10, 30) == (1, none) and run(10, 31) == (0, {**none, "far": 1})               # j - i <= max_dist
    assert run(1, 40, 5) == (0, {**none, "group": 1})                                        # the first failing test counts
    assert run(1, 3) == (0, {**none, "edge": 1}) and run(47, 2) == (0, {**none, "far": 1})
    p = pileup.pileup_sums_host(vb, [], [], None, 2, r)                                      # M = 0
    assert p.kept.tolist() == [0, 0] and not p.sum.any() and not p.count.any() and np.isnan(p.mean).all()
    assert all(np.isnan(v).all() for v in p.scores().values())


def test_scores_on_a_hand_written_mean():
    m = np.ones((7, 7))
    m[3, 3] = 6.0
    m[5:, :2] = [[2.0, 4.0], [np.nan, 3.0]]     # LL at c = 2: mean 3, std(ddof=1) 1; the NaN cell is ignored
    m[:2, 5:] = 2.0                              # UR
    m[0, 0] = np.nan                             # UL: the other three are 1
    s = pileup.apa_scores(m, 2)
    assert s["P2LL"] == 2.0 and s["P2UR"] == 3.0 and s["P2UL"] == 6.0 and s["P2LR"] == 6.0
    assert s["ZscoreLL"] == 3.0
    others = np.delete(m.ravel(), 24)
    assert s["P2M"] == 6.0 / np.nanmean(others)
    s1 = pileup.apa_scores(m, 1)
    assert np.isnan(s1["ZscoreLL"]) and np.isnan(s1["P2UL"]) and np.isnan(s1["P2LL"]) and s1["P2UR"] == 3.0
    both = pileup.apa_scores(np.stack([m, 2.0 * m]), 2)
    assert both["P2LL"].tolist() == [2.0, 2.0] and both["ZscoreLL"].tolist() == [3.0, 3.0]
    with pytest.raises(ValueError):
        pileup.apa_scores(m, 4)
    with pytest.raises(ValueError):
        pileup.apa_scores(np.ones((6, 6)), 2)


def test_centre_lists():
    rng = np.random.default_rng(3)
    n = 30
    g = sp.random(n, n, 0.2, random_state=5, format="csr")
    ws = np.sort(rng.choice(np.arange(0, 400000, 1000), n, replace=False))
    i, j, entry = pileup.centres_of_graph(g, ws, 10000)
    want = []
    for row in range(n):
        for q in range(g.indptr[row], g.indptr[row + 1]):
            if g.indices[q] > row:
                a, b = ws[row] // 10000, ws[g.indices[q]] // 10000
                want.append((min(a, b), max(a, b), q))
    assert len(want) > 20 and [tuple(x) for x in zip(i.tolist(), j.tolist(), entry.tolist())] == want
    i2, j2, e2 = pileup.centres_of_graph((g.indptr, g.indices), ws, 10000)
    assert np.array_equal(i, i2) and np.array_equal(entry, e2)
    with pytest.raises(ValueError):
        pileup.centres_of_graph(g, ws[:-1], 10000)
    si, sj = pileup.shifted_centres(i, j, 9)
    assert np.array_equal(si, i + 9) and np.array_equal(sj - si, j - i)
    assert pileup.distance_groups([0, 0, 0, 0, 9], [4, 5, 19, 20, 0], [5, 10, 20]).tolist() == [-1, 0, 1, -1, 0]
    with pytest.raises(ValueError):
        pileup.distance_groups([0], [1], [5])
    q = pileup.quantile_groups([0.3, np.nan, 0.1, 0.2, 0.4, 0.1], 2)
    assert q.tolist() == [1, -1, 0, 0, 1, 0]
    assert np.bincount(pileup.quantile_groups(rng.random(1000), 4)).tolist() == [250] * 4


def test_slice_table():
    so, go = pileup.slice_table([0, 1, 256, 0, 257, 600])
    assert go.tolist() == [0, 0, 1, 2, 2, 4, 7] and so.tolist() == [0, 1, 257, 513, 514, 770, 1026, 1114]
    so, go = pileup.slice_table([0, 0])
    assert so.tolist() == [0] and go.tolist() == [0, 0, 0]


def test_guards():
    rule = pileup.pileup_rule
    assert rule(10000)[1:] == ("oe", 10, 6, 30, 200) and rule(25000)[1:] == ("oe", 5, 3, 15, 80)
    assert rule(10000, w=4).corner == 3 and rule(10000).width == 221
    for bad in (dict(w=11), dict(w=0), dict(w=3, corner=4), dict(w=3, corner=0), dict(w=3, min_dist=5), dict(value="kr"),
                dict(max_distance_bp=-1)):
        with pytest.raises(ValueError):
            rule(10000, **bad)
    assert rule(10000, w=3, min_dist=6).min_dist == 6
    rule(10000, n=(1 << 28) // 221)
    with pytest.raises(ValueError, match="2\\^28"):
        rule(10000, n=(1 << 28) // 221 + 1)
    rule(10000, n_groups=65536)
    with pytest.raises(ValueError):
        rule(10000, n_groups=65537)
    with pytest.raises(TypeError):
        rule(10000, p=1)
    r = rule(10000, 64, w=2, max_distance_bp=200000)
    vb = np.zeros((64, r.width))
    with pytest.raises(ValueError, match="different lengths"):
        pileup.pileup_sums_host(vb, [1, 2], [3], None, 1, r)
    with pytest.raises(ValueError, match="different lengths"):
        pileup.pileup_sums_host(vb, [1, 2], [30, 40], [0], 1, r)
    with pytest.raises(ValueError):
        pileup.pileup_sums_host(vb[:, :-1], [10], [30], None, 1, r)
    with pytest.raises(ValueError):
        pileup.pileup_sums_host(vb, [10.5], [30.0], None, 1, r)
    with pytest.raises(ValueError):
        pileup.pileup_sums_host(vb, [10], [30], None, 65537, r)
    with pytest.raises(ValueError):
        pileup.pileup_host([0], [50000], [1.0], ([1], [2, 3]), resolution_bp=10000)
    with pytest.raises(ValueError):
        pileup.pileup_host([0], [50000], [1.0], ([1], [30]), resolution_bp=10000, w=11)
    with pytest.raises(ValueError):
        pileup.pileup_host([0], [50000], [1.0], ([1], [30]), resolution_bp=10000, expected="mean")


# P2LL of the six plants and of their control shifted by 9 bins, measured on the restatement
@pytest.mark.parametrize("seed", LC.SEEDS)
def test_planted_loops_stand_out_from_their_shifted_control(seed):
    plants, control = PC.planted_scores(seed)
    assert plants.kept.tolist() == [LC.P_BLOBS] and control.kept[0] >= LC.P_BLOBS - 2
    p, c = plants.scores(), control.scores()
    print("seed %d: P2LL %.4f against %.4f, P2M %.4f against %.4f, ZscoreLL %.3f against %.3f (%d control centres)"
          % (seed, p["P2LL"][0], c["P2LL"][0], p["P2M"][0], c["P2M"][0], p["ZscoreLL"][0], c["ZscoreLL"][0], control.kept[0]))
    assert p["P2LL"][0] > c["P2LL"][0]


def test_host_pileup_from_records_is_the_pieces():
    c = LC.planted(3)
    A = hicnorm.contact_matrix_host(c["pos1"], c["pos2"], c["count"], c["res"], c["n_bins"])
    vc, ex = LC.planted_vectors(3)
    r = pileup.pileup_rule(c["res"], c["n_bins"], w=3, max_distance_bp=LC.P_D * LC.P_RES)
    found = LC.planted_host(3)
    got = pileup.pileup_host(c["pos1"], c["pos2"], c["count"], found, norm="VC", resolution_bp=c["res"], expected=ex,
                             n_bins=c["n_bins"], w=3, max_distance_bp=LC.P_D * LC.P_RES)
    want = pileup.pileup_sums_host(host_band(A, vc, ex, r), found.peak_i, found.peak_j, None, 1, r)
    PC.assert_same_pileup(got, want)
    assert got.kept[0] == len(found) > 0 and got.scores()["P2LL"][0] > 1.5


def test_hic_apa_tool_on_a_tiny_fixture(tmp_path, capsys):
    spec = importlib.util.spec_from_file_location("hic_apa", os.path.join(ROOT, "tools", "hic_apa.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    c = LC.planted(2)
    cache = str(tmp_path / "chrT.cghic")
    hic.save_contacts_cache(cache, hic.HostContacts(c["pos1"], c["pos2"], c["count"], {}, LC.P_RES, None))
    bedpe = str(tmp_path / "plants.bedpe")
    with open(bedpe, "w") as f:
        f.write("# planted\n")
        for i, j in c["plants"]:
            f.write("chrT\t%d\t%d\tchrT\t%d\t%d\n" % (i * LC.P_RES, (i + 1) * LC.P_RES, j * LC.P_RES, (j + 1) * LC.P_RES))
        f.write("chrU\t0\t10000\tchrU\t200000\t210000\n")                  # another chromosome: not read
    out = str(tmp_path / "out" / "chrT.apa")
    tool.main([cache, "--chrom", "chrT", "--bedpe", bedpe, "--res", str(LC.P_RES), "--window", "3", "--max-distance",
               str(LC.P_D * LC.P_RES), "--host", "--out", out])
    want, _ = PC.planted_scores(2)
    z = np.load(out + ".npz")
    assert PC.same_bits(z["sum"], want.sum) and np.array_equal(z["count"], want.count) and z["kept"].tolist() == [6]
    assert PC.same_bits(z["P2LL"], want.scores()["P2LL"]) and int(z["w"]) == 3 and str(z["value"]) == "oe"
    text = np.loadtxt(out + ".group0.txt")
    assert text.shape == (7, 7) and np.allclose(text, want.mean[0], rtol=1e-9, equal_nan=True)
    assert "group 0: 6 centres" in capsys.readouterr().out
    # --call-loops: the loops of the restatement are the centres
    out2 = str(tmp_path / "loops.apa")
    tool.main([cache, "--chrom", "chrT", "--call-loops", "--peak", "1", "--loop-window", "3", "--res", str(LC.P_RES), "--window", "3", "--max-distance",
               str(LC.P_D * LC.P_RES), "--host", "--out", out2])
    found = loops.loops_host(c["pos1"], c["pos2"], c["count"], "VC", LC.P_RES, "auto", **LC.P_RULE)
    assert np.load(out2 + ".npz")["kept"].tolist() == [len(found)]
    with pytest.raises(SystemExit):
        tool.main([cache, "--chrom", "chrT", "--host", "--out", out])        # no centre source
    with pytest.raises(SystemExit):
        tool.main([cache, "--chrom", "chrT", "--bedpe", bedpe, "--call-loops", "--host", "--out", out])


def test_train_arguments(capsys):
    from chromegcn_amd import train
    opt = train.parse(["-feat_dir", "f", "-hic_contacts", "caches"])
    assert (opt.hic_apa, opt.hic_apa_res) == (0, 10000)
    opt = train.parse(["-feat_dir", "f", "-hic_contacts", "caches", "-hic_apa", "5", "-hic_apa_res", "25000"])
    assert (opt.hic_apa, opt.hic_apa_res) == (5, 25000)
    for bad in (["-hic_apa", "5"], ["-hic_contacts", "c", "-hic_apa", "11"], ["-hic_contacts", "c", "-hic_apa", "-1"],
                ["-hic_contacts", "c", "-hic_apa", "5", "-hic_apa_res", "0"]):
        with pytest.raises(SystemExit):
            train.parse(["-feat_dir", "f"] + bad)
    capsys.readouterr()
    plants, control = PC.planted_scores(0)
    train.report_apa("train", {"chrT": {"edges": plants, "control": control}})
    lines = capsys.readouterr().out.splitlines()
    assert len(lines) == 2 and lines[0].startswith("[hic_apa] train chrT edges: 6 centres kept (0 skipped), P2LL ")


def test_entry_point_argument_checks():
    from chromegcn_amd import _build, _lib
    _build.build_library()
    _lib.load()
    q = 0x10000   # never read: every call below returns before a launch

    def rc(fn, ok, **kw):
        return _lib.query(fn, **{**ok, **kw})
    val = dict(stream=None, n=10, width=27, band=q, vc=q, norm=None, n_norm=0, expected=q, n_expected=10, kind=2, vband=q)
    for ptr in ("band", "vc", "vband"):
        assert rc("cgcn_pileup_values", val, **{ptr: None}) == -1
    assert rc("cgcn_pileup_values", val, expected=None) == -1 and rc("cgcn_pileup_values", val, kind=3) == -1
    assert rc("cgcn_pileup_values", val, kind=-1) == -1 and rc("cgcn_pileup_values", val, width=0) == -1
    assert rc("cgcn_pileup_values", val, norm=q, n_norm=0) == -1 and rc("cgcn_pileup_values", val, n=-1) == -1
    assert rc("cgcn_pileup_values", val, n=2 ** 21, width=129) == -2
    assert rc("cgcn_pileup_values", val, n=0, band=None, vc=None, vband=None) == 0
    wsp = _lib.query("cgcn_pileup_workspace_bytes", n_slices=5, w=3)
    assert wsp >= 5 * 49 * 12 and _lib.query("cgcn_pileup_workspace_bytes", n_slices=5, w=11) == 0
    assert _lib.query("cgcn_pileup_workspace_bytes", n_slices=-1, w=3) == 0 and _lib.query("cgcn_pileup_workspace_bytes", n_slices=0, w=3) > 0
    sl = dict(stream=None, n=64, width=40, vband=q, w=3, n_slices=5, slice_off=q, n_centres=1200, ci=q, cj=q, workspace=q,
              workspace_bytes=wsp)
    for ptr in ("vband", "slice_off", "ci", "cj", "workspace"):
        assert rc("cgcn_pileup_slices", sl, **{ptr: None}) == -1
    assert rc("cgcn_pileup_slices", sl, w=11) == -2 and rc("cgcn_pileup_slices", sl, w=0) == -1
    assert rc("cgcn_pileup_slices", sl, n=2 ** 21, width=129) == -2 and rc("cgcn_pileup_slices", sl, workspace_bytes=wsp - 1) == -4
    assert rc("cgcn_pileup_slices", sl, n_slices=-1) == -1 and rc("cgcn_pileup_slices", sl, n_centres=-1) == -1
    empty = _lib.query("cgcn_pileup_workspace_bytes", n_slices=0, w=3)
    assert rc("cgcn_pileup_slices", sl, n_slices=0, n_centres=0, slice_off=None, ci=None, cj=None, vband=None, workspace_bytes=empty) == 0
    fo = dict(stream=None, n_groups=3, w=3, n_slices=5, group_off=q, workspace=q, workspace_bytes=wsp, P=q, N=q)
    for ptr in ("group_off", "workspace", "P", "N"):
        assert rc("cgcn_pileup_fold", fo, **{ptr: None}) == -1
    assert rc("cgcn_pileup_fold", fo, n_groups=65537) == -2 and rc("cgcn_pileup_fold", fo, w=11) == -2
    assert rc("cgcn_pileup_fold", fo, workspace_bytes=wsp - 1) == -4 and rc("cgcn_pileup_fold", fo, n_groups=-1) == -1
    assert rc("cgcn_pileup_fold", fo, n_groups=0, group_off=None, P=None, N=None) == 0
    with pytest.raises(RuntimeError, match=r"cgcn_pileup_slices failed: unsupported.*\(code -2\)"):
        _lib.call("cgcn_pileup_slices", **{**sl, "w": 11})
