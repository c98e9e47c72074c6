"""The top-K Hi-C contact graph, CPU tier: build_hic_graph_host against the matrices the reference's own step 7 wrote
(tests/golden/g8_hic_build.npz, recorded by tests/golden/make_golden_hic.py), the synthetic contact records, the text parser
and the binary cache, the C ABI entries and the command-line flag."""
import os
import re

import numpy as np
import pytest

from chromegcn_amd import _lib, hic, synth, train

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def golden_cases(golden):
    z = golden("g8_hic_build.npz")
    for c in range(int(z["n_cases"])):
        p = "c%d_" % c
        yield c, dict(pos1=z[p + "pos1"], pos2=z[p + "pos2"], count=z[p + "count"],
                      norm=z[p + "norm"] if p + "norm" in z.files else None, resolution_bp=int(z[p + "res"]),
                      window_start=z[p + "ws"], hic_edges=int(z[p + "edges"])), z[p + "adj"], int(z[p + "tie"])


def test_host_build_equals_every_recorded_matrix_of_the_reference(golden):
    seen = {"norm": 0, "plain": 0, "tie": 0, "all": 0, "cut": 0, "n": set()}
    for c, args, adj, tie in golden_cases(golden):
        a = hic.build_hic_graph_host(**args)
        assert a.shape == adj.shape and a.dtype == np.float64, c
        assert np.array_equal(np.asarray(a.todense()), adj.astype(np.float64)), c
        assert a.has_sorted_indices and np.all(a.data == 1.0) and a.diagonal().sum() == 0 and (a != a.T).nnz == 0, c
        s = hic.survivor_values(**{k: v for k, v in args.items() if k != "hic_edges"})[3].size
        seen["norm" if args["norm"] is not None else "plain"] += 1
        seen["tie"] += tie
        seen["all" if args["hic_edges"] // 2 >= s else "cut"] += 1
        seen["n"].add(adj.shape[0])
    assert seen["n"] == {1, 7, 257} and min(seen["norm"], seen["plain"], seen["tie"], seen["all"], seen["cut"]) >= 4, seen


def test_golden_inputs_hold_the_cases_the_rule_names(golden):
    both = diag = off = bad_norm = 0
    for c, args, adj, tie in golden_cases(golden):
        p1, p2, ws = args["pos1"].astype(np.int64), args["pos2"].astype(np.int64), args["window_start"]
        pairs = set(zip(p1.tolist(), p2.tolist()))
        assert len(pairs) == p1.size                                     # no ordered pair twice (outside the contract)
        both += any((b, a) in pairs for a, b in pairs if a != b)        # records in both orientations
        diag += bool(np.any(p1 == p2))
        off += bool(np.any(~np.isin(p1, ws)))
        if args["norm"] is not None:
            bad_norm += bool(np.isnan(args["norm"]).any() and (args["norm"] == 0).any())
    assert both >= 20 and diag >= 20 and off >= 20 and bad_norm >= 10


def test_header_table_and_version_agree():
    src = open(os.path.join(ROOT, "include", "chromegcn.h")).read()
    assert re.search(r"#define CGCN_ABI_VERSION 26\b", src) and _lib.ABI_VERSION == 26
    for fn in ("cgcn_hic_workspace_bytes", "cgcn_hic_count", "cgcn_hic_build"):
        assert re.search(r"\b%s\s*\(" % fn, src) and fn in _lib._ABI, fn
    names = [p for p, _ in _lib._ABI["cgcn_hic_build"][1]]
    assert names[:6] == ["stream", "M", "pos1", "pos2", "count", "norm"] and names[-4:] == ["rowptr_out", "col_out", "nnz_out",
                                                                                             "n_survivors"]
    lib = _lib.load()
    assert lib.cgcn_abi_version() == 26
    assert _lib.query("cgcn_hic_workspace_bytes", M=10 ** 6, N=5000, capacity=20000, K=250000) > 0
    assert _lib.query("cgcn_hic_workspace_bytes", M=10 ** 6, N=5000, capacity=20000, K=2 ** 30) == 0     # 2 K >= 2^31
    assert _lib.query("cgcn_hic_workspace_bytes", M=-1, N=5000, capacity=20000, K=10) == 0


@pytest.fixture(scope="module")
def chr21():
    return synth.raw_contacts("chr21")


def test_synthetic_contacts_are_deterministic_sorted_and_make_the_budget_bind(chr21):
    r = chr21
    again = synth.raw_contacts("chr21")
    for k in ("pos1", "pos2", "count", "norm", "window_start"):
        assert np.array_equal(r[k], again[k], equal_nan=True), k
    assert r["pos1"].dtype == r["pos2"].dtype == r["window_start"].dtype == np.int32 and r["count"].dtype == np.float64
    n_bins = -(-synth.HG19_LEN["chr21"] // 1000)
    assert r["norm"].shape == (n_bins,) and np.isnan(r["norm"]).any() and (r["norm"] == 0).any()
    assert r["window_start"].shape == (synth.chrom_nodes("chr21"),) and np.all(np.diff(r["window_start"]) > 0)
    key = r["pos1"].astype(np.int64) * 2 ** 32 + r["pos2"]
    assert np.all(np.diff(key) > 0)                                   # sorted by (pos1, pos2), no ordered pair twice
    assert np.all(r["pos1"] <= r["pos2"]) and np.any(r["pos1"] == r["pos2"])
    assert np.all(r["count"] == np.round(r["count"])) and r["count"].min() >= 1
    near, far = (r["pos2"] - r["pos1"]) < 10000, (r["pos2"] - r["pos1"]) > 1000000
    assert r["count"][near].mean() > 2 * r["count"][far].mean()       # counts fall with distance
    K = 500000 // 2
    _, _, _, v = hic.survivor_values(r["pos1"], r["pos2"], r["count"], None, 1000, r["window_start"])
    assert v.size > K                                                 # the budget binds ...
    t = np.sort(v)[::-1][K - 1]
    at, above = int((v == t).sum()), int((v > t).sum())
    assert at > K - above > 0                                         # ... and the tie rule decides who is taken
    _, _, _, vn = hic.survivor_values(r["pos1"], r["pos2"], r["count"], r["norm"], 1000, r["window_start"])
    assert vn.size == v.size and (vn == 0).any()                      # NaN / 0 norm entries: value 0, still competing


def test_host_build_takes_tied_values_in_file_order():
    ws = np.arange(6, dtype=np.int32) * 1000
    pos1 = np.array([0, 1000, 2000, 3000, 4000, 0], np.int32)
    pos2 = np.array([1000, 2000, 3000, 4000, 5000, 5000], np.int32)
    count = np.array([2., 3., 2., 2., 3., 2.])
    a = hic.build_hic_graph_host(pos1, pos2, count, None, 1000, ws, 8)      # K = 4: both 3s, then the FIRST two 2s
    want = np.zeros((6, 6))
    for i, j in ((1, 2), (4, 5), (0, 1), (2, 3)):
        want[i, j] = want[j, i] = 1
    assert np.array_equal(np.asarray(a.todense()), want)
    with pytest.raises(ValueError, match="strictly increasing"):
        hic.build_hic_graph_host(pos1, pos2, count, None, 1000, ws[::-1], 8)
    with pytest.raises(ValueError, match="bins"):
        hic.build_hic_graph_host(pos1, pos2, count, np.ones(3), 1000, ws, 8)


def test_text_files_and_the_cache_round_trip(tmp_path):
    rng = np.random.RandomState(3)
    m, n_bins = 500, 90
    pos1, pos2 = (rng.randint(0, n_bins, m) * 1000).astype(np.int32), (rng.randint(0, n_bins, m) * 1000).astype(np.int32)
    count = (1 + rng.poisson(3.0, m)).astype(np.float64) + (rng.random_sample(m) < 0.2) * 0.5
    norm = 0.5 + rng.random_sample(n_bins)
    norm[[3, 40]] = np.nan
    norm[[7]] = 0.0
    ws = (np.sort(rng.choice(n_bins, 30, replace=False)) * 1000).astype(np.int32)
    raw, kr = tmp_path / "chrT_1kb.RAWobserved", tmp_path / "chrT_1kb.KRnorm"
    raw.write_text("".join("%d\t%d\t%s\n" % (a, b, repr(float(c))) for a, b, c in zip(pos1, pos2, count)))
    kr.write_text("".join("NaN\n" if np.isnan(x) else "%s\n" % repr(float(x)) for x in norm))
    c = hic.load_contacts_text(str(raw), {"KR": str(kr)}, 1000, ws)
    assert np.array_equal(c.pos1, pos1) and np.array_equal(c.pos2, pos2) and np.array_equal(c.count, count)
    assert np.array_equal(c.norms["KR"], norm, equal_nan=True) and c.M == m
    path = str(tmp_path / "chrT.cghic")
    hic.save_contacts_cache(path, c)
    d = hic.load_contacts_cache(path)
    assert np.array_equal(d.pos1, pos1) and np.array_equal(d.pos2, pos2) and np.array_equal(d.count, count)
    assert list(d.norms) == ["KR"] and np.array_equal(d.norms["KR"], norm, equal_nan=True)
    assert d.resolution_bp == 1000 and np.array_equal(d.window_start, ws)
    a = hic.build_hic_graph_host(pos1, pos2, count, norm, 1000, ws, 40)
    b = hic.build_hic_graph_host(d.pos1, d.pos2, d.count, d.norms["KR"], d.resolution_bp, d.window_start, 40)
    assert (a != b).nnz == 0 and a.nnz > 0
    with open(path, "r+b") as f:
        f.truncate(os.path.getsize(path) - 9)
    with pytest.raises(ValueError, match="truncated"):
        hic.load_contacts_cache(path)
    (tmp_path / "junk.cghic").write_bytes(b"not a cache at all")
    with pytest.raises(ValueError, match="not a chromegcn contact cache"):
        hic.load_contacts_cache(str(tmp_path / "junk.cghic"))


def test_train_parses_the_contacts_flag():
    opt = train.parse(["-feat_dir", "f", "-hic_contacts", "caches", "-hicsize", "250000", "-hicnorm", "KR"])
    assert opt.hic_contacts == "caches" and opt.hicsize == "250000" and opt.hicnorm == "KR"
    assert train.parse(["-feat_dir", "f"]).hic_contacts is None


def test_device_entry_points_refuse_the_cpu():
    with pytest.raises(RuntimeError, match="needs a GPU"):
        hic.HicContacts(np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(1), device="cpu")
