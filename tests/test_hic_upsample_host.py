"""Contact graphs from records coarser than the windows, CPU tier: build_hic_graph_host(window_bp=...) against the matrices the
reference's own step 7 wrote for the expanded records (tests/golden/g9_hic_upsample.npz, recorded by
tests/golden/make_golden_hic_upsample.py), against the same function on the expanded file written out
(expand_contacts_host), the unchanged default path, the error cases, the C ABI entries and the command-line flags."""
import os
import re

import numpy as np
import pytest

from chromegcn_amd import _lib, hic, synth, train

from test_hic_host import golden_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG, UNSUPPORTED = -1, -2


def upsample_cases(golden):
    """(case, arguments of build_hic_graph_host with window_bp, recorded matrix, flags) of g9_hic_upsample.npz"""
    z = golden("g9_hic_upsample.npz")
    for c in range(int(z["n_cases"])):
        p = "c%d_" % c
        flags = {"tie": int(z[p + "tie"]), "diag": int(z[p + "diag"]),
                 "inblock": int(z[p + "inblock"]) if p + "inblock" in z.files else 0}
        yield c, dict(pos1=z[p + "pos1"], pos2=z[p + "pos2"], count=z[p + "count"],
                      norm=z[p + "norm"] if p + "norm" in z.files else None, resolution_bp=int(z[p + "res"]),
                      window_start=z[p + "ws"], hic_edges=int(z[p + "edges"]), window_bp=int(z[p + "wbp"])), z[p + "adj"], flags


def random_case(seed, up, on_grid, wbp=200, n=60, n_coarse=40, m=400, with_norm=True):
    """compact records at resolution up * wbp (both orientations, diagonal records, shuffled, each ordered pair once, small
    integer counts) and windows on the wbp grid or off it (arbitrary positions, some of them on the grid all the same)"""
    rng = np.random.RandomState(seed)
    res = up * wbp
    n = min(n, n_coarse * up * 3 // 4)
    if on_grid:
        ws = np.sort(rng.choice(n_coarse * up, n, replace=False)) * wbp
    else:
        ws = np.unique(np.concatenate([rng.choice(n_coarse * up, n // 2, replace=False) * wbp,
                                       rng.choice(n_coarse * res, n // 2, replace=False)]))
    a, b = rng.randint(0, n_coarse, m), rng.randint(0, n_coarse, m)
    a[: m // 8] = b[: m // 8]
    _, first = np.unique(a * n_coarse + b, return_index=True)
    first = first[rng.permutation(first.size)]
    norm = None
    if with_norm:
        norm = 0.5 + rng.random_sample(n_coarse)
        norm[rng.random_sample(n_coarse) < 0.08] = np.nan
        norm[rng.random_sample(n_coarse) < 0.08] = 0.0
    return dict(pos1=(a[first] * res).astype(np.int32), pos2=(b[first] * res).astype(np.int32),
                count=(1 + rng.poisson(2.0, first.size)).astype(np.float64), norm=norm, resolution_bp=res,
                window_start=ws.astype(np.int32), window_bp=wbp)


def random_cases():
    seed = 100
    for up in (1, 2, 5, 8):
        for on_grid in (True, False):
            for with_norm in (False, True):
                seed += 1
                args = random_case(seed, up, on_grid, with_norm=with_norm)
                s = hic.survivor_values(**args)[3].size
                for edges in sorted({2, 2 * (s // 3) + 1, 2 * (s // 2), 2 * s + 10}):
                    yield (up, on_grid, with_norm, edges), dict(args, hic_edges=edges)


def expanded(args):
    """the arguments of the same build on the expanded file written out, without window_bp"""
    e1, e2, ec = hic.expand_contacts_host(args["pos1"], args["pos2"], args["count"], args["resolution_bp"], args["window_bp"])
    out = {k: v for k, v in args.items() if k != "window_bp"}
    return dict(out, pos1=e1, pos2=e2, count=ec)


def same_matrix(a, b):
    return a.shape == b.shape and np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices) and \
        np.array_equal(a.data, b.data)


def test_expand_contacts_host_is_the_loop_of_the_reference():
    e1, e2, ec = hic.expand_contacts_host([5000, 20000], [10000, 20000], [3.0, 7.5], 5000, 1000)
    want = [(p + a, q + b, v) for p, q, v in ((5000, 10000, 3.0), (20000, 20000, 7.5))
            for a in (0, 1000, 2000, 3000, 4000) for b in (0, 1000, 2000, 3000, 4000)]      # data/extras/upsample_hic.py:42-44
    assert list(zip(e1.tolist(), e2.tolist(), ec.tolist())) == want
    assert e1.dtype == e2.dtype == np.int32 and ec.dtype == np.float64
    one = hic.expand_contacts_host([5000], [10000], [3.0], 5000, 5000)
    assert [x.tolist() for x in one] == [[5000], [10000], [3.0]]


def test_host_build_equals_every_recorded_matrix_of_the_reference(golden):
    seen = {"norm": 0, "plain": 0, "tie": 0, "inblock": 0, "diag": 0, "all": 0, "cut": 0, "n": set()}
    for c, args, adj, flags in upsample_cases(golden):
        a = hic.build_hic_graph_host(**args)
        assert a.shape == adj.shape and a.dtype == np.float64, c
        assert np.array_equal(np.asarray(a.todense()), adj.astype(np.float64)), c
        assert a.has_sorted_indices and np.all(a.data == 1.0) and a.diagonal().sum() == 0 and (a != a.T).nnz == 0, c
        s = hic.survivor_values(**{k: v for k, v in args.items() if k != "hic_edges"})[3].size
        seen["norm" if args["norm"] is not None else "plain"] += 1
        for k in ("tie", "inblock", "diag"):
            seen[k] += flags[k]
        seen["all" if args["hic_edges"] // 2 >= s else "cut"] += 1
        seen["n"].add(adj.shape[0])
        assert (args["resolution_bp"], args["window_bp"]) == (5000, 1000)
    assert seen["n"] == {1, 7, 211} and seen["diag"] >= 2, seen
    assert min(seen["norm"], seen["plain"], seen["tie"], seen["inblock"], seen["all"], seen["cut"]) >= 4, seen


def test_golden_inputs_hold_the_cases_the_rule_names(golden):
    both = diag = off = bad_norm = 0
    for c, args, adj, flags in upsample_cases(golden):
        p1, p2 = args["pos1"].astype(np.int64), args["pos2"].astype(np.int64)
        assert not np.any(p1 % 5000) and not np.any(p2 % 5000) and not np.any(args["window_start"] % 1000)
        pairs = set(zip(p1.tolist(), p2.tolist()))
        assert len(pairs) == p1.size
        both += any((b, a) in pairs for a, b in pairs if a != b)
        diag += bool(np.any(p1 == p2))
        off += bool(np.any(~np.isin(p1 // 5000, args["window_start"] // 5000)))
        if args["norm"] is not None:
            bad_norm += bool(np.isnan(args["norm"]).any() and (args["norm"] == 0).any())
    assert both >= 20 and diag >= 20 and off >= 20 and bad_norm >= 10


def test_compact_build_equals_the_build_on_the_expanded_file(golden):
    cases = [("g9", c, args) for c, args, _, _ in upsample_cases(golden)] + [("random",) + x for x in random_cases()]
    ups, grids, cut_in_block = set(), set(), 0
    for kind, c, args in cases:
        want = hic.build_hic_graph_host(**expanded(args))
        got = hic.build_hic_graph_host(**args)
        assert same_matrix(got, want), (kind, c)
        both = {k: v for k, v in args.items() if k != "hic_edges"}
        sv = hic.survivor_values(**both)
        sw = hic.survivor_values(**{k: v for k, v in expanded(both).items()})
        for x, y in zip(sv, sw):
            assert x.dtype == y.dtype and np.array_equal(x, y), (kind, c)      # order included
        if kind == "random":
            ups.add(c[0])
            grids.add(c[1])
            k, v, up = args["hic_edges"] // 2, sv[3], c[0]
            if up > 1 and 0 < k < v.size:
                order = np.argsort(-v, kind="stable")
                cut_in_block += int(sv[0][order[k - 1]] // (up * up) == sv[0][order[k]] // (up * up))
    assert ups == {1, 2, 5, 8} and grids == {True, False} and cut_in_block >= 4


def test_a_diagonal_record_yields_both_orientations_and_each_counts_against_the_budget():
    ws = np.array([5000, 6000, 8000], np.int32)
    args = dict(pos1=np.array([5000], np.int32), pos2=np.array([5000], np.int32), count=np.array([2.0]), norm=None,
                resolution_bp=5000, window_start=ws, window_bp=1000)
    idx, i, j, v = hic.survivor_values(**args)
    assert idx.tolist() == [1, 3, 5, 8, 15, 16] and list(zip(i.tolist(), j.tolist())) == [(0, 1), (0, 2), (1, 0), (1, 2), (2, 0), (2, 1)]
    assert np.all(v == 2.0)
    a = hic.build_hic_graph_host(hic_edges=6, **args)        # K = 3: (0, 1), (0, 2), (1, 0) -- the pair (1, 2) is left out
    assert np.array_equal(np.asarray(a.todense()), np.array([[0, 1, 1], [1, 0, 0], [1, 0, 0]], float))


def test_the_default_path_is_what_it_was(golden):
    for c, args, adj, tie in golden_cases(golden):
        for wbp in (None, args["resolution_bp"]):
            a = hic.build_hic_graph_host(window_bp=wbp, **args)
            assert np.array_equal(np.asarray(a.todense()), adj.astype(np.float64)), (c, wbp)
            both = {k: v for k, v in args.items() if k != "hic_edges"}
            for x, y in zip(hic.survivor_values(window_bp=wbp, **both), hic.survivor_values(**both)):
                assert x.dtype == y.dtype and np.array_equal(x, y), (c, wbp)


def test_error_cases_raise():
    args = random_case(7, 5, True)
    for fn, extra in ((hic.build_hic_graph_host, dict(hic_edges=10)), (hic.survivor_values, {})):
        with pytest.raises(ValueError, match="does not divide"):
            fn(**dict(args, window_bp=300, **extra))
        with pytest.raises(ValueError, match="does not divide"):
            fn(**dict(args, window_bp=0, **extra))
        with pytest.raises(ValueError, match="more than 8"):
            fn(**dict(args, resolution_bp=9000, window_bp=1000, **extra))
        off = args["pos2"].copy()
        off[3] += args["window_bp"]
        with pytest.raises(ValueError, match="no multiple of resolution_bp"):
            fn(**dict(args, pos2=off, **extra))
    with pytest.raises(ValueError, match="does not divide"):
        hic.expand_contacts_host(args["pos1"], args["pos2"], args["count"], 5000, 1500)
    with pytest.raises(ValueError, match="more than 8"):
        hic.expand_contacts_host(args["pos1"], args["pos2"], args["count"], 9000, 1000)
    with pytest.raises(ValueError, match="does not divide"):      # checked before a device is asked for
        hic.build_hic_graph(args["pos1"], args["pos2"], args["count"], None, 1000, args["window_start"], 10, window_bp=300,
                            device="cpu")


def test_header_table_and_workspace_query_agree():
    src = open(os.path.join(ROOT, "include", "chromegcn.h")).read()
    assert re.search(r"#define CGCN_ABI_VERSION 26\b", src) and _lib.ABI_VERSION == 26
    for fn in ("cgcn_hic_up_workspace_bytes", "cgcn_hic_count_up", "cgcn_hic_build_up"):
        assert re.search(r"\b%s\s*\(" % fn, src) and fn in _lib._ABI, fn
    names = [p for p, _ in _lib._ABI["cgcn_hic_build_up"][1]]
    assert names[6:12] == ["n_bins", "resolution_bp", "window_bp", "n_window_bins", "window_start", "N"]
    q = dict(M=10 ** 6, N=5000, capacity=20000, K=250000, resolution_bp=5000, window_bp=1000, n_window_bins=250000)
    base = _lib.query("cgcn_hic_workspace_bytes", M=q["M"], N=q["N"], capacity=q["capacity"], K=q["K"])
    need = _lib.query("cgcn_hic_up_workspace_bytes", **q)
    assert need >= base + 2 * 4 * (250000 // 32) > 0                    # the sibling's buffers and the two tables
    assert _lib.query("cgcn_hic_up_workspace_bytes", **dict(q, n_window_bins=2 ** 31)) > need      # tables beyond the LDS
    for over in (dict(window_bp=1500), dict(window_bp=0), dict(resolution_bp=0), dict(resolution_bp=9000), dict(K=2 ** 30),
                 dict(M=-1), dict(n_window_bins=-1), dict(M=2 ** 31 // 25 + 1), dict(capacity=2 ** 31)):
        assert _lib.query("cgcn_hic_up_workspace_bytes", **dict(q, **over)) == 0, over
    assert _lib.query("cgcn_hic_up_workspace_bytes", **dict(q, M=2 ** 31 // 25)) > 0
    # rejected before anything is launched (no device here): the codes of the header
    n = None
    count = dict(M=10, pos1=8, pos2=8, window_start=8, N=5, resolution_bp=5000, window_bp=1000, n_window_bins=10, workspace=8,
                 workspace_bytes=1 << 30, n_survivors=8, stream=None)
    for over, code in ((dict(window_bp=0), BAD_ARG), (dict(window_bp=1500), BAD_ARG), (dict(resolution_bp=0), BAD_ARG),
                       (dict(n_window_bins=-1), BAD_ARG), (dict(pos2=n), BAD_ARG), (dict(n_survivors=n), BAD_ARG),
                       (dict(resolution_bp=9000), UNSUPPORTED), (dict(M=2 ** 31 // 25 + 1), UNSUPPORTED),
                       (dict(workspace_bytes=16), -4)):
        assert _lib.query("cgcn_hic_count_up", **dict(count, **over)) == code, over


def test_coarse_synthetic_contacts_are_the_fine_ones_binned():
    r = synth.raw_contacts_coarse("chr21", background_per_bin=2.0, peak_pairs_per_window=10.0)
    f = synth.raw_contacts("chr21", background_per_bin=2.0, peak_pairs_per_window=10.0)
    assert (r["resolution_bp"], r["window_bp"]) == (5000, 1000) and np.array_equal(r["window_start"], f["window_start"])
    assert r["pos1"].dtype == r["pos2"].dtype == np.int32 and r["count"].dtype == np.float64
    assert not np.any(r["pos1"] % 5000) and not np.any(r["pos2"] % 5000)
    key = r["pos1"].astype(np.int64) * 2 ** 32 + r["pos2"]
    assert np.all(np.diff(key) > 0) and np.all(r["pos1"] <= r["pos2"]) and np.any(r["pos1"] == r["pos2"])
    assert r["count"].sum() == f["count"].sum() and r["pos1"].size < f["pos1"].size
    assert len(set(zip((f["pos1"] // 5000).tolist(), (f["pos2"] // 5000).tolist()))) == r["pos1"].size
    assert r["norm"].shape == (-(-synth.HG19_LEN["chr21"] // 5000),) and np.isnan(r["norm"]).any() and (r["norm"] == 0).any()
    again = synth.raw_contacts_coarse("chr21", background_per_bin=2.0, peak_pairs_per_window=10.0)
    for k in ("pos1", "pos2", "count", "norm", "window_start"):
        assert np.array_equal(r[k], again[k], equal_nan=True), k
    s = hic.survivor_values(r["pos1"], r["pos2"], r["count"], r["norm"], 5000, r["window_start"], window_bp=1000)[3].size
    assert s > 10000                                                  # the windows are reached through the expansion ...
    assert hic.survivor_values(r["pos1"], r["pos2"], r["count"], r["norm"], 5000, r["window_start"])[3].size < s // 4   # ... only


def test_train_flags_reach_the_build(monkeypatch, tmp_path):
    opt = train.parse(["-feat_dir", "f", "-hic_contacts", "caches", "-hic_upsample", "-window_size", "1000"])
    assert opt.hic_upsample is True and opt.window_size == 1000
    plain = train.parse(["-feat_dir", "f", "-hic_contacts", "caches"])
    assert plain.hic_upsample is False and plain.window_size == 1000
    args = random_case(9, 5, True, wbp=1000)
    coarse = hic.HostContacts(args["pos1"], args["pos2"], args["count"], {"KR": np.nan_to_num(args["norm"], nan=1.0)}, 5000,
                              args["window_start"])
    fine = hic.HostContacts(args["pos1"], args["pos2"], args["count"], {"KR": coarse.norms["KR"]}, 1000, args["window_start"])
    hic.save_contacts_cache(hic.contact_cache_path(str(tmp_path), "chrA"), coarse)
    hic.save_contacts_cache(hic.contact_cache_path(str(tmp_path), "chrB"), fine)
    calls = []

    def stub(pos1, pos2, count, norm, resolution_bp, window_start, hic_edges, **kw):
        calls.append((int(resolution_bp), int(hic_edges), dict(kw)))
        return "graph"

    monkeypatch.setattr(hic, "build_hic_graph", stub)
    out = hic.graphs_from_contact_caches(str(tmp_path), ["chrA", "chrB"], "500", "KR", device="cpu", window_bp=opt.window_size)
    assert out == {"chrA": "graph", "chrB": "graph"}
    assert calls[0][:2] == (5000, 500) and calls[0][2]["window_bp"] == 1000       # the 5 kb cache: expanded
    assert calls[1][0] == 1000 and "window_bp" not in calls[1][2]                  # records at the window size: as before
    del calls[:]
    hic.graphs_from_contact_caches(str(tmp_path), ["chrA"], "500", "KR", device="cpu")      # without the flag
    assert calls[0][0] == 5000 and "window_bp" not in calls[0][2]
