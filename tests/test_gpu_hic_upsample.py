"""Contact graphs from records coarser than the windows, built on the device (cgcn_hic_count_up / cgcn_hic_build_up,
csrc/cgcn_hic.hip) against (a) the numpy restatement build_hic_graph_host(window_bp=...), which
tests/test_hic_upsample_host.py ties to the reference's step 7, and (b) the device path for records at the windows' own
resolution, run on the expanded file written out (expand_contacts_host).  Every comparison is exact: rowptr, col[:nnz], nnz
and the survivor count S."""
import math

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from chromegcn_amd import ChromeGCN, _lib, graph as G, hic, synth

from test_hic_upsample_host import random_cases, upsample_cases

pytestmark = pytest.mark.gpu
DEV = "cuda"
BAD_ARG, UNSUPPORTED, WORKSPACE = -1, -2, -4


def device_csr(args, contacts=None):
    """(rowptr, col[:nnz], nnz, S) of the device build for the arguments of build_hic_graph_host"""
    c = contacts if contacts is not None else hic.HicContacts(args["pos1"], args["pos2"], args["count"], DEV)
    rowptr, col, sizes = c.build_raw(args["norm"], args["resolution_bp"], args["window_start"], args["hic_edges"],
                                     window_bp=args.get("window_bp"))
    nnz, s = sizes.tolist()
    assert col.numel() >= nnz
    return rowptr.cpu().numpy(), col[:nnz].cpu().numpy(), nnz, s


def assert_is_host_build(got, args, what):
    a = hic.build_hic_graph_host(**args)
    s = hic.survivor_values(**{k: v for k, v in args.items() if k != "hic_edges"})[3].size
    rowptr, col, nnz, surv = got
    assert (nnz, surv) == (a.nnz, s), what
    assert np.array_equal(rowptr, a.indptr) and np.array_equal(col, a.indices), what
    return a


@pytest.mark.timeout(600)
def test_golden_and_random_cases_equal_the_host_restatement(golden):
    for c, args, adj, flags in upsample_cases(golden):
        a = assert_is_host_build(device_csr(args), args, ("g9", c))
        assert np.array_equal(np.asarray(a.todense()), adj.astype(np.float64)), c
    routes = set()
    for c, args in random_cases():                    # up in 1, 2, 5, 8; windows on the window_bp grid and off it
        assert_is_host_build(device_csr(args), args, ("random", c))
        routes.add((c[0], c[1]))
    assert len(routes) == 8


def _coarse(chrom):
    """chr21: M = 2 489 062 records of 5 kb (62.2 M expanded, 1.0 GB); chr1, at a lower density so that its expanded file
    fits as comfortably: M = 2 345 609 (58.6 M expanded, 0.94 GB)"""
    kw = dict(background_per_bin=8.0, peak_pairs_per_window=30.0) if chrom == "chr1" else {}
    r = synth.raw_contacts_coarse(chrom, **kw)
    assert r["pos1"].size == {"chr21": 2489062, "chr1": 2345609}[chrom]
    return r


def _args(r, norm, edges, up=True):
    a = dict(pos1=r["pos1"], pos2=r["pos2"], count=r["count"], norm=r["norm"] if norm else None,
             resolution_bp=r["resolution_bp"], window_start=r["window_start"], hic_edges=edges)
    return dict(a, window_bp=r["window_bp"]) if up else a


@pytest.mark.timeout(1500)
@pytest.mark.parametrize("chrom", ["chr21", "chr1"])
def test_full_size_equals_the_merged_device_path_on_the_expanded_file(chrom):
    r = _coarse(chrom)
    compact = hic.HicContacts(r["pos1"], r["pos2"], r["count"], DEV)
    e1, e2, ec = hic.expand_contacts_host(r["pos1"], r["pos2"], r["count"], r["resolution_bp"], r["window_bp"])
    written_out = hic.HicContacts(e1, e2, ec, DEV)
    del e1, e2, ec
    s = compact.survivors(r["window_start"], r["resolution_bp"], r["window_bp"])
    assert s == written_out.survivors(r["window_start"]) > 500000
    host_checked = False
    for norm in (False, True):
        for edges in (250000, 500000, 1000000):
            got = device_csr(_args(r, norm, edges), compact)
            want = device_csr(_args(r, norm, edges, up=False), written_out)
            assert got[2:] == want[2:] and got[3] == s, (chrom, norm, edges)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (chrom, norm, edges)
            assert got[2] > 0
            if chrom == "chr21" and norm and edges == 500000:      # and once against the host restatement at this size
                assert_is_host_build(got, _args(r, norm, edges), (chrom, norm, edges))
                host_checked = True
    assert host_checked == (chrom == "chr21")


def _records_2kb(target, seed=5, n_bins=124626):
    """more than `target` records on chr1's 2 kb grid, made as synth.raw_contacts makes its background (the truncated 1/k law
    of distances, each ordered pair once, sorted by (pos1, pos2), the diagonal present, counts that fall with distance, a norm
    vector with NaN and zeros), and 50 000 windows of 1 kb"""
    rng = np.random.RandomState(seed)
    k = int(1.12 * target)
    dist = np.clip(np.floor(np.exp(rng.random_sample(k) * math.log(n_bins - 1))).astype(np.int64) - 1, 0, n_bins - 1)
    a = (rng.random_sample(k) * (n_bins - dist)).astype(np.int64)
    key = np.unique(a * n_bins + a + dist)
    bin1, bin2 = key // n_bins, key % n_bins
    count = 1.0 + rng.poisson(40.0 / (1.0 + (bin2 - bin1)) ** 0.8)
    norm = 0.5 + rng.random_sample(n_bins)
    norm[rng.random_sample(n_bins) < 0.02] = np.nan
    norm[rng.random_sample(n_bins) < 0.01] = 0.0
    ws = np.sort(rng.choice(2 * n_bins, 50000, replace=False)).astype(np.int32) * 1000
    return {"pos1": (bin1 * 2000).astype(np.int32), "pos2": (bin2 * 2000).astype(np.int32), "count": count.astype(np.float64),
            "norm": norm, "window_start": ws, "resolution_bp": 2000, "window_bp": 1000}


@pytest.mark.timeout(600)
def test_more_records_than_one_sweep_of_the_persistent_filter():
    """k_hic_filter_up's waves stride over the 512-record wave tiles: a grid of 2 x CUs workgroups of 16 waves visits
    2 x CUs x 16 tiles in its first trip, so records from 2 x CUs x 16 x 512 on are read in the second one (about 4.4 M
    records of 2 kb for 1 kb windows, up = 2, at 256 CUs).  Exactly the host restatement, and exactly the merged device path
    on the expanded file; on the bitmap route (every window on the 1 kb grid) and on the search route (one window off it)."""
    sweep_tiles = 2 * torch.cuda.get_device_properties(torch.device(DEV)).multi_processor_count * 16
    r = _records_2kb(int(1.05 * sweep_tiles * 512))
    M = r["pos1"].size
    tiles = -(-M // 512)
    assert M > sweep_tiles * 512 and tiles - 1 > sweep_tiles, (M, sweep_tiles)
    compact = hic.HicContacts(r["pos1"], r["pos2"], r["count"], DEV)
    written_out = hic.HicContacts(*hic.expand_contacts_host(r["pos1"], r["pos2"], r["count"], 2000, 1000), DEV)
    off_grid = r["window_start"].copy()
    off_grid[1000] += 500
    for ws in (r["window_start"], off_grid):
        # survivors of every record from the positions: (children of pos1 that are windows) x (of pos2), less the pairs (w, w)
        c1 = np.isin(r["pos1"], ws).astype(np.int64) + np.isin(r["pos1"] + 1000, ws)
        c2 = np.isin(r["pos2"], ws).astype(np.int64) + np.isin(r["pos2"] + 1000, ws)
        surv = c1 * c2 - (r["pos1"] == r["pos2"]) * c1
        tile = np.arange(M) // 512
        in_last, in_second_trip = surv[tile == tiles - 1].sum(), surv[(tile >= sweep_tiles) & (tile < tiles - 1)].sum()
        print("M %d, %d wave tiles, %d in a sweep; survivors: %d, %d of them in the second trip before the last tile, %d in the last"
              % (M, tiles, sweep_tiles, surv.sum(), in_second_trip, in_last))
        assert in_last > 0 and in_second_trip > 1000 and surv[tile < sweep_tiles].sum() > 1000
        for norm in (False, True):
            args = dict(_args(r, norm, 500000), window_start=ws)
            got = device_csr(args, compact)
            assert got[3] == surv.sum() and got[2] > 400000
            assert_is_host_build(got, args, ("beyond one sweep", ws is off_grid, norm))
            want = device_csr({k: v for k, v in args.items() if k != "window_bp"}, written_out)
            assert got[2:] == want[2:] and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (ws is off_grid, norm)


def _buffers(n, K, fill=-7):
    return (torch.full((n + 1,), fill, dtype=torch.int32, device=DEV), torch.full((2 * K + 64,), fill, dtype=torch.int32, device=DEV),
            torch.full((2,), fill, dtype=torch.int64, device=DEV))


@pytest.mark.timeout(600)
def test_up_1_through_the_new_entry_points_is_byte_identical():
    r = synth.raw_contacts("chr21", background_per_bin=8.0, peak_pairs_per_window=30.0)
    c = hic.HicContacts(r["pos1"], r["pos2"], r["count"], DEV)
    ws = torch.from_numpy(r["window_start"]).to(DEV)
    norm = torch.from_numpy(r["norm"]).to(DEV)
    n, bins = int(ws.numel()), int(r["window_start"][-1]) // 1000 + 1
    cnt = torch.zeros(2, dtype=torch.int64, device=DEV)
    need = _lib.query("cgcn_hic_workspace_bytes", M=c.M, N=n, capacity=0, K=0)
    _lib.call("cgcn_hic_count", M=c.M, pos1=c.pos1, pos2=c.pos2, window_start=ws, N=n, workspace=torch.empty(need, dtype=torch.uint8, device=DEV),
              workspace_bytes=need, n_survivors=cnt.data_ptr())
    need = _lib.query("cgcn_hic_up_workspace_bytes", M=c.M, N=n, capacity=0, K=0, resolution_bp=1000, window_bp=1000, n_window_bins=bins)
    _lib.call("cgcn_hic_count_up", M=c.M, pos1=c.pos1, pos2=c.pos2, window_start=ws, N=n, resolution_bp=1000, window_bp=1000,
              n_window_bins=bins, workspace=torch.empty(need, dtype=torch.uint8, device=DEV), workspace_bytes=need,
              n_survivors=cnt.data_ptr() + 8)
    s, s_up = cnt.tolist()
    assert s == s_up > 60000
    for nv in (None, norm):
        for K, cap in ((30000, s), (2 * s, s), (30000, s + 1000), (1000, s // 2)):
            shared = dict(M=c.M, pos1=c.pos1, pos2=c.pos2, count=c.count, norm=nv, n_bins=0 if nv is None else int(nv.numel()),
                          resolution_bp=1000, window_start=ws, N=n, K=K, capacity=cap)
            old, new = _buffers(n, K), _buffers(n, K)
            need = _lib.query("cgcn_hic_workspace_bytes", M=c.M, N=n, capacity=cap, K=K)
            _lib.call("cgcn_hic_build", workspace=torch.empty(need, dtype=torch.uint8, device=DEV), workspace_bytes=need,
                      rowptr_out=old[0], col_out=old[1], nnz_out=old[2].data_ptr(), n_survivors=old[2].data_ptr() + 8, **shared)
            need = _lib.query("cgcn_hic_up_workspace_bytes", M=c.M, N=n, capacity=cap, K=K, resolution_bp=1000, window_bp=1000,
                              n_window_bins=bins)
            _lib.call("cgcn_hic_build_up", workspace=torch.empty(need, dtype=torch.uint8, device=DEV), workspace_bytes=need,
                      window_bp=1000, n_window_bins=bins, rowptr_out=new[0], col_out=new[1], nnz_out=new[2].data_ptr(),
                      n_survivors=new[2].data_ptr() + 8, **shared)
            for a, b in zip(old, new):
                assert torch.equal(a, b), (nv is not None, K, cap)
            assert int(new[2][1]) == s and int(new[2][0] & 0xFFFFFFFF) > 0


@pytest.mark.timeout(600)
def test_builds_repeat_bitwise_and_a_sweep_counts_once_per_window_set_and_window_bp(monkeypatch):
    r = synth.raw_contacts_coarse("chr21", background_per_bin=8.0, peak_pairs_per_window=30.0)
    ws, other = r["window_start"], r["window_start"][::2].copy()
    calls, real = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda fn, **kw: (calls.append(fn), real(fn, **kw))[1])
    syncs, tolist, item = [], torch.Tensor.tolist, torch.Tensor.item
    monkeypatch.setattr(torch.Tensor, "tolist", lambda t: (syncs.append(1), tolist(t))[1])
    monkeypatch.setattr(torch.Tensor, "item", lambda t: (syncs.append(1), item(t))[1])
    c = hic.HicContacts(r["pos1"], r["pos2"], r["count"], DEV)
    uploaded = (c.pos1.data_ptr(), c.pos2.data_ptr(), c.count.data_ptr())
    before = c.build_raw(r["norm"], 5000, ws, 100000)                   # the default path on the 5 kb records, first
    assert calls == ["cgcn_hic_count", "cgcn_hic_build"] and len(syncs) == 1
    del calls[:], syncs[:]
    out = {}
    for w in (ws, other):
        for wbp in (1000, 2500):
            for norm in (None, r["norm"]):
                for edges in (100000, 250000, 2 * 10 ** 6):
                    out[(w.size, wbp, norm is None, edges)] = c.build_raw(norm, 5000, w, edges, window_bp=wbp)
    # (ws, 1000), (ws, 2500), (other, 1000), (other, 2500): one count and one read-back each, whatever the budget and the vector
    assert calls.count("cgcn_hic_count_up") == 4 and len(syncs) == 4
    assert calls.count("cgcn_hic_build_up") == 24 and "cgcn_hic_build" not in calls and "cgcn_hic_count" not in calls
    assert (c.pos1.data_ptr(), c.pos2.data_ptr(), c.count.data_ptr()) == uploaded
    monkeypatch.undo()
    fresh = hic.HicContacts(r["pos1"], r["pos2"], r["count"], DEV)
    for (n, wbp, plain, edges), (rowptr, col, sizes) in out.items():
        w = ws if n == ws.size else other
        again = fresh.build_raw(None if plain else r["norm"], 5000, w, edges, window_bp=wbp)
        nnz = int(sizes[0])
        assert torch.equal(again[2], sizes) and torch.equal(again[0], rowptr) and torch.equal(again[1][:nnz], col[:nnz])
        assert nnz > 0
    after = c.build_raw(r["norm"], 5000, ws, 100000)                    # the default path again, after the upsampled builds
    assert torch.equal(after[2], before[2]) and torch.equal(after[0], before[0])
    assert torch.equal(after[1][:int(before[2][0])], before[1][:int(before[2][0])])
    assert int(before[2][1]) < int(out[(ws.size, 1000, True, 100000)][2][1])      # fewer survivors without the expansion


def _first_survivors_graph(args, cap):
    """the rule on the first `cap` survivors of the expanded file"""
    _, i, j, v = hic.survivor_values(**{k: v for k, v in args.items() if k != "hic_edges"})
    i, j, v = i[:cap], j[:cap], v[:cap]
    take = np.argsort(-v, kind="stable")[:args["hic_edges"] // 2]
    n = args["window_start"].size
    a = sp.coo_matrix((np.ones(2 * take.size), (np.concatenate([i[take], j[take]]), np.concatenate([j[take], i[take]]))),
                      shape=(n, n)).tocsr()
    a.sum_duplicates()
    a.sort_indices()
    return a


@pytest.mark.timeout(600)
def test_a_capacity_below_the_survivor_count_is_reported_and_nothing_is_overrun():
    r = synth.raw_contacts_coarse("chr21", background_per_bin=2.0, peak_pairs_per_window=10.0)
    c = hic.HicContacts(r["pos1"], r["pos2"], r["count"], DEV)
    s = c.survivors(r["window_start"], 5000, 1000)
    ws, norm = c._ws_dev, torch.from_numpy(r["norm"]).to(DEV)
    n, bins = int(ws.numel()), int(r["window_start"][-1]) // 1000 + 1
    for cap, K in ((s // 2 + 3, 10 ** 6), (s // 3, 5000), (7, 100)):      # 7: the cut falls inside the first records' blocks
        need = _lib.query("cgcn_hic_up_workspace_bytes", M=c.M, N=n, capacity=cap, K=K, resolution_bp=5000, window_bp=1000,
                          n_window_bins=bins)
        wsp = torch.empty(need + 4096, dtype=torch.uint8, device=DEV)
        wsp[need:] = 0x5A
        width = 2 * min(K, cap)
        rowptr = torch.full((n + 1,), -7, dtype=torch.int32, device=DEV)
        col = torch.full((width + 1024,), -7, dtype=torch.int32, device=DEV)       # guard words behind col_out
        sizes = torch.full((2,), -7, dtype=torch.int64, device=DEV)
        _lib.call("cgcn_hic_build_up", M=c.M, pos1=c.pos1, pos2=c.pos2, count=c.count, norm=norm, n_bins=int(norm.numel()),
                  resolution_bp=5000, window_bp=1000, n_window_bins=bins, window_start=ws, N=n, K=K, capacity=cap, workspace=wsp,
                  workspace_bytes=need, rowptr_out=rowptr, col_out=col, nnz_out=sizes.data_ptr(), n_survivors=sizes.data_ptr() + 8)
        torch.cuda.synchronize()
        assert int(sizes[1]) == s > cap and bool((wsp[need:] == 0x5A).all()) and bool((col[width:] == -7).all())
        a = _first_survivors_graph(_args(r, True, 2 * K), cap)
        nnz = int(sizes[0] & 0xFFFFFFFF)
        assert nnz == a.nnz > 0
        assert np.array_equal(rowptr.cpu().numpy(), a.indptr) and np.array_equal(col[:nnz].cpu().numpy(), a.indices)


@pytest.mark.timeout(300)
def test_error_codes_and_nothing_is_launched_on_a_rejected_call():
    r = synth.raw_contacts_coarse("chr21", background_per_bin=1.0, peak_pairs_per_window=5.0)
    c = hic.HicContacts(r["pos1"], r["pos2"], r["count"], DEV)
    cap = c.survivors(r["window_start"], 5000, 1000)
    ws, norm = c._ws_dev, torch.from_numpy(r["norm"]).to(DEV)
    n, bins, K = int(ws.numel()), int(r["window_start"][-1]) // 1000 + 1, 1000
    q = dict(M=c.M, N=n, capacity=cap, K=K, resolution_bp=5000, window_bp=1000, n_window_bins=bins)
    need = _lib.query("cgcn_hic_up_workspace_bytes", **q)
    assert need > _lib.query("cgcn_hic_workspace_bytes", M=c.M, N=n, capacity=cap, K=K) > 0
    wsp = torch.empty(need, dtype=torch.uint8, device=DEV)
    rowptr, col, sizes = _buffers(n, K)
    good = dict(M=c.M, pos1=c.pos1, pos2=c.pos2, count=c.count, norm=norm, n_bins=int(norm.numel()), resolution_bp=5000,
                window_bp=1000, n_window_bins=bins, window_start=ws, N=n, K=K, capacity=cap, workspace=wsp, workspace_bytes=need,
                rowptr_out=rowptr, col_out=col, nnz_out=sizes.data_ptr(), n_survivors=sizes.data_ptr() + 8)
    build_cases = ((dict(M=-1), BAD_ARG), (dict(N=-1), BAD_ARG), (dict(K=-1), BAD_ARG), (dict(pos1=None), BAD_ARG),
                   (dict(count=None), BAD_ARG), (dict(window_start=None), BAD_ARG), (dict(rowptr_out=None), BAD_ARG),
                   (dict(col_out=None), BAD_ARG), (dict(nnz_out=None), BAD_ARG), (dict(workspace=None), BAD_ARG),
                   (dict(resolution_bp=0), BAD_ARG), (dict(window_bp=0), BAD_ARG), (dict(window_bp=-1000), BAD_ARG),
                   (dict(window_bp=1500), BAD_ARG), (dict(n_window_bins=-1), BAD_ARG), (dict(K=2 ** 30), UNSUPPORTED),
                   (dict(capacity=2 ** 31), UNSUPPORTED), (dict(resolution_bp=9000), UNSUPPORTED),
                   (dict(M=2 ** 31 // 25 + 1), UNSUPPORTED), (dict(workspace_bytes=need - 1), WORKSPACE))
    for over, code in build_cases:
        assert _lib.query("cgcn_hic_build_up", **dict(good, **over)) == code, over
    count = {k: good[k] for k in ("M", "pos1", "pos2", "window_start", "N", "resolution_bp", "window_bp", "n_window_bins", "workspace")}
    need0 = _lib.query("cgcn_hic_up_workspace_bytes", **dict(q, capacity=0, K=0))
    count.update(workspace_bytes=need0, n_survivors=sizes.data_ptr() + 8)
    for over, code in ((dict(M=-1), BAD_ARG), (dict(pos2=None), BAD_ARG), (dict(window_start=None), BAD_ARG),
                       (dict(n_survivors=None), BAD_ARG), (dict(window_bp=0), BAD_ARG), (dict(window_bp=1500), BAD_ARG),
                       (dict(resolution_bp=9000), UNSUPPORTED), (dict(M=2 ** 31 // 25 + 1), UNSUPPORTED),
                       (dict(workspace_bytes=need0 - 1), WORKSPACE)):
        assert _lib.query("cgcn_hic_count_up", **dict(count, **over)) == code, over
    for over in (dict(window_bp=1500), dict(window_bp=0), dict(resolution_bp=9000), dict(M=2 ** 31 // 25 + 1), dict(K=2 ** 30),
                 dict(capacity=2 ** 31), dict(M=-1)):
        assert _lib.query("cgcn_hic_up_workspace_bytes", **dict(q, **over)) == 0, over
    with pytest.raises(RuntimeError, match=r"chromegcn_amd: cgcn_hic_build_up failed: bad argument.*\(code -1\)"):
        _lib.call("cgcn_hic_build_up", **dict(good, window_bp=1500))
    torch.cuda.synchronize()
    assert bool((rowptr == -7).all()) and bool((col == -7).all()) and bool((sizes == -7).all())     # nothing was launched
    # python-side checks
    with pytest.raises(ValueError, match="does not divide"):
        c.build(None, 5000, r["window_start"], 1000, window_bp=1500)
    with pytest.raises(ValueError, match="more than 8"):
        c.build(None, 9000, r["window_start"], 1000, window_bp=1000)
    with pytest.raises(ValueError, match="no multiple of resolution_bp"):
        c.build(None, 10000, r["window_start"], 1000, window_bp=2000)       # 5 kb positions are not on a 10 kb grid
    # a window set beyond the LDS tables (n_window_bins > 262 112): the same graph through the tables in global memory
    far = dict(_args(r, False, 50000), window_start=np.concatenate([r["window_start"], [400000000]]).astype(np.int32))
    assert_is_host_build(device_csr(far, hic.HicContacts(r["pos1"], r["pos2"], r["count"], DEV)), far, "tables in global memory")


@pytest.mark.timeout(600)
def test_one_eval_forward_on_the_device_built_graph_equals_the_host_built_one():
    r = synth.raw_contacts_coarse("chr21", background_per_bin=8.0, peak_pairs_per_window=30.0)
    n, d, C = r["window_start"].size, 128, 12
    args = _args(r, True, 60000)
    a = hic.build_hic_graph_host(**args)
    assert a.nnz > 50000
    rowptr, col, sizes = hic.HicContacts(r["pos1"], r["pos2"], r["count"], DEV).build_raw(r["norm"], 5000, r["window_start"], 60000,
                                                                                         window_bp=1000)
    g_dev = G.normalize_device_csr("hic", n, rowptr, col, None, DEV)
    also = hic.build_hic_graph(r["pos1"], r["pos2"], r["count"], r["norm"], 5000, r["window_start"], 60000, device=DEV, window_bp=1000)
    g_host = G.process_graph("hic", {"chrT": a}, n, "chrT", DEV)
    x = synth.chrom_features(n, d, C, 77)["forward"].to(DEV)
    torch.manual_seed(5)
    model = ChromeGCN(d, d, C, 0.2, True, 2).to(DEV).eval()
    with torch.no_grad():
        outs = [model(x, g) for g in (g_dev, also, g_host)]
    outs = [o[0] if isinstance(o, (tuple, list)) else o for o in outs]
    torch.cuda.synchronize()
    assert torch.equal(g_dev.rowptr, g_host.rowptr) and torch.equal(g_dev.col, g_host.col)
    assert torch.equal(outs[0], outs[2]) and torch.equal(outs[1], outs[2]) and bool(torch.isfinite(outs[0]).all())
