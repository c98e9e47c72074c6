"""Thresholded multi-label counts on the device (chromegcn_amd.thresholds, csrc/cgcn_threshold.hip) against the numpy
restatement that tests/test_thresholds_host.py holds to the reference -- by exact equality (dtype, shape, values) of EVERY
output array of every case.  Every case goes through the C ABI with a workspace of exactly the queried size full of stale
bytes and sentinel-filled guard bands around every output (`device_counts`): every element is written, nothing else is.

The second half of the file walks the launch plans: threshold_plan() picks one of six kernel instances, 1 to 8 waves per team
(workgroups of 320, 384, 448 or 512 threads), the threshold groups of grid.y and a tile from (n, C, T).  threshold_cases.plan
restates that arithmetic, is pinned here to the library for every (C, T), and every case below asserts through it the
property it is there for before it launches -- a retuned plan fails the case instead of moving it onto another path.
Out of scope: the bound of an LDS histogram word, rows * C < 2^26 (65 535 rows of 1 024 labels in ONE workgroup: about 270 GB
of input), and the refusal of n >= 2^47."""
import functools
import time

import numpy as np
import pytest
import torch

import threshold_cases as tc
from chromegcn_amd import _lib, curves, metrics
from chromegcn_amd import thresholds as th

pytestmark = pytest.mark.gpu

GUARD = 512                     # int64 elements on each side of every output
SENTINEL = -7
FIELDS = ("pos", "tp", "pp", "exact", "rows", "tpsum")


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


def _banded(shape):
    total = int(np.prod(shape))
    buf = torch.full((total + 2 * GUARD,), SENTINEL, device="cuda", dtype=torch.int64)
    return buf, buf[GUARD:GUARD + total].view(*shape)


def call_counts(p, t, thr, outs, ws, nbytes):
    n, C = p.shape
    _lib.call("cgcn_threshold_counts", n=n, C=C, T=thr.shape[0], probs=p, targets=t, thresholds=thr, pos=outs[0], tp=outs[1],
              pp=outs[2], exact=outs[3], rows=outs[4], tpsum=outs[5], workspace=ws, workspace_bytes=nbytes)


def device_counts(probs, targets, thresholds):
    """the six arrays as numpy from one cgcn_threshold_counts call (T <= 64)"""
    p = torch.as_tensor(probs).cuda().contiguous()
    t = torch.as_tensor(targets).cuda().contiguous()
    n, C = p.shape
    thr = torch.from_numpy(th.threshold_matrix(thresholds, C)).cuda()
    T = thr.shape[0]
    nbytes = _lib.query("cgcn_threshold_workspace_bytes", n=n, C=C, T=T)
    assert nbytes > 0
    arena = torch.randint(0, 256, (nbytes + 256 + 8,), device="cuda", dtype=torch.uint8)   # stale bytes, a canary behind
    start = (-arena.data_ptr()) % 256
    ws = arena[start:start + nbytes]
    behind, before = arena[start + nbytes:].clone(), arena[:start].clone()
    bufs = [_banded(s) for s in ((C,), (T, C), (T, C), (T,), (T, 2 * C + 1), (T, 2 * C + 1))]
    call_counts(p, t, thr, [v for _, v in bufs], ws, nbytes)
    torch.cuda.synchronize()
    for (buf, v), name in zip(bufs, FIELDS):
        assert (buf[:GUARD] == SENTINEL).all() and (buf[buf.numel() - GUARD:] == SENTINEL).all(), "guard band of %s" % name
    assert torch.equal(arena[start + nbytes:], behind) and torch.equal(arena[:start], before), "written outside the workspace"
    return tuple(v.cpu().numpy() for _, v in bufs)


@functools.lru_cache(maxsize=None)
def _reference(kind, name):
    p, y, thr = CASES[kind](name)
    c = th.threshold_counts_host(p, y, thr)
    return tuple(getattr(c, f) for f in FIELDS)


def _edge(name):
    n, C = name
    return tc.quantised(n, C) + (tc.GRID7,)


CASES = {"edge": _edge, "special": tc.special_case, "shape": tc.shape_case}


def check(kind, name):
    p, y, thr = CASES[kind](name)
    got = device_counts(p, y, thr)
    want = _reference(kind, name)
    for g, w, f in zip(got, want, FIELDS):
        assert same(g, w), (kind, name, f)          # whole arrays: a sentinel left in any element fails here
    return got


@pytest.mark.parametrize("n", tc.EDGE_N)
def test_lane_chunk_and_row_block_edges(n):
    for C in tc.EDGE_C:
        check("edge", (n, C))


@pytest.mark.parametrize("name", tc.SPECIAL)
def test_special_values_and_threshold_matrices(name):
    got = check("special", name)
    p, y, thr = tc.special_case(name)
    n, C = p.shape
    rows = got[4]
    if name == "all_ones":
        assert (rows[:-1, 2 * C] == n).all() and rows[-1, C] == n and (got[3][:-1] == n).all() and got[3][-1] == 0
    if name == "all_zero":
        assert (rows[:, 0] == n).all() and rows[:, 1:].sum() == 0 and (got[3] == n).all()
    if name == "infinities":        # +inf: only the +inf row; -inf: everything; 0: -0.0 is predicted
        assert got[2][0].sum() == C and got[2][1].sum() == n * C and got[2][2].sum() == (p >= 0).sum() > (p > 0).sum()
    if name == "nan":
        assert got[2][0].sum() == (p >= thr[0]).sum() < np.isfinite(p).sum() + 1
    if name == "soft_targets":      # the same counts as the 0 / 1 targets they were made from
        hard = th.threshold_counts_host(p, (y > 0.5).astype(np.float32), thr)
        assert all(same(g, getattr(hard, f)) for g, f in zip(got, FIELDS))
    if name in ("per_label", "square_matrix"):
        swapped = thr.T.copy() if name == "square_matrix" else thr[:, ::-1].copy()
        assert not same(got[2], th.threshold_counts_host(p, y, swapped).pp)


@pytest.mark.parametrize("name", sorted(tc.SHAPES))
def test_many_workgroups_threshold_limits_and_large_labels(name):
    n, C, T = tc.SHAPES[name]
    passes = _lib.query("cgcn_debug_threshold_route", n=n, C=C, T=T)
    if name in ("c1024", "c600"):
        assert passes > 1           # the slow route: the thresholds in groups, every group streams the rows again
    if name in ("grid27", "t1"):
        assert passes == 1          # the project's shape: one pass, every histogram in LDS
    check("shape", name)


@pytest.mark.parametrize("T", [65, 130])
def test_more_than_64_thresholds_through_python(T):
    p, y = tc.quantised(300, 37)
    grid = tc.grid_of(T)
    assert grid.size == T
    c = th.threshold_counts(torch.from_numpy(p).cuda(), torch.from_numpy(y).cuda(), grid)
    want = th.threshold_counts_host(p, y, grid)
    for f in FIELDS:
        g = getattr(c, f)
        assert g.is_cuda and g.dtype == torch.int64 and same(g.cpu().numpy(), getattr(want, f)), f
    assert (c.n, c.C) == (300, 37) and same(c.thresholds.cpu().numpy(), want.thresholds)


def test_python_forms_and_metrics():
    p, y = tc.quantised(1000, 103)
    dp, dy = torch.from_numpy(p).cuda(), torch.from_numpy(y).cuda()
    for thr in (0.5, tc.GRID7, torch.from_numpy(tc.GRID7).cuda(), tc.per_label_matrix(4, 103)):
        c = th.threshold_counts(dp, dy, thr)
        host_thr = thr.cpu().numpy() if isinstance(thr, torch.Tensor) else thr
        want = th.threshold_counts_host(p, y, host_thr)
        assert all(same(getattr(c, f).cpu().numpy(), getattr(want, f)) for f in FIELDS)
        got_m, want_m = th.metrics_from_counts(c), th.metrics_from_counts(want)
        assert sorted(got_m) == sorted(want_m)
        for k in want_m:
            assert got_m[k].dtype == np.float64 and np.array_equal(got_m[k], want_m[k], equal_nan=True), k
    m = th.threshold_metrics(dp, dy)                               # the default: one threshold, 0.5
    assert all(m[k].shape == (1,) for k in th.METRIC_KEYS) and m["f1"].shape == (1, 103)
    best = th.best_thresholds(th.threshold_counts(dp, dy, tc.GRID7))
    want = th.best_thresholds(th.threshold_counts_host(p, y, tc.GRID7))
    assert best.dtype == np.float32 and np.array_equal(best, want, equal_nan=True) and np.isnan(best[-1])


def test_two_runs_give_the_same_bits():
    p, y, thr = tc.shape_case("t64")
    a, b = device_counts(p, y, thr), device_counts(p, y, thr)
    assert all(x.tobytes() == z.tobytes() for x, z in zip(a, b))


def test_the_call_is_capturable():
    p, y, thr = tc.shape_case("t64")
    dp, dy = torch.from_numpy(p).cuda(), torch.from_numpy(y).cuda()
    n, C = p.shape
    dthr = torch.from_numpy(th.threshold_matrix(thr, C)).cuda()
    T = dthr.shape[0]
    nbytes = _lib.query("cgcn_threshold_workspace_bytes", n=n, C=C, T=T)
    ws = torch.empty(nbytes, device="cuda", dtype=torch.uint8)
    shapes = ((C,), (T, C), (T, C), (T,), (T, 2 * C + 1), (T, 2 * C + 1))
    eager = [torch.full(s, SENTINEL, device="cuda", dtype=torch.int64) for s in shapes]
    call_counts(dp, dy, dthr, eager, ws, nbytes)                   # the code object is loaded outside the capture
    torch.cuda.synchronize()
    outs = [torch.full(s, SENTINEL, device="cuda", dtype=torch.int64) for s in shapes]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            call_counts(dp, dy, dthr, outs, ws, nbytes)
    torch.cuda.current_stream().wait_stream(s)
    for o in outs:
        o.fill_(SENTINEL)                                          # whatever the capture left: the replay writes everything
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(outs, eager))
    assert all(same(a.cpu().numpy(), w) for a, w in zip(outs, _reference("shape", "t64")))


def test_compute_metrics_adds_the_five_keys():
    p, y = tc.quantised(1000, 103)
    base = metrics.compute_metrics(p, y, 0.25)
    keep = p.copy()
    out = metrics.compute_metrics(p, y, 0.25, br_threshold=0.5)
    assert np.array_equal(p, keep)                                 # all_predictions is not thresholded in place
    assert sorted(set(out) - set(base)) == sorted(th.METRIC_KEYS)
    for k in base:
        assert np.array_equal(np.asarray(out[k]), np.asarray(base[k]), equal_nan=True), k
    want = th.threshold_metrics_host(p, y, 0.5)
    for k in th.METRIC_KEYS:
        assert isinstance(out[k], float) and out[k] == want[k][0], k

    class Args:
        br_threshold = 0.3
    via_args = metrics.compute_metrics(p, y, 0.25, Args())          # what train.py's -br_threshold hands through
    want = th.threshold_metrics_host(p, y, 0.3)
    assert all(via_args[k] == want[k][0] for k in th.METRIC_KEYS)
    assert sorted(metrics.compute_metrics(p, y, 0.25, object())) == sorted(base)


def test_optimal_cutoffs_feed_a_one_row_matrix():
    rng = np.random.RandomState(11)
    n, C = 2000, 103
    y = (rng.rand(n, C) < 0.3).astype(np.float32)                  # every label has both classes
    p = np.clip(0.35 * y + 0.6 * rng.rand(n, C), 0, 1).astype(np.float32)
    assert y.min(axis=0).max() == 0 and y.max(axis=0).min() == 1
    dp, dy = torch.from_numpy(p).cuda(), torch.from_numpy(y).cuda()
    cut = curves.optimal_cutoffs(dp, dy)
    assert not torch.isnan(cut).any()
    m = th.threshold_metrics(dp, dy, cut[None])
    want = th.threshold_metrics_host(p, y, cut.cpu().numpy()[None])
    for k in want:
        assert m[k].shape == want[k].shape and np.array_equal(m[k], want[k], equal_nan=True), k
    assert m["maF1"][0] > th.threshold_metrics_host(p, y, 0.9)["maF1"][0]     # a cutoff per label beats a poor shared one


def test_bad_inputs_raise():
    p, y = tc.quantised(64, 7)
    dp, dy = torch.from_numpy(p).cuda(), torch.from_numpy(y).cuda()
    with pytest.raises(RuntimeError, match="on the GPU"):
        th.threshold_counts(torch.from_numpy(p), dy, 0.5)
    with pytest.raises(RuntimeError, match="on the GPU"):
        th.threshold_counts(dp, torch.from_numpy(y), 0.5)
    with pytest.raises(RuntimeError, match=r"\[n, C\]"):
        th.threshold_counts(dp, dy[:, :6], 0.5)
    with pytest.raises(ValueError, match="NaN"):
        th.threshold_counts(dp, dy, [0.5, float("nan")])
    wide = torch.zeros(4, 1025, device="cuda")
    with pytest.raises(RuntimeError, match="unsupported"):
        th.threshold_counts(wide, wide, 0.5)
    assert _lib.query("cgcn_threshold_workspace_bytes", n=4, C=1025, T=1) == 0
    assert _lib.query("cgcn_threshold_workspace_bytes", n=4, C=7, T=65) == 0
    assert _lib.query("cgcn_threshold_workspace_bytes", n=0, C=7, T=1) == 0
    ws = torch.empty(256, device="cuda", dtype=torch.uint8)
    o = torch.empty(64, device="cuda", dtype=torch.int64)
    args = dict(n=4, C=7, T=1, probs=dp, targets=dy, thresholds=dp, pos=o, tp=o, pp=o, exact=o, rows=o, tpsum=o, workspace=ws,
                workspace_bytes=256)
    assert _lib.query("cgcn_threshold_counts", **dict(args, tpsum=None)) == -1
    assert _lib.query("cgcn_threshold_counts", **dict(args, C=1025)) == -2
    assert _lib.query("cgcn_threshold_counts", **dict(args, T=65)) == -2


# ---- every instance, team shape and bound of the launch plan ----------------------------------------------------------------
def equal_counts(got, want, what, T=None):
    """all six arrays; with T, the first T thresholds of a reference that has more"""
    assert len(got) == len(want) == len(FIELDS)
    for g, w, f in zip(got, want, FIELDS):
        assert same(g, w if T is None or f == "pos" else w[:T]), (what, f)


def host_counts(p, y, thr):
    c = th.threshold_counts_host(p, y, thr)
    return tuple(getattr(c, f) for f in FIELDS)


def test_the_restated_plan_gives_the_librarys_groups_at_every_C_and_T():
    """host arithmetic on both sides, nothing is launched"""
    for C in range(1, tc.THR_MAX_C + 1):
        got = [_lib.query("cgcn_debug_threshold_route", n=tc.SWEEP_N, C=C, T=T) for T in range(1, tc.THR_MAX_T + 1)]
        assert got == [tc.plan(tc.SWEEP_N, C, T)["groups"] for T in range(1, tc.THR_MAX_T + 1)], C


@pytest.mark.parametrize("C", sorted(tc.CHUNK_EDGE_C))
def test_every_instance_at_the_edges_of_its_label_chunks(C):
    """193, 257, 449 and 513 have ONE live label in their last live chunk (257: three wholly dead chunks behind it); the dead
    labels and the dead slot of the wave's last threshold hold NaN and must count nothing"""
    q = tc.plan(300, C, tc.GRID7.size)
    assert q["CH"] == tc.CHUNK_EDGE_C[C] and q["grid_x"] == 3 and q["last_nt"] < q["TT"]     # a dead slot
    check("edge", (300, C))


@pytest.mark.parametrize("C", [193, 257, 513])
def test_one_live_label_in_the_last_chunk_against_the_brute_force_loop(C):
    assert C % 64 == 1 and tc.plan(12, C, 7)["CH"] == tc.CHUNK_EDGE_C[C]
    p, y = tc.quantised(12, C)
    equal_counts(device_counts(p, y, tc.GRID7), tc.brute_force_counts(p, y, th.threshold_matrix(tc.GRID7, C)), C)


@pytest.mark.parametrize("name,n,C", tc.WIDE_SPECIAL)
def test_special_values_in_the_wide_instances(name, n, C):
    p, y, thr = tc.special_at(name, n, C)
    q = tc.plan(n, C, thr.size)
    assert q["CH"] == (16 if C == 1024 else 8) and C % 64 in (0, 1) and q["grid_x"] == 2
    got = device_counts(p, y, thr)
    equal_counts(got, host_counts(p, y, thr), (name, C))
    rows, tpsum = got[4], got[5]
    if name == "all_ones":          # k = 2048 and both = 1024: the largest value of either field of the row record
        assert 2 * C == 2048 and (rows[:-1, 2048] == n).all() and (tpsum[:-1, 2048] == n * 1024).all()
        assert rows[-1, 1024] == n and tpsum[-1].sum() == 0 and rows.sum() == thr.size * n
    if name == "infinities":
        assert got[2][0].sum() == C and got[2][1].sum() == n * C and got[2][2].sum() == (p >= 0).sum() > (p > 0).sum()
    if name == "nan":
        assert got[2][0].sum() == (p >= thr[0]).sum() < np.isfinite(p).sum() + 1


@functools.lru_cache(maxsize=None)
def _sweep_reference(C):
    return host_counts(*tc.sweep_case(C))


@pytest.mark.parametrize("C", sorted(tc.SWEEP_C))
def test_every_team_shape_one_call_per_T(C):
    """T = 1 .. 64 against the first T rows of ONE host evaluation: every waves-per-team count this C has (5, 6 and 7 waves
    are workgroups of 320, 384 and 448 threads), spare waves behind a short last group, every fill of the last wave, and --
    the matrix being per label -- threshold rows read at blockIdx.y > 0"""
    p, y, thr = tc.sweep_case(C)
    want = _sweep_reference(C)
    plans = [tc.plan(tc.SWEEP_N, C, T) for T in range(1, tc.THR_MAX_T + 1)]
    assert {q["waves"] for q in plans} == set(range(1, tc.SWEEP_C[C] + 1)) and all(q["grid_x"] == 3 for q in plans)
    assert {q["last_nt"] for q in plans} == set(range(1, plans[0]["TT"] + 1))
    assert any(q["spare"] for q in plans) == (C != 5) and any(q["groups"] > 1 for q in plans) == (C != 5)
    for T, q in enumerate(plans, 1):
        equal_counts(device_counts(p, y, thr[:T]), want, (C, T, q), T)


def test_a_second_group_reads_its_own_threshold_rows():
    C, T = 103, 40
    q = tc.plan(tc.SWEEP_N, C, T)
    assert (q["groups"], q["TW"], q["spare"]) == (2, 32, 3)
    p, y, thr = tc.sweep_case(C)
    got = device_counts(p, y, thr[:T])
    equal_counts(got, _sweep_reference(C), (C, T), T)
    swapped = host_counts(p, y, thr[:T, ::-1].copy())
    assert not same(got[2][:32], swapped[2][:32]) and not same(got[2][32:], swapped[2][32:])
    assert not same(got[2][32:], got[2][:8])            # ... and not those of the first group again


@pytest.mark.parametrize("n", [127, 128, 129])
def test_either_side_of_the_smallest_row_block(n):
    for C, T in tc.MIN_ROWS_SHAPES:
        q = tc.plan(n, C, T)
        assert q["rows_per_wg"] == tc.THR_MIN_ROWS == 128 and q["grid_x"] == (2 if n == 129 else 1)   # 129: one row
        p, y = tc.quantised(n, C)
        thr = tc.per_label_matrix(T, C)
        equal_counts(device_counts(p, y, thr), host_counts(p, y, thr), (n, C, T))


@pytest.mark.parametrize("CH", sorted(tc.TILE_PLANS))
def test_one_row_less_and_more_than_whole_tiles(CH):
    """as the rows of a single workgroup and of the last of three; tile_rows set by the LDS room in three of the plans and
    by the registers in flight in the other three"""
    C, T, tile_by = tc.TILE_PLANS[CH]
    thr = tc.per_label_matrix(T, C)
    for n, groups in tc.tile_edge_rows(C, T):
        q = tc.plan(n, C, T)
        tail = n - (groups - 1) * q["rows_per_wg"]
        assert q["CH"] == CH and q["tile_by"] == tile_by and q["grid_x"] == groups
        assert (tail + 1) % q["tile_rows"] <= 2 and tail >= q["tile_rows"] - 1
        p, y = tc.quantised(n, C)
        equal_counts(device_counts(p, y, thr), host_counts(p, y, thr), (n, C, T, q))


def test_both_16_bit_halves_of_a_count_register_at_65535():
    """C = 1, n = 512 * 65535 + 1: 513 workgroups of 65 535 rows (the last owns one row), one team, so every wave counts
    every row of its workgroup.  The first workgroup's rows are all positive and theta_0 = -inf predicts them all: its
    register of threshold 0 ends at 0xFFFFFFFF, 65 535 in both halves -- one more row would carry.  Expected values from the
    joint histogram of (level, target), which tests/test_thresholds_host.py holds to threshold_counts_host."""
    n, T = tc.HALVES_N, tc.HALVES_T
    q = tc.plan(n, 1, T)
    assert (q["rows_per_wg"], q["grid_x"], q["teams"], q["groups"]) == (65535, 513, 1, 1) and n - 512 * 65535 == 1
    assert tc.plan(n - 1, 1, T)["grid_x"] == 512
    idx, y = tc.halves_case(n)
    thr = tc.HALVES_GRID
    assert thr[0] == -np.inf and (y[:65535] == 1).all()
    want = tc.single_label_counts(idx, y, thr)
    assert want[2][0, 0] == n and want[1][0, 0] == want[0][0] > 65535
    p = tc.LEVELS[idx].reshape(n, 1)
    start = time.perf_counter()
    got = device_counts(p, y, thr)
    print("C = 1, n = %d, T = %d: %.2f s for upload, call and guard checks" % (n, T, time.perf_counter() - start))
    equal_counts(got, want, "halves")


@pytest.mark.parametrize("C,T,CH,waves", [(257, 12, 8, 3), (65, 40, 2, 5)])
def test_two_runs_of_a_wide_and_of_a_five_wave_plan_give_the_same_bits(C, T, CH, waves):
    q = tc.plan(tc.SWEEP_N, C, T)
    assert (q["CH"], q["waves"], q["block"]) == (CH, waves, 64 * waves * (8 // waves))
    p, y, thr = tc.sweep_case(C)
    a, b = device_counts(p, y, thr[:T]), device_counts(p, y, thr[:T])
    assert all(x.tobytes() == z.tobytes() for x, z in zip(a, b))
    equal_counts(a, _sweep_reference(C), (C, T), T)
