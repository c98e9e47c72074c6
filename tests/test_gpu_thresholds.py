"""Thresholded multi-label counts on the device (chromegcn_amd.thresholds, csrc/cgcn_threshold.hip) against the numpy
restatement that tests/test_thresholds_host.py holds to the reference -- by exact equality (dtype, shape, values) of EVERY
output array of every case.  Every case goes through the C ABI with a workspace of exactly the queried size full of stale
bytes and sentinel-filled guard bands around every output (`device_counts`): every element is written, nothing else is."""
import functools

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
