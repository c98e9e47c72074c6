"""ROC / precision-recall curves and cutoffs on the device (chromegcn_amd.curves, csrc/cgcn_metrics.hip) against the numpy
restatements that tests/test_curves_host.py holds to scikit-learn -- by exact equality: offsets, integer counts, thresholds
and the derived float64 tensors.  Every device run of this file goes through the C ABI with a workspace of exactly the queried
size full of stale bytes and 4096-byte guard bands around every output (`device_points`)."""
import functools
import warnings

import numpy as np
import pytest
import torch

import curves_cases as cc
from chromegcn_amd import _lib, curves, metrics

pytestmark = pytest.mark.gpu

GUARD = 1024                    # elements of 4 bytes on each side of every output
KINDS = [("roc", True), ("roc", False), ("pr", False)]


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def _banded(total, dtype, fill):
    buf = torch.full((total + 2 * GUARD,), fill, device="cuda", dtype=dtype)
    return buf, buf[GUARD:GUARD + total]


def device_points(preds, targets, kind, drop, ws_shift=0):
    """(offsets, tps, fps, thresholds) as numpy arrays from cgcn_curves_count / cgcn_curves_fill, or ValueError when the
    device flags the scores.  ws_shift: bytes past a 256-aligned address at which the workspace starts."""
    p = torch.as_tensor(preds).cuda().contiguous()
    t = torch.as_tensor(targets).cuda().contiguous()
    n, C = p.shape
    nbytes = _lib.query("cgcn_curves_workspace_bytes", n=n, C=C)
    assert nbytes > 0
    arena = torch.randint(0, 256, (nbytes + 256 + 8,), device="cuda", dtype=torch.uint8)   # stale bytes, a canary behind
    start = (-arena.data_ptr()) % 256 + ws_shift
    ws = arena[start:start + nbytes]
    assert ws.data_ptr() % 256 == ws_shift
    behind = arena[start + nbytes:].clone()
    before = arena[:start].clone()
    head_buf, head = _banded(C + 2, torch.int64, -7)       # offsets [C + 1], then the `bad` word in the low half of a word
    head[C + 1] = 0
    _lib.call("cgcn_curves_count", n=n, C=C, probs=p, targets=t, kind=_lib.CURVE_ROC if kind == "roc" else _lib.CURVE_PR,
              drop_intermediate=int(drop), offsets=head, bad=head.data_ptr() + 8 * (C + 1), workspace=ws, workspace_bytes=nbytes)
    host = head.cpu().numpy()
    if host[C + 1] != 0:
        raise ValueError("bad scores")
    offsets, total = host[:C + 1].copy(), int(host[C])
    bufs = [_banded(total, torch.int32, -7), _banded(total, torch.int32, -7), _banded(total, torch.float32, -7.0)]
    _lib.call("cgcn_curves_fill", n=n, C=C, offsets=head, capacity=total, tps=bufs[0][1], fps=bufs[1][1], thresholds=bufs[2][1],
              workspace=ws, workspace_bytes=nbytes)
    torch.cuda.synchronize()
    for buf, _ in bufs + [(head_buf, head)]:
        assert (buf[:GUARD] == -7).all() and (buf[buf.numel() - GUARD:] == -7).all(), "a guard band was written"
    assert torch.equal(arena[start + nbytes:], behind) and torch.equal(arena[:start], before), "written outside the workspace"
    return (offsets,) + tuple(v.cpu().numpy() for _, v in bufs)


def host_points(preds, targets, kind, drop):
    """the same four arrays from the restatement, label after label"""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        per = []
        for c in range(preds.shape[1]):
            if kind == "roc":
                fps, tps, thr = curves.roc_points_host(targets[:, c], preds[:, c], drop)
            else:
                fps, tps, thr = curves._binary_clf_curve_host(targets[:, c], preds[:, c])
            per.append((tps, fps, thr))
    offsets = np.concatenate([[0], np.cumsum([p[0].size for p in per])]).astype(np.int64)
    return (offsets, np.concatenate([p[0] for p in per]).astype(np.int32), np.concatenate([p[1] for p in per]).astype(np.int32),
            np.concatenate([p[2] for p in per]).astype(np.float32))


@functools.lru_cache(maxsize=None)
def _reference(name, kind, drop):
    return host_points(*CASES[name], kind, drop)


CASES = cc.all_cases()


def check_points(name, ws_shift=0):
    preds, targets = CASES[name]
    for kind, drop in KINDS:
        got = device_points(preds, targets, kind, drop, ws_shift)
        want = _reference(name, kind, drop)
        assert got[1].size == got[2].size == got[3].size == got[0][-1]      # exactly offsets[C] long
        for g, w, what in zip(got, want, ("offsets", "tps", "fps", "thresholds")):
            assert same(g, w), (name, kind, drop, what)


@pytest.mark.parametrize("n", cc.EDGE_N)
def test_chunk_edges(n):
    for C in cc.EDGE_C:
        for q in cc.EDGE_LEVELS:
            check_points("edge_n%d_C%d_q%d" % (n, C, q), ws_shift=8 if q == 3 else 0)


@pytest.mark.parametrize("name", ["runs", "corner", "degenerate", "saturated", "width_33", "width_103", "many_chunks"])
def test_points_equal_the_restatement(name):
    check_points(name)


@pytest.mark.parametrize("name", ["corner", "degenerate"])
def test_workspace_eight_bytes_past_an_aligned_address(name):
    check_points(name, ws_shift=8)


def _derived_host(preds, targets, kind, drop):
    a, b = [], []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for c in range(preds.shape[1]):
            if kind == "roc":
                x, y, _ = curves.roc_curve_host(targets[:, c], preds[:, c], drop)
            else:
                x, y, _ = curves.pr_curve_host(targets[:, c], preds[:, c])
                x, y = x[:-1][::-1], y[:-1][::-1]       # the flat arrays: descending thresholds, no terminal point
            a.append(x)
            b.append(y)
    return np.concatenate(a), np.concatenate(b)


@pytest.mark.parametrize("name", ["runs", "corner", "degenerate", "width_33", "edge_n1_C3_q1", "edge_n4097_C3_q16"])
def test_python_objects_and_derived_tensors(name):
    preds, targets = CASES[name]
    p, t = torch.from_numpy(preds).cuda(), torch.from_numpy(targets).cuda()
    for kind, drop in KINDS:
        obj = curves.roc_curves(p, t, drop_intermediate=drop) if kind == "roc" else curves.pr_curves(p, t)
        want = _reference(name, kind, drop)
        for g, w in zip((obj.offsets, obj.tps, obj.fps, obj.thresholds), want):
            assert same(g.cpu().numpy(), w), (name, kind, drop)
        a, b = (obj.fpr, obj.tpr) if kind == "roc" else (obj.precision, obj.recall)
        assert a.dtype == b.dtype == torch.float64 and a.is_cuda
        wa, wb = _derived_host(preds, targets, kind, drop)
        assert same(a.cpu().numpy(), wa) and same(b.cpu().numpy(), wb), (name, kind, drop)
        assert len(obj) == preds.shape[1]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for c in range(preds.shape[1]):          # the triple in scikit-learn's order, length and dtype
                w3 = (curves.roc_curve_host(targets[:, c], preds[:, c], drop) if kind == "roc"
                      else curves.pr_curve_host(targets[:, c], preds[:, c]))
                assert all(same(g, w) for g, w in zip(obj[c], w3)), (name, kind, drop, c)


@pytest.mark.parametrize("value", [-0.25, float("nan")])
def test_bad_scores_raise(value):
    preds, targets = (a.copy() for a in cc.edge_case(4097, 3, 16))
    preds[4000, 1] = value
    p, t = torch.from_numpy(preds).cuda(), torch.from_numpy(targets).cuda()
    for fn in (curves.roc_curves, curves.pr_curves, curves.optimal_cutoffs):
        with pytest.raises(ValueError, match="negative or NaN"):
            fn(p, t)
    with pytest.raises(ValueError):
        device_points(preds, targets, "roc", True)


def test_two_runs_give_the_same_bits():
    preds, targets = CASES["corner"]
    for kind, drop in KINDS:
        a = device_points(preds, targets, kind, drop)
        b = device_points(preds, targets, kind, drop, ws_shift=8)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def _cutoff_names(key):
    return [name for name in sorted(CASES) if name.startswith("edge_n%d_" % key)] if isinstance(key, int) else [key]


@pytest.mark.parametrize("key", ["runs", "corner", "degenerate", "saturated", "width_33", "width_103", "many_chunks"] + cc.EDGE_N)
def test_cutoffs_equal_the_restatement(key):
    for name in _cutoff_names(key):
        check_cutoffs(name)


def check_cutoffs(name):
    preds, targets = CASES[name]
    got = curves.optimal_cutoffs(torch.from_numpy(preds).cuda(), torch.from_numpy(targets).cuda())
    assert got.dtype == torch.float32 and tuple(got.shape) == (preds.shape[1],)
    want = np.array([curves.optimal_cutoff_host(targets[:, c], preds[:, c]) for c in range(preds.shape[1])], dtype=np.float32)
    assert same(got.cpu().numpy(), want), name
    if name == "corner":     # the tie label: the earlier of its two equal minima
        c = cc.corner_case()[2].index("tie")
        srt, _ = cc.mc.sorted_view(preds[:, c], targets[:, c])
        assert got[c].item() == srt[3 * cc.TIE_M - 1]


def test_cutoff_guard_bands():
    preds, targets = CASES["degenerate"]
    roc = curves.roc_curves(torch.from_numpy(preds).cuda(), torch.from_numpy(targets).cuda())
    buf, out = _banded(len(roc), torch.float32, -7.0)
    _lib.call("cgcn_curves_cutoff", C=len(roc), offsets=roc.offsets, tps=roc.tps, fps=roc.fps, thresholds=roc.thresholds,
              cutoffs=out)
    assert (buf[:GUARD] == -7).all() and (buf[buf.numel() - GUARD:] == -7).all()
    assert same(out.cpu().numpy(), curves.cutoffs_of(roc).cpu().numpy())


@pytest.mark.parametrize("name", ["runs", "corner", "degenerate", "saturated", "width_103"])
def test_areas_agree_with_multilabel_metrics(name):
    """the trapezoid under every device curve, summed on the host in float64, is the auroc / aupr of the existing scan (its
    stated tolerance: DESIGN.md section 2), and the same labels are undefined"""
    preds, targets = CASES[name]
    p, t = torch.from_numpy(preds).cuda(), torch.from_numpy(targets).cuda()
    m = {k: v.cpu().numpy().astype(np.float64) for k, v in metrics.multilabel_metrics(p, t).items()}
    roc, pr = curves.roc_curves(p, t), curves.pr_curves(p, t)
    for c in range(preds.shape[1]):
        fpr, tpr, _ = roc[c]
        undefined = np.isnan(fpr).any() or np.isnan(tpr).any()
        assert undefined == np.isnan(m["auroc"][c]), (name, c)
        if not undefined:
            area = float(np.sum(np.diff(fpr) * (tpr[1:] + tpr[:-1]) * 0.5))
            assert np.isclose(area, m["auroc"][c], rtol=3e-6, atol=3e-7), (name, c, area, m["auroc"][c])
        precision, recall, _ = pr[c]
        area = -float(np.sum(np.diff(recall) * (precision[1:] + precision[:-1]) * 0.5))    # recall descends
        assert not np.isnan(m["aupr"][c])
        assert np.isclose(area, m["aupr"][c], rtol=3e-6, atol=3e-7), (name, c, area, m["aupr"][c])


def test_group_means_through_compute_metrics():
    preds, targets, names = cc.degenerate_case()
    groups = {"first": [0, 1], "mixed": [1, 2, 4], "rest": [3, 5]}
    base = metrics.compute_metrics(preds, targets, 0.0)
    out = metrics.compute_metrics(preds, targets, 0.0, label_groups=groups)
    assert sorted(set(out) - set(base)) == sorted("%s_%s" % (g, k) for g in groups for k in ("meanAUC", "meanAUPR", "meanFDR"))
    for k in base:
        assert np.array_equal(np.asarray(out[k]), np.asarray(base[k]), equal_nan=True), k
    per = {k: v.cpu().numpy().astype(np.float64)
           for k, v in metrics.multilabel_metrics(torch.from_numpy(preds).cuda(), torch.from_numpy(targets).cuda()).items()}
    want = metrics.group_means(per, groups)
    assert np.isnan(out["first_meanAUC"]) and not np.isnan(out["first_meanAUPR"])    # all positive / all negative: no AUROC
    for k, v in want.items():
        assert (np.isnan(v) and np.isnan(out[k])) or out[k] == v, k
