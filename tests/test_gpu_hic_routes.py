"""The routing table of HicContacts.build_raw: which of the eight top-K entry points of csrc/cgcn_hic.hip a build reaches
(direct / `_up`, plain / `_dist`, count / build), with which scalar arguments and which workspace size, and how often the host
reads a count back.  The expected lists are literal; the sizes in them come from the inputs and from the host restatement
(hic.survivor_values).  What the kernels compute is the business of test_gpu_hic*.py."""
import numpy as np
import pytest
import torch

from chromegcn_amd import _lib, hic

pytestmark = pytest.mark.gpu
DEV = "cuda"
RES, WBP, EDGES, GAP = 5000, 1000, 200, 10000
QUERY = _lib.query   # the unwrapped one, for the sizes the test itself asks for
SCALARS = ("M", "N", "K", "capacity", "resolution_bp", "window_bp", "n_window_bins", "min_distance_bp", "n_bins", "n_expected")


def _inputs():
    """300 records on the 5000 grid over 40 bins (20 of them diagonal, 60 one bin apart and so closer than GAP) and 61 windows
    on the 1000 grid: 26 of the first 30 multiples of 5000 (so bins 3, 10, 17, 24 and 30 .. 39 are off the window set) and 35
    in between"""
    rng = np.random.RandomState(7)
    pairs = np.stack(np.meshgrid(np.arange(40), np.arange(40), indexing="ij"), -1).reshape(-1, 2)
    far = pairs[np.abs(pairs[:, 0] - pairs[:, 1]) >= 2]
    near = pairs[np.abs(pairs[:, 0] - pairs[:, 1]) == 1]
    diag = np.repeat(np.arange(0, 40, 2)[:, None], 2, 1)
    recs = np.concatenate([far[rng.permutation(len(far))[:220]], near[rng.permutation(len(near))[:60]], diag])
    recs = recs[rng.permutation(len(recs))]
    ws = [RES * b for b in range(30) if b % 7 != 3]
    ws += [RES * b + 2000 for b in range(0, 30, 2)] + [RES * b + o for b in range(1, 30, 3) for o in (1000, 4000)]
    return dict(pos1=(recs[:, 0] * RES).astype(np.int32), pos2=(recs[:, 1] * RES).astype(np.int32),
                count=rng.randint(1, 50, len(recs)).astype(np.float64), ws=np.array(sorted(ws), dtype=np.int32),
                norm=rng.uniform(0.5, 2.0, 40), expected=rng.uniform(0.5, 2.0, 40))


@pytest.fixture(scope="module")
def inp():
    d = _inputs()
    assert d["pos1"].size == 300 and d["ws"].size == 61 and int((d["pos1"] == d["pos2"]).sum()) == 20
    return d


class Spy:
    """_lib.call, _lib.query, Tensor.item and Tensor.tolist wrapped: `calls` = [(entry point, its scalar arguments,
    workspace_bytes)], `asked` = [(workspace function, its sizes)], `syncs` = the read-backs"""

    def __init__(self, monkeypatch):
        self.calls, self.asked, self.syncs = [], [], []
        real_call, real_query, tolist, item = _lib.call, _lib.query, torch.Tensor.tolist, torch.Tensor.item

        def call(fn, **kw):
            self.calls.append((fn, {k: kw[k] for k in SCALARS if k in kw}, kw["workspace_bytes"]))
            return real_call(fn, **kw)

        def query(fn, **kw):
            if fn.endswith("_workspace_bytes"):
                self.asked.append((fn, dict(kw)))
            return real_query(fn, **kw)

        monkeypatch.setattr(_lib, "call", call)
        monkeypatch.setattr(_lib, "query", query)
        monkeypatch.setattr(torch.Tensor, "tolist", lambda t: (self.syncs.append(1), tolist(t))[1])
        monkeypatch.setattr(torch.Tensor, "item", lambda t: (self.syncs.append(1), item(t))[1])

    def clear(self):
        del self.calls[:], self.asked[:], self.syncs[:]


def _survivors(inp, window_bp=None, gap=0, ws=None):
    return hic.survivor_values(inp["pos1"], inp["pos2"], inp["count"], None, RES, inp["ws"] if ws is None else ws,
                               window_bp=window_bp, min_distance_bp=gap)[0].size


def _expect(inp, up, gap, dist, n_bins=0, n_expected=0, ws=None, edges=EDGES):
    """the (entry point, scalars, workspace_bytes) pairs of one first build, and the workspace questions behind them"""
    ws = inp["ws"] if ws is None else ws
    m, n, k = 300, int(ws.size), edges // 2
    cap = _survivors(inp, WBP if up else None, gap, ws)
    suffix, fn = ("_up", "cgcn_hic_up_workspace_bytes") if up else ("", "cgcn_hic_workspace_bytes")
    extra = dict(resolution_bp=RES, window_bp=WBP, n_window_bins=int(ws[-1]) // WBP + 1) if up else {}
    count_sizes, build_sizes = dict(M=m, N=n, capacity=0, K=0, **extra), dict(M=m, N=n, capacity=cap, K=k, **extra)
    count = dict(M=m, N=n, **extra, **(dict(min_distance_bp=gap) if gap else {}))
    build = dict(M=m, N=n, K=k, capacity=cap, n_bins=n_bins, **{"resolution_bp": RES, **extra},
                 **(dict(min_distance_bp=gap, n_expected=n_expected) if dist else {}))
    calls = [("cgcn_hic_count" + suffix + ("_dist" if gap else ""), count, QUERY(fn, **count_sizes)),
             ("cgcn_hic_build" + suffix + ("_dist" if dist else ""), build, QUERY(fn, **build_sizes))]
    assert all(c[2] > 0 for c in calls) and cap > 0
    return calls, [(fn, count_sizes), (fn, build_sizes)], cap


def _fresh(inp):
    return hic.HicContacts(inp["pos1"], inp["pos2"], inp["count"], DEV)


def _build(c, inp, norm=None, **kw):
    return c.build_raw(norm, RES, kw.pop("ws", inp["ws"]), kw.pop("edges", EDGES), **kw)


def test_direct_without_gap_or_expected(inp, monkeypatch):
    want, asked, cap = _expect(inp, up=False, gap=0, dist=False)
    c, spy = _fresh(inp), Spy(monkeypatch)
    sizes = _build(c, inp)[2]
    assert [x[0] for x in spy.calls] == ["cgcn_hic_count", "cgcn_hic_build"]
    assert spy.calls == want and spy.asked == asked and len(spy.syncs) == 1
    assert int(sizes[1]) == cap


def test_direct_with_a_gap(inp, monkeypatch):
    want, asked, cap = _expect(inp, up=False, gap=GAP, dist=True)
    assert cap < _survivors(inp)   # some records are closer than the gap
    c, spy = _fresh(inp), Spy(monkeypatch)
    sizes = _build(c, inp, min_distance_bp=GAP)[2]
    assert [x[0] for x in spy.calls] == ["cgcn_hic_count_dist", "cgcn_hic_build_dist"]
    assert spy.calls == want and spy.asked == asked and len(spy.syncs) == 1
    assert spy.calls[0][1]["min_distance_bp"] == GAP and spy.calls[1][1]["min_distance_bp"] == GAP
    assert int(sizes[1]) == cap


def test_direct_with_an_expected_vector_counts_plain_and_builds_dist(inp, monkeypatch):
    want, asked, _ = _expect(inp, up=False, gap=0, dist=True, n_bins=40, n_expected=40)
    c, spy = _fresh(inp), Spy(monkeypatch)
    _build(c, inp, norm=inp["norm"], expected=inp["expected"])
    assert [x[0] for x in spy.calls] == ["cgcn_hic_count", "cgcn_hic_build_dist"]
    assert spy.calls == want and spy.asked == asked
    assert spy.calls[1][1]["min_distance_bp"] == 0 and "min_distance_bp" not in spy.calls[0][1]


def test_an_empty_expected_vector_is_one_nan(inp, monkeypatch):
    want, asked, _ = _expect(inp, up=False, gap=0, dist=True, n_expected=1)
    c, spy = _fresh(inp), Spy(monkeypatch)
    _build(c, inp, expected=np.zeros(0))
    assert spy.calls[1][1]["n_expected"] == 1
    assert spy.calls == want and spy.asked == asked


def test_window_bp_without_gap(inp, monkeypatch):
    want, asked, cap = _expect(inp, up=True, gap=0, dist=False)
    assert cap > _survivors(inp)   # the expanded file reaches the windows between the multiples of 5000
    c, spy = _fresh(inp), Spy(monkeypatch)
    sizes = _build(c, inp, window_bp=WBP)[2]
    assert [x[0] for x in spy.calls] == ["cgcn_hic_count_up", "cgcn_hic_build_up"]
    assert spy.calls == want and spy.asked == asked
    assert spy.calls[1][1]["n_window_bins"] == int(inp["ws"][-1]) // WBP + 1
    assert int(sizes[1]) == cap


def test_window_bp_with_a_gap(inp, monkeypatch):
    want, asked, cap = _expect(inp, up=True, gap=GAP, dist=True, n_bins=40)
    c, spy = _fresh(inp), Spy(monkeypatch)
    sizes = _build(c, inp, norm=inp["norm"], window_bp=WBP, min_distance_bp=GAP)[2]
    assert [x[0] for x in spy.calls] == ["cgcn_hic_count_up_dist", "cgcn_hic_build_up_dist"]
    assert spy.calls == want and spy.asked == asked
    assert int(sizes[1]) == cap


def test_window_bp_with_an_expected_vector_counts_plain_and_builds_dist(inp, monkeypatch):
    want, asked, _ = _expect(inp, up=True, gap=0, dist=True, n_expected=40)
    c, spy = _fresh(inp), Spy(monkeypatch)
    _build(c, inp, window_bp=WBP, expected=inp["expected"])
    assert [x[0] for x in spy.calls] == ["cgcn_hic_count_up", "cgcn_hic_build_up_dist"]
    assert spy.calls == want and spy.asked == asked


def test_window_bp_equal_to_resolution_bp_is_the_direct_route(inp, monkeypatch):
    want, asked, _ = _expect(inp, up=False, gap=0, dist=False)
    c, spy = _fresh(inp), Spy(monkeypatch)
    _build(c, inp, window_bp=RES)
    assert [x[0] for x in spy.calls] == ["cgcn_hic_count", "cgcn_hic_build"]
    assert spy.calls == want and spy.asked == asked and len(spy.syncs) == 1
    spy.clear()
    _build(c, inp)   # and it shares the count of window_bp=None
    assert [x[0] for x in spy.calls] == ["cgcn_hic_build"] and not spy.syncs


@pytest.mark.parametrize("up, gap", [(False, 0), (False, GAP), (True, 0), (True, GAP)])
def test_a_window_set_is_counted_once_per_route_and_gap(inp, monkeypatch, up, gap):
    kw = dict(window_bp=WBP if up else None, min_distance_bp=gap)
    c, spy = _fresh(inp), Spy(monkeypatch)
    _build(c, inp, **kw)
    first = [x[0] for x in spy.calls]
    spy.clear()
    _build(c, inp, edges=40, **kw)                      # another budget
    _build(c, inp, norm=inp["norm"], **kw)              # another norm vector
    assert [x[0] for x in spy.calls] == [first[1]] * 2 and not spy.syncs
    assert spy.calls[0][1]["K"] == 20 and spy.calls[0][1]["capacity"] == spy.calls[1][1]["capacity"]
    spy.clear()
    other = inp["ws"][::2].copy()
    want, asked, _ = _expect(inp, up=up, gap=gap, dist=bool(gap), ws=other)
    _build(c, inp, ws=other, **kw)                      # another window set counts again
    assert spy.calls == want and spy.asked == asked and len(spy.syncs) == 1
    spy.clear()
    _build(c, inp, **kw)                                # and so does the first one, which is no longer the current set
    assert [x[0] for x in spy.calls] == first and len(spy.syncs) == 1


@pytest.mark.parametrize("gap", [0, GAP])
def test_a_position_off_the_grid_is_refused_on_the_up_route(inp, gap):
    pos1 = inp["pos1"].copy()
    pos1[5] += 1000
    pos1[9] += 2000
    c = hic.HicContacts(pos1, inp["pos2"], inp["count"], DEV)
    with pytest.raises(ValueError, match=r"^pos1 / pos2 hold 2 positions that are no multiple of resolution_bp=5000$"):
        c.build_raw(None, RES, inp["ws"], EDGES, window_bp=WBP, min_distance_bp=gap)
    assert c.survivors(inp["ws"]) == _survivors(dict(inp, pos1=pos1))   # the direct route takes them as they are
