"""k_eff_plan, k_eff_rows1 and k_eff_rows2 (csrc/cgcn_effects.hip) one by one, called through ops.effects_plan / effects_rows1 /
effects_rows2 on tables the tests fill themselves: no model, no dense layer, no head.

Exact tests: planted graphs (tests/effects_kernel_cases.py), integer tables, integer values, power-of-two row scales -- every
product, difference and fused multiply-add is exact in float32, so the device must give the numpy restatement bit for bit
(np.array_equal, no tolerance).  Every output table lies inside a larger buffer filled with a sentinel: the words before and
behind it must survive and every word inside must be written.

Float test: the normalised graphs of tests/effects_cases.py with standard-normal tables, against the float64 restatement,
element by element, within bounds that follow from the operation count (u = 2^-24), not from a measurement:
    rows1   4u (|H1[v]| + |row_scale[v] val_t| |alt - X0[u]|)
            the coefficient, the difference and the fused multiply-add round once each: 3u on the product term, u on H1[v];
            the fourth u covers the terms of second order
    rows2   (k + 4)u (|H2[v]| + row_scale[v] sum_w |val[v, w]| |X1_inst[w] - X1[w]|),   k = members of row v
            the member added first passes its own difference, k multiply-adds of the running sum and the final one: k + 2
            roundings; two u cover the second order (k < 2^9 here)"""
import functools

import numpy as np
import pytest
import torch

import effects_cases as EC
import effects_kernel_cases as KC
from chromegcn_amd import _lib, ops
from chromegcn_amd import effects as E
from chromegcn_amd import graph as G

pytestmark = pytest.mark.gpu
DEV = "cuda"
S = KC.S
DIMS = (128, 256)
GRAPHS = [(p, v, s) for p in KC.PATTERNS for v, s in KC.FIELDS]
SENTINEL = 0x7FC5A5A5          # a NaN's bits as float32 and an impossible window as int32: no result looks like it
FRONT, BACK = 64, 4096         # guard words before (keeps the table 256-byte aligned) and behind


class Guarded:
    """a table inside a flat buffer of sentinel words, itself pre-filled with them"""

    def __init__(self, shape, dtype=torch.float32):
        self.numel = int(np.prod(shape))
        self.buf = torch.full((FRONT + self.numel + BACK,), SENTINEL, dtype=torch.int32, device=DEV)
        self.t = self.buf[FRONT:FRONT + self.numel].view(dtype).view(*shape)

    def check(self):
        assert bool((self.buf[:FRONT] == SENTINEL).all()), "words before the table were written"
        assert bool((self.buf[FRONT + self.numel:] == SENTINEL).all()), "words behind the table were written"
        assert not bool((self.buf[FRONT:FRONT + self.numel] == SENTINEL).any()), "words of the table were not written"
        return self.t

    def np(self):
        return self.check().cpu().numpy()


def _up(a):
    return torch.tensor(np.asarray(a), device=DEV)


@functools.lru_cache(maxsize=None)
def _device_case(pattern, with_val, with_scale, d):
    c = KC.exact_case(pattern, with_val, with_scale, d)
    dev = {k: _up(c[k]) for k in ("windows", "X0", "H1", "X1", "H2", "alt", "offsets", "X1_inst")}
    assert dev["windows"].dtype == torch.int32 and dev["offsets"].dtype == torch.int64 and dev["X0"].dtype == torch.float32
    dev["graph"] = G.upload(c["h"], DEV)
    dev["diag"] = _up(KC.plan_host(c["h"], c["windows"])[1])
    return c, dev


def _plan(g, win):
    counts, diag = Guarded((win.numel(),), torch.int32), Guarded((win.numel(),), torch.int32)
    _lib.call("cgcn_effects_plan", n=g.n, rowptr_t=g.rowptr_t, col_t=g.col_t, n_var=int(win.numel()), windows=win,
              counts=counts.t, diag_pos=diag.t)
    return counts.np(), diag.np()


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("pattern,with_val,with_scale", GRAPHS)
def test_plan_and_the_torch_helpers(pattern, with_val, with_scale, d):
    c, dev = _device_case(pattern, with_val, with_scale, d)
    h, g, n = c["h"], dev["graph"], c["h"].n
    assert n > 256 and n % 256                                                # two workgroups, the second ragged
    planted = KC.HUB if pattern == "lanes" else KC.LONG_COL
    for windows in (c["windows"], np.array([planted] * 3 + [0, n - 1, KC.NO_IN], np.int32)):
        win = _up(windows)
        want_counts, want_diag = KC.plan_host(h, windows)
        counts, diag = _plan(g, win)
        assert np.array_equal(counts, want_counts) and np.array_equal(diag, want_diag)
        again = ops.effects_plan(g, win)                                       # the package's call; the same bits again
        assert np.array_equal(again[0].cpu().numpy(), counts) and np.array_equal(again[1].cpu().numpy(), diag)
        # the torch helpers of the composed route and of the knock-out map's scatter
        diag_rel = E._plan_torch(g)
        assert diag_rel.dtype == torch.int64 and np.array_equal(diag_rel.cpu().numpy()[windows], want_diag)
        offsets = KC.offsets_of(h, windows)
        rows = KC.rows1_host(h, c["X0"][:, :, :1], c["H1"][:, :, :1], windows, np.zeros((len(windows), S, 1)), 0)[0]
        var, k, v, pos = E._instances_torch(g, diag_rel, win, _up(offsets), int(offsets[-1]))
        rp, ct = E._host_transpose(h)
        assert np.array_equal(v.cpu().numpy(), rows)
        assert np.array_equal(pos.cpu().numpy(), E._entry_positions(rp, ct, offsets, rows, windows))
        assert np.array_equal(var.cpu().numpy(), np.repeat(np.arange(len(windows)), np.diff(offsets)))
        assert np.array_equal(k.cpu().numpy(), np.arange(offsets[-1]) - np.repeat(offsets[:-1], np.diff(offsets)))


def _rows1(dev, d, own, m0, m1, ni, with_rows=True):
    H, X = Guarded((S, ni, d)), Guarded((S, ni, d))
    rows = Guarded((ni,), torch.int32) if with_rows else None
    ops.effects_rows1(dev["graph"], dev["X0"], dev["H1"], dev["windows"][m0:], dev["alt"][m0:], dev["offsets"][m0:],
                      dev["diag"][m0:], m1 - m0, own, ni, H.t, X.t, rows.t if with_rows else None)
    return H.np(), X.np(), (rows.np() if with_rows else None)


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("pattern,with_val,with_scale", GRAPHS)
def test_rows1_every_instance_is_exact(pattern, with_val, with_scale, d):
    c, dev = _device_case(pattern, with_val, with_scale, d)
    n, off = c["h"].n, c["offsets"]
    want_rows, want_H, want_X = c["rows1", 0]
    H, X, rows = _rows1(dev, d, 0, 0, n, int(off[-1]))
    assert np.array_equal(rows, want_rows) and np.array_equal(H, want_H) and np.array_equal(X, want_X)
    H2, X2, rows2 = _rows1(dev, d, 0, 0, n, int(off[-1]))                     # repeatable
    assert H2.tobytes() == H.tobytes() and X2.tobytes() == X.tobytes() and rows2.tobytes() == rows.tobytes()
    for b, (m0, m1) in enumerate(KC.batches_of(n)):                            # the views _run_restricted passes
        a, z = int(off[m0]), int(off[m1])
        Hb, Xb, rb = _rows1(dev, d, 0, m0, m1, z - a, with_rows=b != 1)
        assert np.array_equal(Hb, want_H[:, a:z]) and np.array_equal(Xb, want_X[:, a:z])
        assert rb is None or np.array_equal(rb, want_rows[a:z])


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("pattern,with_val,with_scale", GRAPHS)
def test_rows1_own_rows_are_exact(pattern, with_val, with_scale, d):
    c, dev = _device_case(pattern, with_val, with_scale, d)
    n = c["h"].n
    want_rows, want_H, want_X = c["rows1", 1]
    H, X, rows = _rows1(dev, d, 1, 0, n, n)
    assert np.array_equal(rows, c["windows"]) and np.array_equal(rows, want_rows)
    assert np.array_equal(H, want_H) and np.array_equal(X, want_X)
    bare = np.flatnonzero(KC.plan_host(c["h"], c["windows"])[1] < 0)          # windows without a stored diagonal
    assert bare.size >= 2 and bare.size < n
    assert np.array_equal(H[:, bare], c["H1"][:, bare]) and np.array_equal(X, np.swapaxes(c["alt"], 0, 1))
    assert _rows1(dev, d, 1, 0, n, n)[0].tobytes() == H.tobytes()
    for m0, m1 in KC.batches_of(n):
        Hb, Xb, rb = _rows1(dev, d, 1, m0, m1, m1 - m0)
        assert np.array_equal(Hb, want_H[:, m0:m1]) and np.array_equal(Xb, want_X[:, m0:m1]) and np.array_equal(rb, want_rows[m0:m1])


def _rows2(dev, d, own, m0, m1, a, z, with_res=True):
    ni, no = z - a, (m1 - m0 if own else z - a)
    x1_inst = dev["X1_inst"][:, a:z].contiguous()
    H = Guarded((S, no, d))
    R = Guarded((S, no, d)) if with_res else None
    ops.effects_rows2(dev["graph"], dev["X1"], dev["H2"], dev["windows"][m0:], dev["offsets"][m0:], dev["diag"][m0:], m1 - m0,
                      own, ni, x1_inst, H.t, R.t if with_res else None)
    assert torch.equal(x1_inst, dev["X1_inst"][:, a:z])                        # its input is left alone
    return H.np(), (R.np() if with_res else None)


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("own", (0, 1))
@pytest.mark.parametrize("pattern,with_val,with_scale", GRAPHS)
def test_rows2_is_exact(pattern, with_val, with_scale, own, d):
    c, dev = _device_case(pattern, with_val, with_scale, d)
    n, off = c["h"].n, c["offsets"]
    want_H, want_R = c["rows2", own]
    if own:
        assert np.array_equal(want_R, c["X1_inst"][:, off[:-1]])
    else:
        assert np.array_equal(want_R, c["X1_inst"])
    H, R = _rows2(dev, d, own, 0, n, 0, int(off[-1]))
    assert np.array_equal(H, want_H) and np.array_equal(R, want_R)
    H2, R2 = _rows2(dev, d, own, 0, n, 0, int(off[-1]))                        # repeatable
    assert H2.tobytes() == H.tobytes() and R2.tobytes() == R.tobytes()
    if not own:
        assert np.array_equal(_rows2(dev, d, 0, 0, n, 0, int(off[-1]), with_res=False)[0], want_H)
    for m0, m1 in KC.batches_of(n):
        a, z = int(off[m0]), int(off[m1])
        Hb, Rb = _rows2(dev, d, own, m0, m1, a, z)
        lo, hi = (m0, m1) if own else (a, z)
        assert np.array_equal(Hb, want_H[:, lo:hi]) and np.array_equal(Rb, want_R[:, lo:hi])


@pytest.mark.parametrize("d", DIMS)
def test_identities_hold_bit_for_bit_on_random_floats(d):
    """alt = X0[u] leaves H1[v], X1_inst = the gathered rows of X1 leaves H2[v]: a zero difference times anything finite
    added to h is h"""
    h = EC.host_graph("both")
    g, n = G.upload(h, DEV), h.n
    gen = torch.Generator(device=DEV).manual_seed(9 + d)
    X0, H1, X1, H2 = (torch.randn(S, n, d, device=DEV, generator=gen) for _ in range(4))
    windows = np.arange(n, dtype=np.int32)
    win = _up(windows)
    offsets_h, rows_h = E.effect_rows_host(h, windows)
    offsets, total = _up(offsets_h), int(offsets_h[-1])
    diag = _up(KC.plan_host(h, windows)[1])
    alt = X0.transpose(0, 1).contiguous()                                      # [n, S, d]: alt[m] = X0[:, m]
    H, X, rows = Guarded((S, total, d)), Guarded((S, total, d)), Guarded((total,), torch.int32)
    ops.effects_rows1(g, X0, H1, win, alt, offsets, diag, n, 0, total, H.t, X.t, rows.t)
    assert np.array_equal(rows.np(), rows_h)
    idx = rows.t.to(torch.int64)
    assert torch.equal(H.check(), H1[:, idx]) and torch.equal(X.check(), X0[:, idx])
    for own in (0, 1):
        no = n if own else total
        Ho, R = Guarded((S, no, d)), Guarded((S, no, d))
        ops.effects_rows2(g, X1, H2, win, offsets, diag, n, own, total, X1[:, idx].contiguous(), Ho.t, R.t)
        sel = win.to(torch.int64) if own else idx
        assert torch.equal(Ho.check(), H2[:, sel]) and torch.equal(R.check(), X1[:, sel])


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("kind", EC.GRAPH_KINDS)
def test_float_rows_stay_inside_the_derived_bounds(kind, d):
    c = KC.float_case(kind, d)
    g = G.upload(c["h"], DEV)
    dev = {k: _up(c[k]) for k in ("windows", "X0", "H1", "X1", "H2", "alt", "offsets", "X1_inst")}
    M, total = len(c["windows"]), int(c["offsets"][-1])
    counts, diag = ops.effects_plan(g, dev["windows"])
    assert np.array_equal(np.diff(c["offsets"]), counts.cpu().numpy())
    H, X, rows = Guarded((S, total, d)), Guarded((S, total, d)), Guarded((total,), torch.int32)
    ops.effects_rows1(g, dev["X0"], dev["H1"], dev["windows"], dev["alt"], dev["offsets"], diag, M, 0, total, H.t, X.t, rows.t)
    assert np.array_equal(rows.np(), c["rows"])
    Ho = Guarded((S, total, d))
    ops.effects_rows2(g, dev["X1"], dev["H2"], dev["windows"], dev["offsets"], diag, M, 0, total, dev["X1_inst"], Ho.t, None)
    worst = []
    for got, want, bound in ((H.np(), c["H_inst"], c["bound1"]), (Ho.np(), c["H_out"], c["bound2"])):
        assert bound.min() > 0
        worst.append(float((np.abs(got.astype(np.float64) - want) / bound).max()))
    moved = float(np.abs(c["H_inst"] - c["H1"][:, c["rows"]]).max()), float(np.abs(c["H_out"] - c["H2"][:, c["rows"]]).max())
    print("effects kernels %s d=%d: worst error / bound  rows1 %.3f  rows2 %.3f  (largest update %.3f, %.3f)"
          % (kind, d, worst[0], worst[1], moved[0], moved[1]))
    assert moved[0] > 1e3 * c["bound1"].max() and moved[1] > 1e3 * c["bound2"].max()      # echoing H1 / H2 cannot pass
    assert worst[0] <= 1.0 and worst[1] <= 1.0, worst
