"""CPU checks of tests/effects_kernel_cases.py: the planted graphs hold what they promise (the builders assert it), the
numpy restatements of k_eff_plan / k_eff_rows1 / k_eff_rows2 agree with the package's host enumeration and with dense float64
algebra, and the exact cases tell ten deliberately wrong rules from the right one."""
import numpy as np
import pytest

import effects_kernel_cases as KC
from chromegcn_amd import effects as E

GRAPHS = [(p, v, s) for p in KC.PATTERNS for v, s in KC.FIELDS]


def _dense(h):
    """A = diag(row_scale) Ahat in float64"""
    val, scale = KC._fields(h)
    a = np.zeros((h.n, h.n))
    a[np.repeat(np.arange(h.n), np.diff(h.rowptr)), h.col] = val
    return scale[:, None] * a


@pytest.mark.parametrize("pattern,with_val,with_scale", GRAPHS)
def test_planted_graphs_hold_their_conditions(pattern, with_val, with_scale):
    h = KC.host_graph(pattern, with_val, with_scale)                          # (the builder asserts the planted conditions)
    assert 300 <= h.n <= 450 and (h.val is not None) == with_val and (h.row_scale is not None) == with_scale
    assert h.symmetric == (pattern == "lanes" and not with_val)
    for v in range(h.n):
        row = h.col[h.rowptr[v]:h.rowptr[v + 1]]
        assert (np.diff(row) > 0).all()
    if with_scale:
        assert set(np.unique(h.row_scale)) == set(KC.SCALES.tolist())
    if with_val:                                                                # val_t[pos(v, u)] != val[pos(u, v)]
        rp, ct = E._host_transpose(h)
        at = h.ahat().T.tocsr()
        at.sort_indices()
        assert np.array_equal(at.indices, ct)
        a = h.ahat().toarray()
        n_both = 0
        for u in range(h.n):
            for p in range(rp[u], rp[u + 1]):
                v = ct[p]
                assert at.data[p] == a[v, u]
                if v != u and a[u, v] != 0:
                    n_both += 1
                    assert at.data[p] != a[u, v]
        assert n_both >= 20


@pytest.mark.parametrize("pattern,with_val,with_scale", GRAPHS)
def test_plan_and_rows_match_the_host_enumeration(pattern, with_val, with_scale):
    h = KC.host_graph(pattern, with_val, with_scale)
    rng = np.random.RandomState(3)
    for windows in (np.arange(h.n), np.array([KC.HUB] * 3 + [0, h.n - 1]), rng.randint(0, h.n, 50)):
        counts, diag = KC.plan_host(h, windows)
        offsets, rows = E.effect_rows_host(h, windows)
        assert np.array_equal(np.diff(offsets), counts) and np.array_equal(KC.offsets_of(h, windows), offsets)
        z = np.zeros((KC.S, h.n, 1))
        got_rows = KC.rows1_host(h, z, z, windows, np.zeros((len(windows), KC.S, 1)), 0)[0]
        assert got_rows.dtype == np.int32 and np.array_equal(got_rows, rows)
        assert np.array_equal(KC.rows1_host(h, z, z, windows, np.zeros((len(windows), KC.S, 1)), 1)[0], windows)
        rp, ct = E._host_transpose(h)
        pos = E._entry_positions(rp, ct, offsets, rows, windows)
        for m, u in enumerate(windows):
            assert diag[m] == (pos[offsets[m]] - rp[u] if pos[offsets[m]] >= 0 else -1)
            assert (pos[offsets[m] + 1:offsets[m + 1]] >= 0).all()


@pytest.mark.parametrize("pattern,with_val,with_scale", GRAPHS)
def test_restatements_match_dense_algebra(pattern, with_val, with_scale):
    h = KC.host_graph(pattern, with_val, with_scale)
    n, d = h.n, 3
    A = _dense(h)
    rng = np.random.RandomState(4)
    X0, X1 = rng.randn(KC.S, n, d), rng.randn(KC.S, n, d)
    H1, H2 = A @ X0, A @ X1
    planted = [KC.HUB, KC.EMPTY, KC.ALONE, KC.VGAP, KC.V2] if pattern == "lanes" else [KC.NO_IN, KC.NO_OUT, KC.LONG_ROW, KC.LONG_COL]
    windows = np.array(planted + [0, n - 1, 7, 7] + rng.randint(0, n, 30).tolist())
    alt = rng.randn(len(windows), KC.S, d)
    offsets = KC.offsets_of(h, windows)
    rows, Hi, Xi = KC.rows1_host(h, X0, H1, windows, alt, 0)
    _, Hi_own, Xi_own = KC.rows1_host(h, X0, H1, windows, alt, 1)
    X1_inst = rng.randn(KC.S, rows.shape[0], d)
    Ho, Xr = KC.rows2_host(h, X1, H2, windows, X1_inst, 0)
    Ho_own, Xr_own = KC.rows2_host(h, X1, H2, windows, X1_inst, 1)
    assert np.array_equal(Xr, X1_inst)
    for m, u in enumerate(windows):
        a, b = offsets[m], offsets[m + 1]
        Xp = X0.copy()
        Xp[:, u] = alt[m]
        np.testing.assert_allclose(Hi[:, a:b], (A @ Xp)[:, rows[a:b]], rtol=0, atol=1e-12)
        assert np.array_equal(Xi[:, a:b], Xp[:, rows[a:b]])
        assert np.array_equal(Hi_own[:, m], Hi[:, a]) and np.array_equal(Xi_own[:, m], alt[m])
        Xp = X1.copy()
        Xp[:, rows[a:b]] = X1_inst[:, a:b]
        np.testing.assert_allclose(Ho[:, a:b], (A @ Xp)[:, rows[a:b]], rtol=0, atol=1e-11)
        assert np.array_equal(Ho_own[:, m], Ho[:, a]) and np.array_equal(Xr_own[:, m], X1_inst[:, a])


def test_exact_cases_are_exact_and_batches_start_past_zero():
    for pattern, with_val, with_scale in GRAPHS:
        case = KC.exact_case(pattern, with_val, with_scale, 128)                # (asserts 4 x largest partial sum < 2^24)
        assert 4 * case["largest"] < 2 ** 24
        n = case["h"].n
        assert n > 256 and n % 256 != 0                                        # k_eff_plan: two workgroups, the last ragged
        for m0, m1 in KC.batches_of(n)[1:]:
            assert m0 > 0 and case["offsets"][m0] > 0 and m1 > m0
        for key in (("rows1", 0), ("rows1", 1), ("rows2", 0), ("rows2", 1)):
            assert all(np.abs(a).max() <= case["largest"] for a in case[key] if a.dtype != np.int32)
    c = KC.code(np.arange(33 ** 3), 128)
    assert c.min() == -16 and c.max() == 16 and np.unique(c[0, :, :3], axis=0).shape[0] == 33 ** 3


def _differs(a, b):
    return a.shape != b.shape or not np.array_equal(a, b)


@pytest.mark.parametrize("rule", KC.WRONG_RULES)
def test_the_exact_cases_tell_a_wrong_rule_apart(rule):
    """Every wrong rule changes at least one element of the exact cases' answers; the rules that speak of a graph field
    change one on every graph that has the field."""
    hits = []
    for pattern, with_val, with_scale in GRAPHS:
        c = KC.exact_case(pattern, with_val, with_scale, 128)
        h, win = c["h"], c["windows"]
        if rule == "ignore_offsets0":
            for m0, m1 in KC.batches_of(h.n)[1:]:
                g = KC.rows_ignoring_offsets0(c["offsets"], m0, m1)
                right = np.arange(c["offsets"][m0], c["offsets"][m1])
                assert (g < 0).any()                                          # rows the kernel would leave unwritten
                ok = g >= 0
                hits.append(True)
                if ok.any():                                                  # and the written ones hold another instance's row
                    for H in (c["rows1", 0][1], c["rows2", 0][0]):
                        assert _differs(H[:, g[ok]], H[:, right[ok]])
            continue
        for own in (0, 1):
            rows, Hi, Xi = KC.rows1_host(h, c["X0"], c["H1"], win, c["alt"], own, wrong=rule)
            Ho, Xr = KC.rows2_host(h, c["X1"], c["H2"], win, c["X1_inst"], own, wrong=rule)
            d1 = _differs(Hi, c["rows1", own][1]) or _differs(Xi, c["rows1", own][2]) or _differs(rows, c["rows1", own][0])
            d2 = _differs(Ho, c["rows2", own][0]) or _differs(Xr, c["rows2", own][1])
            hits.append(d1 or d2)
            if rule == "no_shift":
                assert d1 == (own == 0) and _differs(rows, c["rows1", own][0]) == (own == 0)
            if rule == "inverse_ge":
                assert d2 and not d1
            if rule == "val_for_val_t":
                assert not d2 and (d1 == with_val if own == 0 else with_val or not d1)
            if rule == "scale_u":                                              # instance 0: v is u, nothing to confuse
                assert (d1, d2) == ((with_scale, with_scale) if own == 0 else (False, False))
            if rule == "strand0_alt":
                assert d1
            if rule == "nodiag_update":
                assert d1 and not d2
            if rule in ("drop_lane63", "drop_last_partial", "skip_after_empty"):
                assert not d1 and (d2 or own == 1)
                if pattern == "lanes":                                         # the planted row VGAP under window HUB shows it alone
                    k = int(c["offsets"][KC.HUB] + list(c["rows1", 0][0][c["offsets"][KC.HUB]:c["offsets"][KC.HUB + 1]]).index(KC.VGAP))
                    assert own == 1 or _differs(Ho[:, k], c["rows2", 0][0][:, k])
    assert any(hits)
