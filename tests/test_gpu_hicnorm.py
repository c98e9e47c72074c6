"""KR / VC / SQRTVC norm vectors computed on the device (csrc/cgcn_hicnorm.hip, chromegcn_amd/hicnorm.py) against the numpy
restatement that tests/test_hicnorm_host.py ties to the definitions.  Structure (rowptr, col, NaN positions, graphs) is
compared exactly; sums of integer counts bit for bit; fractional sums and Knight-Ruiz within bounds that come from the
number format and from the host restatement alone (each test's docstring says which).  Every figure is printed before it is
asserted."""
import functools
import math

import numpy as np
import pytest
import torch

from chromegcn_amd import HicNormError, build_hic_graph, build_hic_graph_host, hic, hic_norm_vector, hicnorm

import hicnorm_cases as HC

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -53
ALL_LONG, ALL_SHORT = 0, 1 << 30   # cgcn_hicnorm_spmv's long_row_nnz: every row by the workgroup / every row by 16 lanes
ROUTED = ("n65", "n257", "fullrow")


@functools.lru_cache(maxsize=None)
def contacts(name):
    c = HC.case(name)
    return hic.HicContacts(c["pos1"], c["pos2"], c["count"], DEV)


def device_matrix(name):
    c = HC.case(name)
    return contacts(name).contact_matrix(c["res"], c["n_bins"])


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def largest_merge(c):
    i, j = c["pos1"].astype(np.int64) // c["res"], c["pos2"].astype(np.int64) // c["res"]
    return int(np.unique(np.minimum(i, j) * c["n_bins"] + np.maximum(i, j), return_counts=True)[1].max())


@functools.lru_cache(maxsize=None)
def big_case():
    return HC.hic_like(20000, 4400000, 31, dup_share=0.1, n_empty=150)   # 3 020 136 records once the pairs are distinct


def check_matrix(c, m, a, what):
    assert (m.n, m.nnz) == (a.shape[0], a.nnz), what
    assert np.array_equal(m.rowptr.cpu().numpy(), a.indptr) and np.array_equal(m.col[:m.nnz].cpu().numpy(), a.indices), what
    val = m.val[:m.nnz].cpu().numpy()
    if np.all(c["count"] == np.floor(c["count"])):
        assert same_bits(val, a.data), what                        # integer counts below 2^53: exact in any order
    else:
        k = largest_merge(c)
        err = float(np.abs(val / a.data - 1.0).max())
        print("%s: largest merge %d, val relative error %.3g (bound %.3g)" % (what, k, err, (k - 1) * U))
        assert err <= (k - 1) * U, what                            # a reordered sum of k non-negative terms


@pytest.mark.parametrize("name", list(HC.CASES))
def test_aggregated_csr_vc_and_sqrtvc(name):
    """CSR: exact structure, values bit-equal for integer counts and within (k - 1) 2^-53 for fractional ones (k = the most
    records merged into one entry).  VC: bit-equal / within (t - 1) 2^-53, t = the entries of the row.  SQRTVC: bit-equal to
    numpy.sqrt of the device's own VC (IEEE square root, no fast-math).  Two device aggregations: the same bits."""
    c, a = HC.case(name), HC.host_matrix(name)
    m = device_matrix(name)
    check_matrix(c, m, a, name)
    again = hicnorm.aggregate_contacts(contacts(name).pos1, contacts(name).pos2, contacts(name).count, c["res"], c["n_bins"])
    assert torch.equal(again.rowptr, m.rowptr) and torch.equal(again.col, m.col)
    assert torch.equal(again.val.view(torch.int64), m.val.view(torch.int64))
    assert torch.equal(again.vc.view(torch.int64), m.vc.view(torch.int64)) and torch.equal(again.row_nnz, m.row_nnz)
    vc_host, nnz_host = hicnorm._row_stats_host(a)
    assert np.array_equal(m.row_nnz.cpu().numpy(), nnz_host)
    vc = contacts(name).norm_vector("VC", c["res"], c["n_bins"]).cpu().numpy()
    assert np.array_equal(np.flatnonzero(np.isnan(vc)), c["empty"])
    keep = ~np.isnan(vc)
    if np.all(c["count"] == np.floor(c["count"])):
        assert same_bits(vc[keep], vc_host[keep])
    else:
        t = np.diff(a.indptr)[keep]
        err = np.abs(vc[keep] / vc_host[keep] - 1.0)
        print("%s: VC relative error %.3g of at most %.3g" % (name, err.max(), ((t.max() - 1) * U)))
        assert np.all(err <= np.maximum(t - 1, 0) * U)             # a reordered sum of t non-negative terms
    sq = contacts(name).norm_vector("SQRTVC", c["res"], c["n_bins"]).cpu().numpy()
    assert np.array_equal(np.isnan(sq), np.isnan(vc)) and same_bits(sq[keep], np.sqrt(vc[keep]))


def test_three_million_records_over_twenty_thousand_bins():
    """the multi-block sort and scan paths: 3 020 136 records, 6 040 272 keys, 23 595 tiles of 256"""
    c = big_case()
    assert c["pos1"].size >= 3000000
    a = hicnorm.contact_matrix_host(c["pos1"], c["pos2"], c["count"], c["res"], c["n_bins"])
    dev = hic.HicContacts(c["pos1"], c["pos2"], c["count"], DEV)
    m = dev.contact_matrix(c["res"], c["n_bins"])
    check_matrix(c, m, a, "big")
    vc_host, nnz_host = hicnorm._row_stats_host(a)
    vc = dev.norm_vector("VC", c["res"], c["n_bins"]).cpu().numpy()
    assert np.array_equal(np.flatnonzero(np.isnan(vc)), c["empty"]) and same_bits(vc[~np.isnan(vc)], vc_host[vc_host > 0])
    assert np.array_equal(m.row_nnz.cpu().numpy(), nnz_host)


def test_default_n_bins_bad_counts_and_a_small_n_bins():
    c = HC.case("n65")
    top = int(max(c["pos1"].max(), c["pos2"].max())) // c["res"] + 1
    dev = contacts("n65")
    assert dev.contact_matrix(c["res"]).n == top
    assert dev.norm_vector("VC", c["res"]).shape == (top,) and dev.norm_vector("VC", c["res"], top + 70).shape == (top + 70,)
    assert dev.norm_vector("VC", c["res"]) is dev.norm_vector("VC", c["res"])                  # kept per argument tuple
    with pytest.raises(ValueError, match="n_bins"):
        dev.norm_vector("VC", c["res"], top - 1)
    for bad in (-1.0, float("nan"), float("inf")):
        cnt = c["count"].copy()
        cnt[17] = bad
        with pytest.raises(ValueError, match="finite and non-negative"):
            hic_norm_vector(c["pos1"], c["pos2"], cnt, "SQRTVC", c["res"], device=DEV)
    with pytest.raises(ValueError, match="none of"):
        dev.norm_vector("kr", c["res"])
    empty = hic.HicContacts(np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0), DEV)
    assert empty.norm_vector("KR", 1000).shape == (0,) and empty.norm_vector("VC", 1000, 5).isnan().all()


@pytest.mark.parametrize("route", [-1, ALL_LONG, ALL_SHORT])
@pytest.mark.parametrize("name", ROUTED + ("n1000",))
def test_spmv_routes(name, route):
    """y = m o (A (m o x o p)) with positive x and p against scipy in float64.  Both sides add t non-negative products of two
    roundings each, t = the entries of the row: each is within (t + 1) 2^-53 of the exact sum, so they differ by at most
    2 (t + 2) 2^-53 relative.  The same call twice gives the same bits on every route."""
    a, m = HC.host_matrix(name), device_matrix(name)
    rng = np.random.default_rng(5)
    x, p = rng.uniform(0.5, 2.0, m.n), rng.uniform(0.1, 3.0, m.n)
    mask = (rng.random(m.n) < 0.8).astype(np.float64)
    xd, pd, md = (torch.from_numpy(v).to(DEV) for v in (x, p, mask))
    t = np.diff(a.indptr)
    for use_m, use_x, use_p in ((True, True, True), (False, True, False), (False, False, False)):
        f = (mask if use_m else 1.0) * (x if use_x else 1.0) * (p if use_p else 1.0) * np.ones(m.n)
        want = (mask if use_m else 1.0) * (a @ f)
        y = hicnorm.spmv(m, x=xd if use_x else None, p=pd if use_p else None, mask=md if use_m else None, long_row_nnz=route)
        y2 = hicnorm.spmv(m, x=xd if use_x else None, p=pd if use_p else None, mask=md if use_m else None, long_row_nnz=route)
        assert torch.equal(y.view(torch.int64), y2.view(torch.int64))
        got = y.cpu().numpy()
        assert np.array_equal(got == 0, want == 0)
        nz = want != 0
        err = np.abs(got[nz] / want[nz] - 1.0)
        print("%s route %d: spmv relative error %.3g" % (name, route, err.max() if err.size else 0.0))
        assert np.all(err <= 2 * (t[nz] + 2) * U)


def device_kr(name, tol, **kw):
    c = HC.case(name)
    v, info = contacts(name).norm_vector("KR", c["res"], c["n_bins"], tol=tol, return_info=True, **kw)
    with np.errstate(divide="ignore"):
        return 1.0 / v.cpu().numpy(), info


KR_RUNS = [(n, -1) for n in HC.KR_CASES] + [(n, r) for n in ROUTED for r in (ALL_LONG, ALL_SHORT)]


@pytest.mark.parametrize("tol", [1e-6, 1e-10])
@pytest.mark.parametrize("name,route", KR_RUNS)
def test_kr_residual_recomputed_on_the_host(name, route, tol):
    """max_i |x_i (A_S x)_i - 1| <= tol + (k_row + 2) 2^-52 with the host's matrix in float64: the device stops at a 2-norm of
    tol, which bounds the largest component; the second term is the rounding of this recomputation over the longest kept row"""
    x, info = device_kr(name, tol, long_row_nnz=route)
    worst, k_row = HC.kr_residual(HC.host_matrix(name), x)
    host = HC.host_kr(name, tol)
    print("%s route %d tol %g: device residual %.3g recomputed max %.3g, %d products (host %d), %d outer, %d host syncs"
          % (name, route, tol, info["residual"], worst, info["mvp"], host[1]["mvp"], info["outer"], info["host_syncs"]))
    assert info["converged"] is True and info["residual"] <= tol
    assert np.array_equal(np.isnan(x), np.isnan(host[0]))
    assert worst <= tol + (k_row + 2) * 2.0 ** -52
    assert info["kept"] == host[1]["kept"] and info["excluded"] == 0 and info["min_row_nnz"] == 1


@pytest.mark.parametrize("name", HC.KR_CASES)
def test_kr_closeness_to_the_solution(name):
    """x* = the host restatement at tol 1e-13.  kappa = the largest ||x / x* - 1||_inf / residual among the host's own stops
    at tol 1e-4, 1e-6, 1e-8, 1e-10; the device at 1e-6 and 1e-10 must lie within 4 kappa of ITS residual: a different fusion
    order stops at a different point under the same tolerance, and the four host stops sample that spread.  kappa never sees
    the device.  A residual of exactly 0 (possible at one bin, where the yardstick's own is 0) leaves no spread to scale: x and
    x* then both round x (A x) to 1, which pins each within 2^-53 of the root, so they differ by at most 2^-52 relative."""
    xs, istar = HC.host_kr(name, 1e-13)
    assert istar["converged"], istar
    keep = ~np.isnan(xs)
    kappa = 0.0
    for tol in (1e-4, 1e-6, 1e-8, 1e-10):
        xh, ih = HC.host_kr(name, tol)
        kappa = max(kappa, float(np.abs(xh[keep] / xs[keep] - 1.0).max()) / ih["residual"])
    for tol in (1e-6, 1e-10):
        x, info = device_kr(name, tol)
        dist = float(np.abs(x[keep] / xs[keep] - 1.0).max())
        print("%s tol %g: kappa %.3g, device ||x/x* - 1|| %.3g, residual %.3g, ratio %.3g"
              % (name, tol, kappa, dist, info["residual"], dist / info["residual"]))
        assert dist <= (4 * kappa * info["residual"] if info["residual"] > 0 else 2.0 ** -52)


def test_cap_excluded_rows_and_determinism():
    c = HC.case("n257")
    dev = contacts("n257")
    v, info = dev.norm_vector("KR", c["res"], c["n_bins"], max_mvp=5, kr_retry=False, return_info=True)
    assert info["converged"] is False and info["mvp"] == 5 and np.isfinite(info["residual"]) and info["residual"] > 1e-6
    v, info = dev.norm_vector("KR", c["res"], c["n_bins"], max_mvp=5, return_info=True)          # the ladder, every run capped
    host = hicnorm.kr_balance_host(HC.host_matrix("n257"), max_mvp=5)
    assert info["converged"] is False and info["ladder"] == host[1]["ladder"] and len(info["ladder"]) == 6
    assert np.array_equal(np.isnan(v.cpu().numpy()), np.isnan(host[0]))
    gc, ws = HC.graph_case()
    with pytest.raises(HicNormError) as e:
        hic.HicContacts(gc["pos1"], gc["pos2"], gc["count"], DEV).build("KR", gc["res"], ws, HC.GRAPH_EDGES, norm_args=dict(max_mvp=5))
    assert e.value.info["converged"] is False
    # rows with fewer than three entries are left out, exactly the host's
    c63 = HC.case("n63_leafy")
    xh, ih = hicnorm.kr_balance_host(HC.host_matrix("n63_leafy"), min_row_nnz=3, kr_retry=False)
    v, info = contacts("n63_leafy").norm_vector("KR", c63["res"], c63["n_bins"], min_row_nnz=3, kr_retry=False, return_info=True)
    x = 1.0 / v.cpu().numpy()
    assert ih["excluded"] == 3 and (info["kept"], info["excluded"]) == (ih["kept"], ih["excluded"]) and info["converged"]
    assert np.array_equal(np.isnan(x), np.isnan(xh))
    worst, k_row = HC.kr_residual(HC.host_matrix("n63_leafy"), x)
    assert worst <= 1e-6 + (k_row + 2) * 2.0 ** -52
    # two runs, the same bits
    for name in ("n1000", "fullrow"):
        m = device_matrix(name)
        a, ia = hicnorm.kr_balance_device(m, tol=1e-10)
        b, ib = hicnorm.kr_balance_device(m, tol=1e-10)
        assert torch.equal(a.view(torch.int64), b.view(torch.int64)) and ia == ib


@pytest.mark.parametrize("tol", [1e-6, 1e-10])
@pytest.mark.parametrize("name", sorted(set(HC.UPPER_CLIP + HC.LOWER_CLIP)))
def test_kr_clips_the_steps_the_host_clips(name, tol):
    """OP_CLIP with either flag inside a whole run, the two step-length minima of OP_Y read, an inner loop left without a
    flip of the parity: the device reports the host's (lower, upper) pair -- tests/test_hicnorm_host.py shows that no run
    comes within 1e-6 of another branch -- and the run meets test_kr_residual_recomputed_on_the_host's criterion"""
    x, info = device_kr(name, tol)
    host = HC.host_kr(name, tol)
    worst, k_row = HC.kr_residual(HC.host_matrix(name), x)
    print("%s tol %g: clips %s (host %s), device residual %.3g recomputed max %.3g, %d products (host %d)"
          % (name, tol, info["clips"], host[1]["clips"], info["residual"], worst, info["mvp"], host[1]["mvp"]))
    assert info["clips"] == host[1]["clips"]
    assert (info["clips"][1] >= 1) == (name in HC.UPPER_CLIP) and (info["clips"][0] >= 1) == (name in HC.LOWER_CLIP)
    assert info["converged"] is True and info["residual"] <= tol and np.array_equal(np.isnan(x), np.isnan(host[0]))
    assert worst <= tol + (k_row + 2) * 2.0 ** -52


@pytest.mark.timeout(600)
@pytest.mark.parametrize("tol", [1e-6, 1e-10])
@pytest.mark.parametrize("name", HC.KR_LARGE)
def test_kr_beyond_one_trip_of_the_vector_step(name, tol):
    """70 001 bins: 274 partials, k_hn_finish folds them in two trips; 262 401 bins: 1026 tiles for a grid of 1024, k_hn_vec
    strides.  The criterion of test_kr_residual_recomputed_on_the_host."""
    c = HC.case(name)
    blocks = -(-c["n_bins"] // 256)
    assert blocks > 256 and (blocks > 1024) == (name == "n262401")
    x, info = device_kr(name, tol)
    host = HC.host_kr(name, tol)
    worst, k_row = HC.kr_residual(HC.host_matrix(name), x)
    print("%s tol %g: device residual %.3g recomputed max %.3g, %d products (host %d), clips %s (host %s)"
          % (name, tol, info["residual"], worst, info["mvp"], host[1]["mvp"], info["clips"], host[1]["clips"]))
    assert info["converged"] is True and info["residual"] <= tol
    assert np.array_equal(np.isnan(x), np.isnan(host[0])) and info["kept"] == host[1]["kept"] == c["n_bins"] - c["empty"].size
    assert worst <= tol + (k_row + 2) * 2.0 ** -52
    assert info["clips"] == host[1]["clips"] and (info["clips"][1] >= 1) == (name in HC.UPPER_CLIP)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("name", ["n70001", "n262401"])
def test_vc_and_row_nnz_beyond_65536_bins(name):
    c, a = HC.case(name), HC.host_matrix(name)
    vc_host, nnz_host = hicnorm._row_stats_host(a)
    m = device_matrix(name)
    assert np.array_equal(m.row_nnz.cpu().numpy(), nnz_host)
    vc = contacts(name).norm_vector("VC", c["res"], c["n_bins"]).cpu().numpy()
    assert np.array_equal(np.flatnonzero(np.isnan(vc)), c["empty"]) and c["empty"].size > 30
    assert same_bits(vc[~np.isnan(vc)], vc_host[vc_host > 0])                    # integer counts: exact in any order


# ----------------------------------------------------------------------------------------------
# cgcn_hicnorm_kr_step, one operation at a time
# ----------------------------------------------------------------------------------------------
STEP_SIZES = [1, 31, 256, 257, 65536, 65537, 262144, 262145, 300001]
REC_SUMS = {(HC.OP_RES, 0): ("rk", "rk"), (HC.OP_RES, 8): ("rk", "rk"), (HC.OP_FIRST, 0): ("rk", "z"), (HC.OP_W, 2): ("p", "w"),
            (HC.OP_Y, 7): ("rk'", "z'")}     # (op, slot): the two vectors whose product the slot sums; ' = the other parity


def _random_state(n, seed):
    """a state of seeded vectors and scalars: x, y, v away from 0, w so that x w and x y w stay below 1.7, a mask with 15 %
    zeros, alpha = 0.1, every other scalar its own value (a slot read in place of another one shows)"""
    rng = np.random.default_rng(seed)
    vec = {"m": (rng.random(n) < 0.85).astype(np.float64), "x": rng.uniform(0.5, 2.0, n), "v": rng.uniform(0.5, 2.0, n),
           "p": rng.standard_normal(n), "w": rng.uniform(0.1, 0.4, n), "y0": rng.uniform(0.5, 2.0, n), "y1": rng.uniform(0.5, 2.0, n),
           "rk0": 0.3 * rng.standard_normal(n), "rk1": 0.3 * rng.standard_normal(n), "z0": rng.standard_normal(n),
           "z1": rng.standard_normal(n)}
    rec = np.zeros(32)
    rec[:12] = [1.3, 0.7, 2.1, 0.4, 2.6, 0.61, 0.23, 0.9, 1.7, 0.1, 5.0, 6.0]
    rec[12:] = 100.0 + np.arange(20)                                  # the slots no step writes
    return vec, rec


def _trip_positions(n):
    """four rows: the first, the last (alone in a second trip at n = 65 537 and 262 145), one that only the second trip of
    k_hn_vec's grid stride reaches (rows from 262 144) where there is one, and one whose partial only the second trip of
    k_hn_finish's fold reaches (partials from 256: rows from 65 536); without such rows, two in the middle"""
    if n < 31:
        return None
    fold = 65536 + 1000 if n > 65536 + 1001 else n // 2 + 1
    stride = 262144 + (n - 1 - 262144) // 2 if n > 262144 + 1 else 65536 + (n - 1 - 65536) // 2 if n > 65536 + 1 else n // 2
    assert len({0, n - 1, stride, fold}) == 4
    return [0, n - 1, stride, fold]


def _planted_y_state(n, seed, variant, c):
    """the state of an OP_Y step whose four extremes are each decided by one known row.  The other kept rows have
    y in (0.5, 2) and alpha p in (-0.2, 0.3): ynew in (0.3, 2.3), step lengths to the lower bound above 2, none to the upper
    one.  Rows outside the mask hold y = 0.5, alpha p = -50 or 50 and must not count.  variant 2: alpha p >= 0 on every kept
    row and no ynew above 3: both step lengths stay +inf."""
    vec, rec = _random_state(n, seed)
    rng = np.random.default_rng(seed + 1)
    alpha, y = rec[9], "y%d" % c
    ap = rng.uniform(-0.2, 0.3, n) if variant < 2 else rng.uniform(0.0, 0.3, n)
    off = vec["m"] == 0.0
    ap[off] = np.where(rng.random(int(off.sum())) < 0.5, -50.0, 50.0)
    vec[y][off] = 0.5
    pos = _trip_positions(n)
    want = {}
    if pos is not None and variant < 2:
        i_min, i_max, i_lo, i_up = pos if variant == 0 else (pos[2], pos[3], pos[1], pos[0])
        vec["m"][[i_min, i_max, i_lo, i_up]] = 1.0
        vec[y][[i_min, i_max, i_lo, i_up]] = [0.5, 2.0, 0.2, 2.9]
        ap[[i_min, i_max, i_lo, i_up]] = [-0.45, 2.5, -0.13, 0.5]     # ynew 0.05, 4.5, 0.07, 3.4; lengths 0.889, 0.4, 0.769, 0.2
        want = {3: i_min, 4: i_max, 5: i_lo, 6: i_up}
    vec["p"] = ap / alpha
    return vec, rec, want


def _pack(n, vec, rec):
    from chromegcn_amd import _lib
    nbytes = _lib.query("cgcn_hicnorm_kr_state_bytes", n=n)
    ns = (n + 31) & ~31
    st = np.zeros(nbytes // 8)
    st[:32] = rec
    for k, name in enumerate(HC.KR_VECTORS):
        st[hicnorm._HDR + k * ns:hicnorm._HDR + k * ns + n] = vec[name]
    return st, nbytes, ns


def _check_step(n, op, flag, c, vec, rec, vc, nnz, worst):
    from chromegcn_amd import _lib
    st, nbytes, ns = _pack(n, vec, rec)
    first = torch.from_numpy(st).to(DEV)
    second = first.clone()
    for state in (first, second):
        _lib.call("cgcn_hicnorm_kr_step", n=n, op=op, flag=flag, parity=c, vc=vc[1], row_nnz=nnz[1], state=state, state_bytes=nbytes)
    assert torch.equal(first.view(torch.int64), second.view(torch.int64)), (op, flag, c, "two calls, two results")
    got = first.cpu().numpy()
    gvec = {name: got[hicnorm._HDR + k * ns:hicnorm._HDR + k * ns + n] for k, name in enumerate(HC.KR_VECTORS)}
    pad = np.concatenate([got[hicnorm._HDR + k * ns + n:hicnorm._HDR + (k + 1) * ns] for k in range(len(HC.KR_VECTORS))])
    assert not pad.any(), (op, flag, c, "a write behind a vector's n rows")
    out, slots = HC.kr_step_host(op, flag, c, vec, rec, vc[0], nnz[0])
    what = (n, op, flag, c)
    for name in HC.KR_VECTORS:
        if name not in out:
            assert same_bits(gvec[name], vec[name]), (what, name, "written, and the step does not own it")
            continue
        val, mag = out[name]
        err, bound = np.abs(gvec[name] - val), 2.0 ** -52 * mag
        quotient = op == HC.OP_Y and name == "z%d" % (c ^ 1)     # held to the device's own new rk below, bit for bit
        assert quotient or np.all(err <= bound), (what, name, float(err.max()))
        k = ("quotient" if quotient else "vector", op)
        worst[k] = max(worst.get(k, 0.0), float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0)
    other = {"rk'": gvec["rk%d" % (c ^ 1)], "z'": gvec["z%d" % (c ^ 1)], "rk": gvec["rk%d" % c], "z": gvec["z%d" % c],
             "p": gvec["p"], "w": gvec["w"]}
    keep = vec["m"] != 0.0
    if op == HC.OP_Y:       # Z of the new parity is one IEEE division of the device's own new rk
        assert same_bits(other["z'"], np.where(keep, other["rk'"] / vec["v"], 0.0)), what
    for slot in range(32):
        if slot not in slots:
            assert got[slot] == rec[slot], (what, slot, "written, and the step does not own it")
            continue
        val, mag = slots[slot]
        if (op, slot) in REC_SUMS:          # a sum: of the products of the vectors the device itself holds
            a, b = REC_SUMS[(op, slot)]
            terms = other[a] * other[b]
            exact, size = math.fsum(terms.tolist()), math.fsum(np.abs(terms).tolist())
            err = abs(got[slot] - exact)
            k = ("sum", op)
            worst[k] = max(worst.get(k, 0.0), err / ((n + 1) * U * size) if size else 0.0)
            assert err <= (n + 1) * U * size, (what, slot, got[slot], exact)
        elif op == HC.OP_W and slot == 9:   # alpha: one IEEE division by the device's own p . w
            assert got[9] == (rec[7] if flag else rec[0]) / got[2], what
        elif op == HC.OP_Y:                 # a minimum or a maximum
            assert got[slot] == val if np.isinf(val) else abs(got[slot] - val) <= 4 * U * abs(val), (what, slot, got[slot], val)
            if not np.isinf(val):
                worst[("extreme", op)] = max(worst.get(("extreme", op), 0.0), abs(got[slot] / val - 1.0) / (4 * U))
        else:                               # a count or a copy
            assert got[slot] == val, (what, slot, got[slot], val)
    return slots


@pytest.mark.timeout(600)
@pytest.mark.parametrize("n", STEP_SIZES)
def test_kr_step_one_operation_at_a_time(n):
    """Every operation of cgcn_hicnorm_kr_step (OP_MASK, OP_RES and OP_W and OP_CLIP with either flag, OP_FIRST, OP_DIR, OP_Y)
    at either parity, once from a seeded state, every vector and every record slot against HC.kr_step_host -- the float64
    numpy restatement that tests/test_hicnorm_host.py ties to _kr_run_host's listing.  n = 65 537 gives 257 partials
    (k_hn_finish's second trip), n > 262 144 more tiles than the grid (k_hn_vec's stride).
    Bounds, from the number format (the compiler may contract a multiply-add):  a vector element within 2^-52 x the sum of the
    magnitudes of its terms; a quotient (Z = rk / v) bit for bit from the device's own operands -- OP_Y's new Z divides the new rk,
    whose contracted multiply-add may differ from the restatement's by one rounding that the division then carries, up to
    2.5 x 2^-52 (|rk| + |alpha w|) / |v| against the restatement's own Z (observed: up to 1.95 of 2^-52 x those terms, at n = 262 145): its
    figure is printed, the assertion is the exact one;  a sum
    within (n + 1) 2^-53 x the sum of the magnitudes of its terms -- the terms being the products of the vectors the device
    holds after the step, which are the ones it added (against the restatement's own vectors the comparison would also
    carry the element errors above);  a minimum or maximum within 4 x 2^-53 relative;  counts, copied scalars, +inf and
    everything the step does not own: bit for bit.  The same call on the same state twice: the same bits."""
    rng = np.random.default_rng(n)
    vc_h = np.where(rng.random(n) < 0.8, rng.uniform(1.0, 50.0, n), 0.0)
    nnz_h = rng.integers(0, 5, n).astype(np.int32)
    vc, nnz = (vc_h, torch.from_numpy(vc_h).to(DEV)), (nnz_h, torch.from_numpy(nnz_h).to(DEV))
    worst = {}
    for c in (0, 1):
        vec, rec = _random_state(n, 1000 + n + c)
        for op, flag in HC.KR_STEPS:
            if op != HC.OP_Y:
                slots = _check_step(n, op, flag, c, vec, rec, vc, nnz, worst)
                if op == HC.OP_MASK and n >= 31:
                    assert 0 < slots[10][0] < slots[11][0] < n                               # kept rows, non-empty rows
        for variant in (0, 1, 2):
            vec_y, rec_y, want = _planted_y_state(n, 2000 + n + c, variant, c)
            slots = _check_step(n, HC.OP_Y, 0, c, vec_y, rec_y, vc, nnz, worst)
            if variant == 2:
                assert np.isinf(slots[5][0]) and np.isinf(slots[6][0]) and slots[4][0] < 3.0
            elif want:       # the planted rows decide: the restatement's extremes are theirs
                y, ap = vec_y["y%d" % c], rec_y[9] * vec_y["p"]
                assert slots[3][0] == (y + ap)[want[3]] < 0.1 and slots[4][0] == (y + ap)[want[4]] > 3.0
                assert slots[5][0] == ((0.1 - y) / ap)[want[5]] and slots[6][0] == ((3.0 - y) / ap)[want[6]]
    print("kr_step n=%d: worst error / bound %s" % (n, ", ".join("%s op %d: %.3g" % (k[0], k[1], v) for k, v in sorted(worst.items()))))


def test_string_norms_end_to_end(tmp_path):
    """build_hic_graph(norm=kind) == build_hic_graph_host with the HOST's vector: exact, no edge left out -- the generator's
    values are apart at the threshold (tests/test_hicnorm_host.py checks the gap)"""
    c, ws = HC.graph_case()
    dev = hic.HicContacts(c["pos1"], c["pos2"], c["count"], DEV)
    for kind in ("KR", "VC", "SQRTVC"):
        nv, _ = hicnorm.hic_norm_vector_host(c["pos1"], c["pos2"], c["count"], kind, c["res"], c["n_bins"])
        want = build_hic_graph_host(c["pos1"], c["pos2"], c["count"], nv, c["res"], ws, HC.GRAPH_EDGES)
        _, raw = build_hic_graph(dev, None, None, kind, c["res"], ws, HC.GRAPH_EDGES, device=DEV, return_raw=True)
        assert np.array_equal(raw.indptr, want.indptr) and np.array_equal(raw.indices, want.indices), kind
        assert want.nnz > 0
    for chrom, seed in (("chrA", 41), ("chrB", 42)):
        g, w = HC.graph_case(seed)
        hic.save_contacts_cache(hic.contact_cache_path(str(tmp_path), chrom),
                                hic.HostContacts(g["pos1"], g["pos2"], g["count"], {}, g["res"], w))
    with pytest.raises(ValueError, match="holds no 'KR' norm vector"):
        hic.graphs_from_contact_caches(str(tmp_path), ["chrA", "chrB"], HC.GRAPH_EDGES, "KR", device=DEV)
    for kind in ("KR", "SQRTVC"):
        graphs = hic.graphs_from_contact_caches(str(tmp_path), ["chrA", "chrB"], HC.GRAPH_EDGES, kind, device=DEV, compute_norm=True)
        assert sorted(graphs) == ["chrA", "chrB"] and all(g.n == 90 and g.nnz > 0 for g in graphs.values())


def test_entry_points_reject_bad_arguments_before_any_launch():
    from chromegcn_amd import _lib
    m = device_matrix("n65")
    dev = contacts("n65")
    sizes = torch.zeros(4, dtype=torch.int64, device=DEV)
    need = _lib.query("cgcn_hicnorm_workspace_bytes", M=dev.M, n_bins=0)
    wsp = torch.empty(need, dtype=torch.uint8, device=DEV)
    args = dict(M=dev.M, pos1=dev.pos1, pos2=dev.pos2, count=dev.count, resolution_bp=1000, n_bins=0, workspace=wsp,
                workspace_bytes=need, sizes=sizes)
    assert _lib.query("cgcn_hicnorm_count", **{**args, "workspace_bytes": need - 1}) == -4
    assert _lib.query("cgcn_hicnorm_count", **{**args, "resolution_bp": 0}) == -1
    assert _lib.query("cgcn_hicnorm_count", **{**args, "count": None}) == -1
    assert _lib.query("cgcn_hicnorm_count", **{**args, "M": 2 ** 31}) == -2 and _lib.query("cgcn_hicnorm_workspace_bytes", M=2 ** 31, n_bins=0) == 0
    y = torch.empty(m.n, dtype=torch.float64, device=DEV)
    assert _lib.query("cgcn_hicnorm_spmv", n=m.n, rowptr=m.rowptr, col=m.col, val=None, mask=None, x=None, p=None, y=y, long_row_nnz=-1) == -1
    nbytes = _lib.query("cgcn_hicnorm_kr_state_bytes", n=m.n)
    state = torch.zeros(nbytes // 8, dtype=torch.float64, device=DEV)
    step = dict(n=m.n, op=0, flag=1, parity=0, vc=m.vc, row_nnz=m.row_nnz, state=state, state_bytes=nbytes)
    assert _lib.query("cgcn_hicnorm_kr_step", **{**step, "op": 7}) == -1 and _lib.query("cgcn_hicnorm_kr_step", **{**step, "parity": 2}) == -1
    assert _lib.query("cgcn_hicnorm_kr_step", **{**step, "state_bytes": nbytes - 8}) == -4
    assert _lib.query("cgcn_hicnorm_kr_step", **{**step, "vc": None}) == -1
    assert _lib.query("cgcn_hicnorm_kr_state_bytes", n=0) == 0
    assert _lib.query("cgcn_hicnorm_vector", n=m.n, kind=3, vc=m.vc, state=None, out=y) == -1
    assert _lib.query("cgcn_hicnorm_vector", n=m.n, kind=2, vc=m.vc, state=None, out=y) == -1


def test_a_capacity_below_the_entry_count_cuts_the_matrix_off():
    """cgcn_hicnorm_fill with half the entries' room: the first `capacity` entries, every row pointer clamped to it, the row
    statistics over what is left, the true entry count in sizes[0]; nothing behind the arrays is touched (a sentinel stays)"""
    from chromegcn_amd import _lib
    c, a, dev = HC.case("n257"), HC.host_matrix("n257"), contacts("n257")
    n, cap = c["n_bins"], a.nnz // 2
    need = _lib.query("cgcn_hicnorm_workspace_bytes", M=dev.M, n_bins=n)
    wsp = torch.empty(need, dtype=torch.uint8, device=DEV)
    rowptr = torch.zeros(n + 1, dtype=torch.int32, device=DEV)
    col = torch.full((cap + 64,), -7, dtype=torch.int32, device=DEV)
    val = torch.full((cap + 64,), -7.0, dtype=torch.float64, device=DEV)
    vc, nnz = torch.zeros(n, dtype=torch.float64, device=DEV), torch.zeros(n, dtype=torch.int32, device=DEV)
    sizes = torch.zeros(4, dtype=torch.int64, device=DEV)
    _lib.call("cgcn_hicnorm_fill", M=dev.M, pos1=dev.pos1, pos2=dev.pos2, count=dev.count, resolution_bp=c["res"], n_bins=n,
              capacity=cap, workspace=wsp, workspace_bytes=need, rowptr=rowptr, col=col, val=val, vc=vc, row_nnz=nnz, sizes=sizes)
    assert sizes.tolist()[:2] == [a.nnz, 0]
    want_ptr = np.minimum(a.indptr, cap)
    assert np.array_equal(rowptr.cpu().numpy(), want_ptr)
    assert np.array_equal(col[:cap].cpu().numpy(), a.indices[:cap]) and same_bits(val[:cap].cpu().numpy(), a.data[:cap])
    assert bool((col[cap:] == -7).all()) and bool((val[cap:] == -7.0).all())
    import scipy.sparse as sp
    cut = sp.csr_matrix((a.data[:cap], a.indices[:cap], want_ptr), shape=a.shape)
    vc_cut, nnz_cut = hicnorm._row_stats_host(cut)
    assert same_bits(vc.cpu().numpy(), vc_cut) and np.array_equal(nnz.cpu().numpy(), nnz_cut)   # integer counts: exact
