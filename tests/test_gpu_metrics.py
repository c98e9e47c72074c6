"""Device metrics (cgcn_multilabel_metrics) against the per-label values recorded from the reference's
utils/metrics.py helpers (G5) and against the oracle (scikit-learn, the reference's dependency) on larger
random inputs.  Curve arithmetic is fp64 on the device; results are returned as fp32."""
import numpy as np
import pytest
import torch

from chromegcn_amd import metrics as M
from oracle import chromegcn_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAIRS = [("ref_auroc", "auroc"), ("ref_aupr", "aupr"), ("ref_fdr", "recall_at_fdr"), ("ref_ap", "average_precision")]


def test_metrics_match_reference_golden(golden):
    z = golden("g5_metrics.npz")
    m = M.multilabel_metrics(torch.from_numpy(z["preds"]).to(DEV), torch.from_numpy(z["targets"]).to(DEV))
    for k_ref, k in PAIRS:
        np.testing.assert_allclose(m[k].cpu().numpy(), z[k_ref], rtol=2e-6, atol=2e-7, equal_nan=True, err_msg=k)


@pytest.mark.parametrize("n,C", [(1, 3), (65, 2), (5000, 103), (40000, 17)])
def test_metrics_match_oracle(n, C):
    rng = np.random.RandomState(n + C)
    tg = (rng.rand(n, C) < rng.rand(C) * 0.5).astype(np.float32)
    pr = (rng.rand(n, C) * 0.7 + 0.3 * tg * rng.rand(n, C)).astype(np.float32)
    pr[:, 0] = np.round(pr[:, 0], 2)   # heavy ties: runs of equal scores cross the 4096-element chunk boundaries
    if C > 1:
        pr[:, 1] = 0.5                 # one run spanning every chunk
    if C > 2:
        pr[:, 2] = np.round(pr[:, 2], 1)
    want = O.multilabel_metrics_np(tg.astype(np.float64), pr)
    got = M.multilabel_metrics(torch.from_numpy(pr).to(DEV), torch.from_numpy(tg).to(DEV))
    for k in ("auroc", "aupr", "recall_at_fdr", "average_precision"):
        np.testing.assert_allclose(got[k].cpu().numpy(), want[k], rtol=3e-6, atol=3e-7, equal_nan=True, err_msg=k)


def test_metrics_order_signed_scores_and_signed_zero():
    """Scores need not be probabilities: logits (both signs), -0.0 / +0.0 (one threshold for sklearn) and subnormals
    must rank exactly as numbers do (the sort key is an order-preserving integer image of the float)."""
    rng = np.random.RandomState(5)
    n, C = 3000, 5
    tg = (rng.rand(n, C) < 0.3).astype(np.float32)
    pr = (rng.randn(n, C) * 3 + tg).astype(np.float32)
    pr[::7, 0] = 0.0
    pr[3::7, 0] = -0.0
    pr[::5, 1] = np.float32(1e-42) * rng.randint(-3, 4, size=pr[::5, 1].shape).astype(np.float32)  # subnormals of both signs
    pr[:, 2] = -np.abs(pr[:, 2])       # all negative
    want = O.multilabel_metrics_np(tg.astype(np.float64), pr)
    got = M.multilabel_metrics(torch.from_numpy(pr).to(DEV), torch.from_numpy(tg).to(DEV))
    for k in ("auroc", "aupr", "recall_at_fdr", "average_precision"):
        np.testing.assert_allclose(got[k].cpu().numpy(), want[k], rtol=3e-6, atol=3e-7, equal_nan=True, err_msg=k)


def test_compute_metrics_keys_and_aggregation(golden):
    z = golden("g5_metrics.npz")
    out = M.compute_metrics(torch.from_numpy(z["preds"]), torch.from_numpy(z["targets"]), 1.25, None, 0.5)
    for k in ["mAP", "meanAUC", "medianAUC", "allAUC", "allFDR", "meanAUPR", "medianAUPR", "allAUPR", "meanFDR",
              "medianFDR", "loss", "time"]:  # utils/evals.py:107-118
        assert k in out
    assert abs(out["meanAUC"] - np.nanmean(z["ref_auroc"])) < 1e-6
    assert abs(out["meanAUPR"] - np.mean(z["ref_aupr"])) < 1e-6
    assert abs(out["meanFDR"] - np.mean(z["ref_fdr"])) < 1e-6
    assert abs(out["mAP"] - np.mean(z["ref_ap"])) < 1e-6
    assert out["loss"] == 1.25 and out["time"] == 0.5
    with pytest.raises(RuntimeError):
        M.multilabel_metrics(torch.zeros(4, 2), torch.zeros(4, 2))


@pytest.mark.parametrize("n,C", [(1, 1), (2, 3), (63, 2), (4096, 3), (4097, 5), (70000, 9), (12289, 103), (37, 2600)])
def test_probability_path_equals_general_path_bit_for_bit(n, C):
    """cgcn_multilabel_metrics_nonneg (32-bit keys, the library's own segmented radix sort: partial last tiles, one-tile and
    many-tile labels, the flat pack and -- thousands of labels -- the tile pack) against cgcn_multilabel_metrics (64-bit keys,
    one device-wide sort) on probabilities: same curve kernels behind both, so the results must be the same bits."""
    g = torch.Generator().manual_seed(n * 131 + C)
    tg = (torch.rand(n, C, generator=g) < 0.2).float()
    pr = torch.sigmoid(torch.randn(n, C, generator=g) * 2 + tg)
    pr[:, 0] = (pr[:, 0] * 50).round() / 50          # heavy ties
    if C > 1:
        pr[:, 1] = 0.5 + pr[:, 1] * 1e-4             # every key in a handful of top digits (skew)
    if C > 2:
        pr[::3, 2] = 0.0                             # exact zeros, and -0.0 folded onto them
        pr[1::3, 2] = -0.0
    pr, tg = pr.to(DEV), tg.to(DEV)
    fast = M._metrics_raw(pr, tg, 0.5, nonneg=True).cpu()
    slow = M._metrics_raw(pr, tg, 0.5, nonneg=False).cpu()
    assert int(fast[4 * C:].view(torch.int32).item()) == 0
    a, b = fast[:4 * C].numpy(), slow[:4 * C].numpy()
    assert np.array_equal(a, b, equal_nan=True), np.abs(np.nan_to_num(a) - np.nan_to_num(b)).max()


def test_probability_path_on_views_that_are_not_16_byte_aligned():
    g = torch.Generator().manual_seed(3)
    n, C = 5000, 7
    buf_p = torch.rand(n * C + 3, generator=g).to(DEV)
    buf_t = (torch.rand(n * C + 3, generator=g) < 0.3).float().to(DEV)
    pr, tg = buf_p[1:1 + n * C].view(n, C), buf_t[3:3 + n * C].view(n, C)   # storage offsets 4 and 12 bytes
    assert pr.data_ptr() % 16 != 0 and pr.is_contiguous()
    fast = M._metrics_raw(pr, tg, 0.5, nonneg=True).cpu()[:4 * C].numpy()
    want = O.multilabel_metrics_np(tg.cpu().numpy().astype(np.float64), pr.cpu().numpy())
    for j, k in enumerate(("auroc", "aupr", "recall_at_fdr", "average_precision")):
        np.testing.assert_allclose(fast[j * C:(j + 1) * C], want[k], rtol=3e-6, atol=3e-7, equal_nan=True, err_msg=k)


def test_probability_path_reports_scores_that_are_not_probabilities():
    pr = torch.rand(300, 4)
    pr[17, 2] = -0.25
    tg = (torch.rand(300, 4) < 0.5).float()
    flat = M._metrics_raw(pr.to(DEV), tg.to(DEV), 0.5, nonneg=True)
    assert int(flat[16:].view(torch.int32).item()) != 0
    pr[17, 2] = float("nan")
    flat = M._metrics_raw(pr.to(DEV), tg.to(DEV), 0.5, nonneg=True)
    assert int(flat[16:].view(torch.int32).item()) != 0


def test_metrics_of_an_empty_split_are_nan_on_both_paths():
    pr, tg = torch.zeros(0, 5, device=DEV), torch.zeros(0, 5, device=DEV)
    for nonneg in (True, False):
        flat = M._metrics_raw(pr, tg, 0.5, nonneg=nonneg).cpu()
        assert torch.isnan(flat[:20]).all()
        if nonneg:
            assert int(flat[20:].view(torch.int32).item()) == 0


def test_recall_at_fdr_when_precision_is_exactly_the_cutoff():
    """Positives and negatives alternating down the ranking: precision is EXACTLY 1/2 at every even depth (tp = fp), so
    1 - precision <= 0.5 holds there with equality in the reference's float64 quotient (utils/metrics.py:153-154) -- at
    depths such as 14, 22, 26, 28 a product with a reciprocal lands one ulp below 1/2 and would miss the deepest such
    point.  Every label stops alternating at another depth; scores are distinct."""
    C, n = 40, 400
    tg = np.zeros((n, C), dtype=np.float32)
    for c in range(C):
        k = 1 + c                                   # c-th label alternates P N for 2 (c + 1) elements, then only negatives
        tg[0:2 * k:2, c] = 1.0
    pr = np.repeat(np.linspace(0.99, 0.01, n, dtype=np.float32)[:, None], C, axis=1)
    want = O.multilabel_metrics_np(tg.astype(np.float64), pr)
    got = M.multilabel_metrics(torch.from_numpy(pr).to(DEV), torch.from_numpy(tg).to(DEV))
    np.testing.assert_allclose(got["recall_at_fdr"].cpu().numpy(), want["recall_at_fdr"], rtol=1e-6, atol=0, err_msg="recall_at_fdr")
    assert (want["recall_at_fdr"] == 1.0).all()     # the deepest point with tp = fp holds every positive
    for k in ("auroc", "aupr", "average_precision"):
        np.testing.assert_allclose(got[k].cpu().numpy(), want[k], rtol=3e-6, atol=3e-7, equal_nan=True, err_msg=k)


# ---------------------------------------------------------------------------------------------------------------------------
# Past 64 chunks per label, every pack width, every cutoff, saturated scores, workspace discipline.  The inputs are built (and
# pinned on the CPU tier, tests/test_metrics_cases_host.py) in tests/metrics_cases.py; the reference is the oracle throughout.
# ---------------------------------------------------------------------------------------------------------------------------
import functools  # noqa: E402

import metrics_cases as MC  # noqa: E402
from chromegcn_amd import _lib  # noqa: E402

KEYS = ("auroc", "aupr", "recall_at_fdr", "average_precision")


def _dev(a):
    return torch.from_numpy(a).to(DEV)


def _oracle(targets, preds, cutoff=0.5, cols=None):
    if cols is not None:
        targets, preds = targets[:, cols], preds[:, cols]
    return O.multilabel_metrics_np(np.ascontiguousarray(targets, dtype=np.float64), np.ascontiguousarray(preds), cutoff)


def _assert_matches_oracle(got, want, cols=None, exact_fdr=()):
    """got: per-label arrays of the device (dict of tensors, or the flat [4 C] result); want: the oracle's, on `cols` of them.
    exact_fdr: positions (in `want`) of labels built to have an exact recall at FDR: rtol = 1e-6, atol = 0 there."""
    for j, k in enumerate(KEYS):
        if isinstance(got, dict):
            g = got[k].cpu().numpy()
        else:
            C = got.size // 4
            g = got[j * C:(j + 1) * C]
        if cols is not None:
            g = g[cols]
        w = want[k]
        with np.errstate(invalid="ignore", divide="ignore"):
            print("%s: max |diff| %.3g, max rel %.3g" % (k, np.nanmax(np.abs(g - w), initial=0.0),
                                                         np.nanmax(np.abs(g - w) / np.abs(w), initial=0.0)))
        np.testing.assert_allclose(g, w, rtol=3e-6, atol=3e-7, equal_nan=True, err_msg=k)
        if k == "recall_at_fdr" and len(exact_fdr):
            e = list(exact_fdr)
            np.testing.assert_allclose(g[e], w[e], rtol=1e-6, atol=0, err_msg=k + " (exact labels)")


def _bits(pr, tg, cutoff, nonneg):
    """the [4 C] results of one path as int32 bit patterns"""
    C = pr.shape[1]
    flat = M._metrics_raw(pr, tg, cutoff, nonneg=nonneg).cpu()
    if nonneg:
        assert int(flat[4 * C:].view(torch.int32).item()) == 0
    return flat[:4 * C].numpy().view(np.int32).copy()


def _assert_paths_agree(pr, tg, cutoff=0.5):
    fast, slow = _bits(pr, tg, cutoff, True), _bits(pr, tg, cutoff, False)
    assert np.array_equal(fast, slow), np.flatnonzero(fast != slow)
    return fast.view(np.float32)


@functools.lru_cache(maxsize=None)
def _many():
    case = MC.many_chunk_case()
    return _dev(case["preds"]), _dev(case["targets"]), _oracle(case["targets"], case["preds"])


@functools.lru_cache(maxsize=None)
def _two():
    case = MC.two_group_case()
    return _dev(case["preds"]), _dev(case["targets"]), _oracle(case["targets"], case["preds"])


def test_many_chunks_three_prefix_groups():
    """130 chunks per label: the second and third step of k_metrics_prefix with a carried curve point (a whole group
    without a run end between them), three chunks per lane in k_metrics_final, T = 130 tiles in k_rs_scan."""
    pr, tg, want = _many()
    _assert_matches_oracle(M.multilabel_metrics(pr, tg), want, exact_fdr=(3, 4, 5))
    assert want["recall_at_fdr"][3] == 1.0
    assert want["recall_at_fdr"][4] == MC.MANY_E_TOP / (MC.MANY_E_TOP + MC.MANY_E_BOTTOM)
    _assert_matches_oracle(_assert_paths_agree(pr, tg), want, exact_fdr=(3, 4, 5))


def test_two_prefix_groups_and_degenerate_labels():
    """65 chunks: the smallest n with a second prefix step; all-positive, all-negative, one-positive and one-negative labels"""
    pr, tg, want = _two()
    got = M.multilabel_metrics(pr, tg)
    _assert_matches_oracle(got, want, exact_fdr=(0, 1, 2, 3))
    assert torch.isnan(got["auroc"][:2]).all() and got["aupr"][:2].tolist() == [1.0, 0.5]
    assert got["recall_at_fdr"][:2].tolist() == [1.0, 0.0] and got["average_precision"][:2].tolist() == [1.0, 0.0]
    _assert_matches_oracle(_assert_paths_agree(pr, tg), want, exact_fdr=(0, 1, 2, 3))


def _mixed_inputs(n, C, seed):
    """probabilities as in test_probability_path_equals_general_path_bit_for_bit: heavy ties in column 0, skewed top digits
    in column 1, signed zeros in column 2 (CPU tensors)"""
    g = torch.Generator().manual_seed(seed)
    tg = (torch.rand(n, C, generator=g) < 0.2).float()
    pr = torch.sigmoid(torch.randn(n, C, generator=g) * 2 + tg)
    pr[:, 0] = (pr[:, 0] * 50).round() / 50
    pr[:, 1] = 0.5 + pr[:, 1] * 1e-4
    pr[::3, 2] = 0.0
    pr[1::3, 2] = -0.0
    return pr, tg


@pytest.mark.parametrize("n,C", [(MC.PACK_N, C) for C in sorted(MC.PACK_CASES)] + MC.PACK_TWO_TILES)
def test_every_pack_width(n, C):
    """rows per block R = 128, 64, 32, 16, 8, 4 of the flat pack and the tile pack, at the values of C on either side of every
    switch (tests/metrics_cases.py: PACK_CASES) and at the product's C = 256; the last block is partial for every R"""
    pr, tg = _mixed_inputs(n, C, n * 131 + C)
    fast = _assert_paths_agree(pr.to(DEV), tg.to(DEV))
    cols = MC.oracle_columns(C)
    _assert_matches_oracle(fast, _oracle(tg.numpy(), pr.numpy(), cols=cols), cols=cols)


@pytest.mark.parametrize("C", [256, 2457])
def test_pack_widths_on_views_that_are_not_16_byte_aligned(C):
    """VEC = 1 at R = 32 and R = 4"""
    n = MC.PACK_N
    p0, t0 = _mixed_inputs(n, C, 7 * C)
    buf_p, buf_t = torch.zeros(n * C + 3), torch.zeros(n * C + 3)
    buf_p[1:1 + n * C] = p0.reshape(-1)
    buf_t[3:3 + n * C] = t0.reshape(-1)
    buf_p, buf_t = buf_p.to(DEV), buf_t.to(DEV)
    pr, tg = buf_p[1:1 + n * C].view(n, C), buf_t[3:3 + n * C].view(n, C)   # storage offsets 4 and 12 bytes
    assert pr.data_ptr() % 16 == 4 and tg.data_ptr() % 16 == 12 and pr.is_contiguous() and tg.is_contiguous()
    fast = _assert_paths_agree(pr, tg)
    cols = MC.oracle_columns(C)
    _assert_matches_oracle(fast, _oracle(t0.numpy(), p0.numpy(), cols=cols), cols=cols)
    assert np.array_equal(fast.view(np.int32), _bits(p0.to(DEV), t0.to(DEV), 0.5, True))   # the aligned read, same bits


@pytest.mark.parametrize("C", sorted(MC.BAD_CASES))
def test_bad_word_at_width(C):
    """one negative score in the last row's last column (a partial block), one NaN in the first element: R = 32 and the tile pack"""
    n = MC.PACK_N
    pr, tg = _mixed_inputs(n, C, 11 * C)
    bad = lambda p: int(M._metrics_raw(p.to(DEV), tg.to(DEV), 0.5, nonneg=True)[4 * C:].view(torch.int32).item())  # noqa: E731
    assert bad(pr) == 0
    neg = pr.clone()
    neg[n - 1, C - 1] = -0.25
    assert bad(neg) != 0
    nan = pr.clone()
    nan[0, 0] = float("nan")
    assert bad(nan) != 0
    cols = MC.oracle_columns(C)
    assert C - 1 in cols
    _assert_matches_oracle(M.multilabel_metrics(neg.to(DEV), tg.to(DEV)), _oracle(tg.numpy(), neg.numpy(), cols=cols), cols=cols)


@functools.lru_cache(maxsize=None)
def _cutoff_inputs():
    preds, targets = MC.cutoff_case()
    pr, tg = _dev(preds), _dev(targets)
    return preds, targets, pr, tg, _bits(pr, tg, 0.5, True).reshape(4, -1)


@pytest.mark.parametrize("cutoff", MC.CUTOFFS)
def test_recall_at_every_fdr_cutoff(cutoff):
    """The C ABI takes the cutoff as a float: the oracle gets the same float32 value.  0: only points with precision 1
    qualify; 1: every point does, the last one wins; 1/4 and 1/2: equality on the three_to_one / alternating labels, which
    alone decides the labels built with the negative first."""
    preds, targets, pr, tg, at_half = _cutoff_inputs()
    want = _oracle(targets, preds, cutoff=float(np.float32(cutoff)))
    got = M.multilabel_metrics(pr, tg, cutoff)
    _assert_matches_oracle(got, want, exact_fdr=range(8))
    fast = _assert_paths_agree(pr, tg, cutoff).view(np.int32).reshape(4, -1)
    assert np.array_equal(fast[[0, 1, 3]], at_half[[0, 1, 3]])      # AUROC, AUPR and AP do not depend on the cutoff
    r = got["recall_at_fdr"].cpu().numpy()
    P = targets.sum(axis=0).astype(np.float64)
    alt, t31, (top_col, top) = sorted(MC.CUTOFF_ALT), sorted(MC.CUTOFF_3TO1), MC.CUTOFF_TOP_POSITIVES
    if cutoff == 1.0:
        assert (r == 1.0).all()                                      # the all-negative label included
    elif cutoff == 0.0:                                              # the last point with precision 1 (none: negative first)
        lead = np.array([0.0 if MC.CUTOFF_ALT[c][1] else 1.0 for c in alt])
        np.testing.assert_allclose(r[alt], lead / P[alt], rtol=1e-6, atol=0)
        lead = np.array([0.0 if MC.CUTOFF_3TO1[c][1] else 3.0 for c in t31])
        np.testing.assert_allclose(r[t31], lead / P[t31], rtol=1e-6, atol=0)
        np.testing.assert_allclose(r[top_col], top / P[top_col], rtol=1e-6, atol=0)
    if cutoff >= 0.25:
        assert (r[t31] == 1.0).all()                                 # the deepest 4 k point holds every positive
    else:                                                            # negative first: nothing is above precision 3/4
        assert all(r[c] == 0.0 for c in t31 if MC.CUTOFF_3TO1[c][1])
    if cutoff >= 0.5:
        assert (r[alt] == 1.0).all()
    if cutoff < 1.0:
        assert r[MC.CUTOFF_ALL_NEGATIVE] == 0.0


def test_saturated_probabilities_match_oracle():
    """runs of exactly 1.0f, 0.0f and +-0 longer than a chunk, and subnormal probabilities, against scikit-learn"""
    preds, targets = MC.saturated_case()
    pr, tg = _dev(preds), _dev(targets)
    want = _oracle(targets, preds)
    _assert_matches_oracle(M.multilabel_metrics(pr, tg), want)
    _assert_matches_oracle(_assert_paths_agree(pr, tg), want)


def test_results_are_deterministic():
    """"a fixed order => deterministic": the same input twice on each path, identical bits"""
    pr, tg, _ = _many()
    for nonneg in (True, False):
        assert np.array_equal(_bits(pr, tg, 0.5, nonneg), _bits(pr, tg, 0.5, nonneg))


GUARD = 4096


def _guarded(nbytes, offset, fill):
    """(buffer, start): a uint8 device buffer filled with `fill` that holds `nbytes` at buffer[start:], start = `offset`
    bytes past a 256-byte boundary, with at least GUARD bytes before and after"""
    buf = torch.full((nbytes + 2 * GUARD + 512,), fill, dtype=torch.uint8, device=DEV)
    start = GUARD + (-(buf.data_ptr() + GUARD)) % 256 + offset
    assert (buf.data_ptr() + start) % 256 == offset and start >= GUARD and buf.numel() - (start + nbytes) >= GUARD
    return buf, start


def _guards_intact(buf, start, nbytes, fill=0xA5):
    return bool((buf[:start] == fill).all()) and bool((buf[start + nbytes:] == fill).all())


@pytest.mark.parametrize("n,C", [(4097, 5), (301, 373)])
@pytest.mark.parametrize("nonneg", [True, False])
def test_workspace_out_and_bad_are_all_the_kernels_touch(n, C, nonneg):
    """A caller-owned workspace of exactly cgcn_metrics_workspace_bytes, at a 256-aligned address and 8 bytes past one, full
    of stale bytes, with guards on either side; guards around `out` and `bad` too.  The guards stay as they were and the
    results are those of a run with a zeroed workspace."""
    p0, t0 = _mixed_inputs(n, C, 17 * n + C)
    pr, tg = p0.to(DEV), t0.to(DEV)
    ws_bytes = _lib.query("cgcn_metrics_workspace_bytes", n=n, C=C)
    assert ws_bytes > 0
    fn = "cgcn_multilabel_metrics_nonneg" if nonneg else "cgcn_multilabel_metrics"
    results = {}
    for offset in (0, 8):
        for fill in (0x00, 0xA5):
            ws, ws0 = _guarded(ws_bytes, offset, 0xA5)
            ws[ws0:ws0 + ws_bytes] = fill
            out, out0 = _guarded(16 * C, 0, 0xA5)
            bad, bad0 = _guarded(4, 0, 0xA5)
            args = dict(n=n, C=C, probs=pr, targets=tg, fdr_cutoff=0.5, out=out.data_ptr() + out0,
                        workspace=ws.data_ptr() + ws0, workspace_bytes=ws_bytes)
            if nonneg:
                args["bad"] = bad.data_ptr() + bad0
            _lib.call(fn, **args)
            torch.cuda.synchronize()
            assert _guards_intact(ws, ws0, ws_bytes), (offset, fill, "workspace")
            assert _guards_intact(out, out0, 16 * C), (offset, fill, "out")
            assert _guards_intact(bad, bad0, 4), (offset, fill, "bad")
            if nonneg:
                assert bad[bad0:bad0 + 4].cpu().view(torch.int32).item() == 0
            results[offset, fill] = out[out0:out0 + 16 * C].cpu().numpy().view(np.int32).copy()
    first = results[0, 0x00]
    assert all(np.array_equal(first, r) for r in results.values())
    assert np.array_equal(first, _bits(pr, tg, 0.5, nonneg))
    cols = MC.oracle_columns(C)
    _assert_matches_oracle(first.view(np.float32), _oracle(t0.numpy(), p0.numpy(), cols=cols), cols=cols)


def test_compute_metrics_skips_undefined_labels_like_nanmean():
    case = MC.two_group_case()
    _, _, want = _two()
    C = case["preds"].shape[1]
    out = M.compute_metrics(case["preds"], case["targets"], 0.75)
    assert np.isnan(want["auroc"]).sum() == 2 and len(out["allAUC"]) == C - 2
    assert len(out["allAUPR"]) == C and len(out["allFDR"]) == C
    close = dict(rtol=3e-6, atol=3e-7)
    np.testing.assert_allclose(out["allAUC"], want["auroc"][~np.isnan(want["auroc"])], **close)
    np.testing.assert_allclose(out["meanAUC"], np.nanmean(want["auroc"]), **close)
    np.testing.assert_allclose(out["medianAUC"], np.nanmedian(want["auroc"]), **close)
    np.testing.assert_allclose(out["meanAUPR"], np.nanmean(want["aupr"]), **close)
    np.testing.assert_allclose(out["medianAUPR"], np.nanmedian(want["aupr"]), **close)
    np.testing.assert_allclose(out["meanFDR"], np.nanmean(want["recall_at_fdr"]), **close)
    np.testing.assert_allclose(out["medianFDR"], np.nanmedian(want["recall_at_fdr"]), **close)
    np.testing.assert_allclose(out["mAP"], np.mean(want["average_precision"]), **close)   # the plain mean over all C labels
    assert not np.isnan(want["average_precision"]).any()
