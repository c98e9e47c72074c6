"""CPU tier: what tests/metrics_cases.py claims about its inputs, checked with numpy and the oracle alone, so that a failure
of tests/test_gpu_metrics.py on these inputs is the kernel's and not the input's."""
import os

import numpy as np
import pytest

import metrics_cases as MC
from oracle import chromegcn_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ends(case, col):
    s, _ = MC.sorted_view(case["preds"][:, col], case["targets"][:, col])
    return MC.run_ends_of(s)


def test_staircase_run_ends_are_where_the_builder_says():
    rng = np.random.RandomState(0)
    runs = [1, 1, 5, 64, 1, 4096, 3, 2]
    s, t, ends = MC.staircase(runs, rng)
    assert s.dtype == np.float32 and t.dtype == np.float32 and set(np.unique(t)) <= {0.0, 1.0}
    assert ends.tolist() == (np.cumsum(runs) - 1).tolist()
    ss, _ = MC.sorted_view(s, t)
    assert (np.diff(ss) <= 0).all() and np.array_equal(MC.run_ends_of(ss), ends)
    assert not (np.diff(s) <= 0).all()   # shuffled: the device sort has work to do


def test_many_chunk_case_shapes_and_run_ends():
    case = MC.many_chunk_case()
    n = MC.MANY_N
    assert case["preds"].shape == (n, 6) and case["targets"].shape == (n, 6)
    assert case["preds"].dtype == np.float32 and case["preds"].min() > 0 and case["preds"].max() < 1
    assert -(-n // MC.CHUNK) == 130 and -(-130 // MC.GROUP) == 3
    # a: distinct
    assert np.unique(case["preds"][:, 0]).size == n
    # b: the builder's run ends, and no run end in chunks 64 .. 127 (one whole group of k_metrics_prefix)
    b = _ends(case, 1)
    assert np.array_equal(b, case["b_ends"])
    lo, hi = MC.MANY_LONG_RUN
    assert lo - 1 in b and hi - 1 in b and not ((b >= lo) & (b < hi - 1)).any()
    chunks = set((b // MC.CHUNK).tolist())
    assert not chunks & set(range(64, 128)) and {63, 128, 129} <= chunks
    # c: exactly the stated run ends; chunk 65 is one run; chunks 2 .. 63 have none
    c = _ends(case, 2)
    assert c.tolist() == MC.MANY_C_ENDS and np.array_equal(c, case["c_ends"])
    assert 65 * MC.CHUNK - 1 in c and 66 * MC.CHUNK - 1 in c
    assert set((c // MC.CHUNK).tolist()) == {0, 1, 63, 64, 65, 129}
    # f: one run
    assert _ends(case, 5).tolist() == [n - 1]


def test_many_chunk_case_fdr_columns():
    case = MC.many_chunk_case()
    n = MC.MANY_N
    # d: tp = fp at every even depth, the deepest one in chunk 128 and holding every positive
    s, t = MC.sorted_view(case["preds"][:, 3], case["targets"][:, 3])
    assert np.unique(s).size == n
    tp = np.cumsum(t.astype(np.float64))
    tot = np.arange(1, n + 1, dtype=np.float64)
    even = np.arange(1, MC.MANY_ALT_DEPTH, 2)   # sorted positions of the even depths
    assert (tp[even] == tot[even] - tp[even]).all() and (1.0 - tp[even] / tot[even] == 0.5).all()
    deepest = MC.MANY_ALT_DEPTH - 1
    assert deepest // MC.CHUNK == 128 and tp[deepest] == tp[-1]
    assert (1.0 - tp[deepest + 1:] / tot[deepest + 1:] > 0.5).all()
    # e: FDR <= 1/2 in chunk 0 only
    s, t = MC.sorted_view(case["preds"][:, 4], case["targets"][:, 4])
    tp = np.cumsum(t.astype(np.float64))
    q = np.flatnonzero(1.0 - tp / tot <= 0.5)
    assert q.size and q.max() == 2 * MC.MANY_E_TOP - 1 and q.max() < MC.CHUNK
    assert t[:MC.MANY_E_TOP].all() and t[n - MC.MANY_E_BOTTOM:].all() and t.sum() == MC.MANY_E_TOP + MC.MANY_E_BOTTOM


def _counts(t):
    tp = np.cumsum(t.astype(np.float64))
    tot = np.arange(1, t.size + 1, dtype=np.float64)
    return tp, tot - tp, tot


@pytest.mark.parametrize("negative_first", [False, True])
@pytest.mark.parametrize("depth,n", [(2, 2), (28, 400), (5000, 9000), (8190, 9000)])
def test_alternating_precision_is_exactly_one_half(depth, n, negative_first):
    s, t = MC.alternating(depth, n, negative_first)
    assert np.unique(s).size == n and (np.diff(s) < 0).all()
    tp, fp, tot = _counts(t)
    even = np.arange(1, depth, 2)
    assert (tp[even] == fp[even]).all() and (1.0 - tp[even] / (tp[even] + fp[even]) == 0.5).all()
    assert tp[depth - 1] == tp[-1] == depth // 2
    assert (1.0 - tp[depth:] / tot[depth:] > 0.5).all()
    if negative_first:                       # no other point qualifies: the answer hangs on the equality
        assert np.array_equal(np.flatnonzero(1.0 - tp / tot <= 0.5), even)


@pytest.mark.parametrize("negative_first", [False, True])
@pytest.mark.parametrize("depth,n", [(4, 4), (28, 400), (5528, 9000), (8180, 9000)])
def test_three_to_one_precision_is_exactly_three_quarters(depth, n, negative_first):
    s, t = MC.three_to_one(depth, n, negative_first)
    assert np.unique(s).size == n and (np.diff(s) < 0).all()
    tp, fp, tot = _counts(t)
    k4 = np.arange(3, depth, 4)
    assert (tp[k4] == 3 * fp[k4]).all() and (1.0 - tp[k4] / (tp[k4] + fp[k4]) == 0.25).all()
    assert tp[depth - 1] == tp[-1] == 3 * depth // 4
    assert (1.0 - tp[depth:] / tot[depth:] > 0.25).all()
    if negative_first:
        assert np.array_equal(np.flatnonzero(1.0 - tp / tot <= 0.25), k4)
    if depth in [d for d, _ in MC.CUTOFF_3TO1.values()]:   # ... and a product with the reciprocal is NOT 3/4 there
        assert 1.0 - tp[depth - 1] * (1.0 / tot[depth - 1]) > 0.25


def test_cutoff_case_columns():
    preds, targets = MC.cutoff_case()
    assert preds.shape == (MC.CUTOFF_N, 8) and preds.dtype == np.float32 and preds.min() >= 0
    built = [(c, MC.alternating, a) for c, a in MC.CUTOFF_ALT.items()] + [(c, MC.three_to_one, a) for c, a in MC.CUTOFF_3TO1.items()]
    assert sorted(nf for _, _, (_, nf) in built) == [False, False, True, True]
    for c, builder, (depth, negative_first) in built:
        assert (depth - 1) // MC.CHUNK >= 1          # the deepest exact point is past the first chunk
        s, t = MC.sorted_view(preds[:, c], targets[:, c])
        want = builder(depth, MC.CUTOFF_N, negative_first)
        assert np.array_equal(s, want[0]) and np.array_equal(t, want[1])
    assert not targets[:, MC.CUTOFF_ALL_NEGATIVE].any()
    col, top = MC.CUTOFF_TOP_POSITIVES
    _, t = MC.sorted_view(preds[:, col], targets[:, col])
    assert t[:top].all() and t[top] == 0.0
    # the oracle on the exact labels: every positive is above the deepest exact point
    got = O.multilabel_metrics_np(targets.astype(np.float64), preds, 0.5)["recall_at_fdr"]
    assert all(got[c] == 1.0 for c in MC.CUTOFF_ALT)
    got = O.multilabel_metrics_np(targets.astype(np.float64), preds, 0.25)["recall_at_fdr"]
    assert all(got[c] == 1.0 for c in MC.CUTOFF_3TO1)


def test_two_group_case_degenerate_columns_against_the_oracle():
    case = MC.two_group_case()
    n = MC.TWO_N
    preds, targets = case["preds"], case["targets"]
    assert preds.shape == (n, 6) and -(-n // MC.CHUNK) == 65
    assert targets[:, 0].all() and not targets[:, 1].any()
    _, t = MC.sorted_view(preds[:, 2], targets[:, 2])
    assert t.sum() == 1 and t[case["positive_rank"]] == 1.0
    _, t = MC.sorted_view(preds[:, 3], targets[:, 3])
    assert t.sum() == n - 1 and t[MC.TWO_NEGATIVE_RANK] == 0.0
    assert np.unique(preds[:, 4]).size <= 11 and np.unique(preds[:, 5]).size == n
    want = O.multilabel_metrics_np(targets[:, :2].astype(np.float64), preds[:, :2])
    assert np.isnan(want["auroc"]).all()
    assert want["aupr"].tolist() == [1.0, 0.5]
    assert want["recall_at_fdr"].tolist() == [1.0, 0.0]
    assert want["average_precision"].tolist() == [1.0, 0.0]


def test_alternating_labels_have_recall_one_in_the_oracle():
    case = MC.many_chunk_case()
    want = O.multilabel_metrics_np(case["targets"][:, 3:4].astype(np.float64), case["preds"][:, 3:4])
    assert want["recall_at_fdr"][0] == 1.0


def test_saturated_case_holds_what_it_says():
    preds, targets = MC.saturated_case()
    assert preds.shape == (9000, 5) and preds.dtype == np.float32
    assert not np.isnan(preds).any() and (preds >= 0).all() and preds.max() == 1.0
    tiny = np.finfo(np.float32).tiny
    assert (preds[:, 0] == 1.0).sum() > MC.CHUNK and (preds[:, 0] == 0.0).sum() > MC.CHUNK
    z = preds[:, 1][preds[:, 1] == 0.0]
    assert z.size > MC.CHUNK and np.signbit(z).any() and not np.signbit(z).all()
    assert (preds[:, 2] == 1.0).sum() > MC.CHUNK and np.signbit(preds[:, 2]).any()
    for c in (0, 1, 4):
        sub = preds[:, c][(preds[:, c] > 0) & (preds[:, c] < tiny)]
        assert sub.size >= 200 and np.unique(sub).size > 10
        assert np.array_equal(sub, (np.round(sub / MC.SUBNORMAL) * MC.SUBNORMAL).astype(np.float32))
    rates = targets.mean(axis=0)
    assert rates.min() < 0.05 and rates.max() > 0.6 and all(0 < t.sum() < t.size for t in targets.T)


def test_every_pack_case_maps_to_the_rows_per_block_it_is_meant_to_hit():
    for C, R in list(MC.PACK_CASES.items()) + list(MC.BAD_CASES.items()):
        assert MC.pack_rows(C) == R, (C, R, MC.pack_rows(C))
    assert sorted(set(MC.PACK_CASES.values())) == [0, 4, 8, 16, 32, 64, 128]
    for C in sorted(MC.PACK_CASES):          # each case sits ON a switch: a neighbour takes another R (but the product's 256)
        if C != 256:
            assert MC.pack_rows(C - 1) != MC.pack_rows(C) or MC.pack_rows(C + 1) != MC.pack_rows(C), C
    for _, C in MC.PACK_TWO_TILES:
        assert C in MC.PACK_CASES
    for R in (4, 8, 16, 32, 64, 128):        # the last block is partial, and an odd C leaves a tail that is no multiple of 4
        assert MC.PACK_N % R != 0
    assert any((MC.PACK_N % R) * C % 4 for C, R in MC.PACK_CASES.items() if R)
    assert MC.oracle_columns(2458) == [0, 1, 2, 1229, 2456, 2457] and MC.oracle_columns(2) == [0, 1]


def test_pack_rows_is_the_rule_in_the_source():
    with open(os.path.join(ROOT, "chromegcn_amd", "csrc", "cgcn_metrics.hip")) as f:
        src = f.read()
    assert "int R = 128, rshift = 7;" in src
    assert "while (R > 4 && (size_t)C * (R + 1) * 4 > 48 * 1024) { R >>= 1; --rshift; }" in src
    assert "if ((size_t)C * (R + 1) * 4 <= 48 * 1024) {" in src
    assert "#define METRIC_CHUNK 4096" in src
