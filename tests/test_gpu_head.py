"""Classifier head (relu -> BatchNorm1d -> dropout -> Linear -> strand mean -> BCE) against a float64 torch
restatement of models/ChromeModels.py:48-51 + finetune.py:43,45,52.  Which kernels each test reaches:
  * test_head_train_matches_float64, test_head_eval_matches_float64, the dropout tests, _probe_mask: ops.head_loss, i.e.
    cgcn_head_fwd / cgcn_head_bwd -- the UNFUSED k_head_fwd / k_head_bwd (+ k_head_colstats, k_head_bn_finalize,
    k_head_bwd_finalize, k_head_bn_bwd_apply);
  * test_layer_fwd_colstats_are_the_tile_statistics_of_relu_output: cgcn_layer_fwd's statistics records;
  * test_head_train_every_instance_matches_float64: cgcn_head_train through the C ABI -- every instance of the training
    step's FUSED head, k_head_fused_sp<MULTI, NB, DROP> (split products) and k_head_fused_rs<MULTI, NB, DROP, NRB> (fp32 chain)
    at d = 128, k_head_fused<256, 8> at d = 256 -- and the same cases through ops.head_loss (k_head_fwd / k_head_bwd at
    C > 128 on both widths);
  * the tests after it (fused_step): cgcn_layer_fwd -> cgcn_head_train -> cgcn_layer_bwd in head mode (cgcn_head_grad: the
    head's gradients finished in the row-local backward), directly and through ChromeGCN.forward_loss.
(The reference-recorded vectors reach this code through tests/test_gpu_loop.py and the model tests, which run the whole step.)"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from chromegcn_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"


def ref_head(x64, bn, out, target64, training):
    """float64 CPU: per-strand BatchNorm (sequential running-stat updates), mean of logits, BCE"""
    logits = []
    for s in range(x64.shape[0]):
        y = bn(F.relu(x64[s]))
        logits.append(out(y))
    pred = sum(logits) / len(logits)
    loss = F.binary_cross_entropy_with_logits(pred, target64)
    return loss, torch.sigmoid(pred)


def make(S, n, d, C, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(S, n, d, generator=g) * 1.3 + 0.2
    tgt = (torch.rand(n, C, generator=g) < 0.2).float()
    bn = nn.BatchNorm1d(d); out = nn.Linear(d, C)
    with torch.no_grad():
        bn.weight.copy_(1 + 0.2 * torch.randn(d, generator=g)); bn.bias.copy_(0.1 * torch.randn(d, generator=g))
        bn.running_mean.copy_(0.1 * torch.randn(d, generator=g)); bn.running_var.copy_(1 + 0.3 * torch.rand(d, generator=g))
        out.weight.copy_(torch.randn(C, d, generator=g) / np.sqrt(d) * 2)
    return x, tgt, bn, out


@pytest.mark.parametrize("S,n,d,C", [(2, 333, 128, 103), (1, 37, 128, 19), (2, 2, 128, 7), (2, 150, 256, 200),
                                     (1, 70, 256, 130), (2, 4100, 128, 103)])
def test_head_train_matches_float64(S, n, d, C):
    x, tgt, bn, out = make(S, n, d, C, 7)
    import copy
    bn64, out64 = copy.deepcopy(bn).double(), copy.deepcopy(out).double()
    bn64.train()
    x64 = x.double().requires_grad_(True)
    loss64, probs64 = ref_head(x64, bn64, out64, tgt.double(), True)
    (loss64 * 1.7).backward()

    bn, out = bn.to(DEV), out.to(DEV)
    xg = x.to(DEV).requires_grad_(True)
    rng = torch.tensor([1, 0], dtype=torch.int64, device=DEV)
    loss, probs = ops.head_loss(xg, bn, out, tgt.to(DEV), True, 0.0, rng)
    (loss * 1.7).backward()
    assert abs(loss.item() - loss64.item()) < 1e-5
    np.testing.assert_allclose(probs.cpu().numpy(), probs64.detach().numpy(), atol=1e-5, rtol=1e-4)
    np.testing.assert_allclose(xg.grad.cpu().numpy(), x64.grad.numpy(), atol=1e-4 * x64.grad.abs().max().item(), rtol=1e-4)
    for a, b in [(bn.weight, bn64.weight), (bn.bias, bn64.bias), (out.weight, out64.weight), (out.bias, out64.bias)]:
        ref = b.grad.numpy()
        np.testing.assert_allclose(a.grad.cpu().numpy(), ref, atol=1e-5 * max(1.0, np.abs(ref).max()), rtol=1e-4)
    np.testing.assert_allclose(bn.running_mean.cpu().numpy(), bn64.running_mean.numpy(), atol=1e-6, rtol=1e-5)
    np.testing.assert_allclose(bn.running_var.cpu().numpy(), bn64.running_var.numpy(), atol=1e-6, rtol=1e-5)
    assert int(bn.num_batches_tracked.item()) == S == int(bn64.num_batches_tracked.item())


@pytest.mark.parametrize("S,n,d,C", [(2, 333, 128, 103), (1, 1, 128, 5), (2, 90, 256, 257 - 1)])
def test_head_eval_matches_float64(S, n, d, C):
    x, tgt, bn, out = make(S, n, d, C, 8)
    import copy
    bn64, out64 = copy.deepcopy(bn).double().eval(), copy.deepcopy(out).double()
    with torch.no_grad():
        loss64, probs64 = ref_head(x.double(), bn64, out64, tgt.double(), False)
    bn, out = bn.to(DEV).eval(), out.to(DEV)
    with torch.no_grad():
        loss, probs = ops.head_loss(x.to(DEV), bn, out, tgt.to(DEV), False, 0.2, None)
    assert abs(loss.item() - loss64.item()) < 1e-5
    np.testing.assert_allclose(probs.cpu().numpy(), probs64.numpy(), atol=1e-5, rtol=1e-4)
    assert int(bn.num_batches_tracked.item()) == 0


def _probe_mask(n_rows, d, p, seed, counter):
    """Recover the kernel's keep-mask for element indices [0, n_rows*d): with bn_w = 0, bn_b = 1,
    W_out = I, b_out = 0 and S = 1 the logits ARE mask / (1-p).  The mask is a pure function of
    (seed, counter, element index), so rows [n, 2n) of this probe are strand 1 of an S = 2 call."""
    bn = nn.BatchNorm1d(d).to(DEV); out = nn.Linear(d, d).to(DEV)
    with torch.no_grad():
        bn.weight.zero_(); bn.bias.fill_(1.0); out.weight.copy_(torch.eye(d)); out.bias.zero_()
    rng = torch.tensor([seed, counter], dtype=torch.int64, device=DEV)
    x = torch.randn(1, n_rows, d, device=DEV)
    _, probs = ops.head_loss(x, bn, out, torch.zeros(n_rows, d, device=DEV), True, p, rng)
    return (probs > 0.6).cpu()  # sigmoid(1/(1-p)) > 0.73 when kept, sigmoid(0) = 0.5 when dropped


def test_head_dropout_forward_and_backward_use_the_same_mask():
    """float64 restatement with the kernel's own mask made explicit: loss, probs and every gradient must
    match, which they only do if forward and backward regenerate identical masks."""
    import copy
    S, n, d, C, p = 2, 61, 128, 11, 0.3
    x, tgt, bn, out = make(S, n, d, C, 9)
    mask = _probe_mask(S * n, d, p, 1234, 5).view(S, n, d).double()
    assert 0.6 < mask.mean().item() < 0.8
    import dropout_ref   # the probed mask is the stated one (tests/dropout_ref.py)
    np.testing.assert_array_equal(mask.numpy() != 0, dropout_ref.mask(1234, 5, dropout_ref.HEAD_STREAM_ID, (S, n, d), p))
    bn64, out64 = copy.deepcopy(bn).double().train(), copy.deepcopy(out).double()
    x64 = x.double().requires_grad_(True)
    logits = [out64(bn64(F.relu(x64[s])) * mask[s] / (1 - p)) for s in range(S)]
    pred = sum(logits) / S
    loss64 = F.binary_cross_entropy_with_logits(pred, tgt.double())
    loss64.backward()

    bn, out = bn.to(DEV), out.to(DEV)
    rng = torch.tensor([1234, 5], dtype=torch.int64, device=DEV)
    xg = x.to(DEV).requires_grad_(True)
    loss, probs = ops.head_loss(xg, bn, out, tgt.to(DEV), True, p, rng)
    loss.backward()
    assert int(rng[1].item()) == 5  # the head only reads the counter (cgcn_sgd_step advances it)
    assert abs(loss.item() - loss64.item()) < 1e-5
    np.testing.assert_allclose(probs.cpu().numpy(), torch.sigmoid(pred).detach().numpy(), atol=1e-5, rtol=1e-4)
    ref = x64.grad.numpy()
    np.testing.assert_allclose(xg.grad.cpu().numpy(), ref, atol=1e-4 * np.abs(ref).max(), rtol=1e-4)
    for a_, b_ in [(bn.weight, bn64.weight), (bn.bias, bn64.bias), (out.weight, out64.weight), (out.bias, out64.bias)]:
        r = b_.grad.numpy()
        np.testing.assert_allclose(a_.grad.cpu().numpy(), r, atol=1e-4 * max(1e-6, np.abs(r).max()), rtol=1e-4)
    # a different step counter draws a different mask
    rng[1] = 6
    l6, _ = ops.head_loss(xg.detach(), bn, out, tgt.to(DEV), True, p, rng)
    assert l6.item() != loss.item()


def test_head_dropout_keep_rate():
    # bn_w = 0, bn_b = 1 -> y = 1 before dropout; W_out = ones/d, so pred = kept fraction / (1-p) per node
    S, n, d, C, p = 2, 500, 128, 3, 0.25
    bn = nn.BatchNorm1d(d).to(DEV); out = nn.Linear(d, C).to(DEV)
    with torch.no_grad():
        bn.weight.zero_(); bn.bias.fill_(1.0); out.weight.fill_(1.0 / d); out.bias.zero_()
    x = torch.randn(S, n, d, device=DEV)
    rng = torch.tensor([99, 0], dtype=torch.int64, device=DEV)
    _, probs = ops.head_loss(x, bn, out, torch.zeros(n, C, device=DEV), True, p, rng)
    pred = torch.logit(probs[:, 0].double())
    keep = (pred * (1 - p)).mean().item()
    assert abs(keep - (1 - p)) < 0.01, keep


@pytest.mark.parametrize("S,n,d", [(2, 333, 128), (1, 37, 128), (2, 5, 128), (2, 1500, 128), (2, 70, 256), (1, 16, 256)])
def test_layer_fwd_colstats_are_the_tile_statistics_of_relu_output(S, n, d):
    """cgcn_layer_fwd's optional colstats output (first stage of the head's BatchNorm statistics): per node tile the
    exact mean / sum of squared deviations of relu(Xn), ragged last tile included."""
    import ctypes
    from chromegcn_amd import _lib, graph as G
    from chromegcn_amd import synth
    lib = _lib.load()
    g = G.upload(G.normalize_graph("hic", synth.contact_graph(n, max(1, 3 * n), n + d), n), DEV)
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(S, n, d, generator=gen).to(DEV)
    W = (torch.randn(d, d, generator=gen) / d ** 0.5).to(DEV); b = (0.1 * torch.randn(d, generator=gen)).to(DEV)
    wg = (torch.randn(d, generator=gen) / d ** 0.5).to(DEV); cg = torch.zeros(1, device=DEV)
    xn = torch.empty_like(x); gate = torch.empty(S, n, device=DEV)
    rows = ctypes.c_int(0)
    tiles = lib.cgcn_layer_fwd_colstats_plan(n, S, d, _lib.COLSTATS_RECORDS, ctypes.byref(rows))
    R = rows.value
    assert tiles == (n + R - 1) // R and R >= 1
    cs = torch.full((tiles, S, d, 2), float("nan"), device=DEV)
    P = _lib.ptr
    _lib.check(lib.cgcn_layer_fwd(_lib.stream_ptr(), n, S, d, P(g.rowptr), P(g.col), P(g.val), P(g.row_scale), P(x), P(W), P(b),
                                  P(wg), P(cg), P(xn), None, None, P(gate), 0.0, None, 0, None, P(cs), R, None), "cgcn_layer_fwd")
    y = torch.relu(xn).double().cpu().numpy()
    cs = cs.cpu().numpy()
    for t in range(tiles):
        blk = y[:, t * R:min(n, (t + 1) * R), :]
        np.testing.assert_allclose(cs[t, :, :, 0], blk.mean(axis=1), atol=1e-6, rtol=1e-5)
        np.testing.assert_allclose(cs[t, :, :, 1], ((blk - blk.mean(axis=1, keepdims=True)) ** 2).sum(axis=1), atol=1e-5, rtol=1e-4)


# ---------------------------------------------------------------------------------------------------------------------------
# cgcn_head_train -- the training step's head (k_head_fused_sp / k_head_fused_rs at d = 128, k_head_fused<256, 8> at d = 256)
# -- called directly through the C ABI, and its gradients finished by cgcn_layer_bwd in head mode (cgcn_head_grad)
# ---------------------------------------------------------------------------------------------------------------------------
FORMS = {"split": 1, "fp32_chain": 0}   # include/chromegcn.h: CGCN_PRODUCTS_*
MOM, EPS = 0.1, 1e-5                    # nn.BatchNorm1d defaults, what the model uses


@pytest.fixture
def lib():
    from chromegcn_amd import _lib
    h = _lib.load()
    default = h.cgcn_debug_get_products()
    yield h
    h.cgcn_debug_set_products(-1)
    assert h.cgcn_debug_get_products() == default


def rs_nrb(n):
    """Row tiles (16 NRB rows) k_head_fused_rs runs at n, restated from cgcn_head_train's dispatch (cgcn_head.hip, `tr16`):
    P = min(ceil(n / 32), 256) workgroups (head_bwd_partials), a launch lasts ceil(tiles / P) + 1 periods, and a period of
    16-row tiles costs 55 % (HEAD_TR16_COST_PCT) of one of 32-row tiles."""
    P = min(max(-(-n // 32), 1), 256)
    periods = lambda tr: (-(-n // tr) + P - 1) // P + 1   # noqa: E731
    return 1 if periods(16) * 55 < periods(32) * 100 else 2


def head_params(d, C, seed):
    g = torch.Generator().manual_seed(seed)
    return {"bn_w": 1 + 0.2 * torch.randn(d, generator=g), "bn_b": 0.1 * torch.randn(d, generator=g),
            "rm": 0.1 * torch.randn(d, generator=g), "rv": 1 + 0.3 * torch.rand(d, generator=g),
            "W": torch.randn(C, d, generator=g) / np.sqrt(d) * 2, "b": 0.1 * torch.randn(C, generator=g)}


def ref_head_train(x, prm, tgt, p=0.0, mask=None):
    """float64 restatement of cgcn_head_train and of the head gradients cgcn_layer_bwd finishes (d loss = 1):
    y_s = BN(relu(X_s)) mask_s / (1 - p) with batch statistics, pred = mean_s y_s W^T + b, BCE with logits (mean over n C),
    probs; running statistics updated once per strand in strand order; dym = (sigmoid(pred) - t) / (n C) W."""
    x = x.double()
    S, n, d = x.shape
    C = prm["W"].shape[0]
    W, bn_w = prm["W"].double(), prm["bn_w"].double()
    r = x.clamp_min(0)
    mean = r.mean(1)
    var = ((r - mean[:, None]) ** 2).mean(1)
    invstd = 1 / (var + EPS).sqrt()
    xh = (r - mean[:, None]) * invstd[:, None]
    keep = None if mask is None else mask.double() / (1 - p)
    y = xh * bn_w + prm["bn_b"].double()
    if keep is not None:
        y = y * keep
    ym = y.mean(0)
    del y
    pred = ym @ W.T + prm["b"].double()
    t = tgt.double()
    loss = F.binary_cross_entropy_with_logits(pred, t)
    probs = torch.sigmoid(pred)
    del pred
    rm, rv = prm["rm"].double(), prm["rv"].double()
    for s in range(S):
        rm = (1 - MOM) * rm + MOM * mean[s]
        rv = (1 - MOM) * rv + MOM * var[s] * n / (n - 1)
    dpred = (probs - t) / (n * C)
    dym = dpred @ W
    dy = dym.expand(S, n, d) / S if keep is None else dym[None] / S * keep
    dbn_b, dbn_w = dy.sum((0, 1)), (dy * xh).sum((0, 1))
    dxh = dy * bn_w
    del dy
    # dX: BatchNorm's backward subtracts two column means from invstd dxh; at n = 2 they cancel it to ~1e-5 of its size, so
    # what fp32 can reach is relative to that size (dX_terms), not to dX
    dx_terms = float((invstd[:, None] * dxh).abs().max())
    dx = invstd[:, None] * (dxh - dxh.mean(1, keepdim=True) - xh * (dxh * xh).mean(1, keepdim=True)) * (x > 0)
    return {"dX_terms": dx_terms, "loss": loss, "probs": probs, "save_mean": mean, "save_invstd": invstd, "rm": rm, "rv": rv, "dym": dym,
            "dW_out": dpred.T @ ym, "db_out": dpred.sum(0), "dbn_w": dbn_w, "dbn_b": dbn_b, "dX": dx}


def _check(name, got, ref, a=1e-5, r=1e-4, scale=0.0):
    """|got - ref| <= a max(max|ref|, scale) + r |ref| elementwise (a: scale-relative bound)"""
    ref = ref.detach().double().cpu().numpy()
    np.testing.assert_allclose(got.detach().double().cpu().numpy(), ref, atol=a * max(np.abs(ref).max(), scale, 1e-30), rtol=r,
                               err_msg=name)


def _nan_buf(nbytes, guard):
    """0xFF bytes (every float32 view reads NaN) with `guard` bytes of tail"""
    return torch.full((nbytes + guard,), 0xFF, dtype=torch.uint8, device=DEV)


def _f32(buf, *shape):
    k = int(np.prod(shape))
    return buf[:4 * k].view(torch.float32).view(*shape)


def head_train_call(lib, x, prm, tgt, p=0.0, rng=None, col_stats=None, tiles=0, rows=0, guard=0):
    """cgcn_head_train on device copies of prm; every output (and the workspace, exactly cgcn_head_workspace_bytes) starts
    as NaN bytes followed by `guard` bytes of NaN tail.  Returns the outputs, dym (read from the workspace at the layout's
    dym offset) and the raw buffers (tails included)."""
    from chromegcn_amd import _lib
    S, n, d = x.shape
    C = prm["W"].shape[0]
    P = _lib.ptr
    dv = {k: v.to(DEV) for k, v in prm.items()}
    wsb = lib.cgcn_head_workspace_bytes(n, S, d, C)
    assert wsb > 0
    bufs = {"ws": _nan_buf(wsb, guard), "probs": _nan_buf(4 * n * C, guard), "loss": _nan_buf(4, guard),
            "save_mean": _nan_buf(4 * S * d, guard), "save_invstd": _nan_buf(4 * S * d, guard)}
    out = {"probs": _f32(bufs["probs"], n, C), "loss": _f32(bufs["loss"], 1), "save_mean": _f32(bufs["save_mean"], S, d),
           "save_invstd": _f32(bufs["save_invstd"], S, d), "rm": dv["rm"], "rv": dv["rv"],
           "nbt": torch.tensor([5], dtype=torch.int64, device=DEV)}
    _lib.check(lib.cgcn_head_train(_lib.stream_ptr(), n, S, d, C, P(x), P(dv["bn_w"]), P(dv["bn_b"]), P(out["rm"]), P(out["rv"]),
                                   P(out["nbt"]), MOM, EPS, P(dv["W"]), P(dv["b"]), P(tgt), float(p), P(rng) if p > 0 else None,
                                   P(out["probs"]), P(out["loss"]), P(out["save_mean"]), P(out["save_invstd"]), P(col_stats),
                                   tiles, rows, P(bufs["ws"]), wsb), "cgcn_head_train")
    torch.cuda.synchronize()
    o = [ctypes.c_size_t() for _ in range(3)]
    _lib.check(lib.cgcn_head_workspace_layout(n, S, d, C, *[ctypes.byref(v) for v in o]), "cgcn_head_workspace_layout")
    out["dym"] = bufs["ws"][o[0].value:o[0].value + 4 * n * d].view(torch.float32).view(n, d)
    out["layout"] = tuple(v.value for v in o)
    out["bufs"], out["guard"], out["dev_prm"] = bufs, guard, dv
    return out


def assert_tails_untouched(bufs, guard):
    for k, b in bufs.items():
        assert bool((b[b.numel() - guard:] == 0xFF).all()), "%s: written past its end" % k


def check_head_train(out, ref, S):
    assert abs(out["loss"].item() - ref["loss"].item()) < 1e-5, (out["loss"].item(), ref["loss"].item())
    _check("probs", out["probs"], ref["probs"], a=1e-5, r=1e-4)
    _check("save_mean", out["save_mean"], ref["save_mean"], a=1e-6, r=1e-5)
    _check("save_invstd", out["save_invstd"], ref["save_invstd"], a=1e-6, r=1e-5)
    _check("running_mean", out["rm"], ref["rm"], a=1e-6, r=1e-5)
    _check("running_var", out["rv"], ref["rv"], a=1e-6, r=1e-5)
    assert int(out["nbt"].item()) == 5 + S
    _check("dym", out["dym"], ref["dym"], a=1e-5, r=1e-4)


# (S, n, d, C, p, NRB of the chain form the case is there for, or None).  A label pass of at most 128 labels runs NB = 7 when it
# has 97..112 labels, MULTI = C > 128 (cgcn_head_train); C = 225 / 240 / 231 put 97 / 112 / 103 labels into the second pass.
TRAIN_CASES = [
    (2, 2, 128, 1, 0.0, None), (2, 17, 128, 96, 0.0, None), (1, 33, 128, 113, 0.0, None), (2, 4097, 128, 128, 0.0, None),     # <F, 8, F>
    (2, 16, 128, 97, 0.0, None), (1, 31, 128, 112, 0.0, None), (2, 333, 128, 103, 0.0, None),                              # <F, 7, F>
    (2, 61, 128, 11, 0.3, None), (2, 8193, 128, 128, 0.2, None), (2, 4100, 128, 103, 0.2, None),                           # <F, 8|7, T>
    (2, 15, 128, 129, 0.0, None), (2, 5000, 128, 256, 0.0, None), (2, 333, 128, 225, 0.0, None), (1, 3000, 128, 240, 0.0, None),  # <T, 8|7, F>
    (2, 777, 128, 231, 0.3, None), (2, 20000, 128, 256, 0.2, None), (2, 100003, 128, 240, 0.2, None),                      # <T, 8|7, T>
    (2, 36864, 128, 103, 0.0, 1), (2, 36865, 128, 103, 0.0, 2), (2, 40960, 128, 240, 0.2, 2),                              # chain: NRB edge
    (2, 40000, 128, 128, 0.0, 2), (1, 40000, 128, 64, 0.2, 2), (2, 40000, 128, 103, 0.2, 2), (2, 40000, 128, 240, 0.0, 2),  # chain: NRB = 2
    (2, 2, 256, 1, 0.0, None), (1, 33, 256, 240, 0.3, None), (2, 150, 256, 200, 0.25, None), (2, 9000, 256, 256, 0.0, None),
    (2, 40000, 256, 97, 0.2, None),                                                                                         # k_head_fused<256, 8>
]


def make_train_case(S, n, d, C, p, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(S, n, d, generator=g) * 1.3 + 0.2
    tgt = (torch.rand(n, C, generator=g) < 0.2).float()
    mask = _probe_mask(S * n, d, p, 1000 + seed, 3).view(S, n, d) if p > 0 else None
    rng = torch.tensor([1000 + seed, 3], dtype=torch.int64, device=DEV)
    return x, tgt, head_params(d, C, seed), mask, rng


@pytest.mark.parametrize("S,n,d,C,p,nrb", TRAIN_CASES, ids=["S%d-n%d-d%d-C%d-p%g" % c[:5] for c in TRAIN_CASES])
def test_head_train_every_instance_matches_float64(lib, S, n, d, C, p, nrb):
    """cgcn_head_train in both product forms (d = 256 has one kernel, k_head_fused<256, 8>): loss, probs, batch and running
    statistics, the call count and dym = Pt W_out (the workspace, before the layer backward mixes anything in) against
    float64; a second identical call gives the same bits.  Then the same case through ops.head_loss (k_head_fwd / k_head_bwd)
    with every gradient."""
    if nrb is not None:
        assert rs_nrb(n) == nrb, "the tile-height rule changed: case (n = %d) no longer reaches NRB = %d" % (n, nrb)
    x, tgt, prm, mask, rng = make_train_case(S, n, d, C, p, n + C)
    if mask is not None:
        assert abs(mask.float().mean().item() - (1 - p)) < 0.05
    ref = ref_head_train(x, prm, tgt, p, mask)
    xd, td = x.to(DEV), tgt.to(DEV)
    for form in (FORMS if d == 128 else ["split"]):
        lib.cgcn_debug_set_products(FORMS[form])
        first = head_train_call(lib, xd, prm, td, p, rng)
        check_head_train(first, ref, S)
        again = head_train_call(lib, xd, prm, td, p, rng)
        for k in ("probs", "loss", "save_mean", "save_invstd", "rm", "rv", "nbt"):
            assert torch.equal(first[k], again[k]), (form, k)
        assert torch.equal(first["bufs"]["ws"], again["bufs"]["ws"]), (form, "workspace")
    lib.cgcn_debug_set_products(-1)
    # the unfused pair (cgcn_head_fwd / cgcn_head_bwd) on the same case
    bn, out = nn.BatchNorm1d(d), nn.Linear(d, C)
    with torch.no_grad():
        for t_, k in ((bn.weight, "bn_w"), (bn.bias, "bn_b"), (bn.running_mean, "rm"), (bn.running_var, "rv"), (out.weight, "W"),
                      (out.bias, "b")):
            t_.copy_(prm[k])
    bn, out = bn.to(DEV), out.to(DEV)
    xg = xd.clone().requires_grad_(True)
    loss, probs = ops.head_loss(xg, bn, out, td, True, p, rng)
    loss.backward()
    assert abs(loss.item() - ref["loss"].item()) < 1e-5
    _check("probs", probs, ref["probs"], a=1e-5, r=1e-4)
    _check("running_mean", bn.running_mean, ref["rm"], a=1e-6, r=1e-5)
    _check("running_var", bn.running_var, ref["rv"], a=1e-6, r=1e-5)
    assert int(bn.num_batches_tracked.item()) == S
    _check("dX", xg.grad, ref["dX"], a=1e-4, r=1e-4, scale=ref["dX_terms"])
    for t_, k in ((bn.weight, "dbn_w"), (bn.bias, "dbn_b"), (out.weight, "dW_out"), (out.bias, "db_out")):
        _check(k, t_.grad, ref[k], a=2e-5, r=1e-4)


def fused_step(lib, x, prm, tgt, p=0.0, rng=None, source="head", guard=0, want_dx=True):
    """The engine's last layer + head with the layer made transparent -- W = 0, b = 0, gate weight 0, gate bias -30, so
    g = sigmoid(-30) and Xn = x up to 1e-13 relative -- then cgcn_head_train and cgcn_layer_bwd in head mode, which finishes
    dW_out, db_out, dbn_w, dbn_b (d loss = 1) and, want_dx, dX (else the head's second stage rides in the row-local launch).
    source: where the head's batch statistics come from -- 'head' (its own first pass, col_stats = NULL), 'records'
    (cgcn_layer_fwd's per-tile records) or 'accumulate' (cgcn_layer_fwd's fixed-point totals).  Returns head_train_call's
    dict plus the gradients and 'xn', the head's input."""
    from chromegcn_amd import _lib, graph as G, synth
    S, n, d = x.shape
    C = prm["W"].shape[0]
    P, st = _lib.ptr, _lib.stream_ptr
    g = G.upload(G.normalize_graph("hic", synth.contact_graph(n, max(1, 3 * n), 11), n), DEV)
    W, b, wg = torch.zeros(d, d, device=DEV), torch.zeros(d, device=DEV), torch.zeros(d, device=DEV)
    cg = torch.full((1,), -30.0, device=DEV)
    xn, z, h = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    gate = torch.empty(S, n, device=DEV)
    cs, tiles, rows = None, 0, 0
    if source != "head":
        r = ctypes.c_int(0)
        tiles = lib.cgcn_layer_fwd_colstats_plan(n, S, d, _lib.COLSTATS_ACCUMULATE if source == "accumulate" else _lib.COLSTATS_RECORDS,
                                                 ctypes.byref(r))
        rows = r.value
        assert tiles > 0 and (rows == -1) == (source == "accumulate")
        cs = torch.empty((tiles, S, d, 2), device=DEV)
    _lib.check(lib.cgcn_layer_fwd(st(), n, S, d, P(g.rowptr), P(g.col), P(g.val), P(g.row_scale), P(x), P(W), P(b), P(wg), P(cg),
                                  P(xn), P(z), P(h), P(gate), 0.0, None, 1, None, P(cs), rows, G.aux_ptr(g.col)), "cgcn_layer_fwd")
    out = head_train_call(lib, xn, prm, tgt, p, rng, cs, tiles, rows, guard)
    bufs, dv = out["bufs"], out["dev_prm"]
    for k, sh in (("dW_out", (C, d)), ("db_out", (C,)), ("dbn_w", (d,)), ("dbn_b", (d,))):
        bufs[k] = _nan_buf(4 * int(np.prod(sh)), guard)
        out[k] = _f32(bufs[k], *sh)
    o_dym, o_bnc, o_part = out["layout"]
    wsp = bufs["ws"].data_ptr()
    dloss = torch.ones(1, device=DEV)
    hg = _lib.HeadGrad(wsp + o_dym, wsp + o_bnc, P(out["save_mean"]), P(out["save_invstd"]), P(dv["bn_w"]), float(p),
                       P(rng) if p > 0 else None, wsp + o_part, lib.cgcn_head_bwd_partials(n), C, P(out["dW_out"]), P(out["db_out"]),
                       0, P(dloss), P(out["dbn_w"]), P(out["dbn_b"]), P(cs) if rows == -1 else None)
    dx = torch.empty_like(x) if want_dx else None
    dhs = torch.empty_like(x) if want_dx else None
    dW, db, dwg, dcg = torch.empty_like(W), torch.empty_like(b), torch.empty_like(wg), torch.empty_like(cg)
    lwb = lib.cgcn_layer_bwd_workspace_bytes(n, S, d)
    lw = torch.empty(lwb, dtype=torch.uint8, device=DEV)
    _lib.check(lib.cgcn_layer_bwd(st(), n, S, d, P(g.rowptr_t), P(g.col_t), P(g.val_t), P(g.row_scale), P(x), P(z), P(h), P(gate),
                                  P(W), P(wg), None, None, P(dx), P(dhs), P(dW), P(db), P(dwg), P(dcg), 0, 0.0,
                                  P(rng) if p > 0 else None, 0, ctypes.byref(hg), P(lw), lwb, None, None, G.aux_ptr(g.col_t)),
               "cgcn_layer_bwd")
    torch.cuda.synchronize()
    out["dX"], out["xn"] = dx, xn
    return out


def check_head_grads(out, ref, a=2e-5):
    for k in ("dW_out", "db_out", "dbn_w", "dbn_b"):
        _check(k, out[k], ref[k], a=a, r=1e-4)
    if out["dX"] is not None:
        _check("dX", out["dX"], ref["dX"], a=1e-4, r=1e-4, scale=ref["dX_terms"])


GUARD_CASES = [(128, 97, "split"), (128, 97, "fp32_chain"), (128, 225, "split"), (128, 225, "fp32_chain"), (256, 225, "split")]


@pytest.mark.parametrize("d,C,form", GUARD_CASES)
@pytest.mark.parametrize("p", [0.0, 0.3])
def test_head_train_and_its_gradients_write_nothing_past_their_buffers(lib, d, C, form, p):
    """n = 17 (a ragged 16-row tile, one workgroup): probs, loss, save_*, the workspace (exactly cgcn_head_workspace_bytes),
    dW_out, db_out, dbn_w, dbn_b each followed by 4 KiB of NaN bytes that must come back untouched; the values against float64."""
    S, n, guard = 2, 17, 4096
    x, tgt, prm, mask, rng = make_train_case(S, n, d, C, p, 77 + C)
    lib.cgcn_debug_set_products(FORMS[form])
    out = fused_step(lib, x.to(DEV), prm, tgt.to(DEV), p, rng, guard=guard)
    assert_tails_untouched(out["bufs"], guard)
    ref = ref_head_train(out["xn"].cpu(), prm, tgt, p, mask)
    check_head_train(out, ref, S)
    check_head_grads(out, ref)


def conditioning_features(S, n, d, seed):
    """relu(x) columns: [0, d/4) zero everywhere (var 0), [d/4, d/2) a positive constant (var 0), [d/2, 3d/4) mean / sd = 10,
    [3d/4, d) mean / sd = 100 (sd exactly 1 over the n rows of each strand)"""
    g = torch.Generator().manual_seed(seed)
    q = d // 4
    zz = torch.randn(S, n, d, generator=g, dtype=torch.float64)
    zz = (zz - zz.mean(1, keepdim=True)) / zz.std(1, unbiased=False, keepdim=True)
    x = torch.empty(S, n, d, dtype=torch.float64)
    x[..., :q] = -0.5 - torch.rand(S, n, q, generator=g, dtype=torch.float64)
    x[..., q:2 * q] = 0.25 + 0.05 * torch.arange(q, dtype=torch.float64)
    x[..., 2 * q:3 * q] = 10 + zz[..., 2 * q:3 * q]
    x[..., 3 * q:] = 100 + zz[..., 3 * q:]
    return x.float()


@pytest.mark.parametrize("source", ["head", "records", "accumulate"])
@pytest.mark.parametrize("n", [2, 3])
def test_head_batch_statistics_conditioning_edges(lib, source, n):
    """BatchNorm statistics of the head from each of its three sources on ill-conditioned columns (see conditioning_features)
    at n = 2 and 3, where the unbiased running-variance factor n / (n - 1) is 2 and 1.5.  A naive E[x^2] - E[x]^2 in fp32
    is off by ~1e-3 at mean / sd = 100; every statistic, the loss, probs, dym and the head gradients here must be within
    1e-4 of float64 (element-relative for the statistics: the zero-variance columns' invstd = 1 / sqrt(eps) must not mask the
    others)."""
    S, d, C = 2, 128, 19
    x = conditioning_features(S, n, d, 40 + n)
    prm = head_params(d, C, 50 + n)
    tgt = (torch.rand(n, C, generator=torch.Generator().manual_seed(n)) < 0.3).float()
    out = fused_step(lib, x.to(DEV), prm, tgt.to(DEV), source=source)
    ref = ref_head_train(out["xn"].cpu(), prm, tgt)
    assert abs(out["loss"].item() - ref["loss"].item()) < 1e-4 * max(1.0, abs(ref["loss"].item()))
    for k in ("save_mean", "save_invstd", "rm", "rv"):
        _check(k, out[k], ref[k], a=1e-7, r=1e-4)
    assert int(out["nbt"].item()) == 5 + S
    for k in ("probs", "dym"):
        _check(k, out[k], ref[k], a=1e-4, r=1e-4)
    check_head_grads(out, ref, a=1e-4)


ENGINE_CASES = [(128, C, p) for C in (225, 240, 256) for p in (0.0, 0.3)] + [(256, 240, 0.2)]


@pytest.mark.parametrize("d,C,p", ENGINE_CASES)
def test_every_head_gradient_through_the_engine_matches_float64(lib, d, C, p):
    """A one-layer ChromeGCN through forward_loss (ops.LastLayerHeadLossFn: cgcn_layer_fwd -> cgcn_head_train -> cgcn_layer_bwd
    in head mode) at C > 128 (256-row partial layout, two label passes), with and without dropout, in both product forms
    (d = 128), both statistics modes (records, accumulate) and with input_grad on and off (off: the head's second stage rides in
    the row-local launch): loss, probs, dX and every parameter gradient against a float64 restatement with the head's mask
    made explicit."""
    import copy
    import chromegcn_amd as CG
    from oracle import chromegcn_oracle as O
    S, n = 2, 1000
    a = O.random_symmetric_graph(n, 4 * n, 3)
    graph = CG.process_graph("hic", {"c": a}, n, "c", device=DEV)
    A64 = torch.from_numpy(O.normalized_adjacency("hic", a, n).toarray()).double()
    torch.manual_seed(C + d + int(10 * p))
    m0 = CG.ChromeGCN(d, d, C, p, True, 1)
    with torch.no_grad():
        m0.GC1.weight.copy_(torch.randn(d, d) / np.sqrt(d) * 1.5)
        for q in (m0.GC1.bias, m0.W1.bias, m0.batch_norm.bias, m0.out.bias):
            q.copy_(torch.randn_like(q) * 0.2)
        m0.batch_norm.weight.copy_(1 + 0.2 * torch.randn(d))
        m0.batch_norm.running_var.copy_(1 + 0.3 * torch.rand(d))
        m0.out.weight.copy_(torch.randn(C, d) / np.sqrt(d) * 2)
    x = torch.randn(S, n, d)
    tgt = (torch.rand(n, C) < 0.2).float()
    maskh = _probe_mask(S * n, d, p, 77, 3).view(S, n, d).double() if p > 0 else None
    m64 = copy.deepcopy(m0).double().train()
    x64 = x.double().requires_grad_(True)
    logits = []
    for s in range(S):
        h = x64[s]
        zz = torch.tanh(A64 @ (h @ m64.GC1.weight) + m64.GC1.bias)
        gg = torch.sigmoid(m64.W1(zz))
        h = (1 - gg) * h + gg * zz
        y = m64.batch_norm(F.relu(h))
        if maskh is not None:
            y = y * maskh[s] / (1 - p)
        logits.append(m64.out(y))
    loss64 = F.binary_cross_entropy_with_logits(sum(logits) / S, tgt.double())
    loss64.backward()
    probs64 = torch.sigmoid(sum(logits) / S).detach()
    p64 = dict(m64.named_parameters())
    for form in (FORMS if d == 128 else ["split"]):
        lib.cgcn_debug_set_products(FORMS[form])
        for acc in (False, True):
            for ig in (True, False):
                what = "%s acc=%s input_grad=%s" % (form, acc, ig)
                m = copy.deepcopy(m0).to(DEV).train()
                m._rng_managed = True          # the test pins the step counter itself
                m.seed_dropout(77)
                m._rng_state[1] = 3
                xg = x.to(DEV).requires_grad_(ig)
                loss, probs, _ = m.forward_loss(xg, graph, tgt.to(DEV), stat_acc=acc)
                loss.backward()
                assert abs(loss.item() - loss64.item()) < 2e-5, what
                _check("probs " + what, probs, probs64, a=1e-5, r=1e-4)
                if ig:
                    _check("dX " + what, xg.grad, x64.grad, a=1e-4, r=1e-4)
                for k, q in m.named_parameters():
                    _check(k + " " + what, q.grad, p64[k].grad, a=1e-4, r=1e-4)
                _check("running_var " + what, m.batch_norm.running_var, m64.batch_norm.running_var, a=1e-6, r=1e-5)
                assert int(m.batch_norm.num_batches_tracked.item()) == S
