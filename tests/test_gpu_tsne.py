"""The t-SNE kernels (chromegcn_amd/csrc/cgcn_tsne.hip), their driver (chromegcn_amd.tsne) and the hidden-state selection
(chromegcn_amd.embed) against the numpy restatements that tests/test_tsne_host.py pins to scikit-learn.

Single evaluations and short runs are compared tightly; a long run only by the objective it reaches, because a t-SNE
trajectory is chaotic (two correct implementations are the embedding's whole extent apart after 50 iterations)."""
import functools

import numpy as np
import pytest
import torch

import chromegcn_amd as C
from chromegcn_amd import _lib, embed, synth, tsne

pytestmark = pytest.mark.gpu
DEV = "cuda"
BAD_ARG, UNSUPPORTED = -1, -2
NS = [2, 63, 64, 65, 257]
# One n above every tile the kernels use (64 x 64 tiles of D and P, 8 rows of P per workgroup, 2 048 columns of Y per LDS
# chunk) and a multiple of none of them, nor of the 4 floats of a 16-byte load: a prime
N_LARGE = 2053
# Seeds of the affinity tests' points, chosen on the CPU so that no row of any case is ever within 1e-9 of the search's
# stopping threshold (conditional_probabilities_host's `margin`): the float64 sums of the kernel and of numpy differ by
# ~1e-15, so a row cannot stop one step earlier or later in one of them, and no row needs an exemption.
AFFINITY_SEEDS = {63: 0, 64: 0, 65: 4, 257: 1}


def _pitched(a, fill=float("nan")):
    """the n x n matrix `a` on the device in the library's layout; the pad columns hold `fill` (never read for their value)"""
    n = len(a)
    buf = torch.full((n, tsne._pitch(n)), fill, device=DEV, dtype=torch.float32)
    buf[:, :n] = torch.from_numpy(np.asarray(a, np.float32)).to(DEV)
    return buf[:, :n]


def _points(n, d, seed, special=True):
    x = np.random.RandomState(seed).standard_normal((n, d)).astype(np.float32)
    if special and n >= 8:
        x[5] = x[2]                      # two identical rows
        x[n - 1] = 1000.0 * x[n - 1]     # one far outlier
    return x


@functools.lru_cache(maxsize=None)
def _affinity_case(n):
    D = tsne.sqdist_host(_points(n, 16, AFFINITY_SEEDS[n], special=False)).astype(np.float32)
    return D, {p: tsne.joint_probabilities_host(D, p, return_info=True) for p in (2, 5, 30) if p < n}


@functools.lru_cache(maxsize=None)
def _host_P(n):
    """joint probabilities of n clustered points from the host restatement, as the fp32 matrix the kernels read"""
    rng = np.random.RandomState(100 + n)
    x = (rng.standard_normal((n, 8)) + 3.0 * rng.randint(0, 3, (n, 1))).astype(np.float32)
    perplexity = {2: 1.0, 3: 1.5}.get(n, 30.0)
    return tsne.joint_probabilities_host(tsne.sqdist_host(x).astype(np.float32), perplexity).astype(np.float32)


def _embedding(n, form):
    rng = np.random.RandomState(n)
    if form == "start":
        return (1e-4 * rng.standard_normal((n, 2))).astype(np.float32)
    if form == "unit":
        return rng.standard_normal((n, 2)).astype(np.float32)
    y = rng.standard_normal((n, 2)).astype(np.float32)     # two clusters 1e6 apart: w / Z falls below eps between them
    y[n // 2:, 0] += np.float32(1e6)
    return y


@pytest.fixture(scope="module")
def fixture(golden):
    f = golden("g8_tsne.npz")
    P = tsne.joint_probabilities_host(tsne.sqdist_host(f["X"]).astype(np.float32), 30.0).astype(np.float32)
    return {"X": f["X"], "Y0": f["Y0"], "P": P, "kl_bound": float(f["kl_bound"])}


@pytest.mark.parametrize("d", [4, 36, 100, 128, 256])     # 36 and 100: a partly filled slice of 32 features behind a full one
@pytest.mark.parametrize("n", NS)
def test_sqdist(n, d):
    x = _points(n, d, 7 * n + d)
    D = tsne.sqdist(torch.from_numpy(x).to(DEV))
    assert D.shape == (n, n) and D.stride() == (tsne._pitch(n), 1)
    got = D.cpu().numpy()
    ref = tsne.sqdist_host(x)
    err = np.abs(got - ref).max(1)
    print("sqdist n=%d d=%d: worst error / row maximum = %.3g" % (n, d, (err / ref.max(1)).max()))
    assert np.all(err <= 1e-5 * ref.max(1))
    if n >= 8:
        # The outlier makes every row's largest distance ~1e6 d, so the bound above only holds the outlier's row and column
        # to their scale.  The ordinary entries are held to theirs: the same bound with the outlier left out of both the
        # entries and the row maximum.
        inner, inner_ref = got[:n - 1, :n - 1], ref[:n - 1, :n - 1]
        err = np.abs(inner - inner_ref).max(1)
        print("sqdist n=%d d=%d: without the outlier, worst error / row maximum = %.3g" % (n, d, (err / inner_ref.max(1)).max()))
        assert np.all(err <= 1e-5 * inner_ref.max(1))
        # and entry by entry: a sum of d squares in fp32 is within (d + 2) 2^-24 of its value
        np.testing.assert_allclose(got, ref, rtol=(d + 2) * 2.0 ** -24, atol=0)
    assert np.all(np.diag(got) == 0)
    assert np.array_equal(got.view(np.uint32), got.T.view(np.uint32))           # bitwise symmetric
    if n >= 8:
        assert got[2, 5] == 0 and np.array_equal(got[2], got[5])
    assert torch.equal(tsne.sqdist(torch.from_numpy(x).to(DEV)), D)


@pytest.mark.parametrize("perplexity", [2, 5, 30])
@pytest.mark.parametrize("n", NS)
def test_affinities_and_symmetrisation(n, perplexity):
    if perplexity >= n:
        with pytest.raises(ValueError, match="less than n_samples"):
            tsne.TsneAffinities(torch.zeros(n, 4, device=DEV)).joint(perplexity)
        return
    D, cases = _affinity_case(n)
    P_ref, info = cases[perplexity]
    assert info["margin"].min() > 1e-9, "choose another seed: a row sits on the stopping threshold"
    Dg = _pitched(D)
    Cg, beta = tsne.affinities(Dg, perplexity)
    np.testing.assert_allclose(beta.cpu().numpy(), info["beta"], rtol=1e-9, atol=0)
    np.testing.assert_allclose(Cg.cpu().numpy(), info["conditional"].astype(np.float32), rtol=1e-6, atol=1e-12)
    P = tsne.symmetrize(Cg)
    got = P.cpu().numpy()
    rel = np.abs(got - P_ref.astype(np.float32)) / np.maximum(P_ref, 1e-300)
    print("P n=%d perplexity=%d: worst relative error %.3g" % (n, perplexity, rel[P_ref > 1e-6 * P_ref.max()].max()))
    np.testing.assert_allclose(got, P_ref.astype(np.float32), rtol=1e-6, atol=1e-12)
    assert abs(got.astype(np.float64).sum() - 1.0) <= 1e-6
    assert np.all(np.diag(got) == 0) and np.array_equal(got, got.T)
    # in place gives the same matrix, and a second call the same bits
    C2, beta2 = tsne.affinities(Dg, perplexity)
    assert torch.equal(C2, Cg) and torch.equal(beta2, beta)
    assert torch.equal(tsne.symmetrize(C2, out=C2), P)


@pytest.mark.parametrize("exaggeration", [1.0, 12.0])
@pytest.mark.parametrize("form", ["start", "unit", "apart"])
@pytest.mark.parametrize("n", [2, 3, 65, 257, 700, N_LARGE])
def test_gradient_and_kl(n, form, exaggeration):
    P_host, y = _host_P(n), _embedding(n, form)
    kl_ref, g_ref, Z_ref = tsne.kl_gradient_host(P_host, y, exaggeration)
    if form == "apart" and n >= 257:
        assert 1.0 / (1.0 + 1e12) / Z_ref < tsne.EPS                              # the clamp of Q is active
    P, Y = _pitched(P_host), torch.from_numpy(y).to(DEV)
    ws = tsne.workspace(n, DEV)
    grad, plain = torch.empty_like(Y), torch.empty_like(Y)
    tsne.kl_gradient(P, Y, exaggeration, grad, True, ws)
    upd, gains, rec = torch.zeros_like(Y), torch.ones_like(Y), torch.zeros(4, device=DEV, dtype=torch.float64)
    Y_step = Y.clone()
    tsne.update_step(Y_step, upd, gains, grad, 0.5, 50.0, True, rec, ws)
    kl, gnorm, Z, _ = rec.tolist()
    g = grad.cpu().numpy()
    print("gradient n=%d %s e=%g: |g - ref| / max|g| = %.3g, KL %.9g against %.9g, Z %.9g against %.9g"
          % (n, form, exaggeration, np.abs(g - g_ref).max() / max(np.abs(g_ref).max(), 1e-300), kl, kl_ref, Z, Z_ref))
    assert np.abs(g - g_ref).max() <= 1e-4 * np.abs(g_ref).max()
    np.testing.assert_allclose(kl, kl_ref, rtol=1e-5, atol=0)
    np.testing.assert_allclose(Z, Z_ref, rtol=1e-5)
    np.testing.assert_allclose(gnorm, np.linalg.norm(0.8 * g.astype(np.float64)), rtol=1e-6)
    # without the KL: the same gradient, and the record says NaN
    tsne.kl_gradient(P, Y, exaggeration, plain, False, ws)
    tsne.update_step(Y.clone(), torch.zeros_like(Y), torch.ones_like(Y), plain, 0.5, 50.0, False, rec, ws)
    assert np.isnan(rec[0].item())
    assert torch.equal(plain, grad)
    again = torch.empty_like(Y)
    tsne.kl_gradient(P, Y, exaggeration, again, True, ws)
    assert torch.equal(again, grad)
    if n > 512:
        _check_update_from_a_random_state(n, Y, grad, rec, ws)


def _check_update_from_a_random_state(n, Y, grad, rec, ws):
    """k_tsne_update is one workgroup of 1024 threads that strides over the 2 n values: at 2 n > 1024 there is a second trip.
    From a seeded non-zero `update` and gains in [0.01, 2] (both branches of the gain rule, and its floor), Y, update and
    gains after one step against the rule in float32 numpy on the device's own gradient: gains within one ulp; update within
    2^-23 (|momentum u| + |lr g gain|) -- one rounding of each product and one of the difference, or fewer when the compiler
    contracts them --; Y within that plus 2^-23 |Y|; the gradient-norm record as above."""
    assert 2 * n > 1024
    rng = np.random.RandomState(n + 1)
    f32 = np.float32
    g, y0 = grad.cpu().numpy(), Y.cpu().numpy()
    u0 = (np.abs(g).max() * 50.0 * rng.standard_normal((n, 2))).astype(f32)     # the size of a step: lr x gradient
    gain0 = rng.uniform(0.01, 2.0, (n, 2)).astype(f32)
    gain0[rng.random_sample((n, 2)) < 0.05] = f32(0.01)                          # 0.8 x 0.01 is below the floor
    momentum, lr = f32(0.8), f32(200.0)
    inc = u0 * g < 0
    assert 0.2 < inc.mean() < 0.8 and inc[:512].any() and inc[512:].any() and (~inc[512:]).any()   # row 512 on: the second trip
    gain = np.maximum(np.where(inc, gain0 + f32(0.2), gain0 * f32(0.8)), f32(0.01)).astype(f32)
    assert (gain == f32(0.01)).any() and gain.dtype == f32
    gg = g * gain
    u = momentum * u0 - lr * gg
    y = y0 + u
    assert u.dtype == f32 and y.dtype == f32
    Yd, ud, gd = Y.clone(), torch.from_numpy(u0).to(DEV), torch.from_numpy(gain0).to(DEV)
    tsne.update_step(Yd, ud, gd, grad, float(momentum), float(lr), False, rec, ws)
    got_y, got_u, got_gain = Yd.cpu().numpy(), ud.cpu().numpy(), gd.cpu().numpy()
    e = 2.0 ** -23
    size_u = np.abs(momentum * u0).astype(np.float64) + np.abs(lr * gg)
    err_gain = np.abs(got_gain - gain) / np.spacing(gain)
    err_u, err_y = np.abs(got_u.astype(np.float64) - u) / (e * size_u), np.abs(got_y.astype(np.float64) - y) / (e * (size_u + np.abs(y0)))
    print("update n=%d: gains off by %.3g ulp; update %.3g, Y %.3g of their bounds; rows of the second trip: update %.3g, Y %.3g"
          % (n, err_gain.max(), err_u.max(), err_y.max(), err_u[512:].max(), err_y[512:].max()))
    assert err_gain.max() <= 1 and err_u.max() <= 1 and err_y.max() <= 1
    np.testing.assert_allclose(rec[1].item(), np.linalg.norm((g.astype(np.float64) * gain.astype(np.float64)).ravel()), rtol=1e-6)


def test_ten_updates_through_the_c_abi(fixture):
    """Y, update and gains after ten iterations against tsne_embed_host(dtype='float32'), each at 1e-4 of its own scale (the
    embedding's extent for Y and the displacement `update`; the largest gain for `gains`): two fp32 forms were 4e-6 of the
    extent apart on the CPU at this point, the margin covers another summation order."""
    n = len(fixture["P"])
    Y_ref, info = tsne.tsne_embed_host(fixture["P"], fixture["Y0"], max_iter=10, dtype="float32")
    P, Y = _pitched(fixture["P"]), torch.from_numpy(fixture["Y0"]).to(DEV)
    ws = tsne.workspace(n, DEV)
    grad, upd, gains = torch.empty_like(Y), torch.zeros_like(Y), torch.ones_like(Y)
    rec = torch.zeros(4, device=DEV, dtype=torch.float64)
    for i in range(10):
        tsne.kl_gradient(P, Y, 12.0, grad, i == 9, ws)
        tsne.update_step(Y, upd, gains, grad, 0.5, info["learning_rate"], i == 9, rec, ws)
    extent = np.ptp(Y_ref)
    errs = [np.abs(t.cpu().numpy() - r).max() for t, r in ((Y, Y_ref), (upd, info["update"]), (gains, info["gains"]))]
    print("ten updates: Y %.3g, update %.3g of the extent; gains %.3g of the largest" %
          (errs[0] / extent, errs[1] / extent, errs[2] / info["gains"].max()))
    assert errs[0] <= 1e-4 * extent and errs[1] <= 1e-4 * extent and errs[2] <= 1e-4 * info["gains"].max()
    np.testing.assert_allclose(rec[0].item(), info["kl_divergence"], rtol=1e-5)


def test_whole_run_reaches_the_recorded_objective_twice_the_same(fixture):
    z = torch.from_numpy(fixture["X"]).to(DEV)
    Y, info = tsne.tsne_embed(z, perplexity=30.0, max_iter=1000, init=fixture["Y0"])
    print("whole run: KL %.6f (bound %.6f) after %d iterations; checks %s" %
          (info["kl_divergence"], fixture["kl_bound"], info["n_iter"] + 1, info["checks"]))
    assert Y.shape == (384, 2) and Y.dtype == torch.float32 and Y.is_cuda and bool(torch.isfinite(Y).all())
    assert info["kl_divergence"] <= fixture["kl_bound"]
    late = [kl for it, kl in info["checks"] if it > 300]
    assert len(late) >= 2 and all(b <= a + 1e-3 for a, b in zip(late, late[1:]))
    assert info["learning_rate"] == 50.0 and info["checks"][0][0] == 50
    Y2, info2 = tsne.tsne_embed(z, perplexity=30.0, max_iter=1000, init=torch.from_numpy(fixture["Y0"]))
    assert torch.equal(Y, Y2) and info2 == info


def test_sweep_equals_separate_runs(fixture):
    z = torch.from_numpy(fixture["X"]).to(DEV)
    sweep = tsne.tsne_sweep(z, [5, 30], max_iter=300, seed=3)
    assert len(sweep) == 2
    for (Y, info), p in zip(sweep, [5, 30]):
        Y1, info1 = C.tsne_embed(z, perplexity=p, max_iter=300, seed=3)
        assert torch.equal(Y, Y1) and info == info1
    assert not torch.equal(sweep[0][0], sweep[1][0])


def _model(d, layers, n_labels=8, seed=0):
    torch.manual_seed(seed)
    model = C.ChromeGCN(d, d, n_labels, 0.3, True, layers)
    with torch.no_grad():
        for k, p in model.named_parameters():
            if "GC" in k and k.endswith("weight"):
                p.copy_(torch.randn_like(p) / np.sqrt(d) * 1.5)
        model.batch_norm.running_mean.copy_(torch.randn(d) * 0.1)
        model.batch_norm.running_var.copy_(torch.rand(d) + 0.5)
    return model.to(DEV).eval()


def _chromosome(n, d, n_labels, seed):
    feats = synth.chrom_features(n, d, n_labels, seed)
    graph = C.process_graph("hic", {"c": synth.contact_graph(n, 4 * n, seed)}, n, "c", device=DEV)
    return feats["forward"].to(DEV), feats["backward"].to(DEV), graph


@pytest.mark.parametrize("layers", [1, 2])
@pytest.mark.parametrize("d", [128, 256])
def test_hidden_strands_feed_the_head(d, layers):
    model = _model(d, layers)
    xf, xr, graph = _chromosome(257, d, 8, 5)
    x = torch.stack([xf, xr])
    with torch.no_grad():
        want = model.forward_strands(x, graph)[0]
        h = model.hidden_strands(x, graph)
        assert h.shape == (2, 257, d) and not h.requires_grad
        assert torch.equal(model._head(h), want)
    h_grad_mode = model.hidden_strands(x, graph)                 # no autograd whatever the caller's mode
    assert not h_grad_mode.requires_grad and torch.equal(h_grad_mode, h)
    model.train()
    assert torch.equal(model.hidden_strands(x, graph), h) and model.training     # the eval forward; the flag stays
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model.hidden_strands(x.cpu(), graph)


def test_class_embeddings_equal_the_numpy_selection():
    d, n_labels, min_count = 128, 6, 12
    model = _model(d, 2, n_labels)
    chroms = [_chromosome(257, d, n_labels, 11), _chromosome(131, d, n_labels, 12)]
    rng = np.random.RandomState(4)
    targets = []
    for n in (257, 131):     # rows with 0, 1 and 2 positives; label 4 stays below min_count over both chromosomes
        t = np.zeros((n, n_labels), np.float32)
        kind = rng.randint(0, 3, n)
        lab = rng.choice(n_labels, n, p=[0.3, 0.25, 0.2, 0.15, 0.02, 0.08])
        t[kind >= 1, lab[kind >= 1]] = 1.0
        t[kind == 2, (lab[kind == 2] + 1) % n_labels] = 1.0
        targets.append(t)
    strands = [model.hidden_strands(torch.stack([xf, xr]), g).cpu().numpy() for xf, xr, g in chroms]
    hidden = np.concatenate([(h[0] + h[1]) / np.float32(2) for h in strands])
    for labels in (None, [0, 3, 4]):
        rows_ref, lab_ref = embed.select_single_label_host(targets, labels, min_count)
        assert len(rows_ref) > 0 and 4 not in lab_ref
        z, lab, rows = C.class_embeddings(model, [c[0] for c in chroms], [c[1] for c in chroms], [c[2] for c in chroms],
                                          [torch.from_numpy(t) for t in targets], labels=labels, min_count=min_count)
        assert z.is_cuda and lab.dtype == rows.dtype == torch.int64
        assert rows.cpu().tolist() == rows_ref.tolist() and lab.cpu().tolist() == lab_ref.tolist()
        assert np.array_equal(z.cpu().numpy(), hidden[rows_ref])
    # one chromosome, not in a list
    xf, xr, g = chroms[0]
    z, lab, rows = C.class_embeddings(model, xf, xr, g, torch.from_numpy(targets[0]).to(DEV), min_count=min_count)
    rows_ref, lab_ref = embed.select_single_label_host(targets[0], None, min_count)
    assert rows.cpu().tolist() == rows_ref.tolist() and lab.cpu().tolist() == lab_ref.tolist() and z.shape == (len(rows_ref), d)


def test_class_map_tool_writes_what_it_says(tmp_path):
    """tools/class_map.py end to end on one synthetic chromosome: the files it names, consistent with each other"""
    import importlib.util
    import json
    import os
    spec = importlib.util.spec_from_file_location("class_map", os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "tools", "class_map.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    out = str(tmp_path / "maps")
    tool.main(["-synthetic", "-synthetic_chroms", "chr21", "--min-count", "2", "--perplexities", "5,30", "--max-iter", "100",
               "--out", out])
    z, lab, rows = (np.load(os.path.join(out, f)) for f in ("z.npy", "labels.npy", "rows.npy"))
    feats, _ = synth.synthetic_chromosome("chr21")
    rows_ref, lab_ref = embed.select_single_label_host(feats["target"].numpy(), None, 2)
    assert len(rows_ref) >= 31 and rows.tolist() == rows_ref.tolist() and lab.tolist() == lab_ref.tolist()
    assert z.shape == (len(rows), 128) and z.dtype == np.float32 and np.isfinite(z).all()
    summary = json.load(open(os.path.join(out, "summary.json")))
    assert summary["windows"] == len(rows) and [r["perplexity"] for r in summary["runs"]] == [5.0, 30.0]
    for r in summary["runs"]:
        y = np.load(os.path.join(out, "embedding_p%g.npy" % r["perplexity"]))
        assert y.shape == (len(rows), 2) and y.dtype == np.float32 and np.isfinite(y).all()
        assert r["iterations"] == 100 and np.isfinite(r["kl_divergence"])


def test_state_tensors_are_checked_before_the_call():
    n = 16
    P = tsne.TsneAffinities(torch.randn(n, 8, device=DEV)).joint(5)
    ws = tsne.workspace(n, DEV)
    Y, rec = torch.zeros(n, 2, device=DEV), torch.zeros(4, device=DEV, dtype=torch.float64)
    good = dict(Y=Y, update=torch.zeros_like(Y), gains=torch.ones_like(Y), grad=torch.zeros_like(Y))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tsne.kl_gradient(P, Y.cpu(), 1.0, good["grad"], False, ws)
    with pytest.raises(RuntimeError, match="float32"):
        tsne.kl_gradient(P, Y, 1.0, good["grad"].double(), False, ws)
    with pytest.raises(ValueError, match=r"\[n, 2\]"):
        tsne.kl_gradient(P, torch.zeros(n + 1, 2, device=DEV), 1.0, good["grad"], False, ws)
    with pytest.raises(ValueError, match="workspace"):
        tsne.kl_gradient(P, Y, 1.0, good["grad"], False, ws.cpu())
    for name in good:
        for bad in (good[name].cpu(), torch.zeros(n, 4, device=DEV)[:, :2], torch.zeros(n - 1, 2, device=DEV)):
            with pytest.raises((RuntimeError, ValueError)):
                tsne.update_step(**dict(good, **{name: bad}), momentum=0.5, learning_rate=50.0, have_kl=False, record=rec, ws=ws)
    with pytest.raises(ValueError, match="record"):
        tsne.update_step(**good, momentum=0.5, learning_rate=50.0, have_kl=False, record=rec.float(), ws=ws)
    with pytest.raises(ValueError, match="init must be"):
        tsne.tsne_embed(torch.randn(n, 8, device=DEV), perplexity=5, init=np.zeros((n, 3), np.float32))


def test_unsupported_shapes_and_cpu_tensors_are_refused():
    lib = _lib.load()
    big = 46341                                                          # 46341^2 >= 2^31
    assert _lib.query("cgcn_tsne_workspace_bytes", n=big) == 0 and _lib.query("cgcn_tsne_workspace_bytes", n=1) == 0
    assert _lib.query("cgcn_tsne_workspace_bytes", n=46340) > 0
    ld = tsne._pitch(big)
    # the shape is judged before any pointer: NULL everywhere still says unsupported, and nothing was launched
    assert lib.cgcn_tsne_sqdist(None, big, 128, ld, None, None) == UNSUPPORTED
    assert lib.cgcn_tsne_affinities(None, big, ld, None, 30.0, None, None) == UNSUPPORTED
    assert lib.cgcn_tsne_symmetrize(None, big, ld, None, None, None, 0) == UNSUPPORTED
    assert lib.cgcn_tsne_gradient(None, big, ld, None, None, 1.0, None, 0, None, 0) == UNSUPPORTED
    assert lib.cgcn_tsne_update(None, big, None, None, None, None, 0.5, 50.0, 0, None, None, 0) == UNSUPPORTED
    assert lib.cgcn_tsne_sqdist(None, 64, 6, 64, None, None) == UNSUPPORTED              # d % 4
    assert lib.cgcn_tsne_sqdist(None, 65, 8, 65, None, None) == UNSUPPORTED              # a pitch that is no multiple of 4
    assert lib.cgcn_tsne_sqdist(None, 64, 8, 64, None, None) == BAD_ARG                  # supported shape, NULL pointers
    assert lib.cgcn_tsne_gradient(None, 64, 64, None, None, 1.0, None, 0, None, 0) == BAD_ARG
    with pytest.raises(RuntimeError, match="unsupported"):
        tsne.sqdist(torch.zeros(8, 6, device=DEV))
    with pytest.raises(RuntimeError, match="unsupported"):
        tsne.sqdist(torch.zeros(1, 8, device=DEV))
    z = torch.randn(16, 8, device=DEV)
    for p in (16, 30.0):
        with pytest.raises(ValueError, match="less than n_samples"):
            tsne.tsne_embed(z, perplexity=p)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tsne.tsne_embed(z.cpu(), perplexity=5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tsne.tsne_sweep(z.cpu(), [5])
    ws = tsne.workspace(16, DEV)
    P = tsne.TsneAffinities(z).joint(5)
    with pytest.raises(RuntimeError, match="workspace"):
        _lib.call("cgcn_tsne_gradient", n=16, ld=16, P=P, Y=z[:, :2].contiguous(), exaggeration=1.0,
                  grad=torch.empty(16, 2, device=DEV), want_kl=0, workspace=ws, workspace_bytes=ws.numel() - 1)
    with pytest.raises(ValueError, match="row pitch"):
        tsne.affinities(torch.zeros(5, 5, device=DEV), 2.0)
