"""Every dropout mask the kernels draw against its numpy statement (tests/dropout_ref.py), and the training paths that depend
on all of them agreeing:

  (a) the forward sites -- k_layer_fwd, k_layer_dense, k_layer_dense256 behind the fused, the forced two-launch, the band and
      the band-plus route -- bit for bit, scale included, with the route asked from the library before every probe;
  (b) the backward sites -- k_bwd_sliced (16-bit, 32-bit and explicit-value instances, band plus) and k_bwd_band -- bit for bit,
      and paired with the forward mask of the layer before, as the model pairs them;
  (c) whole models (three layers, d = 256, the two-launch route, 'constant' / 'both' graphs, one strand) against a float64
      restatement of models/ChromeModels.py:34-52 + finetune.py:43-45 whose masks come from the restatement;
  (d) the stage engine step by step -- eager and captured, fused SGD, fused Adam, d = 256 -- against a float64 model stepped
      by torch's optimizers with the masks of counter c0 + t, and a control that a counter frozen at c0 is told apart.

Nothing here takes a mask from the GPU: a change of the hash, the key schedule, the threshold rule, a stream id or an element
index in any one kernel fails (a) or (b); a counter that a captured graph froze or a step forgot to advance fails (d)."""
import copy
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch
import torch.nn.functional as F

import chromegcn_amd as C
import dropout_ref as R
from chromegcn_amd import _lib, graph as G, ops, synth
from chromegcn_amd.finetune import GCNStage
from oracle import chromegcn_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED_CTR = [(77, 3), (2 ** 40 + 5, 2 ** 32 + 7)]     # both halves of the seed and of the counter
PS = (0.1, 0.5, 0.9)
FORMS = {"fp32_chain": 0, "split": 1}               # CGCN_PRODUCTS_* (include/chromegcn.h)


@pytest.fixture(autouse=True)
def _restore_library_switches():
    yield
    lib = _lib.load()
    lib.cgcn_debug_set_fwd_split_bytes(-1)
    lib.cgcn_debug_set_products(-1)


def _rng(seed, ctr):
    return torch.tensor([seed, ctr], dtype=torch.int64, device=DEV)


def _want(seed, ctr, stream, shape, p):
    """what a probe must return: kept elements hold exactly keep_scale, dropped ones 0"""
    return R.mask(seed, ctr, stream, shape, p).astype(np.float32) * R.keep_scale(p)


@functools.lru_cache(maxsize=None)
def _contacts(n):
    """a symmetric {0,1} contact matrix with entries inside and outside the +-7 band (so that 'both' has values 1 and 2)"""
    rng = np.random.RandomState(n)
    i, j = rng.randint(0, n, 3 * n), rng.randint(0, n, 3 * n)
    near = np.arange(0, n - 3, 5)
    i, j = np.concatenate([i, near]), np.concatenate([j, near + 3])
    keep = i != j
    m = sp.coo_matrix((np.ones(int(keep.sum())), (i[keep], j[keep])), shape=(n, n)).tocsr()
    m = sp.csr_matrix(m + m.T)
    m.data[:] = 1.0
    return m


def _graph(kind, n):
    """kind: 'hic' (16-bit indices), 'none', 'constant' (band), 'both' (band plus), 'asym' (explicit values, its transpose a
    CSR of its own: the HAS_VAL / int32 instances), 'hic32' (the 'hic' graph without a cgcn_graph_aux: int32 indices)"""
    if kind in ("none", "constant"):
        return G.upload(G.normalize_graph(kind, None, n), DEV)
    if kind in ("hic", "both"):
        return G.upload(G.normalize_graph(kind, _contacts(n), n), DEV)
    if kind == "asym":
        a = sp.random(n, n, density=min(1.0, 6.0 / n), random_state=n, format="csr", dtype=np.float32) + sp.identity(n, dtype=np.float32)
        g = G.upload(G.host_csr_from_matrix(a), DEV)
        assert not g.symmetric and g.val is not None and g.col_t is not g.col
        return g
    assert kind == "hic32"
    b = _graph("hic", n)
    col = b.col.clone()   # an index array nothing is registered for: no 16-bit copy, no row order
    g = G._MaskedGraph(n=n, nnz=b.nnz, rowptr=b.rowptr, col=col, val=None, row_scale=b.row_scale, rowptr_t=b.rowptr, col_t=col,
                       val_t=None, symmetric=True, host=None)
    assert G.aux_ptr(g.col) is None
    return g


# ---- (a) forward masks --------------------------------------------------------------------------------------------------
def _probe_fwd(g, S, d, p, rng, layer_id):
    """X = 0, W = 0, b = +30 -> Z = tanh(30) = 1; gate bias +30 -> g = 1; Xn = 1 before dropout: the output IS mask * keep_scale
    on any graph (H = A 0 = 0)"""
    W = torch.zeros(d, d, device=DEV); b = torch.full((d,), 30.0, device=DEV)
    wg = torch.zeros(1, d, device=DEV); cg = torch.full((1,), 30.0, device=DEV)
    xn, gate = ops.gated_layer(torch.zeros(S, g.n, d, device=DEV), W, b, wg, cg, g, dropout_out=p, rng_state=rng, layer_id=layer_id)
    assert torch.equal(gate, torch.ones_like(gate))
    return xn.cpu().numpy()


# route -> (graph kind, split threshold, cgcn_debug_layer_fwd_route, node counts)
ROUTES = {"builtin": ("hic", -1, 0, (333, 70, 9)), "two_launch": ("hic", 0, 1, (333, 70, 9)),
          "band": ("constant", -1, 2, (333, 70, 15)), "band_plus": ("both", -1, 1, (333, 70, 20))}


def _set_route(route, g, S, d):
    kind, split, want, _ = ROUTES[route]
    lib = _lib.load()
    lib.cgcn_debug_set_fwd_split_bytes(split)
    assert lib.cgcn_debug_layer_fwd_route(g.n, S, d, G.aux_ptr(g.col), 0) == want, (route, g.n, S, d)
    if route == "band":
        assert G.is_band(g.col)
    if route == "band_plus":
        assert G.has_band_plus(g.col) and g.val is not None
    if route == "builtin":      # ... and not because a hint forces the small table onto the sliced kernels
        assert not G.is_band(g.col) and not G.has_band_plus(g.col)


@pytest.mark.parametrize("S", [1, 2])
@pytest.mark.parametrize("d", [128, 256])
@pytest.mark.parametrize("route", list(ROUTES))
def test_forward_mask_is_the_restated_mask(route, d, S):
    """every layer id, both (seed, counter) pairs, every p and every node count on every route x d x S"""
    kind, _, _, ns = ROUTES[route]
    base = list(ROUTES).index(route) + (d == 256) + 2 * (S == 2)
    for j, layer_id in enumerate((1, 2, 3)):
        n, p = ns[(base + j) % 3], PS[(base // 3 + j) % 3]
        for seed, ctr in (SEED_CTR if j == 0 else [SEED_CTR[j % 2]]):
            g = _graph(kind, n)
            _set_route(route, g, S, d)
            got = _probe_fwd(g, S, d, p, _rng(seed, ctr), layer_id)
            np.testing.assert_array_equal(got, _want(seed, ctr, layer_id, (S, n, d), p),
                                          err_msg="%s S=%d n=%d d=%d p=%g layer %d seed %d counter %d" % (route, S, n, d, p, layer_id, seed, ctr))


@pytest.mark.parametrize("S", [1, 2])
@pytest.mark.parametrize("d", [128, 256])
@pytest.mark.parametrize("route", ["builtin", "two_launch", "band"])
def test_forward_mask_on_one_node(route, d, S):
    """every one-node graph with its diagonal IS the band, and is recognised as one: the other two routes are reached at
    n = 1 only by a graph that carries no cgcn_graph_aux"""
    g = _graph("constant" if route == "band" else "hic32", 1)
    assert g.n == 1 and g.nnz == 1
    _set_route(route, g, S, d)
    seed, ctr = SEED_CTR[1]
    np.testing.assert_array_equal(_probe_fwd(g, S, d, 0.5, _rng(seed, ctr), 2), _want(seed, ctr, 2, (S, 1, d), 0.5))


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("route", ["builtin", "two_launch"])
def test_forward_mask_under_both_product_forms(route, form):
    """d = 128: k_layer_fwd and k_layer_dense are instantiated once per form of the dense products"""
    lib = _lib.load()
    lib.cgcn_debug_set_products(FORMS[form])
    assert lib.cgcn_debug_get_products() == FORMS[form]
    for S, n, layer_id, (seed, ctr) in ((2, 333, 1, SEED_CTR[1]), (1, 70, 3, SEED_CTR[0])):
        g = _graph("hic", n)
        _set_route(route, g, S, 128)
        np.testing.assert_array_equal(_probe_fwd(g, S, 128, 0.1, _rng(seed, ctr), layer_id), _want(seed, ctr, layer_id, (S, n, 128), 0.1))


def test_forward_probe_tells_neighbouring_keys_apart():
    """negative control: the masks of the next step, the next stream and the seed whose HIGH half differs each disagree with
    the kernel's in about 2 p (1 - p) = 32 % of the elements"""
    S, n, d, p, layer_id = 2, 333, 128, 0.2, 1
    seed, ctr = SEED_CTR[0]
    g = _graph("hic", n)
    _set_route("builtin", g, S, d)
    got = _probe_fwd(g, S, d, p, _rng(seed, ctr), layer_id) != 0
    assert np.array_equal(got, R.mask(seed, ctr, layer_id, (S, n, d), p))
    for other in ((seed, ctr + 1, layer_id), (seed, ctr, layer_id + 1), (seed + 2 ** 32, ctr, layer_id)):
        differ = (got != R.mask(*other, (S, n, d), p)).mean()
        assert differ > 0.25, (other, differ)


# ---- (b) backward masks -------------------------------------------------------------------------------------------------
def _probe_bwd(g, S, d, p, rng, layer_id):
    """X = 0 and every parameter 0: Z = 0, g = 1/2, gamma = 0, dU = 1/2, dHs = dU W^T = 0; with d loss / d Xn = 1 and nothing
    from the gate, dX = (1 - g) * 1 = 1/2 before the input-dropout mask of stream layer_id - 1: dX IS mask * keep_scale / 2"""
    x = torch.zeros(S, g.n, d, device=DEV, requires_grad=True)
    W = torch.zeros(d, d, device=DEV); b = torch.zeros(d, device=DEV)
    wg = torch.zeros(1, d, device=DEV); cg = torch.zeros(1, device=DEV)
    xn, _ = ops.gated_layer(x, W, b, wg, cg, g, dropout_in=p, rng_state=rng, layer_id=layer_id)
    xn.sum().backward()
    return x.grad.cpu().numpy()


def _check_bwd_kernel(kind, g):
    """the graph is what its kind promises, i.e. cgcn_layer_bwd's last launch is the instance the case is meant to hit"""
    if kind == "constant":
        assert G.is_band(g.col_t) and g.val_t is None                              # k_bwd_band
    elif kind == "both":
        assert G.has_band_plus(g.col_t) and g.val_t is not None                    # k_bwd_sliced<.., uint16_t, BP>
    elif kind == "hic":
        assert g.val_t is None and G.col16_ptr(g.col_t) is not None and not G.is_band(g.col_t)   # k_bwd_sliced<.., false, uint16_t>
    elif kind == "hic32":
        assert g.val_t is None and G.aux_ptr(g.col_t) is None                      # k_bwd_sliced<.., false, int>
    else:
        assert g.val_t is not None and not G.has_band_plus(g.col_t)                # k_bwd_sliced<.., true, int>


BWD_KINDS = ["hic", "hic32", "asym", "both", "constant"]


@pytest.mark.parametrize("S", [1, 2])
@pytest.mark.parametrize("d", [128, 256])
@pytest.mark.parametrize("kind", BWD_KINDS)
def test_backward_mask_is_the_restated_mask_and_pairs_with_the_forward(kind, d, S):
    base = BWD_KINDS.index(kind) + (d == 256) + 2 * (S == 2)
    for j in range(2):
        n, layer_id, p = (333, 70)[(base + j) % 2], (2, 3, 4)[(base + j) % 3], PS[(base + 2 * j) % 3]
        seed, ctr = SEED_CTR[j]
        g = _graph(kind, n)
        _check_bwd_kernel(kind, g)
        what = "%s S=%d n=%d d=%d p=%g layer %d seed %d counter %d" % (kind, S, n, d, p, layer_id, seed, ctr)
        dx = _probe_bwd(g, S, d, p, _rng(seed, ctr), layer_id)
        np.testing.assert_array_equal(dx, _want(seed, ctr, layer_id - 1, (S, n, d), p) * np.float32(0.5), err_msg=what)
        # the pairing the model relies on: the layer before drops its output under the same stream id
        fwd = _probe_fwd(g, S, d, p, _rng(seed, ctr), layer_id - 1)
        assert np.array_equal(fwd != 0, dx != 0), what


# ---- (c) whole models against float64 with restated masks -------------------------------------------------------------------
def _ref_loss(m64, x64, A64, tgt64, p, seed, ctr):
    """float64 restatement of ChromeModels.py:34-52 (L layers) + finetune.py:43-45 on [S, n, d] with the masks made explicit:
    stream id k for the output of layer k, HEAD_STREAM_ID for the head; kept elements times the library's float32 scale"""
    S, n, d = x64.shape
    ks = float(R.keep_scale(p)) if p > 0 else 1.0

    def msk(stream):
        return torch.from_numpy(R.mask(seed, ctr, stream, (S, n, d), p)).double() * ks if p > 0 else 1.0

    h = x64
    for k in range(1, m64.n_layers + 1):
        gc, wk = getattr(m64, "GC%d" % k), getattr(m64, "W%d" % k)
        if k > 1:
            h = h * msk(k - 1)
        z = torch.tanh(torch.matmul(A64, torch.matmul(h, gc.weight)) + gc.bias)
        g = torch.sigmoid(wk(z))
        h = (1 - g) * h + g * z
    y = torch.stack([m64.batch_norm(F.relu(h[s])) for s in range(S)]) * msk(R.HEAD_STREAM_ID)
    return F.binary_cross_entropy_with_logits(m64.out(y).mean(0), tgt64)


def _dense_adjacency(adj, hic, n):
    return torch.from_numpy(O.normalized_adjacency(adj, hic, n).toarray()).double()


MODEL_CASES = {   # L, d, S, n, adjacency, forced two-launch route
    "L3-d256-hic": (3, 256, 2, 333, "hic", False),
    "L3-d128-two_launch": (3, 128, 2, 333, "hic", True),
    "L2-d128-constant": (2, 128, 2, 333, "constant", False),
    "L2-d256-both": (2, 256, 2, 333, "both", False),
    "L2-d128-one_strand": (2, 128, 1, 333, "hic", False),
}


@pytest.mark.parametrize("case", list(MODEL_CASES))
def test_model_with_dropout_matches_float64_with_restated_masks(case):
    """tolerances: test_two_layer_model_with_dropout_matches_float64_with_explicit_masks' own"""
    L, d, S, n, adj, split = MODEL_CASES[case]
    c, p, seed, ctr = 9, 0.3, 2 ** 40 + 5, 2 ** 32 + 7
    hic = _contacts(n) if adj in ("hic", "both") else None
    graph = G.upload(G.normalize_graph(adj, hic, n), DEV)
    A64 = _dense_adjacency(adj, hic, n)
    torch.manual_seed(4)
    m = C.ChromeGCN(d, d, c, p, True, L)
    with torch.no_grad():
        for k, q in m.named_parameters():
            if "GC" in k and k.endswith("weight"):
                q.copy_(torch.randn_like(q) / np.sqrt(d) * 1.5)
            elif q.dim() == 1:
                q.copy_(torch.randn_like(q) * 0.2)
    m64 = copy.deepcopy(m).double().train()
    m = m.to(DEV).train()
    m._rng_managed = True          # this test pins the step counter itself
    m.seed_dropout(seed)
    m._rng_state[1] = ctr
    x = torch.randn(S, n, d)
    tgt = (torch.rand(n, c) < 0.2).float()

    x64 = x.double().requires_grad_(True)
    loss64 = _ref_loss(m64, x64, A64, tgt.double(), p, seed, ctr)
    loss64.backward()

    lib = _lib.load()
    lib.cgcn_debug_set_fwd_split_bytes(0 if split else -1)
    want_route = {"constant": 2, "both": 1}.get(adj, 1 if split else 0)
    assert lib.cgcn_debug_layer_fwd_route(n, S, d, G.aux_ptr(graph.col), 0) == want_route
    xg = x.to(DEV).requires_grad_(True)
    loss, probs, gates = m.forward_loss(xg, graph, tgt.to(DEV))
    loss.backward()
    assert int(m._rng_state[1].item()) == ctr and len(gates) == L
    print("%s: loss %.7f, float64 %.7f, difference %.2e" % (case, loss.item(), loss64.item(), abs(loss.item() - loss64.item())))
    assert abs(loss.item() - loss64.item()) < 2e-5
    ref = x64.grad.numpy()
    got = xg.grad.cpu().numpy()
    print("  dX: max error %.2e of max |ref| %.2e" % (np.abs(got - ref).max(), np.abs(ref).max()))
    np.testing.assert_allclose(got, ref, atol=1e-4 * np.abs(ref).max(), rtol=1e-4)
    p64 = dict(m64.named_parameters())
    for k, q in m.named_parameters():
        r = p64[k].grad.numpy()
        np.testing.assert_allclose(q.grad.cpu().numpy(), r, atol=1e-4 * max(1e-6, np.abs(r).max()), rtol=1e-4, err_msg=k)


# ---- (d) the engine, step by step -------------------------------------------------------------------------------------------
ENGINE_P, ENGINE_C, ENGINE_SEED = 0.2, 11, 2 ** 40 + 5
ENGINE_C0 = 2 ** 32 - 2                     # the four steps run under counters 2^32 - 2 .. 2^32 + 1: the carry into the high half
ENGINE_ORDER = ("c1", "c2", "c1", "c2")
ENGINE_SIZES = {"c1": 400, "c2": 333}
TOL = dict(atol=1e-4, rtol=1e-4)            # the suite's
ADAM_TOL = dict(atol=2e-3, rtol=1e-3)       # tests/test_gpu_adam.py: Adam divides by sqrt(v), tiny gradients amplify fp32 differences


def _optimizer(kind, ps, double=False):
    if kind == "sgd":
        return torch.optim.SGD(ps, lr=0.25, momentum=0.9, weight_decay=1e-6)
    return torch.optim.Adam(ps, betas=(0.9, 0.98), lr=1e-3, **({} if double else dict(fused=True)))


def _engine_model(d):
    torch.manual_seed(0)
    m = C.ChromeGCN(d, d, ENGINE_C, ENGINE_P, True, 2)
    with torch.no_grad():
        for k, q in m.named_parameters():
            if "GC" in k and k.endswith("weight"):
                q.mul_(40)                  # xavier with gain 0.02 would leave the gated layers near the identity
        # the frozen-counter control needs a head that weighs its inputs: with the default output weights the third loss moves
        # by 2e-4 (d = 128 Adam, d = 256) when the masks change, with three times the weights by 6e-3 / 1e-3 (float64 model)
        m.out.weight.mul_(3)
    return m


@functools.lru_cache(maxsize=None)
def _engine_data(d):
    feats = {nm: synth.chrom_features(n, d, ENGINE_C, 5 + i) for i, (nm, n) in enumerate(ENGINE_SIZES.items())}
    hics = {nm: synth.contact_graph(n, 7 * n, 5 + i) for i, (nm, n) in enumerate(ENGINE_SIZES.items())}
    return feats, hics


@functools.lru_cache(maxsize=None)
def _engine_gpu(d, kind, hip_graphs):
    """four train steps of the stage -> (losses, parameters afterwards, c0, counter afterwards, graph kinds captured)"""
    feats, hics = _engine_data(d)
    m = _engine_model(d).to(DEV)
    st = GCNStage(m, _optimizer(kind, m.parameters()), "hic", DEV, hip_graphs=hip_graphs)
    for nm in ENGINE_SIZES:
        st.add_chromosome(nm, feats[nm], hics[nm])
    m.seed_dropout(ENGINE_SEED)
    m._rng_state[1] = ENGINE_C0
    seed0, c0 = (int(v) for v in m._rng_state.tolist())
    losses = [st.train_step(nm)[0].item() for nm in ENGINE_ORDER]
    assert st._fused == kind and getattr(m, "_rng_managed", False)
    params = {k: v.detach().cpu().numpy().copy() for k, v in m.named_parameters()}
    return dict(losses=losses, params=params, seed=seed0, c0=c0, ctr=int(m._rng_state[1].item()),
                kinds={k[1] for k in st._graphs})


@functools.lru_cache(maxsize=None)
def _engine_ref(d, kind, frozen=False, steps=4):
    """the same steps on a float64 copy of the model under torch's own optimizer; masks of counter c0 + t (frozen: c0)"""
    feats, hics = _engine_data(d)
    m64 = _engine_model(d).double().train()
    opt = _optimizer(kind, m64.parameters(), double=True)
    A = {nm: _dense_adjacency("hic", hics[nm], n) for nm, n in ENGINE_SIZES.items()}
    losses = []
    for t, nm in enumerate(ENGINE_ORDER[:steps]):
        x64 = torch.stack([feats[nm]["forward"], feats[nm]["backward"]]).double()
        opt.zero_grad()
        loss = _ref_loss(m64, x64, A[nm], feats[nm]["target"].double(), ENGINE_P, ENGINE_SEED, ENGINE_C0 + (0 if frozen else t))
        loss.backward()
        opt.step()
        losses.append(loss.item())
    return dict(losses=losses, params={k: v.detach().numpy().copy() for k, v in m64.named_parameters()})


ENGINE_CASES = {"sgd-eager": (128, "sgd", False), "sgd-captured": (128, "sgd", True), "adam-captured": (128, "adam", True),
                "sgd-captured-d256": (256, "sgd", True)}


@pytest.mark.parametrize("case", list(ENGINE_CASES))
def test_engine_steps_match_float64_with_the_masks_of_each_step(case):
    d, kind, hip_graphs = ENGINE_CASES[case]
    got, ref = _engine_gpu(d, kind, hip_graphs), _engine_ref(d, kind)
    assert (got["seed"], got["c0"]) == (ENGINE_SEED, ENGINE_C0)
    assert got["ctr"] == got["c0"] + 4                  # one advance per step, carried into the high half
    assert got["kinds"] == ({"train"} if hip_graphs else set())
    for t, (a, b) in enumerate(zip(got["losses"], ref["losses"])):
        print("%s step %d: loss %.7f, float64 %.7f, difference %.2e" % (case, t, a, b, abs(a - b)))
    for t, (a, b) in enumerate(zip(got["losses"], ref["losses"])):
        assert abs(a - b) < 2e-5, (t, a, b)
    for k, r in ref["params"].items():
        np.testing.assert_allclose(got["params"][k], r, err_msg=k, **(TOL if kind == "sgd" else ADAM_TOL))


def test_engine_captured_steps_are_the_eager_steps_bit_for_bit():
    a, b = _engine_gpu(128, "sgd", False), _engine_gpu(128, "sgd", True)
    assert a["losses"] == b["losses"] and a["ctr"] == b["ctr"]
    for k, v in a["params"].items():
        assert np.array_equal(v, b["params"][k]), k


@pytest.mark.parametrize("case", list(ENGINE_CASES))
def test_engine_comparison_tells_a_frozen_counter_apart(case):
    """control: the float64 model trained on ONE mask (the counter frozen at c0) misses the GPU's third loss -- the first
    step that meets a chromosome again -- by more than ten times the loss tolerance, so a counter frozen into a captured
    graph, or a step that does not advance it, fails test_engine_steps_match_float64_with_the_masks_of_each_step"""
    d, kind, hip_graphs = ENGINE_CASES[case]
    got, frozen = _engine_gpu(d, kind, hip_graphs), _engine_ref(d, kind, frozen=True, steps=3)
    assert abs(got["losses"][0] - frozen["losses"][0]) < 2e-5      # (the first step's counter IS c0)
    diff = abs(got["losses"][2] - frozen["losses"][2])
    print("%s: third loss %.7f, with the counter frozen %.7f, difference %.2e" % (case, got["losses"][2], frozen["losses"][2], diff))
    assert diff > 10 * 2e-5
