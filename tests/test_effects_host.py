"""Window effects without a GPU: the float64 restatement against the oracle's eval forward, the locality that the restricted
route rests on, the instance enumeration, the knock-out map against a plain loop, the seeds of the GPU cases, and the argument
checks of the C ABI and of the Python entry points (which answer before any launch)."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import chromegcn_amd as C
import effects_cases as EC
from chromegcn_amd import _build, _lib
from chromegcn_amd import graph as G
from chromegcn_amd.effects import (_host_transpose, effect_rows_host, knockout_map_host, window_effects,
                                   window_effects_host)

N, D, NC = 60, 16, 5


def _graph(kind, n=N):
    """the host graphs of the definition test: process_graph's 'hic' and 'both' on the CPU, and the asymmetric weighted graph
    without a diagonal"""
    if kind == "asym":
        return G.host_csr_from_matrix(_asym(n))
    a = EC.O.random_symmetric_graph(n, 150, 3)
    g = C.process_graph(kind, {"c": a}, n, "c", device="cpu")
    return G.to_host(g)


def _asym(n):
    rng = np.random.RandomState(2)
    a = sp.random(n, n, density=0.08, random_state=rng, format="lil", data_rvs=lambda k: rng.rand(k) + 0.25)
    a.setdiag(0)
    a[:, 4] = 0
    a = sp.csr_matrix(a)
    a.eliminate_zeros()
    assert (abs(a - a.T)).nnz > 0
    return a


def _oracle_prob(orc, h, x_f, x_r):
    """two calls of the oracle's eval forward in float64, strand mean and sigmoid by hand"""
    a = sp.coo_matrix(sp.diags(np.ones(h.n) if h.row_scale is None else h.row_scale.astype(np.float64)) @ h.ahat().astype(np.float64))
    adj = torch.sparse_coo_tensor(torch.from_numpy(np.vstack((a.row, a.col)).astype(np.int64)), torch.from_numpy(a.data),
                                  torch.Size(a.shape))
    with torch.no_grad():
        lf, lr = orc(x_f.double(), adj)[1], orc(x_r.double(), adj)[1]
    return (1.0 / (1.0 + torch.exp(-(lf + lr) / 2))).numpy()


def _small_case(kind, layers, seed=0):
    h = _graph(kind)
    orc, model = EC.make_models(D, NC, layers, 20 + seed)
    x_f, x_r = EC.features(N, D, seed)
    rng = np.random.RandomState(seed)
    win = np.array([0, N - 1, 4, 7, 7] + rng.randint(0, N, 4).tolist(), np.int64)
    g = torch.Generator().manual_seed(seed)
    alt_f, alt_r = x_f[win] + torch.randn(len(win), D, generator=g), x_r[win] + torch.randn(len(win), D, generator=g)
    return h, orc, model, x_f, x_r, win, alt_f, alt_r


@pytest.mark.parametrize("layers", [1, 2, 3])
@pytest.mark.parametrize("kind", ["hic", "both", "asym"])
def test_restatement_is_the_oracle_on_replaced_rows(kind, layers):
    h, orc, model, x_f, x_r, win, alt_f, alt_r = _small_case(kind, layers)
    ref = _oracle_prob(orc, h, x_f, x_r)
    for scope in ("own", "contacts"):
        we = window_effects_host(model, x_f, x_r, h, win, alt_f, alt_r, scope=scope)
        offsets, rows = effect_rows_host(h, win)
        if scope == "own":
            offsets, rows = np.arange(len(win) + 1), win.astype(np.int32)
        assert np.array_equal(we.offsets, offsets) and np.array_equal(we.rows, rows) and we.rows.dtype == np.int32
        assert np.abs(we.ref - ref[rows]).max() <= 1e-12
        for m, u in enumerate(win):
            xf, xr = x_f.clone(), x_r.clone()
            xf[u], xr[u] = alt_f[m], alt_r[m]
            want = _oracle_prob(orc, h, xf, xr)[rows[offsets[m]:offsets[m + 1]]]
            r, rf, al = we[m]
            assert np.array_equal(r, rows[offsets[m]:offsets[m + 1]])
            assert np.abs(al - want).max() <= 1e-12
            assert np.abs(al - rf).max() > 1e-6          # the replacement does something


@pytest.mark.parametrize("kind", ["hic", "asym"])
def test_layer_one_changes_the_instances_only_and_layer_two_stays_inside_two_hops(kind):
    for layers in (1, 2):
        h, _orc, model, x_f, x_r, win, alt_f, alt_r = _small_case(kind, layers, seed=1)
        A = sp.csr_matrix((np.ones(h.nnz), h.col, h.rowptr), shape=(h.n, h.n))
        for m, u in enumerate(win):
            full = _full_rows(model, x_f, x_r, h, u, alt_f[m], alt_r[m])
            changed = np.flatnonzero(np.any(full[0] != full[1], 1))
            _, inst = effect_rows_host(h, [u])
            reach = set(inst.tolist())
            if layers == 2:
                hop = np.zeros(h.n)
                hop[list(reach)] = 1
                reach |= set(np.flatnonzero(A @ hop).tolist())     # rows with a stored entry towards an instance
            assert set(changed.tolist()) <= reach, (layers, u)
            assert u in changed


def _full_rows(model, x_f, x_r, h, u, af, ar):
    """(ref, alt) of EVERY window for one variant, through the restatement's own forward"""
    from chromegcn_amd.effects import _matrix64, _np64, _params64, _prob64
    p, A = _params64(model), _matrix64(h)
    xf, xr = _np64(x_f), _np64(x_r)
    ref = _prob64(p, A, xf, xr)
    xf2, xr2 = xf.copy(), xr.copy()
    xf2[u], xr2[u] = _np64(af), _np64(ar)
    return ref, _prob64(p, A, xf2, xr2)


def test_enumeration():
    # stored diagonal (the normaliser's self loop): u first, not repeated; an isolated window has one instance
    h = EC.host_graph("hic")
    offsets, rows = effect_rows_host(h, [EC.HUB, EC.ISOLATED, EC.ROW64, EC.TWICE, EC.TWICE])
    assert offsets.dtype == np.int64 and rows.dtype == np.int32
    deg = np.diff(h.rowptr)
    assert np.diff(offsets).tolist() == [deg[EC.HUB], 1, 64, deg[EC.TWICE], deg[EC.TWICE]]
    for m, u in enumerate([EC.HUB, EC.ISOLATED, EC.ROW64, EC.TWICE, EC.TWICE]):
        seg = rows[offsets[m]:offsets[m + 1]]
        nb = h.col[h.rowptr[u]:h.rowptr[u + 1]]
        assert seg[0] == u and np.array_equal(seg[1:], nb[nb != u]) and (seg[1:] != u).all()
    assert np.array_equal(rows[offsets[3]:offsets[4]], rows[offsets[4]:offsets[5]])       # a duplicate window: the same rows
    # no stored diagonal, asymmetric: u is still reported, then the rows v with A[v, u] (NOT row u's own columns)
    h = EC.host_graph("asym")
    dense = h.ahat().toarray()
    offsets, rows = effect_rows_host(h, [9, 0, 33])
    assert np.diff(offsets)[0] == 1 and rows[0] == 9                                       # no in-edge: one instance
    for m, u in enumerate([9, 0, 33]):
        seg = rows[offsets[m]:offsets[m + 1]]
        assert seg[0] == u and np.array_equal(seg[1:], np.flatnonzero(dense[:, u] != 0))
    rp, ct = _host_transpose(h)
    up = G.upload(h, "cpu")
    assert np.array_equal(rp, up.rowptr_t.numpy()) and np.array_equal(ct, up.col_t.numpy())
    assert effect_rows_host(h, [])[0].tolist() == [0]
    with pytest.raises(ValueError):
        effect_rows_host(h, [EC.N])


@pytest.mark.parametrize("kind", ["hic", "asym"])
def test_knockout_map_is_a_plain_loop(kind):
    h, _orc, model, x_f, x_r, _win, _af, _ar = _small_case(kind, 2, seed=2)
    labels = [0, 3]
    fill = torch.stack([x_f.double().mean(0), x_r.double().mean(0)])      # the default, in float64
    rp, ct = _host_transpose(h)
    want_all, want_sel = np.zeros(ct.shape[0]), np.zeros(ct.shape[0])
    for u in range(h.n):
        ref, alt = _full_rows(model, x_f, x_r, h, u, fill[0], fill[1])
        for p in range(rp[u], rp[u + 1]):
            v = ct[p]
            want_all[p] = np.abs(alt[v] - ref[v]).sum()
            want_sel[p] = np.abs(alt[v, labels] - ref[v, labels]).sum()
    assert np.abs(knockout_map_host(model, x_f, x_r, h) - want_all).max() <= 1e-13
    assert np.abs(knockout_map_host(model, x_f, x_r, h, fill=fill, labels=labels) - want_sel).max() <= 1e-13
    assert want_all.max() > 1e-4


@pytest.mark.parametrize("kind,d,layers,c", [(k, d, l, 7) for k in EC.GRAPH_KINDS for d in (128, 256) for l in (1, 2)]
                         + [("hic", 128, 3, 7), ("hic", 128, 2, 103)])
def test_the_gpu_cases_cannot_be_passed_by_echoing_ref(kind, d, layers, c):
    """the float64 restatement alone: every variant with a contact moves a contact row, and its own row, by >= 1e-3"""
    want = EC.gpu_case(kind, d, layers, c)["want"]
    contact, own = EC.effect_floor(want["contacts"])
    assert contact >= 1e-3 and own >= 1e-3, (contact, own)
    own_scope = want["own"]
    assert np.abs(own_scope.alt - own_scope.ref).max(1).min() >= 1e-3


def test_c_abi_argument_checks_answer_without_launching():
    _build.build_library()
    _lib.load()
    OK, BAD_ARG, UNSUPPORTED = 0, -1, -2
    P = 0x10000                                           # never dereferenced: every call below returns before a launch
    q = lambda n_inst, S=2, d=128, layers=2: _lib.query("cgcn_effects_workspace_bytes", n_inst=n_inst, S=S, d=d, layers=layers)
    al = lambda b: (b + 255) & ~255
    for n_inst, d, layers in ((1, 128, 1), (10, 128, 2), (77, 256, 2), (1000, 256, 1)):
        # [H_inst][X_inst][X1_inst][X2_inst: layers == 2] of n_inst * S * d fp32, [gate: n_inst * S fp32], 256-byte aligned parts
        assert q(n_inst, 2, d, layers) == (2 + layers) * al(n_inst * 2 * d * 4) + al(n_inst * 2 * 4)
    assert q(0) == 0 and q(10, S=1) == 0 and q(10, d=100) == 0 and q(10, layers=3) == 0 and q(10, layers=0) == 0 and q(-1) == 0

    def plan(**kw):
        a = dict(stream=None, n=10, rowptr_t=P, col_t=P, n_var=3, windows=P, counts=P, diag_pos=P)
        a.update(kw)
        return _lib.query("cgcn_effects_plan", **a)

    def rows1(**kw):
        a = dict(stream=None, n=10, S=2, d=128, rowptr_t=P, col_t=P, val_t=None, row_scale=None, X0=P, H1=P, windows=P, alt=P,
                 offsets=P, diag_pos=P, n_var=3, own=0, n_inst=5, H_inst=P, X_inst=P, rows=None)
        a.update(kw)
        return _lib.query("cgcn_effects_rows1", **a)

    def rows2(**kw):
        a = dict(stream=None, n=10, S=2, d=128, rowptr=P, col=P, val=None, row_scale=None, rowptr_t=P, col_t=P, X1=P, H2=P,
                 windows=P, offsets=P, diag_pos=P, n_var=3, own=0, n_inst=5, X1_inst=P, H_out=2 * P, X_res=None)
        a.update(kw)
        return _lib.query("cgcn_effects_rows2", **a)

    for k in ("rowptr_t", "col_t", "windows", "counts", "diag_pos"):
        assert plan(**{k: None}) == BAD_ARG, k
    for k in ("rowptr_t", "col_t", "X0", "H1", "windows", "alt", "offsets", "diag_pos", "H_inst", "X_inst"):
        assert rows1(**{k: None}) == BAD_ARG, k
    for k in ("rowptr", "col", "rowptr_t", "col_t", "X1", "H2", "windows", "offsets", "diag_pos", "X1_inst", "H_out"):
        assert rows2(**{k: None}) == BAD_ARG, k
    assert plan(n=-1) == BAD_ARG and plan(n_var=-1) == BAD_ARG and plan(n_var=0) == OK
    for f in (rows1, rows2):
        assert f(S=1) == UNSUPPORTED and f(d=100) == UNSUPPORTED and f(d=64) == UNSUPPORTED
        assert f(n=-1) == BAD_ARG and f(n_var=-1) == BAD_ARG and f(n_inst=-1) == BAD_ARG
        assert f(n_var=0, n_inst=0) == OK                  # nothing to do: nothing launched
    assert rows1(X0=P + 4) == BAD_ARG and rows1(own=1, n_inst=5, n_var=3) == BAD_ARG
    assert rows2(own=1, X_res=None) == BAD_ARG and rows2(H_out=P) == BAD_ARG and rows2(X_res=P) == BAD_ARG


def test_python_argument_checks_answer_without_launching():
    """every ValueError / RuntimeError of window_effects, on CPU tensors: none of them gets as far as the device"""
    n, d = 30, 128
    _orc, model = EC.make_models(d, 4, 2, 1)
    _orc3, model3 = EC.make_models(d, 4, 3, 1)
    x_f, x_r = EC.features(n, d, 0)
    g = G.upload(G.normalize_graph("hic", EC.O.random_symmetric_graph(n, 60, 1), n), "cpu")
    win = [1, 2]
    alt = torch.zeros(2, d)
    ok = dict(model=model, x_f=x_f, x_r=x_r, adj=g, windows=win, alt_f=alt, alt_r=alt)

    def call(**kw):
        a = dict(ok)
        a.update(kw)
        return window_effects(**a)

    model.train()
    with pytest.raises(RuntimeError, match="eval-mode"):
        call()
    model.eval()
    for bad in (dict(adj=None), dict(scope="all"), dict(route="fast"), dict(x_r=x_r[:-1]), dict(alt_f=alt[:1]),
                dict(alt_r=torch.zeros(2, d + 1)), dict(windows=[1, n]), dict(windows=[-1, 2]), dict(windows=[0.5, 1.0]),
                dict(windows=[[1, 2]]), dict(model=model3, route="restricted"),
                dict(adj=G.upload(G.normalize_graph("none", None, n + 1), "cpu"))):
        with pytest.raises(ValueError):
            call(**bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):       # every check passed: the device is what is missing
        call()
    with pytest.raises(ValueError):
        C.knockout_map(model, x_f, x_r, None)
    with pytest.raises(ValueError):
        C.knockout_map(model, x_f, x_r, g, fill=torch.zeros(3, d))
