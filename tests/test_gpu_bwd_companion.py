"""cgcn_layer_bwd_co: a companion aggregation (cgcn_spmm_job) travelling in the block range behind the backward gather of
cgcn_layer_bwd's last launch.  The reference is always the two separate launches of the SAME library -- cgcn_layer_bwd, then
cgcn_spmm -- and equality is bitwise: both forms run the same walk in the same order, so any difference is a bug.  The
feature-sliced route of cgcn_spmm is forced at every size (cgcn_debug_set_fwd_split_bytes(0)), so that companions of a few
tiles ride; cgcn_debug_layer_bwd_co_route says for every case whether the companion rode or was launched behind."""
import copy
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import chromegcn_amd as CG
from chromegcn_amd import _lib, graph as G, ops, synth
from chromegcn_amd.finetune import GCNStage

pytestmark = pytest.mark.gpu
DEV = "cuda"
P = _lib.ptr
OK, BAD_ARG = 0, -1


@pytest.fixture(autouse=True)
def sliced_route_at_every_size():
    lib = _lib.load()
    lib.cgcn_debug_set_fwd_split_bytes(0)
    try:
        yield lib
    finally:
        lib.cgcn_debug_set_fwd_split_bytes(-1)


def sym_matrix(n, seed, per_row=6, hub=None, ring=False):
    """random symmetric {0,1} matrix without diagonal; hub = (row, neighbours): one long row; ring: i -- i + 1 only"""
    rng = np.random.RandomState(seed)
    if ring:
        i = np.arange(n); j = (i + 1) % n
    else:
        i = rng.randint(0, n, per_row * n // 2); j = rng.randint(0, n, per_row * n // 2)
    if hub is not None:
        row, k = hub
        i = np.concatenate([i, np.full(k, row)]); j = np.concatenate([j, rng.choice(np.delete(np.arange(n), row), k, replace=False)])
    keep = i != j
    m = sp.coo_matrix((np.ones(int(keep.sum()), dtype=np.float32), (i[keep], j[keep])), shape=(n, n)).tocsr()
    m = m + m.T
    m.data[:] = 1.0
    return m


def hic_graph(n, seed, **kw):
    g = G.upload(G.normalize_graph("hic", sym_matrix(n, seed, **kw), n), DEV)
    assert g.val is None
    return g


def valued_graph(n, seed):
    """symmetric, explicit values (no row scale): the HAS_VAL instance of the sliced kernels"""
    m = sp.triu(sym_matrix(n, seed), 1).tocsr()
    m.data[:] = np.random.RandomState(seed + 1).uniform(0.25, 1.5, m.nnz).astype(np.float32)
    g = G.upload(G.host_csr_from_matrix(m + m.T + sp.identity(n, dtype=np.float32, format="csr")), DEV)
    assert g.val is not None and not G.has_band_plus(g.col)
    return g


class Problem:
    """operands of one cgcn_layer_bwd call (dXn form) with the fused SGD step riding, and of one companion aggregation"""

    def __init__(self, gm, S, gc, S_co, d=128, seed=0, sgd=True, want_dx=True):
        self.gm, self.gc, self.S, self.S_co, self.d, self.sgd, self.want_dx = gm, gc, S, S_co, d, sgd, want_dx
        gen = torch.Generator(device=DEV).manual_seed(1000 + seed)
        rnd = lambda *sh: torch.randn(*sh, device=DEV, generator=gen)
        n = gm.n
        self.x, self.z, self.h = rnd(S, n, d), torch.tanh(rnd(S, n, d)), rnd(S, n, d)
        self.gate, self.dxn = torch.rand(S, n, device=DEV, generator=gen), rnd(S, n, d) * 0.1
        self.off = dict(W=1000, b=1000 + d * d, wg=1000 + d * d + d, cg=1000 + d * d + 2 * d)
        self.total = 1000 + d * d + 2 * d + 4 + 2000
        self.param0, self.grad0, self.mom0 = rnd(self.total) * 0.1, rnd(self.total) * 0.01, rnd(self.total) * 0.01
        self.rng0 = torch.tensor([7, 11], dtype=torch.int64, device=DEV)
        self.xc = rnd(S_co, gc.n, d)
        self.ws_bytes = _lib.load().cgcn_layer_bwd_workspace_bytes(n, S, d)

    def job(self, H, X=None):
        gc = self.gc
        return _lib.SpmmJob(gc.n, self.S_co, self.d, P(gc.rowptr), P(gc.col), P(gc.val), P(gc.row_scale),
                            self.xc.data_ptr() if X is None else X, H, G.aux_ptr(gc.col))

    def route(self, lib):
        gm = self.gm
        H = torch.empty_like(self.xc)
        return lib.cgcn_debug_layer_bwd_co_route(gm.n, self.S, self.d, P(gm.rowptr_t), P(gm.col_t), P(gm.val_t), 1 if self.want_dx else 0,
                                                 G.aux_ptr(gm.col_t), ctypes.byref(self.job(H.data_ptr())))

    def run(self, lib, together, job=None):
        """-> (status, [dX, dHs, gradient arena (dW, db, dwg, dcg), parameter arena, momentum, dropout counter, H])"""
        gm, gc, S, d, o = self.gm, self.gc, self.S, self.d, self.off
        param, grad, mom, rng = self.param0.clone(), self.grad0.clone(), self.mom0.clone(), self.rng0.clone()
        nan = lambda t: torch.full_like(t, float("nan"))
        dx, dhs, H = nan(self.x), nan(self.x), nan(self.xc)
        ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=DEV)
        sg = _lib.SgdFuse(param.data_ptr(), grad.data_ptr(), mom.data_ptr(), self.total, 0.25, 0.9, 1e-6, 0.5, 0, rng.data_ptr())
        args = (_lib.stream_ptr(), gm.n, S, d, P(gm.rowptr_t), P(gm.col_t), P(gm.val_t), P(gm.row_scale), P(self.x), P(self.z), P(self.h),
                P(self.gate), param[o["W"]:].data_ptr(), param[o["wg"]:].data_ptr(), P(self.dxn), None,
                P(dx) if self.want_dx else None, P(dhs), grad[o["W"]:].data_ptr(), grad[o["b"]:].data_ptr(), grad[o["wg"]:].data_ptr(),
                grad[o["cg"]:].data_ptr(), 0, 0.0, None, 0, None, P(ws), self.ws_bytes, None, ctypes.byref(sg) if self.sgd else None,
                G.aux_ptr(gm.col_t))
        if together:
            j = self.job(H.data_ptr()) if job is None else job(dx, H)
            rc = lib.cgcn_layer_bwd_co(*args, ctypes.byref(j))
        else:
            rc = lib.cgcn_layer_bwd(*args)
            if rc == OK:
                rc = lib.cgcn_spmm(_lib.stream_ptr(), gc.n, gc.n, self.S_co, d, P(gc.rowptr), P(gc.col), P(gc.val), P(gc.row_scale),
                                   P(self.xc), P(H), G.aux_ptr(gc.col))
        torch.cuda.synchronize()
        return rc, [dx, dhs, grad, param, mom, rng, H]


NAMES = ("dX", "dHs", "gradient arena", "parameter arena", "momentum", "dropout counter", "H")


def same_bits(a, b):
    """torch.equal, with the NaN the buffers were filled with equal to itself (a dX nobody asked for stays NaN in both)"""
    return torch.equal(a.view(torch.int32 if a.dtype == torch.float32 else a.dtype), b.view(torch.int32 if b.dtype == torch.float32 else b.dtype))


def check_equal(lib, pr, rides):
    assert pr.route(lib) == (1 if rides else 0)
    rc_a, a = pr.run(lib, True)
    rc_b, b = pr.run(lib, False)
    assert rc_a == OK and rc_b == OK
    for nm, u, v in zip(NAMES, a, b):
        assert same_bits(u, v), nm
    assert not torch.isnan(a[6]).any() and not torch.equal(a[3], pr.param0)      # H written everywhere, the step taken
    if pr.want_dx:
        assert not torch.isnan(a[0]).any()


@pytest.fixture(scope="module")
def main200():
    return hic_graph(200, 1)   # four tiles, the last partial


@pytest.mark.parametrize("n_co", [75, 1000, 64], ids=["two_tiles", "larger_than_main", "one_tile"])
def test_first_layer_form_equals_the_two_launches_bitwise(sliced_route_at_every_size, main200, n_co):
    lib = sliced_route_at_every_size
    check_equal(lib, Problem(main200, 2, hic_graph(n_co, 2 + n_co), 2, seed=n_co), rides=True)


def test_with_the_built_in_threshold_a_small_companion_is_launched_behind(sliced_route_at_every_size, main200):
    """cgcn_spmm runs the whole-row kernel on a 77 KB table: the companion must then not ride (the sliced walk sums a hub
    row in another order), and the caller still gets cgcn_spmm's bits"""
    lib = sliced_route_at_every_size
    lib.cgcn_debug_set_fwd_split_bytes(-1)
    check_equal(lib, Problem(main200, 2, hic_graph(75, 77), 2, seed=5), rides=False)


def test_head_mode_with_the_head_slabs_riding_in_the_gather(sliced_route_at_every_size):
    """a one-layer model through forward_loss: its backward is cgcn_layer_bwd in head mode (cgcn_head_grad), the head's
    second-stage slabs ride in the gather launch, and the layer is the first one, so ops._co_agg hands it the companion"""
    lib = sliced_route_at_every_size
    S, n, d, C, n_co = 2, 200, 128, 103, 130
    gm, gc = hic_graph(n, 11), hic_graph(n_co, 12)
    torch.manual_seed(3)
    m0 = CG.ChromeGCN(d, d, C, 0.0, True, 1)
    x, tgt, xc = torch.randn(S, n, d), (torch.rand(n, C) < 0.2).float().to(DEV), torch.randn(S, n_co, d, device=DEV)
    outs = []
    for together in (True, False):
        m = copy.deepcopy(m0).to(DEV).train()
        xg = x.to(DEV).requires_grad_(True)
        H = torch.full_like(xc, float("nan"))
        loss, probs, _ = m.forward_loss(xg, gm, tgt)
        if together:
            ops._co_agg = {"job": ops.spmm_job(xc, gc, H), "done": False}
            assert lib.cgcn_debug_layer_bwd_co_route(n, S, d, P(gm.rowptr_t), P(gm.col_t), None, 1, G.aux_ptr(gm.col_t),
                                                     ctypes.byref(ops._co_agg["job"])) == 1
        try:
            loss.backward()
            assert not together or ops._co_agg["done"]
        finally:
            ops._co_agg = None
        if not together:
            _lib.check(lib.cgcn_spmm(_lib.stream_ptr(), n_co, n_co, S, d, P(gc.rowptr), P(gc.col), None, P(gc.row_scale), P(xc), P(H),
                                     G.aux_ptr(gc.col)), "cgcn_spmm")
        torch.cuda.synchronize()
        outs.append([loss.detach(), probs, xg.grad, H] + [q.grad for _, q in sorted(m.named_parameters())])
    for k, (u, v) in enumerate(zip(*outs)):
        assert torch.equal(u, v), k
    assert not torch.isnan(outs[0][3]).any()


def test_hub_rows_in_the_companion_range_and_in_the_main_problem(sliced_route_at_every_size, main200):
    """a row of 900 neighbours (> SLICED_SUPER = 768): all 8 waves of its workgroup walk it, with workgroup barriers -- inside
    the companion range, and in the main gather with an ordinary companion behind it"""
    lib = sliced_route_at_every_size
    hub = hic_graph(1000, 21, hub=(517, 900))
    assert int((hub.rowptr[1:] - hub.rowptr[:-1]).max()) > 768
    check_equal(lib, Problem(main200, 2, hub, 2, seed=21), rides=True)
    check_equal(lib, Problem(hub, 2, hic_graph(75, 22), 2, seed=22), rides=True)


def test_one_strand_instance(sliced_route_at_every_size):
    lib = sliced_route_at_every_size
    check_equal(lib, Problem(hic_graph(200, 31), 1, hic_graph(130, 32), 1, seed=31), rides=True)   # 4 slices: 16 gather workgroups


def test_one_strand_instance_with_a_padded_range(sliced_route_at_every_size):
    """S = 1: four column slices, 3 tiles -> 12 gather workgroups, so the companion range starts 4 workgroups further on"""
    lib = sliced_route_at_every_size
    check_equal(lib, Problem(hic_graph(130, 33), 1, hic_graph(200, 34), 1, seed=33), rides=True)


def test_int32_index_instance(sliced_route_at_every_size):
    lib = sliced_route_at_every_size
    g = hic_graph(66000, 41, ring=True)   # more than 65 536 columns: no 16-bit index copy; degree 3 with the self-loop
    assert G.col16_ptr(g.col) is None and int((g.rowptr[1:] - g.rowptr[:-1]).max()) == 3
    check_equal(lib, Problem(g, 2, g, 2, seed=41), rides=True)


def test_explicit_value_instance(sliced_route_at_every_size):
    lib = sliced_route_at_every_size
    check_equal(lib, Problem(valued_graph(200, 51), 2, valued_graph(130, 52), 2, seed=51), rides=True)


@pytest.mark.parametrize("case", ["values_differ", "strands_differ", "no_dX"])
def test_fallback_launches_the_aggregation_behind(sliced_route_at_every_size, main200, case):
    lib = sliced_route_at_every_size
    if case == "values_differ":
        pr = Problem(main200, 2, valued_graph(130, 61), 2, seed=61)
    elif case == "strands_differ":
        pr = Problem(main200, 2, hic_graph(130, 62), 1, seed=62)
    else:
        pr = Problem(main200, 2, hic_graph(130, 63), 2, seed=63, want_dx=False)
    check_equal(lib, pr, rides=False)


@pytest.mark.parametrize("case", ["null_X", "misaligned_H", "H_is_dX"])
def test_bad_companions_are_refused_before_anything_is_launched(sliced_route_at_every_size, main200, case):
    lib = sliced_route_at_every_size
    pr = Problem(main200, 2, hic_graph(200, 71), 2, seed=71)   # (same shape as the main problem, so that H == dX is the only fault)

    def job(dx, H):
        if case == "null_X":
            j = pr.job(H.data_ptr())
            j.X = None
            return j
        return pr.job(H.data_ptr() + 4 if case == "misaligned_H" else dx.data_ptr())
    rc, out = pr.run(lib, True, job)
    assert rc == BAD_ARG
    for nm, t in zip(("dX", "dHs", "H"), (out[0], out[1], out[6])):
        assert torch.isnan(t).all(), nm
    for t, t0 in ((out[2], pr.grad0), (out[3], pr.param0), (out[4], pr.mom0), (out[5], pr.rng0)):
        assert torch.equal(t, t0)


def _engine_epochs(monkeypatch, co, valued_middle):
    monkeypatch.setenv("CGCN_CO_AGG", "1" if co else "0")
    d, c = 128, 13
    torch.manual_seed(0)
    m = CG.ChromeGCN(d, d, c, 0.2, True, 2).to(DEV)
    m.seed_dropout(99)
    opt = torch.optim.SGD(m.parameters(), lr=0.25, momentum=0.9, weight_decay=1e-6)
    st = GCNStage(m, opt, "hic", DEV, hip_graphs=True, input_grad=True, cache_input_aggregation=False)
    names = ["a", "b", "c"]
    for k, (nm, n) in enumerate(zip(names, (130, 700, 260))):
        st.add_chromosome(nm, synth.chrom_features(n, d, c, 5 + k), synth.contact_graph(n, 6 * n, 3 + k))
    if valued_middle:   # explicit values: another instance of the sliced kernels than its neighbours' (launched behind)
        st.chroms["b"].graph = valued_graph(700, 81)
    res = []
    for _ in range(2):
        preds, _, total = st.run_split("train", names, to_cpu=False)
        torch.cuda.synchronize()
        res += [preds.clone(), torch.tensor(total), st._arena["loss"].clone(), st._graphs[(tuple(names), "epoch")]["dx"].clone()]
    assert sorted(st._h1_co) == (["b", "c"] if co else [])
    return res + [v.clone() for _, v in sorted(m.state_dict().items())] + [m._rng_state.clone()]


@pytest.mark.parametrize("valued_middle", [False, True], ids=["eligible", "middle_chromosome_ineligible"])
def test_engine_hands_the_next_chromosomes_aggregation_to_the_last_launch(sliced_route_at_every_size, monkeypatch, valued_middle):
    """three chromosomes in one captured epoch, the two-launch forward forced: losses, predictions, x.grad of the last
    chromosome, every parameter and buffer after two epochs with CGCN_CO_AGG on and off, from the same seed"""
    on = _engine_epochs(monkeypatch, True, valued_middle)
    off = _engine_epochs(monkeypatch, False, valued_middle)
    assert len(on) == len(off)
    for k, (u, v) in enumerate(zip(on, off)):
        assert torch.equal(u, v), k
    assert int(on[-1][1]) == 6   # six steps taken
