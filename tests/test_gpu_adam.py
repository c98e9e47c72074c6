"""Fused, graph-capturable Adam (cgcn_adam_step, ABI v26) on the GPU: the kernel against a float64 Adam, a captured launch
replayed 2 000 times, and GCNStage with torch.optim.Adam(fused=True) -- per-chromosome graphs, the one-graph epoch,
checkpoints, learning-rate changes, d = 256, and the multi-rank step group over RCCL -- against the oracle and against
torch's own Adam.  A plain Adam(...) keeps torch's eager step."""
import io
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import chromegcn_amd as C  # noqa: E402
from chromegcn_amd import ops, synth  # noqa: E402
from chromegcn_amd.finetune import GCNStage  # noqa: E402
from oracle import chromegcn_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
BETAS, LR = (0.9, 0.98), 1e-3
ADAM_TOL = dict(atol=2e-3, rtol=1e-3)   # test_gpu_modules: Adam divides by sqrt(v), tiny gradients amplify fp32 differences


# ------------------------------------------------------------------ the kernel
def _flat_layout(sizes):
    offs, total = GCNStage._offsets([torch.empty(s) for s in sizes])
    real = np.zeros(total, dtype=bool)
    for o, s in zip(offs, sizes):
        real[o:o + s] = True
    return total, real


@pytest.mark.parametrize("wd", [0.0, 5e-5])
@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
def test_kernel_matches_float64_adam(wd, grad_scale):
    sizes = [1001, 37, 2500, 6, 128]
    total, real = _flat_layout(sizes)
    rs = np.random.RandomState(int(wd * 1e6) + int(grad_scale * 10))
    mags = np.array([0.0, 1e-20, 1e-8, 1e-4, 1e-2, 1.0, 1e3])[rs.randint(0, 7, total)]
    p0 = (rs.randn(total) * real).astype(np.float32)
    eps, steps = 1e-8, 50
    p, g = torch.tensor(p0, device=DEV), torch.zeros(total, device=DEV)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    step = torch.zeros(len(sizes), device=DEV)
    ticket = torch.zeros(1, device=DEV, dtype=torch.int32)
    rng = torch.tensor([12345, 7], device=DEV, dtype=torch.int64)
    # torch's own fp32 Adam on the same gradients, and float64 by hand
    pt = torch.tensor(p0, requires_grad=True)
    topt = torch.optim.Adam([pt], lr=LR, betas=BETAS, eps=eps, weight_decay=wd, foreach=False)
    p64, m64, v64 = p0.astype(np.float64), np.zeros(total), np.zeros(total)
    b1, b2 = BETAS
    # the moments in float64 with the betas the kernel receives (fp32: 1 - 0.9f is 2.4e-7 off 0.1, which biases m / v
    # relatively by that much -- not the parameters, whose error is checked against the exact Adam)
    f1, f2 = float(np.float32(b1)), float(np.float32(b2))
    mf, vf = np.zeros(total), np.zeros(total)
    for t in range(1, steps + 1):
        gr = (rs.randn(total) * mags * real).astype(np.float32)
        g.copy_(torch.from_numpy(gr))
        ops.adam_step(p, g, m, v, step, ticket, LR, b1, b2, eps, wd, rng, grad_scale)
        pt.grad = torch.from_numpy(gr) * grad_scale   # exact: grad_scale is a power of two
        topt.step()
        d = gr.astype(np.float64) * grad_scale + wd * p64
        m64 = b1 * m64 + (1 - b1) * d
        v64 = b2 * v64 + (1 - b2) * d * d
        mf = f1 * mf + (1 - f1) * d
        vf = f2 * vf + (1 - f2) * d * d
        p64 = p64 - LR / (1 - b1 ** t) * m64 / (np.sqrt(v64) / np.sqrt(1 - b2 ** t) + eps)
    torch.cuda.synchronize()
    pk = p.cpu().numpy().astype(np.float64)
    err_k = np.abs(pk - p64).max()
    err_t = np.abs(pt.detach().numpy().astype(np.float64) - p64).max()
    print("max |p - p64|: kernel %.3g, torch fp32 Adam %.3g" % (err_k, err_t))
    assert err_k <= 1.25 * err_t + 1e-7
    assert torch.equal(step.cpu(), torch.full((len(sizes),), float(steps)))
    assert rng.cpu().tolist() == [12345, 7 + steps]
    assert int(ticket.item()) == 0
    for t_ in (p, m, v):
        assert not t_.cpu().numpy()[~real].any()   # padding stays exactly 0
    # the moments: no further from float64 (at the fp32 betas) than torch's fp32 Adam's from the exact ones
    for name, ours, ref, ref_f in (("exp_avg", m, m64, mf), ("exp_avg_sq", v, v64, vf)):
        e_k = np.abs(ours.cpu().numpy().astype(np.float64) - ref_f).max()
        e_t = np.abs(topt.state[pt][name].numpy().astype(np.float64) - ref).max()
        print("max |%s - float64|: kernel %.3g, torch fp32 Adam %.3g" % (name, e_k, e_t))
        assert e_k <= 1.25 * e_t + 1e-12 * np.abs(ref).max(), name


def test_kernel_with_a_scalar_tail_matches_torch_fused_adam():
    """count not a multiple of 4 (scalar tail) and more than one workgroup: the tail is stepped, the steps advance once"""
    n = 256 * 4 * 3 + 3
    p = torch.randn(n, device=DEV)
    g = torch.randn(n, device=DEV)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    step = torch.full((2,), 4.0, device=DEV)
    ticket = torch.zeros(1, device=DEV, dtype=torch.int32)
    pt = p.clone().requires_grad_(True)
    topt = torch.optim.Adam([pt], lr=LR, betas=BETAS, fused=True)
    pt.grad = torch.zeros_like(pt)
    topt.step()   # creates the state (a zero gradient leaves the parameter as it is)
    with torch.no_grad():
        pt.copy_(p)
    st = topt.state[pt]
    st["step"].fill_(4.0)
    st["exp_avg"].zero_()
    st["exp_avg_sq"].zero_()
    ops.adam_step(p, g, m, v, step, ticket, LR, BETAS[0], BETAS[1], 1e-8, 0.0)
    pt.grad = g.clone()
    topt.step()
    torch.cuda.synchronize()
    assert step.tolist() == [5.0, 5.0] and int(ticket.item()) == 0
    torch.testing.assert_close(p, pt.detach(), rtol=1e-6, atol=1e-7)
    torch.testing.assert_close(v, st["exp_avg_sq"], rtol=3e-6, atol=0.0)   # 1 - beta2 of an fp32 beta2: 1e-6 off 0.02


def test_captured_launch_replays_2000_times_like_eager_launches():
    n = 50_000
    torch.manual_seed(3)
    p0, g = torch.randn(n, device=DEV), torch.randn(n, device=DEV) * 1e-2

    def state():
        return (p0.clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV), torch.zeros(14, device=DEV),
                torch.zeros(1, device=DEV, dtype=torch.int32))

    ge = state()
    gg = state()
    warm = state()
    ops.adam_step(warm[0], g, *warm[1:4], warm[4], LR, BETAS[0], BETAS[1], 1e-8, 1e-6)   # module / kernel loaded outside capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.adam_step(gg[0], g, *gg[1:4], gg[4], LR, BETAS[0], BETAS[1], 1e-8, 1e-6)
    for _ in range(2000):
        graph.replay()
        ops.adam_step(ge[0], g, *ge[1:4], ge[4], LR, BETAS[0], BETAS[1], 1e-8, 1e-6)
    torch.cuda.synchronize()
    assert torch.equal(gg[3], torch.full((14,), 2000.0, device=DEV)) and torch.equal(ge[3], gg[3])
    assert int(gg[4].item()) == 0 and int(ge[4].item()) == 0
    for a, b in zip(gg[:3], ge[:3]):
        assert torch.equal(a, b)


# ------------------------------------------------------------------ the stage
def _model(d, c, layers, dropout=0.0, seed=0):
    torch.manual_seed(seed)
    orc = O.GatedGCNOracle(d, c, dropout, layers)
    with torch.no_grad():
        for k, p in orc.named_parameters():
            if "GC" in k and k.endswith("weight"):
                p.mul_(40)
    m = C.ChromeGCN(d, d, c, dropout, True, layers)
    m.load_state_dict(orc.state_dict())
    return m.to(DEV), orc


def _adam(ps, kind, lr=LR):
    kw = {"fused": dict(fused=True), "capturable": dict(capturable=True), "plain": {}}[kind]
    return torch.optim.Adam(ps, betas=BETAS, lr=lr, **kw)


def _small(kind, hip_graphs, d=128, layers=2, n=400, c=11, seed=0):
    """test_gpu_modules._small_stage with the optimizer's kind as a parameter"""
    feats = synth.chrom_features(n, d, c, 5)
    hic = synth.contact_graph(n, 3000, 5)
    m, orc = _model(d, c, layers, seed=seed)
    opt = _adam(m.parameters(), kind)
    st = GCNStage(m, opt, "hic", DEV, hip_graphs=hip_graphs)
    st.add_chromosome("c", feats, hic)
    return st, m, opt, orc, feats, hic


def _kinds(st):
    return {k[1] for k in st._graphs}


def test_stage_fused_adam_graphs_eager_oracle_and_state_dict():
    st_g, m_g, opt_g, orc, feats, hic = _small("fused", True)
    st_e, m_e, opt_e, _, _, _ = _small("fused", False)
    oopt = _adam(orc.parameters(), "plain")
    cache = {}
    for _ in range(3):
        lg, pg, _ = st_g.train_step("c")
        le, pe, _ = st_e.train_step("c")
        _, _, tot = O.finetune_epoch(orc, {"c": feats}, {"c": hic}, oopt, "train", "hic", adj_cache=cache)
        assert torch.equal(lg, le) and torch.equal(pg, pe)
        assert abs(lg.item() - tot) < 1e-4
    assert st_g._fused == "adam" and _kinds(st_g) == {"train"}
    osd = orc.state_dict()
    for (k, vg), (_, ve) in zip(m_g.state_dict().items(), m_e.state_dict().items()):
        assert torch.equal(vg, ve), k
        np.testing.assert_allclose(vg.cpu().numpy(), osd[k].numpy(), **ADAM_TOL, err_msg=k)
    # the optimizer's state_dict is torch's fused-Adam layout: per parameter a 0-d float32 device step and the moments
    sd, osd_opt = opt_g.state_dict(), oopt.state_dict()
    assert sd["param_groups"][0]["fused"] is True
    assert sorted(sd["state"]) == sorted(osd_opt["state"])
    for i, s in sd["state"].items():
        assert list(s) == ["step", "exp_avg", "exp_avg_sq"]
        assert s["step"].dim() == 0 and s["step"].dtype == torch.float32 and s["step"].is_cuda and s["step"].item() == 3.0
        assert float(osd_opt["state"][i]["step"]) == 3.0
        for k in ("exp_avg", "exp_avg_sq"):
            assert s[k].shape == osd_opt["state"][i][k].shape and s[k].is_cuda
            np.testing.assert_allclose(s[k].cpu().numpy(), osd_opt["state"][i][k].numpy(), rtol=2e-2,
                                       atol=1e-6 if k == "exp_avg" else 1e-9, err_msg="%s %s" % (i, k))


def _genome(d=128, c=11, sizes=(420, 300, 520, 260, 380)):
    feats, hics = {}, {}
    for i, n in enumerate(sizes):
        nm = "chr%d" % (i + 1)
        feats[nm] = synth.chrom_features(n, d, c, 10 + i)
        hics[nm] = synth.contact_graph(n, 6 * n, 10 + i)
    return feats, hics


def test_whole_split_is_one_epoch_graph_and_matches_eager_adam():
    feats, hics = _genome()
    res = {}
    for kind in ("fused", "plain"):
        m, _ = _model(128, 11, 2, dropout=0.2, seed=1)
        st = GCNStage(m, _adam(m.parameters(), kind), "hic", DEV, hip_graphs=True)
        st.load(feats, hics)
        losses = [st.run_split("train", to_cpu=False)[2] for _ in range(2)]
        res[kind] = (m, st, losses)
    (mf, sf, lf), (mp, sp_, lp) = res["fused"], res["plain"]
    assert _kinds(sf) == {"epoch"}, _kinds(sf)
    assert "epoch" not in _kinds(sp_) and "train" not in _kinds(sp_)
    np.testing.assert_allclose(lf, lp, rtol=1e-4)
    assert torch.equal(mf._rng_state, mp._rng_state)   # both advanced the dropout counter once per step
    for (k, a), (_, b) in zip(mf.state_dict().items(), mp.state_dict().items()):
        np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), **ADAM_TOL, err_msg=k)


def _roundtrip(sd):
    buf = io.BytesIO()
    torch.save(sd, buf)
    buf.seek(0)
    return torch.load(buf, map_location=DEV, weights_only=True)


def test_checkpoint_round_trip_continues_bit_exactly():
    K, MORE = 2, 3
    st_a, m_a, opt_a, _, feats, hic = _small("fused", True)
    for _ in range(K):
        st_a.train_step("c")
    torch.cuda.synchronize()
    msd = {k: v.clone() for k, v in m_a.state_dict().items()}
    osd = _roundtrip(opt_a.state_dict())
    for _ in range(MORE):
        st_a.train_step("c")

    def resumed(kind):
        m, _ = _model(128, 11, 2, seed=5)          # other initial weights: everything comes from the checkpoint
        m.load_state_dict(msd)
        opt = _adam(m.parameters(), kind)
        opt.load_state_dict(osd)
        if kind == "plain":   # load_state_dict takes the saved group's flags (fused=True) and device steps: undo both
            opt.param_groups[0]["fused"] = None
            for s in opt.state.values():
                s["step"] = s["step"].cpu()
        st = GCNStage(m, opt, "hic", DEV, hip_graphs=True)
        st.add_chromosome("c", feats, hic)
        for _ in range(MORE):
            st.train_step("c")
        torch.cuda.synchronize()
        return m, opt, st

    m_b, opt_b, st_b = resumed("fused")
    assert st_b._fused == "adam"
    for (k, a), (_, b) in zip(m_a.state_dict().items(), m_b.state_dict().items()):
        assert torch.equal(a, b), k
    for i, s in opt_b.state_dict()["state"].items():
        sa = opt_a.state_dict()["state"][i]
        assert s["step"].item() == K + MORE
        assert torch.equal(s["exp_avg"], sa["exp_avg"]) and torch.equal(s["exp_avg_sq"], sa["exp_avg_sq"])
    # the same checkpoint continued by torch's own (eager) Adam step
    m_c, opt_c, st_c = resumed("plain")
    assert st_c._fused is None
    for (k, a), (_, c) in zip(m_a.state_dict().items(), m_c.state_dict().items()):
        np.testing.assert_allclose(a.cpu().numpy(), c.cpu().numpy(), **ADAM_TOL, err_msg=k)
    # load_state_dict into the stage's OWN optimizer: the next step adopts the new state tensors
    opt_a.load_state_dict(_roundtrip(opt_b.state_dict()))
    assert not st_a._adam_adopted(st_a._params())
    st_a.train_step("c")
    assert st_a._adam_adopted(st_a._params())
    assert all(s["step"].item() == K + MORE + 1 for s in opt_a.state_dict()["state"].values())


def test_lr_schedule_recaptures_and_matches_eager_adam():
    st_f, m_f, opt_f, _, _, _ = _small("fused", True)
    st_p, m_p, opt_p, _, _, _ = _small("plain", True)
    sch_f = torch.optim.lr_scheduler.StepLR(opt_f, step_size=2, gamma=0.5)
    sch_p = torch.optim.lr_scheduler.StepLR(opt_p, step_size=2, gamma=0.5)
    for _ in range(5):
        st_f.train_step("c")
        st_p.train_step("c")
        sch_f.step()
        sch_p.step()
    assert st_f._captured_lr[0][0] == LR * 0.25 == opt_f.param_groups[0]["lr"]   # the graph of the last step has the new lr
    for (k, a), (_, b) in zip(m_f.state_dict().items(), m_p.state_dict().items()):
        np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), **ADAM_TOL, err_msg=k)


def test_plain_adam_keeps_the_eager_step():
    st, m, opt, _, _, _ = _small("plain", True)
    st.train_step("c")
    assert st._fused is None and _kinds(st) == {"fwdbwd"}
    assert not opt.state[next(m.parameters())]["step"].is_cuda   # torch's own state, untouched
    feats, hics = _genome(sizes=(200, 240))
    m2, _ = _model(128, 11, 2)
    st2 = GCNStage(m2, _adam(m2.parameters(), "plain"), "hic", DEV, hip_graphs=True)
    st2.load(feats, hics)
    st2.run_split("train", to_cpu=False)
    assert "epoch" not in _kinds(st2) and "train" not in _kinds(st2)
    # what is not eligible stays eager too: amsgrad, decoupled decay, capturable=True is eligible
    for kw, want in ((dict(fused=True, amsgrad=True), None), (dict(fused=True, decoupled_weight_decay=True), None),
                     (dict(capturable=True), "adam")):
        m3, _ = _model(128, 11, 2)
        st3 = GCNStage(m3, torch.optim.Adam(m3.parameters(), lr=LR, **kw), "hic", DEV, hip_graphs=True)
        st3._ensure_flat_grad()
        assert st3._fused == want, kw


def test_d256_four_layers():
    """graph against eager at d = 256 to 1e-5, not bit for bit: the engine's graph and eager steps already differ there by
    ~1e-8 in the parameters with SGD, and Adam's division by sqrt(v) scales that up"""
    st_g, m_g, _, _, _, _ = _small("fused", True, d=256, layers=4, n=300, seed=2)
    st_e, m_e, _, _, _, _ = _small("fused", False, d=256, layers=4, n=300, seed=2)
    st_p, m_p, _, _, _, _ = _small("plain", True, d=256, layers=4, n=300, seed=2)
    for _ in range(3):
        lg, _, _ = st_g.train_step("c")
        le, _, _ = st_e.train_step("c")
        st_p.train_step("c")
        torch.testing.assert_close(lg, le, rtol=1e-6, atol=0.0)
    assert _kinds(st_g) == {"train"}
    for (k, a), (_, b), (_, c) in zip(m_g.state_dict().items(), m_e.state_dict().items(), m_p.state_dict().items()):
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-5, msg=k)
        np.testing.assert_allclose(a.cpu().numpy(), c.cpu().numpy(), **ADAM_TOL, err_msg=k)


# ------------------------------------------------------------------ the multi-rank step group (one child process)
def _child(port):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    feats = synth.chrom_features(400, 128, 11, 5)
    hic = synth.contact_graph(400, 3000, 5)

    def stage(multi, hip_graphs):
        m, _ = _model(128, 11, 2)
        st = GCNStage(m, _adam(m.parameters(), "fused"), "hic", dev, hip_graphs=hip_graphs, group=dist.group.WORLD,
                      force_collectives=multi)
        st.add_chromosome("c", feats, hic)
        return st, m

    g, m_g = stage(True, True)
    with warnings.catch_warnings(record=True) as wl:
        warnings.simplefilter("always")
        for _ in range(2):
            g.train_group("c", 2)
    torch.cuda.synchronize()
    assert not [w for w in wl if "step group" in str(w.message)], [str(w.message) for w in wl]
    assert g._fused == "adam" and g._group_graph_ok and _kinds(g) == {"group"}, _kinds(g)
    # the same two steps without a process group: eager fwd+bwd, then the fused step with grad_scale 1/2 (and 1)
    r, m_r = stage(False, False)
    r1, _ = stage(False, False)
    for _ in range(2):
        r.train_group("c", 2)
    r1.train_group("c", 1)
    torch.cuda.synchronize()
    for (k, a), (_, b) in zip(m_g.state_dict().items(), m_r.state_dict().items()):
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-6, msg=k)
    for p, q in zip(g._params(), r._params()):
        torch.testing.assert_close(g.optimizer.state[p]["exp_avg"], r.optimizer.state[q]["exp_avg"], rtol=1e-5, atol=1e-9)
    # exp_avg after the FIRST step is (1 - beta1) * grad_scale * grad: the group of two halves it
    r2, _ = stage(False, False)
    r2.train_group("c", 2)
    torch.cuda.synchronize()
    torch.testing.assert_close(r2._flat_m * 2, r1._flat_m, rtol=1e-6, atol=0.0)
    dist.destroy_process_group()
    print("child ok")


@pytest.mark.timeout(600)
def test_step_group_with_fused_adam_over_rccl_in_one_child():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), str(port)], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=480)
    print(r.stdout[-4000:], r.stderr[-4000:])
    assert r.returncode == 0 and "child ok" in r.stdout


if __name__ == "__main__":
    _child(int(sys.argv[1]))
