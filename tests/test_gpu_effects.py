"""Window effects on the GPU (chromegcn_amd.effects) against the float64 restatement window_effects_host.

The tolerance is not fixed in advance.  Its yardstick is measured here, per case, on the same perturbed inputs: the worst
absolute difference against float64 of the package's existing device eval forward (model.forward_strands, which this feature
does not touch).  The restricted route is held to 4 x that yardstick (the margin the ablation's instance rows got against
theirs; its extra rounding is the one H + w * delta update per layer), the composed route to 1 x plus 1e-7."""
import functools

import numpy as np
import pytest
import torch

import chromegcn_amd as C
import effects_cases as EC
from chromegcn_amd import effects as E
from chromegcn_amd import graph as G

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = [(kind, d, layers) for kind in EC.GRAPH_KINDS for d in (128, 256) for layers in (1, 2)]


@functools.lru_cache(maxsize=None)
def _device_case(kind, d, layers, c=7):
    case = EC.gpu_case(kind, d, layers, c)
    dev = dict(model=case["model"].to(DEV).eval(), graph=G.upload(case["h"], DEV))
    for k in ("x_f", "x_r", "alt_f", "alt_r"):
        dev[k] = case[k].to(DEV)
    return case, dev


@functools.lru_cache(maxsize=None)
def _yardstick(kind, d, layers, c=7):
    """worst |device forward_strands - float64| of sigmoid(strand-mean logits) over the reported rows: the unperturbed input
    against ref, every variant's perturbed input against alt"""
    case, dev = _device_case(kind, d, layers, c)
    want = case["want"]["contacts"]
    x = torch.stack([dev["x_f"], dev["x_r"]])
    worst = 0.0
    with torch.no_grad():
        p = E._prob(dev["model"].forward_strands(x, dev["graph"])[0]).double().cpu().numpy()
        worst = max(worst, float(np.abs(p[want.rows] - want.ref).max()))
        for m, u in enumerate(case["win"]):
            xp = x.clone()
            xp[0, u], xp[1, u] = dev["alt_f"][m], dev["alt_r"][m]
            p = E._prob(dev["model"].forward_strands(xp, dev["graph"])[0]).double().cpu().numpy()
            a, b = int(want.offsets[m]), int(want.offsets[m + 1])
            worst = max(worst, float(np.abs(p[want.rows[a:b]] - want.alt[a:b]).max()))
    assert 0 < worst < 1e-4          # float32 rounding, not a defect of the yardstick itself
    return worst


def _run(dev, case, **kw):
    return C.window_effects(dev["model"], dev["x_f"], dev["x_r"], dev["graph"], case["win"], dev["alt_f"], dev["alt_r"], **kw)


def _errors(we, want):
    assert we.offsets.dtype == torch.int64 and we.rows.dtype == torch.int32 and we.ref.dtype == we.alt.dtype == torch.float32
    assert all(t.is_cuda for t in (we.offsets, we.rows, we.ref, we.alt))
    assert np.array_equal(we.offsets.cpu().numpy(), want.offsets) and np.array_equal(we.rows.cpu().numpy(), want.rows)
    assert tuple(we.alt.shape) == tuple(we.ref.shape) == want.alt.shape
    return (float(np.abs(we.ref.double().cpu().numpy() - want.ref).max()),
            float(np.abs(we.alt.double().cpu().numpy() - want.alt).max()))


def _bits(we):
    return [t.cpu().numpy().tobytes() for t in (we.offsets, we.rows, we.ref, we.alt)]


@pytest.mark.parametrize("kind,d,layers", CASES)
def test_both_routes_match_float64(kind, d, layers):
    case, dev = _device_case(kind, d, layers)
    y = _yardstick(kind, d, layers)
    contact, own = EC.effect_floor(case["want"]["contacts"])
    assert contact >= 1e-3 and own >= 1e-3                    # float64 alone: echoing ref cannot pass
    for scope in ("own", "contacts"):
        want = case["want"][scope]
        for route, tol in (("restricted", 4 * y), ("composed", y + 1e-7)):
            e_ref, e_alt = _errors(_run(dev, case, scope=scope, route=route), want)
            print("effects %s d=%d L=%d %s %s: yardstick %.3e  ref %.3e  alt %.3e" % (kind, d, layers, scope, route, y, e_ref, e_alt))
            assert e_ref <= tol and e_alt <= tol, (route, scope, e_ref, e_alt, tol)
    we = _run(dev, case, scope="contacts")                    # "auto" is the restricted route here
    assert _bits(we) == _bits(_run(dev, case, scope="contacts", route="restricted"))
    r, rf, al = we[0]
    a = int(case["want"]["contacts"].offsets[1])
    assert r.shape[0] == a and torch.equal(al, we.alt[:a]) and torch.equal(rf, we.ref[:a])


def test_three_layers_run_composed_and_refuse_restricted():
    kind, d, layers = "hic", 128, 3
    case, dev = _device_case(kind, d, layers)
    y = _yardstick(kind, d, layers)
    for scope in ("own", "contacts"):
        e_ref, e_alt = _errors(_run(dev, case, scope=scope), case["want"][scope])      # "auto": composed
        print("effects hic d=128 L=3 %s composed: yardstick %.3e  ref %.3e  alt %.3e" % (scope, y, e_ref, e_alt))
        assert e_ref <= y + 1e-7 and e_alt <= y + 1e-7
    with pytest.raises(ValueError):
        _run(dev, case, route="restricted")


@pytest.mark.parametrize("d,layers", [(128, 1), (128, 2), (256, 2)])
def test_small_workspace_batches_and_repeats_give_the_same_bits(d, layers):
    case, dev = _device_case("hic", d, layers)
    per_inst = 2 * d * 4 * (2 + layers) + 2 * 4
    cap = 100 * per_inst
    counts = np.diff(case["want"]["contacts"].offsets).tolist()
    assert counts[0] > 100 and len(E._batches(counts, 100)) >= 3      # the hub exceeds the cap alone; >= 3 batches
    for scope in ("own", "contacts"):
        one = _bits(_run(dev, case, scope=scope, route="restricted"))
        assert one == _bits(_run(dev, case, scope=scope, route="restricted"))                           # repeatable
        assert one == _bits(_run(dev, case, scope=scope, route="restricted", max_workspace_bytes=cap))
        assert one == _bits(_run(dev, case, scope=scope, route="restricted", max_workspace_bytes=1))    # a variant per batch


@pytest.mark.parametrize("kind", ["hic", "asym"])
def test_knockout_map(kind):
    d, layers, c = 128, 2, 7
    (case, want), (_, dev) = EC.knockout_case(kind), _device_case(kind, d, layers)
    tol = c * 4 * _yardstick(kind, d, layers)
    g = dev["graph"]
    got = C.knockout_map(dev["model"], dev["x_f"], dev["x_r"], g)
    assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == (g.col_t.numel(),) == want.shape
    err = float(np.abs(got.double().cpu().numpy() - want).max())
    print("knockout %s: tolerance %.3e  worst %.3e  largest entry %.3e" % (kind, tol, err, want.max()))
    assert err <= tol and want.max() > 1e-2
    small = C.knockout_map(dev["model"], dev["x_f"], dev["x_r"], g, max_workspace_bytes=1 << 16)       # several calls
    assert torch.equal(small, got)
    comp = C.knockout_map(dev["model"], dev["x_f"], dev["x_r"], g, labels=[1, 5], route="composed")
    sel = C.knockout_map(dev["model"], dev["x_f"], dev["x_r"], g, labels=[1, 5])
    assert float((comp - sel).abs().max()) <= 2 * 5 * _yardstick(kind, d, layers) + 2e-7 and float(sel.max()) < float(got.max())


def test_routes_agree_at_103_labels():
    kind, d, layers, c = "hic", 128, 2, 103
    case, dev = _device_case(kind, d, layers, c)
    y = _yardstick(kind, d, layers, c)
    want = case["want"]["contacts"]
    r, q = _run(dev, case, scope="contacts", route="restricted"), _run(dev, case, scope="contacts", route="composed")
    e_r, e_q = _errors(r, want), _errors(q, want)
    diff = float((r.alt - q.alt).abs().max())
    print("effects C=103: yardstick %.3e  restricted %.3e  composed %.3e  routes apart %.3e" % (y, e_r[1], e_q[1], diff))
    assert max(e_r) <= 4 * y and max(e_q) <= y + 1e-7
    assert torch.equal(r.rows, q.rows) and torch.equal(r.offsets, q.offsets)
    assert diff <= 4 * y + y + 1e-7 and float((r.ref - q.ref).abs().max()) <= 4 * y + y + 1e-7
