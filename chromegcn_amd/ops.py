"""torch.autograd bindings of the C ABI (include/chromegcn.h).  Plumbing only: every tensor
allocation is torch's caching allocator, every launch goes to torch's current HIP stream, so
all of it can be captured into a HIP graph.  No fallbacks: CPU tensors raise."""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from . import graph as G
from .graph import ChromGraph

SUPPORTED_D = (128, 256)


def _require_cuda(t: torch.Tensor, name: str):
    if not t.is_cuda:
        raise RuntimeError(
            "chromegcn_amd: %s is on %s; the gated-GCN path only exists as HIP kernels "
            "(no CPU fallback) -- move the model and inputs to the GPU" % (name, t.device))
    if t.dtype != torch.float32:
        raise RuntimeError("chromegcn_amd: %s must be float32, got %s" % (name, t.dtype))


def _dense(t: torch.Tensor) -> torch.Tensor:
    """contiguous and 16-byte aligned (the kernels use 8/16-byte row accesses): a view that starts in the middle of
    another tensor's storage is copied once instead of being rejected by the C ABI"""
    t = t.contiguous()
    return t.clone() if t.data_ptr() % 16 else t


def _check_rng(rng_state, dropout: bool):
    if dropout and rng_state is None:
        raise RuntimeError("chromegcn_amd: fused dropout needs the model's rng_state tensor")


def _check_momentum(momentum):
    if momentum is None:
        raise RuntimeError("chromegcn_amd: BatchNorm momentum=None (cumulative average) is not supported by the fused head")


def _check_feat(x: torch.Tensor, g: ChromGraph, name="x", any_width=False):
    _require_cuda(x, name)
    ok_d = (x.dim() == 3 and x.shape[2] % 4 == 0 and 4 <= x.shape[2] <= 4096) if any_width else (x.dim() == 3 and x.shape[2] in SUPPORTED_D)
    if x.dim() != 3 or x.shape[0] not in (1, 2) or not ok_d:
        raise RuntimeError("chromegcn_amd: %s must be [S in {1,2}, n, d %s], got %s" %
                           (name, "a multiple of 4, <= 4096" if any_width else "in {128,256}", tuple(x.shape)))
    if x.shape[1] != g.n:
        raise RuntimeError("chromegcn_amd: %s has %d nodes but the graph has %d" % (name, x.shape[1], g.n))


def spmm(x, graph):
    """registered operator torch.ops.chromegcn.spmm (chromegcn_amd/torch_ops.py) on the graph's CSR tensors"""
    _check_feat(x, graph, any_width=True)
    from . import torch_ops  # noqa: F401  (registers the ops)
    return torch.ops.chromegcn.spmm(x, graph.rowptr, graph.col, graph.val, graph.row_scale, graph.rowptr_t, graph.col_t,
                                    graph.val_t)


def sddmm(a, b, graph: ChromGraph, transposed=False, out=None):
    """out[k] = sum_s <a[s,i,:], b[s,col[k],:]> on the graph's pattern (cgcn_sddmm).  No autograd.
    out given: the product is ADDED to it (the saliency sums one product per layer)."""
    _check_feat(a, graph, "a")
    _check_feat(b, graph, "b")
    a, b = _dense(a), _dense(b)
    S, n, d = a.shape
    rowptr, col = (graph.rowptr_t, graph.col_t) if transposed else (graph.rowptr, graph.col)
    acc = out is not None
    if acc:
        if out.shape != (col.shape[0],) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != a.device:
            raise RuntimeError("chromegcn_amd: sddmm accumulates into a contiguous fp32 [nnz] tensor on the features' device")
    else:
        out = torch.empty(col.shape[0], device=a.device, dtype=torch.float32)
    _lib.call("cgcn_sddmm", n=n, S=S, d=d, rowptr=rowptr, col=col, A=a, B=b, out=out, accumulate=1 if acc else 0)
    return out


def saliency_normalize(raw, graph: ChromGraph):
    """|val * raw| divided by its row sum, then by the row maximum of the quotients (scripts/visualize.py:49-55) on the
    graph's pattern, one launch (cgcn_saliency_normalize)."""
    _require_cuda(raw, "raw")
    raw = raw.contiguous()
    out = torch.empty_like(raw)
    _lib.call("cgcn_saliency_normalize", n=graph.n, rowptr=graph.rowptr, val=graph.val, raw=raw, out=out)
    return out


_EVAL_BWD_MSG = ("chromegcn_amd: backward through the fused classifier head needs train mode (the eval-mode kernel "
                 "saves nothing for it); call model.train(), or use ChromeGCN.forward / forward_strands, whose "
                 "torch head differentiates in eval mode like the reference's")

_saliency_tap = None  # set by chromegcn_amd.saliency while it collects per-layer (X, dHs)

# Set by the stage engine around one train step (finetune.GCNStage): the flat parameter / gradient / momentum arenas and
# the SGD hyper-parameters.  The FIRST layer's backward -- the last launch of the step -- then carries the optimizer step
# in extra workgroups of its gather (or, without an input gradient, its partial-sum) launch (cgcn_sgd_fuse) and marks
# the request done; anything it cannot fuse (gradients not in the flat arena) is left for cgcn_sgd_step.
_sgd_fuse = None


def _sgd_fuse_arg(layer_id, sink):
    """the cgcn_sgd_fuse for this cgcn_layer_bwd call (of a layer whose gradients go into `sink`), or None"""
    rq = _sgd_fuse
    if rq is None or rq.get("done") or layer_id != 1 or sink is None:
        return None
    fg = rq["grad"]
    lo, hi = fg.data_ptr(), fg.data_ptr() + 4 * fg.numel()
    if not all(lo <= t.data_ptr() and t.data_ptr() + 4 * t.numel() <= hi for t in sink):
        return None
    return _lib.SgdFuse(rq["param"].data_ptr(), fg.data_ptr(), _lib.ptr(rq["mom"]), fg.numel(), float(rq["lr"]),
                        float(rq["momentum"]), float(rq["weight_decay"]), float(rq["grad_scale"]), 1 if rq["nesterov"] else 0,
                        _lib.ptr(rq["rng_state"]))


# Set by the stage engine around one chromosome's step inside a captured epoch (finetune.GCNStage, CGCN_CO_AGG): the NEXT
# chromosome's first aggregation H1 = A X0 as a cgcn_spmm_job {"job": _lib.SpmmJob, "done": False}.  The first layer's
# backward -- the last launch of the step -- takes it along (cgcn_layer_bwd_co) and marks it done.
_co_agg = None


def spmm_job(x, graph, h):
    """the cgcn_spmm_job  h = diag(row_scale) A x  on `graph` (x, h: dense [S, n, d]; the caller keeps them alive)"""
    S, n, d = x.shape
    return _lib.SpmmJob(n, S, d, _lib.ptr(graph.rowptr), _lib.ptr(graph.col), _lib.ptr(graph.val), _lib.ptr(graph.row_scale),
                        x.data_ptr(), h.data_ptr(), G.aux_ptr(graph.col))


# The one call site of each launch, shared with torch_ops.py.  Inputs arrive dense (_dense, _layer_params, _head_params);
# csr / csr_t: (rowptr, col, val, row_scale) of the graph and (rowptr_t, col_t, val_t, row_scale) of its transpose.
def _layer_params(weight, bias, gate_w, gate_b):
    return _dense(weight), bias.contiguous(), gate_w.contiguous().view(-1), gate_b.contiguous().view(-1)


def _head_params(bn_w, bn_b, w_out, b_out):
    return _dense(bn_w), _dense(bn_b), _dense(w_out), b_out.contiguous()


def layer_fwd(x, params, csr, z, h, dropout_p=0.0, rng_state=None, layer_id=0, h_in=None, colstats=None, colstats_rows=0):
    """cgcn_layer_fwd -> (X', gate); z / h: the Z and H buffers to fill, or None"""
    S, n, d = x.shape
    weight, bias, wg, cg = params
    rowptr, col, val, row_scale = csr
    xn, gate = torch.empty_like(x), torch.empty((S, n), device=x.device, dtype=torch.float32)
    _lib.call("cgcn_layer_fwd", n=n, S=S, d=d, rowptr=rowptr, col=col, val=val, row_scale=row_scale, X=x, W=weight, b=bias,
              wg=wg, cg=cg, Xn=xn, Z=z, H=h, gate=gate, dropout_p=float(dropout_p),
              rng_state=rng_state if dropout_p > 0 else None, stream_id=int(layer_id), H_in=h_in, colstats=colstats,
              colstats_rows=colstats_rows, aux=G.aux_ptr(col))
    return xn, gate


def layer_bwd(x, z, h, gate, weight, wg, csr_t, dx, dhs, dropout_in, rng_state, layer_id, dxn=None, dgate=None, head=None,
              sink=None, fuse_sink=None, aux_stream=None):
    """cgcn_layer_bwd -> (dW, db, dwg, dcg), written into `sink` when one is given.  dL/dX' comes as dxn (+ dgate) or from
    the fused head (head: a _lib.HeadGrad).  fuse_sink: the engine's gradient sink of this layer, which lets the call carry
    the step's SGD update (_sgd_fuse) when there is no aux_stream (_lib.aux_stream_ptr)."""
    S, n, d = x.shape
    f32 = dict(device=x.device, dtype=torch.float32)
    if sink is not None:
        dw, db, dwg, dcg = sink
    else:
        dw, db, dwg, dcg = torch.empty_like(weight), torch.empty(d, **f32), torch.empty(d, **f32), torch.empty(1, **f32)
    ws = _lib.layer_bwd_workspace(n, S, d, x.device)
    sgd = _sgd_fuse_arg(layer_id, fuse_sink) if aux_stream is None else None
    rowptr_t, col_t, val_t, row_scale = csr_t
    co = _co_agg if (layer_id == 1 and _co_agg is not None and not _co_agg["done"]) else None
    args = dict(n=n, S=S, d=d, rowptr_t=rowptr_t, col_t=col_t, val_t=val_t, row_scale=row_scale, X=x, Z=z,
                H=h, gate=gate, W=weight, wg=wg, dXn=dxn, dgate=dgate, dX=dx, dHs=dhs, dW=dw, db=db, dwg=dwg, dcg=dcg,
                accumulate=0, in_dropout_p=float(dropout_in), rng_state=rng_state, in_stream_id=max(layer_id - 1, 0),
                head=head, workspace=ws, workspace_bytes=ws.numel(), aux_stream=aux_stream, sgd=sgd, aux_t=G.aux_ptr(col_t))
    if co is None:
        _lib.call("cgcn_layer_bwd", **args)
    else:
        _lib.call("cgcn_layer_bwd_co", companion=co["job"], **args)
        co["done"] = True
    if sgd is not None:
        _sgd_fuse["done"] = True
    return dw, db, dwg, dcg


def head_fwd(x, params, target, run_mean, run_var, nbt, momentum, eps, training, dropout_p, rng_state, probs, loss, dpred,
             save_mean, save_invstd):
    """cgcn_head_fwd; dpred / save_mean / save_invstd: buffers to fill, or None"""
    S, n, d = x.shape
    bn_w, bn_b, w_out, b_out = params
    ws = _lib.head_workspace(n, S, d, w_out.shape[0], x.device)
    _lib.call("cgcn_head_fwd", n=n, S=S, d=d, C=w_out.shape[0], X=x, bn_w=bn_w, bn_b=bn_b, run_mean=run_mean, run_var=run_var,
              num_batches_tracked=nbt, momentum=float(momentum), eps=float(eps), training=1 if training else 0, W_out=w_out,
              b_out=b_out, target=target, dropout_p=float(dropout_p),
              rng_state=rng_state if training and dropout_p > 0 else None, probs=probs, loss=loss, dpred=dpred,
              save_mean=save_mean, save_invstd=save_invstd, workspace=ws, workspace_bytes=ws.numel())


def _head_grad_bufs(sink, d, w_out):
    """(dbn_w, dbn_b, dW_out, db_out): the gradient sink, or new buffers"""
    if sink is not None:
        return sink
    f32 = dict(device=w_out.device, dtype=torch.float32)
    return torch.empty(d, **f32), torch.empty(d, **f32), torch.empty_like(w_out), torch.empty(w_out.shape[0], **f32)


def head_bwd(dloss, x, bn_w, bn_b, w_out, dpred, save_mean, save_invstd, dropout_p, rng_state, sink=None):
    """cgcn_head_bwd -> (dX, dbn_w, dbn_b, dW_out, db_out); the parameter gradients go into `sink` when one is given"""
    S, n, d = x.shape
    C = w_out.shape[0]
    ws = _lib.head_workspace(n, S, d, C, x.device)
    dx = torch.empty_like(x)
    dbn_w, dbn_b, dw_out, db_out = _head_grad_bufs(sink, d, w_out)
    _lib.call("cgcn_head_bwd", n=n, S=S, d=d, C=C, X=x, bn_w=bn_w, bn_b=bn_b, save_mean=save_mean, save_invstd=save_invstd,
              W_out=w_out, dpred=dpred.contiguous(), dloss=dloss.contiguous().view(1), dropout_p=float(dropout_p),
              rng_state=rng_state if dropout_p > 0 else None, dX=dx, dW_out=dw_out, db_out=db_out, dbn_w=dbn_w, dbn_b=dbn_b,
              accumulate=0, workspace=ws, workspace_bytes=ws.numel())
    return dx, dbn_w, dbn_b, dw_out, db_out


# feature tables from this size on do not fit the L2s: cgcn_layer_fwd's split route (FWD_SPLIT_TABLE_BYTES in csrc)
_SPLIT_TABLE_BYTES = 6 << 20


def _resolve_h_cache(h_cache, x, need_bwd):
    """h_cache: None, or a dict holder {'h': tensor-or-None} for H = A X of a layer whose input never changes
    (the engine keeps one per chromosome for the first layer).  Returns (H_in to stream, H buffer to write)."""
    if h_cache is not None and h_cache.get("h") is not None:
        hc = h_cache["h"]
        if hc.shape != x.shape or hc.device != x.device:
            raise RuntimeError("chromegcn_amd: cached aggregation does not match the input")
        return hc, None
    if need_bwd or h_cache is not None or (x.numel() * 4 >= _SPLIT_TABLE_BYTES and x.shape[0] * x.shape[2] <= 256):
        # inference on a large table too: with an H buffer cgcn_layer_fwd takes the feature-sliced two-launch route
        return None, torch.empty_like(x)
    return None, None


def _store_h_cache(h_cache, h_in, h):
    if h_in is not None:
        return h_in
    if h_cache is not None and h is not None:
        h_cache["h"] = h
    return h


def _out_slots(out_slots, n, C, device):
    """(probs [n,C], loss [1]) buffers for the fused head.  out_slots: None, or a holder {'probs': [n,C] view,
    'loss': [1] view} into caller-owned arenas (GCNStage lays every chromosome's predictions out in one buffer in
    chromosome order, so a split's concatenated predictions -- finetune.py:52 -- need no copy at all)."""
    if out_slots is not None:
        probs, loss = out_slots["probs"], out_slots["loss"]
        if tuple(probs.shape) != (n, C) or loss.numel() != 1 or not probs.is_contiguous() or probs.device != device:
            raise RuntimeError("chromegcn_amd: out_slots do not match [n, C] = [%d, %d]" % (n, C))
        return probs, loss.view(1)
    return (torch.empty((n, C), device=device, dtype=torch.float32), torch.empty(1, device=device, dtype=torch.float32))


def _sink_ok(sink, shapes):
    return sink is not None and all(t is not None and tuple(t.shape) == tuple(sh) and t.is_contiguous()
                                    for t, sh in zip(sink, shapes))


class GatedLayerFn(torch.autograd.Function):
    """One gated GCN layer (models/ChromeModels.py:37-40), fused; see cgcn_layer_fwd / cgcn_layer_bwd.

    dropout_out / dropout_in implement the F.dropout between layers (models/ChromeModels.py:42) inside the
    kernels: this layer's output is dropped with stream id `layer_id`; its input was dropped by the previous
    layer (stream id layer_id - 1), which the backward undoes on dX.  rng_state: uint64[2] device tensor
    {seed, step counter}, constant over one step.
    grad_sink (engine use): tensors (dW, db, dgate_w, dgate_b) the backward writes the parameter gradients
    INTO (overwrite); autograd then receives None for them, which skips its per-parameter accumulate kernels."""

    @staticmethod
    def forward(ctx, x, weight, bias, gate_w, gate_b, graph: ChromGraph, dropout_out, dropout_in, rng_state,
                layer_id, grad_sink, h_cache, zero_stat=None):
        _check_feat(x, graph)
        for t, nm in ((weight, "weight"), (bias, "bias"), (gate_w, "gate weight"), (gate_b, "gate bias")):
            _require_cuda(t, nm)
        x = _dense(x)
        S, n, d = x.shape
        if tuple(weight.shape) != (d, d):
            raise RuntimeError("chromegcn_amd: fused layer needs a square [d,d] weight, got %s" % (tuple(weight.shape),))
        params = _layer_params(weight, bias, gate_w, gate_b)
        need_bwd = any(ctx.needs_input_grad[:5])
        z = torch.empty_like(x) if need_bwd else None
        h_in, h = _resolve_h_cache(h_cache, x, need_bwd)
        _check_rng(rng_state, dropout_out > 0 or dropout_in > 0)
        # zero_stat: the NEXT (last) layer's statistics totals, zeroed by this call's first launch
        xn, gate = layer_fwd(x, params, (graph.rowptr, graph.col, graph.val, graph.row_scale), z, h, dropout_out, rng_state,
                             layer_id, h_in, zero_stat, _lib.COLSTATS_ROWS_ZERO_ONLY if zero_stat is not None else 0)
        h = _store_h_cache(h_cache, h_in, h)
        if need_bwd:
            ctx.save_for_backward(x, z, h, gate, params[0], params[2], rng_state if dropout_in > 0 else None)
        ctx.graph = graph
        ctx.gate_w_shape = gate_w.shape
        ctx.gate_b_shape = gate_b.shape
        ctx.dropout_in = float(dropout_in)
        ctx.layer_id = int(layer_id)
        ctx.sink = grad_sink if _sink_ok(grad_sink, ((d, d), (d,), gate_w.shape, gate_b.shape)) else None
        ctx.set_materialize_grads(False)  # an unused gate output must not cost a zero-fill + an extra read
        return xn, gate

    @staticmethod
    def backward(ctx, dxn, dgate):
        x, z, h, gate, weight, wg, rng_state = ctx.saved_tensors
        g = ctx.graph
        if dxn is None and dgate is None:
            return (None,) * 13
        dxn = torch.zeros_like(x) if dxn is None else _dense(dxn)
        dgate = None if dgate is None else dgate.contiguous()
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None  # None: skip the gather over Ahat^T
        # dHs = diag(row_scale) dL/dU W^T: the gather's operand (and the saliency SDDMM's); not computed when unused
        dhs = torch.empty_like(x) if (dx is not None or _saliency_tap is not None) else None
        dw, db, dwg, dcg = layer_bwd(x, z, h, gate, weight, wg, (g.rowptr_t, g.col_t, g.val_t, g.row_scale), dx, dhs,
                                     ctx.dropout_in, rng_state, ctx.layer_id, dxn, dgate, sink=ctx.sink, fuse_sink=ctx.sink,
                                     aux_stream=_lib.aux_stream_ptr())
        if _saliency_tap is not None:
            _saliency_tap.append((x, dhs, g))
        if ctx.sink is not None:
            return (dx, None, None, None, None) + (None,) * 8
        return (dx, dw, db, dwg.view(ctx.gate_w_shape), dcg.view(ctx.gate_b_shape)) + (None,) * 8


def gated_layer(x, weight, bias, gate_w, gate_b, graph, dropout_out=0.0, dropout_in=0.0, rng_state=None,
                layer_id=0, grad_sink=None, h_cache=None, zero_stat=None):
    """One gated layer -> (X', gate).  Plain callers (ChromeGCN.forward, tests) go through the registered operator
    torch.ops.chromegcn.gated_layer; the engine's extras (gradient sinks, cached aggregation, the saliency tap) need
    the autograd node below.
    zero_stat: the statistics-totals buffer of the LAST layer's call (stat_buffer), zeroed by this call's first launch so
    that the last layer may accumulate into it on any route (cgcn_layer_fwd, colstats_rows = -2 / -3)."""
    if grad_sink is None and h_cache is None and _saliency_tap is None and zero_stat is None:
        _check_feat(x, graph)
        from . import torch_ops  # noqa: F401
        xn, gate, _z, _h = torch.ops.chromegcn.gated_layer(
            x, weight, bias, gate_w, gate_b, graph.rowptr, graph.col, graph.val, graph.row_scale, graph.rowptr_t,
            graph.col_t, graph.val_t, float(dropout_out), float(dropout_in), rng_state, int(layer_id))
        return xn, gate
    return GatedLayerFn.apply(x, weight, bias, gate_w, gate_b, graph, float(dropout_out), float(dropout_in),
                              rng_state, int(layer_id), grad_sink, h_cache, zero_stat)


def stat_buffer(x):
    """The accumulate-mode statistics buffer for features x [S, n, d] (include/chromegcn.h, cgcn_layer_fwd_colstats_plan with
    CGCN_COLSTATS_ACCUMULATE), or None when the shape has none (n < 2).  Uninitialised: a launch of the step zeroes it."""
    S, n, d = x.shape
    rows = ctypes.c_int(0)
    tiles = _lib.query("cgcn_layer_fwd_colstats_plan", n=n, S=S, d=d, mode=_lib.COLSTATS_ACCUMULATE, rows_per_tile=rows)
    if tiles <= 0 or rows.value != -1:
        return None
    return torch.empty((tiles, S, d, 2), device=x.device, dtype=torch.float32)


class HeadLossFn(torch.autograd.Function):
    """relu -> BatchNorm1d -> dropout -> Linear, mean over strands, BCE-with-logits, sigmoid -- fused
    (models/ChromeModels.py:48-51 + finetune.py:43,45,52); see cgcn_head_fwd / cgcn_head_bwd.
    Returns (loss [], probs [n,C]).  Running statistics / num_batches_tracked are updated in place when
    training, exactly as two successive ChromeGCN.forward calls would.  grad_sink: (dbn_w, dbn_b, dW_out, db_out)."""

    @staticmethod
    def forward(ctx, x, bn_w, bn_b, w_out, b_out, target, run_mean, run_var, nbt, momentum, eps, training,
                dropout_p, rng_state, grad_sink, out_slots=None):
        _require_cuda(x, "x")
        for t, nm in ((bn_w, "bn weight"), (bn_b, "bn bias"), (w_out, "out.weight"), (b_out, "out.bias"), (target, "target")):
            _require_cuda(t, nm)
        _check_momentum(momentum)
        x = _dense(x)
        S, n, d = x.shape
        C = w_out.shape[0]
        target = target.contiguous()
        if tuple(target.shape) != (n, C):
            raise RuntimeError("chromegcn_amd: target must be [n, C] = [%d, %d], got %s" % (n, C, tuple(target.shape)))
        params = _head_params(bn_w, bn_b, w_out, b_out)
        need_bwd = training and any(ctx.needs_input_grad[:5])
        ctx.eval_grad = (not training) and any(ctx.needs_input_grad[:5])
        probs, loss = _out_slots(out_slots, n, C, x.device)
        dpred = torch.empty((n, C), device=x.device, dtype=torch.float32) if need_bwd else None
        save_mean = torch.empty((S, d), device=x.device, dtype=torch.float32) if training else None
        save_invstd = torch.empty((S, d), device=x.device, dtype=torch.float32) if training else None
        drop = bool(training) and dropout_p > 0
        _check_rng(rng_state, drop)
        head_fwd(x, params, target, run_mean, run_var, nbt, momentum, eps, training, dropout_p, rng_state, probs, loss, dpred,
                 save_mean, save_invstd)
        if need_bwd:
            ctx.save_for_backward(x, *params[:3], dpred, save_mean, save_invstd, rng_state if drop else None)
            ctx.dropout_p = float(dropout_p) if drop else 0.0
            ctx.sink = grad_sink if _sink_ok(grad_sink, ((d,), (d,), (C, d), (C,))) else None
        ctx.mark_non_differentiable(probs)
        return loss.view(()), probs

    @staticmethod
    def backward(ctx, dloss, _dprobs):
        if ctx.eval_grad:
            raise RuntimeError(_EVAL_BWD_MSG)
        x, bn_w, bn_b, w_out, dpred, save_mean, save_invstd, rng_state = ctx.saved_tensors
        dx, dbn_w, dbn_b, dw_out, db_out = head_bwd(dloss, x, bn_w, bn_b, w_out, dpred, save_mean, save_invstd, ctx.dropout_p,
                                                    rng_state, ctx.sink)
        if ctx.sink is not None:
            return (dx,) + (None,) * 15
        return (dx, dbn_w, dbn_b, dw_out, db_out) + (None,) * 11


class LastLayerHeadLossFn(torch.autograd.Function):
    """Last gated layer + classifier head + loss as ONE autograd node (engine path).  Forward = cgcn_layer_fwd
    then cgcn_head_fwd.  Backward = cgcn_head_bwd in deferred mode, then cgcn_layer_bwd in head mode: the
    gradient w.r.t. the layer's output never exists in memory as a tensor of its own (include/chromegcn.h,
    cgcn_head_grad).  Inputs/semantics as GatedLayerFn + HeadLossFn; returns (loss [], probs [n,C], gate [S,n])."""

    @staticmethod
    def forward(ctx, x, weight, bias, gate_w, gate_b, bn_w, bn_b, w_out, b_out, graph, target, run_mean, run_var, nbt,
                momentum, eps, training, dropout_p, dropout_in, rng_state, layer_id, layer_sink, head_sink, h_cache,
                out_slots=None, stat_acc=False, stat_buf=None):
        _check_feat(x, graph)
        for t, nm in ((weight, "weight"), (bias, "bias"), (gate_w, "gate weight"), (gate_b, "gate bias"),
                      (bn_w, "bn weight"), (bn_b, "bn bias"), (w_out, "out.weight"), (b_out, "out.bias"), (target, "target")):
            _require_cuda(t, nm)
        _check_momentum(momentum)
        x = _dense(x)
        S, n, d = x.shape
        C = w_out.shape[0]
        target = target.contiguous()
        if tuple(weight.shape) != (d, d) or tuple(target.shape) != (n, C):
            raise RuntimeError("chromegcn_amd: bad shapes for the fused last layer + head")
        weight, bias, wg, cg = _layer_params(weight, bias, gate_w, gate_b)
        bn_w, bn_b, w_out, b_out = _head_params(bn_w, bn_b, w_out, b_out)
        need_bwd = training and any(ctx.needs_input_grad[:9])
        ctx.eval_grad = (not training) and any(ctx.needs_input_grad[:9])
        z = torch.empty_like(x) if need_bwd else None
        h_in, h = _resolve_h_cache(h_cache, x, need_bwd)
        colstats, cs_tiles, cs_rows, fwd_rows = None, 0, 0, 0
        if need_bwd:
            # the layer kernel also emits the first stage of the head's BatchNorm statistics (tile still on chip)
            # stat_acc: the caller vouches for the range of the fixed-point totals (include/chromegcn.h,
            # cgcn_layer_fwd_colstats_plan; GCNStage does, per chromosome) -> accumulate mode: no finalize / finish launches;
            # otherwise per-workgroup records.  Accumulate mode needs the two-launch route, i.e. an H buffer of this call.
            # stat_buf: totals an EARLIER launch of this step has zeroed (the previous layer's forward: gated_layer(zero_stat=...));
            # this layer then accumulates on whatever route its table size gives it -- the fused kernel for small tables.
            if stat_acc and stat_buf is not None:
                colstats, cs_tiles, cs_rows = stat_buf, stat_buf.shape[0], -1
                fwd_rows = _lib.COLSTATS_ROWS_ACCUMULATE_ZEROED
            else:
                mode = _lib.COLSTATS_ACCUMULATE if (stat_acc and (h is not None or h_in is not None)) else _lib.COLSTATS_RECORDS
                rows = ctypes.c_int(0)
                cs_tiles = _lib.query("cgcn_layer_fwd_colstats_plan", n=n, S=S, d=d, mode=mode, rows_per_tile=rows)
                cs_rows = fwd_rows = rows.value
                colstats = torch.empty((cs_tiles, S, d, 2), device=x.device, dtype=torch.float32)
        xn, gate = layer_fwd(x, (weight, bias, wg, cg), (graph.rowptr, graph.col, graph.val, graph.row_scale), z, h,
                             layer_id=layer_id, h_in=h_in, colstats=colstats, colstats_rows=fwd_rows)
        h = _store_h_cache(h_cache, h_in, h)
        probs, loss = _out_slots(out_slots, n, C, x.device)
        save_mean = torch.empty((S, d), device=x.device, dtype=torch.float32) if training else None
        save_invstd = torch.empty((S, d), device=x.device, dtype=torch.float32) if training else None
        drop = bool(training) and dropout_p > 0
        _check_rng(rng_state, drop or dropout_in > 0)
        if need_bwd:
            # forward of the head + the tile-local half of its backward in one pass (cgcn_head_train); the workspace
            # carries dym and the partial sums to backward()
            ws = _lib.head_workspace(n, S, d, C, x.device)
            _lib.call("cgcn_head_train", n=n, S=S, d=d, C=C, X=xn, bn_w=bn_w, bn_b=bn_b, run_mean=run_mean, run_var=run_var,
                      num_batches_tracked=nbt, momentum=float(momentum), eps=float(eps), W_out=w_out, b_out=b_out,
                      target=target, dropout_p=float(dropout_p) if drop else 0.0, rng_state=rng_state if drop else None,
                      probs=probs, loss=loss, save_mean=save_mean, save_invstd=save_invstd, col_stats=colstats,
                      col_stats_tiles=cs_tiles, col_stats_rows=cs_rows, workspace=ws, workspace_bytes=ws.numel())
        else:
            head_fwd(xn, (bn_w, bn_b, w_out, b_out), target, run_mean, run_var, nbt, momentum, eps, training, dropout_p,
                     rng_state, probs, loss, None, save_mean, save_invstd)
        if need_bwd:
            ctx.save_for_backward(x, z, h, gate, weight, wg, xn, bn_w, bn_b, w_out, ws, save_mean, save_invstd,
                                  rng_state if (drop or dropout_in > 0) else None,
                                  # accumulate mode (ABI v23, rows = -1): the backward reads the BatchNorm-backward column sums
                                  # from the statistics buffer (cgcn_head_grad.stat_acc), not from the workspace's bnc
                                  colstats if cs_rows == -1 else None)
            ctx.graph = graph
            ctx.dropout_p = float(dropout_p) if drop else 0.0
            ctx.dropout_in = float(dropout_in)
            ctx.layer_id = int(layer_id)
            ctx.shapes = (gate_w.shape, gate_b.shape)
            ctx.layer_sink = layer_sink if _sink_ok(layer_sink, ((d, d), (d,), gate_w.shape, gate_b.shape)) else None
            ctx.head_sink = head_sink if _sink_ok(head_sink, ((d,), (d,), (C, d), (C,))) else None
        ctx.mark_non_differentiable(probs, gate)
        ctx.set_materialize_grads(False)  # no zero-fill kernels for the two non-differentiable outputs
        return loss.view(()), probs, gate

    @staticmethod
    def backward(ctx, dloss, _dprobs, _dgate):
        if ctx.eval_grad:
            raise RuntimeError(_EVAL_BWD_MSG)
        if dloss is None:
            return (None,) * 27
        (x, z, h, gate, weight, wg, xn, bn_w, bn_b, w_out, hws, save_mean, save_invstd, rng_state, stat_acc) = ctx.saved_tensors
        g = ctx.graph
        S, n, d = x.shape
        C = w_out.shape[0]
        dbn_w, dbn_b, dw_out, db_out = _head_grad_bufs(ctx.head_sink, d, w_out)
        dloss = dloss.contiguous().view(1)
        # dym, bnc and the partials are already in the workspace cgcn_head_train filled (for d loss = 1); every head
        # gradient is finished inside cgcn_layer_bwd (cgcn_head_grad.dloss / dbn_w / dbn_b), so no head launch here
        o_dym, o_bnc, o_part = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
        _lib.call("cgcn_head_workspace_layout", n=n, S=S, d=d, C=C, dym_offset=o_dym, bnc_offset=o_bnc, part_offset=o_part)
        hg = _lib.HeadGrad(hws.data_ptr() + o_dym.value, hws.data_ptr() + o_bnc.value, save_mean.data_ptr(),
                           save_invstd.data_ptr(), bn_w.data_ptr(), ctx.dropout_p, _lib.ptr(rng_state),
                           hws.data_ptr() + o_part.value, _lib.query("cgcn_head_bwd_partials", n=n), C, dw_out.data_ptr(),
                           db_out.data_ptr(), 0, dloss.data_ptr(), dbn_w.data_ptr(), dbn_b.data_ptr(), _lib.ptr(stat_acc))
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dhs = torch.empty_like(x) if dx is not None else None
        # a one-layer model: this IS the first layer's backward, i.e. the last launch of the step
        dw, db, dwg, dcg = layer_bwd(x, z, h, gate, weight, wg, (g.rowptr_t, g.col_t, g.val_t, g.row_scale), dx, dhs,
                                     ctx.dropout_in, rng_state, ctx.layer_id, head=hg, sink=ctx.layer_sink,
                                     fuse_sink=ctx.layer_sink if ctx.head_sink is not None else None,
                                     aux_stream=_lib.aux_stream_ptr())
        gl = (None,) * 4 if ctx.layer_sink is not None else (dw, db, dwg.view(ctx.shapes[0]), dcg.view(ctx.shapes[1]))
        gh = (None,) * 4 if ctx.head_sink is not None else (dbn_w, dbn_b, dw_out, db_out)
        return (dx,) + gl + gh + (None,) * 18


def last_layer_head_loss(x, gc, wk, bn, out, graph, target, training, dropout_p, dropout_in, rng_state, layer_id,
                         layer_sink=None, head_sink=None, h_cache=None, out_slots=None, stat_acc=False, stat_buf=None):
    """stat_acc: accumulate mode of the head's BatchNorm sums (fixed-point integer totals, two launches fewer per step).  Its
    range is finite (sum relu(x)^2 < 2.1e9 per column) and outside it the loss is NaN, so it is the caller's statement about
    its inputs: False (records, any magnitude) unless the caller has bounded them -- finetune.GCNStage does per chromosome.
    stat_buf (with stat_acc): stat_buffer(x) that an earlier launch of this step zeroes (gated_layer(zero_stat=stat_buf) of the
    layer before): the last layer then keeps the route its table size gives it (small tables: the one-launch forward)."""
    return LastLayerHeadLossFn.apply(x, gc.weight, gc.bias, wk.weight, wk.bias, bn.weight, bn.bias, out.weight, out.bias,
                                     graph, target, bn.running_mean, bn.running_var, bn.num_batches_tracked, bn.momentum,
                                     bn.eps, bool(training), float(dropout_p), float(dropout_in), rng_state, int(layer_id),
                                     layer_sink, head_sink, h_cache, out_slots, bool(stat_acc), stat_buf)


def head_loss(x, bn: torch.nn.BatchNorm1d, out: torch.nn.Linear, target, training, dropout_p, rng_state, grad_sink=None,
              out_slots=None):
    if grad_sink is None and out_slots is None:
        from . import torch_ops
        _require_cuda(x, "x")
        return torch_ops.head_loss_module(x, bn, out, target, training, dropout_p, rng_state)  # torch.ops.chromegcn.head_loss
    return HeadLossFn.apply(x, bn.weight, bn.bias, out.weight, out.bias, target, bn.running_mean, bn.running_var,
                            bn.num_batches_tracked, bn.momentum, bn.eps, bool(training), float(dropout_p), rng_state,
                            grad_sink, out_slots)


def head_logits(x, bn: torch.nn.BatchNorm1d, out: torch.nn.Linear):
    """The eval-mode head of ChromeGCN.forward per strand (models/ChromeModels.py:48-51 with running statistics and
    dropout off): relu -> BatchNorm1d -> Linear in one kernel (torch.ops.chromegcn.head_logits -> cgcn_head_logits).
    x: [S, n, d] -> logits [S, n, C].  No autograd: callers use it when nothing needs a gradient (layers.ChromeGCN._head)."""
    _require_cuda(x, "x")
    from . import torch_ops  # noqa: F401  (registers the ops)
    return torch.ops.chromegcn.head_logits(x.detach(), bn.weight.detach(), bn.bias.detach(), bn.running_mean, bn.running_var,
                                           float(bn.eps), out.weight.detach(), out.bias.detach())


def sgd_step(flat_param, flat_grad, flat_mom, lr, momentum, weight_decay, nesterov, rng_state=None, grad_scale=1.0):
    """torch.optim.SGD step on flat buffers in one launch (cgcn_sgd_step); also advances the dropout counter."""
    if not (flat_param.is_contiguous() and flat_grad.is_contiguous() and flat_param.numel() == flat_grad.numel()):
        raise RuntimeError("chromegcn_amd: sgd_step: param and grad must be contiguous and of equal size")
    _lib.call("cgcn_sgd_step", count=flat_param.numel(), param=flat_param, grad=flat_grad, momentum_buf=flat_mom, lr=float(lr),
              momentum=float(momentum), weight_decay=float(weight_decay), nesterov=1 if nesterov else 0,
              grad_scale=float(grad_scale), rng_state=rng_state)


def adam_step(flat_param, flat_grad, exp_avg, exp_avg_sq, step, ticket, lr, beta1, beta2, eps, weight_decay,
              rng_state=None, grad_scale=1.0):
    """torch.optim.Adam step on flat buffers in one launch (cgcn_adam_step): `step` is a float32 device tensor of
    per-parameter counts (all advanced by one), `ticket` an int32 device word that stays 0 between launches; also
    advances the dropout counter."""
    n = flat_param.numel()
    if not all(t.is_contiguous() and t.numel() == n for t in (flat_param, flat_grad, exp_avg, exp_avg_sq)):
        raise RuntimeError("chromegcn_amd: adam_step: param, grad, exp_avg and exp_avg_sq must be contiguous and of equal size")
    if step.dtype != torch.float32 or not step.is_contiguous() or ticket.dtype != torch.int32 or ticket.numel() < 1:
        raise RuntimeError("chromegcn_amd: adam_step: step must be contiguous float32, ticket int32 with one element")
    _lib.call("cgcn_adam_step", count=n, param=flat_param, grad=flat_grad, exp_avg=exp_avg, exp_avg_sq=exp_avg_sq, step=step,
              n_step=step.numel(), ticket=ticket, lr=float(lr), beta1=float(beta1), beta2=float(beta2), eps=float(eps),
              weight_decay=float(weight_decay), grad_scale=float(grad_scale), rng_state=rng_state)


# -- label-pair edge ablation (chromegcn_amd/ablation.py; cgcn_ablation_* in include/chromegcn.h) ----------------------
def ablation_workspace_bytes(n_inst, S, d, layers):
    """bytes of the restricted route's workspace for n_inst row instances (0: unsupported shape)"""
    return _lib.query("cgcn_ablation_workspace_bytes", n_inst=int(n_inst), S=int(S), d=int(d), layers=int(layers))


def ablation_prepare(targets):
    """targets [n, C] (nonzero = positive) -> (label_bits uint32 [n, ceil(C/32)] as int32, pos_lists [C, n],
    pos_ranks [C, n], pos_counts [C]), all on targets' device"""
    _require_cuda(targets, "targets")
    t = targets.contiguous()
    n, C = t.shape
    bits = torch.empty((max(n, 1), (C + 31) // 32), device=t.device, dtype=torch.int32)
    lists = torch.empty((C, max(n, 1)), device=t.device, dtype=torch.int32)
    ranks = torch.empty_like(lists)
    counts = torch.empty(C, device=t.device, dtype=torch.int32)
    _lib.call("cgcn_ablation_prepare", n=n, C=C, targets=t, label_bits=bits, pos_lists=lists, pos_ranks=ranks,
              pos_counts=counts)
    return bits, lists, ranks, counts


def ablation_layer(graph: ChromGraph, x, x_inst, params, bits, C, pos_list, pos_rank, n_pos, cols, n_cols, x_out, removed):
    """cgcn_ablation_layer: one gated layer for the (column label, row of P_i) instances; params = _layer_params(...)"""
    S, n, d = x.shape
    weight, bias, wg, cg = params
    _lib.call("cgcn_ablation_layer", n=n, S=S, d=d, rowptr=graph.rowptr, col=graph.col, val=graph.val,
              row_scale=graph.row_scale, X=x, X_inst=x_inst, W=weight, b=bias, wg=wg, cg=cg, label_bits=bits, C=C,
              pos_list=pos_list, pos_rank=pos_rank, n_pos=n_pos, cols=cols, n_cols=n_cols, X_out=x_out, removed=removed)


def ablation_head(x, x_inst, bn: torch.nn.BatchNorm1d, out: torch.nn.Linear, pos_lists, pos_counts, label, n_pos, cols, n_cols,
                  removed, base, M, d):
    """cgcn_ablation_head: label < 0 fills base[C] from x [S, n, d]; label = i fills row i of M from the instances"""
    S, n = (x.shape[0], x.shape[1]) if x is not None else (2, pos_lists.shape[1])
    _lib.call("cgcn_ablation_head", n=n, S=S, d=d, C=out.weight.shape[0], X=x, X_inst=x_inst, bn_w=bn.weight, bn_b=bn.bias,
              run_mean=bn.running_mean, run_var=bn.running_var, eps=float(bn.eps), W_out=out.weight, b_out=out.bias,
              pos_lists=pos_lists, pos_counts=pos_counts, label=int(label), n_pos=int(n_pos), cols=cols, n_cols=int(n_cols),
              removed=removed, base=base, M=M)


def ablation_mask(graph: ChromGraph, bits, C, label_i, label_j, val_out, rs_out, removed):
    """cgcn_ablation_mask: the masked values and row scales of pair (label_i, label_j) on graph's pattern"""
    _lib.call("cgcn_ablation_mask", n=graph.n, C=C, rowptr=graph.rowptr, col=graph.col, val=graph.val,
              row_scale=graph.row_scale, label_bits=bits, label_i=int(label_i), label_j=int(label_j), val_out=val_out,
              row_scale_out=rs_out, removed=removed)


def ablation_reduce(logits, pos_lists, pos_counts, label, col_label, removed, base, M):
    """cgcn_ablation_reduce: label < 0 fills base[C] from logits [S, n, C]; label = i writes M[i, col_label]"""
    S, n, C = logits.shape
    _lib.call("cgcn_ablation_reduce", n=n, S=S, C=C, logits=logits, pos_lists=pos_lists, pos_counts=pos_counts,
              label=int(label), col_label=int(col_label), removed=removed, base=base, M=M)


# -- window effects (chromegcn_amd/effects.py; cgcn_effects_* in include/chromegcn.h) -----------------------------------
def effects_workspace_bytes(n_inst, S, d, layers):
    """bytes of the restricted route's workspace for a batch of n_inst instances (0: unsupported shape)"""
    return _lib.query("cgcn_effects_workspace_bytes", n_inst=int(n_inst), S=int(S), d=int(d), layers=int(layers))


def effects_plan(graph: ChromGraph, windows):
    """windows int32 [M] on the graph's device -> (counts int32 [M]: instances per variant, diag_pos int32 [M]: position of
    the stored diagonal in the transposed row, -1 without one)"""
    M = int(windows.numel())
    counts = torch.empty(max(M, 1), device=windows.device, dtype=torch.int32)[:M]
    diag = torch.empty(max(M, 1), device=windows.device, dtype=torch.int32)[:M]
    _lib.call("cgcn_effects_plan", n=graph.n, rowptr_t=graph.rowptr_t, col_t=graph.col_t, n_var=M, windows=windows,
              counts=counts, diag_pos=diag)
    return counts, diag


def effects_rows1(graph: ChromGraph, x0, h1, windows, alt, offsets, diag_pos, n_var, own, n_inst, h_inst, x_inst, rows):
    """cgcn_effects_rows1: the layer-1 instance rows of n_var variants (windows, alt, offsets, diag_pos: views that start at
    the batch's first variant) into h_inst / x_inst [S][n_inst][d]; rows (or None) gets the window of every instance"""
    S, n, d = x0.shape
    _lib.call("cgcn_effects_rows1", n=n, S=S, d=d, rowptr_t=graph.rowptr_t, col_t=graph.col_t, val_t=graph.val_t,
              row_scale=graph.row_scale, X0=x0, H1=h1, windows=windows, alt=alt, offsets=offsets, diag_pos=diag_pos,
              n_var=int(n_var), own=1 if own else 0, n_inst=int(n_inst), H_inst=h_inst, X_inst=x_inst, rows=rows)


def effects_rows2(graph: ChromGraph, x1, h2, windows, offsets, diag_pos, n_var, own, n_inst, x1_inst, h_out, x_res):
    """cgcn_effects_rows2: the layer-2 rows of the read-out instances (own: instance 0 of every variant) from the instances'
    layer-1 output x1_inst [S][n_inst][d]; x_res (needed when own) gets their residual input"""
    S, n, d = x1.shape
    _lib.call("cgcn_effects_rows2", n=n, S=S, d=d, rowptr=graph.rowptr, col=graph.col, val=graph.val, row_scale=graph.row_scale,
              rowptr_t=graph.rowptr_t, col_t=graph.col_t, X1=x1, H2=h2, windows=windows, offsets=offsets, diag_pos=diag_pos,
              n_var=int(n_var), own=1 if own else 0, n_inst=int(n_inst), X1_inst=x1_inst, H_out=h_out, X_res=x_res)


def layer_dense_rows(h_in, x, params, graph: ChromGraph, xn, gate):
    """The row-local part of one eval gated layer on a table of rows [S, rows, d] whose aggregation is already there:
    cgcn_layer_fwd with H_in (it then launches the row-local kernel alone and never reads the graph arrays, which it only
    requires to be non-NULL) into the caller's xn [S, rows, d] and gate [S, rows]."""
    S, rows, d = x.shape
    weight, bias, wg, cg = params
    _lib.call("cgcn_layer_fwd", n=rows, S=S, d=d, rowptr=graph.rowptr, col=graph.col, val=None, row_scale=None, X=x, W=weight,
              b=bias, wg=wg, cg=cg, Xn=xn, Z=None, H=None, gate=gate, dropout_p=0.0, rng_state=None, stream_id=0, H_in=h_in,
              colstats=None, colstats_rows=0, aux=None)
