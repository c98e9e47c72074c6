"""Exact t-SNE into the plane on the GPU: the class-embedding maps of scripts/visualize.py:148-188, which run scikit-learn's
TSNE for thirteen perplexities over the same points.

The objective and the optimiser are scikit-learn's (sklearn/manifold/_t_sne.py, version 1.7.2), in the O(n^2) form it
defines them by (method='exact'), function by function:
    _joint_probabilities   cgcn_tsne_sqdist (once per point set), cgcn_tsne_affinities + cgcn_tsne_symmetrize (per perplexity)
    _kl_divergence         cgcn_tsne_gradient (degrees of freedom 1; Z in a pass of its own because Q is clamped)
    _gradient_descent      cgcn_tsne_update, and the schedule in tsne_embed below
    TSNE._tsne             250 exploration iterations with P * early_exaggeration and momentum 0.5, then momentum 0.8
The n x n matrices are fp32 with a row pitch of (n + 3) & ~3 floats; P is streamed once per iteration.  One 32-byte record
is read back per convergence check (every 50 iterations); nothing else synchronises.

The *_host functions restate the same definitions in numpy (float64 unless said otherwise): they are what the GPU tests
compare with, and tests/test_tsne_host.py pins them to scikit-learn's own functions.  A t-SNE trajectory is chaotic: after
about 50 iterations two correct implementations differ by the embedding's whole extent, so only single evaluations, short
runs and the objective reached are comparable."""
from __future__ import annotations

from typing import Iterable, Optional, Union

import numpy as np
import torch

from . import _lib, ops

EPS = float(np.finfo(np.float64).eps)      # scikit-learn's MACHINE_EPSILON
EXPLORATION_ITER = 250                     # TSNE._EXPLORATION_MAX_ITER
N_ITER_CHECK = 50                          # TSNE._N_ITER_CHECK
PERPLEXITY_TOLERANCE = 1e-5
_FMAX = float(np.finfo(float).max)


def _pitch(n: int) -> int:
    return (n + 3) & ~3


def _square(n: int, device) -> torch.Tensor:
    """an n x n fp32 matrix with the library's row pitch (a view of a [n, pitch] buffer)"""
    return torch.empty((n, _pitch(n)), device=device, dtype=torch.float32)[:, :n]


def _check_square(m: torch.Tensor, name: str) -> int:
    ops._require_cuda(m, name)
    n = m.shape[0]
    if m.dim() != 2 or m.shape[1] != n or m.stride() != (_pitch(n), 1) or m.data_ptr() % 16:
        raise ValueError("chromegcn_amd.tsne: %s must be an n x n matrix with a row pitch of (n + 3) & ~3 floats" % name)
    return n


def workspace(n: int, device) -> torch.Tensor:
    """the uint8 workspace every cgcn_tsne_* call of one point count shares"""
    return _lib.workspace_for("cgcn_tsne_workspace_bytes", device, "t-SNE, n=%d" % n, n=n)[0]


def sqdist(x: torch.Tensor) -> torch.Tensor:
    """D [n, n]: squared Euclidean distances of the rows of x [n, d], d % 4 == 0 (cgcn_tsne_sqdist)"""
    ops._require_cuda(x, "x")
    if x.dim() != 2:
        raise ValueError("chromegcn_amd.tsne: x must be [n, d], got %s" % (tuple(x.shape),))
    n, d = x.shape
    if _lib.query("cgcn_tsne_workspace_bytes", n=n) == 0:
        raise RuntimeError("chromegcn_amd: t-SNE: unsupported shape (n = %d; 2 <= n and n * n < 2^31)" % n)
    x = ops._dense(x.detach())
    D = _square(n, x.device)
    _lib.call("cgcn_tsne_sqdist", n=n, d=d, ld=_pitch(n), X=x, D=D)
    return D


def affinities(D: torch.Tensor, perplexity: float):
    """(C [n, n] fp32, beta [n] fp64): the conditional probabilities of the perplexity search (cgcn_tsne_affinities)"""
    n = _check_square(D, "D")
    C = _square(n, D.device)
    beta = torch.empty(n, device=D.device, dtype=torch.float64)
    _lib.call("cgcn_tsne_affinities", n=n, ld=_pitch(n), D=D, perplexity=float(perplexity), C=C, beta=beta)
    return C, beta


def symmetrize(C: torch.Tensor, ws: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """P = max((C + C^T) / sum, eps) with a zero diagonal (cgcn_tsne_symmetrize); out may be C itself"""
    n = _check_square(C, "C")
    P = _square(n, C.device) if out is None else out
    _check_square(P, "out")
    ws = workspace(n, C.device) if ws is None else ws
    _lib.call("cgcn_tsne_symmetrize", n=n, ld=_pitch(n), C=C, P=P, workspace=ws, workspace_bytes=ws.numel())
    return P


def _check_state(n: int, **tensors):
    """the optimiser's [n, 2] arrays: float32, on the device, contiguous"""
    for name, t in tensors.items():
        ops._require_cuda(t, name)
        if tuple(t.shape) != (n, 2) or not t.is_contiguous():
            raise ValueError("chromegcn_amd.tsne: %s must be a contiguous [n, 2] = [%d, 2] tensor, got %s" % (name, n, tuple(t.shape)))


def _check_workspace(ws: torch.Tensor):
    if not ws.is_cuda or ws.dtype != torch.uint8 or not ws.is_contiguous():
        raise ValueError("chromegcn_amd.tsne: the workspace must be a contiguous uint8 tensor on the device (tsne.workspace)")


def kl_gradient(P: torch.Tensor, Y: torch.Tensor, exaggeration: float, grad: torch.Tensor, want_kl: bool, ws: torch.Tensor):
    """one evaluation of the objective's gradient into grad [n, 2]; Z and the KL row partials stay in ws (cgcn_tsne_gradient)"""
    n = _check_square(P, "P")
    _check_state(n, Y=Y, grad=grad)
    _check_workspace(ws)
    _gradient_call(n, P, Y, exaggeration, grad, want_kl, ws)


def _gradient_call(n, P, Y, exaggeration, grad, want_kl, ws):
    """cgcn_tsne_gradient on arguments already checked (tsne_embed's loop checks its own buffers once)"""
    _lib.call("cgcn_tsne_gradient", n=n, ld=_pitch(n), P=P, Y=Y, exaggeration=float(exaggeration), grad=grad,
              want_kl=int(bool(want_kl)), workspace=ws, workspace_bytes=ws.numel())


def update_step(Y, update, gains, grad, momentum: float, learning_rate: float, have_kl: bool, record, ws):
    """one optimiser step on Y / update / gains; record (fp64 [4]) = {KL, |gains * grad|, Z, 0} (cgcn_tsne_update)"""
    ops._require_cuda(Y, "Y")
    n = Y.shape[0]
    _check_state(n, Y=Y, update=update, gains=gains, grad=grad)
    _check_workspace(ws)
    if not record.is_cuda or record.dtype != torch.float64 or record.numel() < 4 or not record.is_contiguous():
        raise ValueError("chromegcn_amd.tsne: record must be a contiguous float64 [4] tensor on the device")
    _update_call(n, Y, update, gains, grad, momentum, learning_rate, have_kl, record, ws)


def _update_call(n, Y, update, gains, grad, momentum, learning_rate, have_kl, record, ws):
    """cgcn_tsne_update on arguments already checked"""
    _lib.call("cgcn_tsne_update", n=n, Y=Y, update=update, gains=gains, grad=grad, momentum=float(momentum),
              learning_rate=float(learning_rate), have_kl=int(bool(have_kl)), record=record, workspace=ws,
              workspace_bytes=ws.numel())


def _check_perplexity(perplexity: float, n: int):
    if not perplexity > 0:
        raise ValueError("perplexity must be positive, got %r" % (perplexity,))
    if perplexity >= n:
        raise ValueError("perplexity must be less than n_samples (perplexity = %r, n = %d)" % (perplexity, n))


class TsneAffinities:
    """The squared distances of one point set z [n, d] (float32, on the device, d % 4 == 0), computed once;
    `.joint(perplexity)` builds the joint probabilities P [n, n] of one perplexity from them."""

    def __init__(self, z: torch.Tensor):
        self.D = sqdist(z)
        self.n = self.D.shape[0]
        self.ws = workspace(self.n, self.D.device)

    def joint(self, perplexity: float) -> torch.Tensor:
        _check_perplexity(perplexity, self.n)
        C, _ = affinities(self.D, perplexity)
        return symmetrize(C, self.ws, out=C)


def _learning_rate(learning_rate, n, early_exaggeration):
    if isinstance(learning_rate, str):
        if learning_rate != "auto":
            raise ValueError("learning_rate must be a number or 'auto', got %r" % learning_rate)
        return max(n / early_exaggeration / 4.0, 50.0)
    return float(learning_rate)


def _initial(init, n, seed):
    if init is None:
        return 1e-4 * np.random.RandomState(seed).standard_normal((n, 2)).astype(np.float32)
    return init


def _run_schedule(stage, max_iter, n_iter_without_progress, early_exaggeration):
    """TSNE._tsne's two calls of _gradient_descent; stage(it, max_iter, momentum, patience, exaggeration) -> (error, it)"""
    explore = min(EXPLORATION_ITER, max_iter)
    error, it = stage(0, explore, 0.5, EXPLORATION_ITER, early_exaggeration)
    if it + 1 < max_iter:
        error, it = stage(it + 1, max_iter, 0.8, n_iter_without_progress, 1.0)
    return error, it


def _descent_loop(evaluate, it, max_iter, patience, min_grad_norm, checks):
    """_gradient_descent's control flow; evaluate(want_error) does one step and returns (error, |grad|) when asked"""
    error = best_error = _FMAX
    best_iter = i = it
    for i in range(it, max_iter):
        check = (i + 1) % N_ITER_CHECK == 0
        want = check or i == max_iter - 1
        res = evaluate(want)
        if want:
            error, grad_norm = res
        if check:
            checks.append((i + 1, error))
            if error < best_error:
                best_error, best_iter = error, i
            elif i - best_iter > patience:
                break
            if grad_norm <= min_grad_norm:
                break
    return error, i


def tsne_embed(z_or_affinities: Union[torch.Tensor, TsneAffinities], perplexity: float = 30.0, max_iter: int = 1000,
               n_iter_without_progress: int = 300, early_exaggeration: float = 12.0, learning_rate="auto",
               min_grad_norm: float = 1e-7, init=None, seed: int = 0):
    """(Y [n, 2] float32 on the device, info): scikit-learn's TSNE(method='exact', n_components=2) of z [n, d].
    z_or_affinities: the points, or a TsneAffinities of them (shared between perplexities).  init: None draws
    1e-4 * RandomState(seed).standard_normal((n, 2)) as float32 (scikit-learn's init='random'); an array or tensor [n, 2] is
    taken as it is.  learning_rate 'auto' is max(n / early_exaggeration / 4, 50).
    info: 'kl_divergence' (the last one computed), 'n_iter' (the index of the last iteration, scikit-learn's n_iter_),
    'checks' ([(iterations done, KL)] of every convergence check), 'learning_rate'."""
    if not isinstance(z_or_affinities, TsneAffinities):
        ops._require_cuda(z_or_affinities, "z")
        _check_perplexity(perplexity, z_or_affinities.shape[0])         # before anything is launched
    aff = z_or_affinities if isinstance(z_or_affinities, TsneAffinities) else TsneAffinities(z_or_affinities)
    n, dev = aff.n, aff.D.device
    lr = _learning_rate(learning_rate, n, early_exaggeration)
    y0 = torch.as_tensor(_initial(init, n, seed))
    if tuple(y0.shape) != (n, 2):
        raise ValueError("init must be [n, 2] = [%d, 2], got %s" % (n, tuple(y0.shape)))
    Y = y0.to(device=dev, dtype=torch.float32).clone().contiguous()
    P = aff.joint(perplexity)
    update, gains, grad = torch.empty_like(Y), torch.empty_like(Y), torch.empty_like(Y)
    record = torch.zeros(4, device=dev, dtype=torch.float64)
    checks = []

    def stage(it, stop, momentum, patience, exaggeration):
        update.zero_()
        gains.fill_(1.0)

        def evaluate(want):
            _gradient_call(n, P, Y, exaggeration, grad, want, aff.ws)
            _update_call(n, Y, update, gains, grad, momentum, lr, want, record, aff.ws)
            if want:
                rec = record.tolist()                      # the one device-to-host read of a check
                return rec[0], rec[1]
        return _descent_loop(evaluate, it, stop, patience, min_grad_norm, checks)

    error, it = _run_schedule(stage, int(max_iter), n_iter_without_progress, early_exaggeration)
    return Y, {"kl_divergence": error, "n_iter": it, "checks": checks, "learning_rate": lr}


def tsne_sweep(z: Union[torch.Tensor, TsneAffinities], perplexities: Iterable[float], **kw):
    """[(Y, info)] of tsne_embed for every perplexity, over one distance matrix (the reference's thirteen runs, 5 ... 65)"""
    aff = z if isinstance(z, TsneAffinities) else TsneAffinities(z)
    return [tsne_embed(aff, perplexity=p, **kw) for p in perplexities]


# ------------------------------------------------------------------------------------------------------------------
# host restatements
# ------------------------------------------------------------------------------------------------------------------
def sqdist_host(x) -> np.ndarray:
    """float64 squared distances of the rows of x, in the difference form"""
    x = np.asarray(x, np.float64)
    D = np.empty((len(x), len(x)))
    for i in range(len(x)):
        D[i] = ((x[i] - x) ** 2).sum(1)
    return D


def conditional_probabilities_host(D, perplexity: float):
    """scikit-learn's _binary_search_perplexity on the fp32 distances D [n, n], in float64.
    Returns (C [n, n], beta [n], margin [n]): the conditional rows (zero diagonal), the last evaluated beta of every row and
    the smallest | |H - log perplexity| - 1e-5 | over the row's steps -- how far the row ever was from stopping one step
    earlier or later."""
    D = np.asarray(D, np.float32).astype(np.float64)
    n = len(D)
    log_perp = np.log(float(np.float32(perplexity)))
    beta, lo, hi = np.ones(n), np.full(n, -np.inf), np.full(n, np.inf)
    used, total, margin = np.ones(n), np.ones(n), np.full(n, np.inf)
    active = np.arange(n)
    for _ in range(100):
        d, b = D[active], beta[active]
        e = np.exp(-d * b[:, None])
        e[np.arange(len(active)), active] = 0.0
        s0 = e.sum(1)
        s0[s0 == 0.0] = 1e-8
        diff = np.log(s0) + b * ((d * e).sum(1) / s0) - log_perp
        used[active], total[active] = b, s0
        margin[active] = np.minimum(margin[active], np.abs(np.abs(diff) - PERPLEXITY_TOLERANCE))
        up = diff > 0.0
        lo[active[up]] = b[up]
        hi[active[~up]] = b[~up]
        nb = np.where(up, np.where(np.isinf(hi[active]), b * 2.0, (b + hi[active]) / 2.0),
                      np.where(np.isinf(lo[active]), b / 2.0, (b + lo[active]) / 2.0))
        beta[active] = nb
        active = active[np.abs(diff) > PERPLEXITY_TOLERANCE]
        if not len(active):
            break
    C = np.exp(-D * used[:, None]) / total[:, None]
    np.fill_diagonal(C, 0.0)
    return C, used, margin


def joint_probabilities_host(D, perplexity: float, return_info: bool = False):
    """scikit-learn's _joint_probabilities as a full matrix: P = max((C + C^T) / sum (C + C^T), eps) [n, n] float64 with a
    zero diagonal (scikit-learn's condensed form is squareform(P)).  D: squared distances, read as fp32.
    return_info: also {'beta', 'margin', 'conditional'} of conditional_probabilities_host."""
    C, beta, margin = conditional_probabilities_host(D, perplexity)
    P = C + C.T
    P = np.maximum(P / np.maximum(P.sum(), EPS), EPS)
    np.fill_diagonal(P, 0.0)
    return (P, {"beta": beta, "margin": margin, "conditional": C}) if return_info else P


def kl_gradient_host(P, Y, exaggeration: float = 1.0, dtype=np.float64, block: int = 1024):
    """scikit-learn's _kl_divergence at one degree of freedom on the full matrix: (KL, grad [n, 2], Z), everything in
    `dtype`.  P [n, n] (zero diagonal) is multiplied by `exaggeration` first, as TSNE._tsne does before it calls it."""
    dt = np.dtype(dtype).type
    P, Y = np.asarray(P), np.asarray(Y, dtype)
    n = len(Y)
    eps, e = dt(EPS), dt(exaggeration)

    def weights(r0, r1):
        dx = Y[r0:r1, None, 0] - Y[None, :, 0]
        dy = Y[r0:r1, None, 1] - Y[None, :, 1]
        w = dt(1) / (dt(1) + dx * dx + dy * dy)
        w[np.arange(r1 - r0), np.arange(r0, r1)] = 0
        return w, dx, dy

    Z = dt(0)
    for r0 in range(0, n, block):
        Z += weights(r0, min(n, r0 + block))[0].sum(dtype=dtype)
    kl, grad = dt(0), np.empty((n, 2), dtype)
    for r0 in range(0, n, block):
        r1 = min(n, r0 + block)
        w, dx, dy = weights(r0, r1)
        ep = P[r0:r1].astype(dtype) * e
        q = np.maximum(w / Z, eps)
        m = (ep - q) * w
        grad[r0:r1, 0] = dt(4) * (m * dx).sum(1, dtype=dtype)
        grad[r0:r1, 1] = dt(4) * (m * dy).sum(1, dtype=dtype)
        kl += (ep * np.log(np.maximum(ep, eps) / q)).sum(dtype=dtype)
    return kl, grad, Z


def tsne_embed_host(P, Y0, max_iter: int = 1000, n_iter_without_progress: int = 300, early_exaggeration: float = 12.0,
                    learning_rate="auto", min_grad_norm: float = 1e-7, dtype: str = "float64"):
    """tsne_embed's schedule in numpy from the joint probabilities P [n, n] and the start Y0 [n, 2]: (Y, info).
    dtype: 'float64' or 'float32' (state and objective alike), or 'mixed' -- scikit-learn's own arrangement, an fp32 state
    with the objective evaluated in float64.  info as tsne_embed's, and the final 'update' and 'gains'."""
    if dtype not in ("float64", "float32", "mixed"):
        raise ValueError("dtype must be 'float64', 'float32' or 'mixed', got %r" % (dtype,))
    st = np.float32 if dtype in ("float32", "mixed") else np.float64
    ob = np.float32 if dtype == "float32" else np.float64
    Y = np.array(Y0, dtype=st)
    n = len(Y)
    lr = st(_learning_rate(learning_rate, n, early_exaggeration))
    state = {"update": np.zeros_like(Y), "gains": np.ones_like(Y)}
    checks = []

    def stage(it, stop, momentum, patience, exaggeration):
        state["update"], state["gains"] = np.zeros_like(Y), np.ones_like(Y)

        def evaluate(want):
            kl, grad, _ = kl_gradient_host(P, Y, exaggeration, ob)
            grad = grad.astype(st)
            update, gains = state["update"], state["gains"]
            inc = update * grad < 0.0
            gains[inc] += st(0.2)
            gains[~inc] *= st(0.8)
            np.clip(gains, st(0.01), np.inf, out=gains)
            grad *= gains
            state["update"] = update = st(momentum) * update - lr * grad
            Y[...] += update
            if want:
                return float(kl), float(np.linalg.norm(grad))
        return _descent_loop(evaluate, it, stop, patience, min_grad_norm, checks)

    error, it = _run_schedule(stage, int(max_iter), n_iter_without_progress, early_exaggeration)
    return Y, {"kl_divergence": error, "n_iter": it, "checks": checks, "learning_rate": float(lr), "update": state["update"],
               "gains": state["gains"]}
