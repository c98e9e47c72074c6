"""Random contact graphs that keep what a top-K Hi-C graph trivially encodes, and the null-graph test built on them.

The reference advertises the control (`-adj_type random`, config_args.py:45) and dies on it (process_graph has no branch
for it: UnboundLocalError).  Here the null graph stands in for the Hi-C MATRIX -- it is not a normaliser branch, and
`adj_type="random"` keeps raising ValueError -- so that 'hic' and 'both' normalise it like the real one.

This docstring is the specification; `null_graph_host` restates it in numpy and the kernels of csrc/cgcn_nullgraph.hip
are held to that restatement bit for bit (tests/test_gpu_nullgraph.py), as tests/dropout_ref.py does for the dropout
mask.  All arithmetic is integer.

INPUT.  A CSR on N windows; values are ignored.  The edges are the stored entries (i, j) with j > i, numbered
e = 0 .. m-1 in storage order (row by row, within a row in the stored order).  The diagonal and the lower triangle are
ignored, so a raw {0,1} matrix from `HicContacts.build_raw` and the (rowptr, col) of a normalised 'hic' ChromGraph give the
same edges.  Distance means |j - i| in WINDOW INDICES, not base pairs: windows that were dropped from the chromosome do
not count.

DRAWS.  The hash family of the dropout mask (mix32 and the dropout_key mixing of csrc/cgcn_common.hpp), restated here:
    mix32(x):  x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16      (mod 2^32)
    key(seed, attempt, stream) = dropout_key with the step counter replaced by `attempt`:
        k = mix32(lo32(seed) ^ 0x9E3779B9); k = mix32(k ^ hi32(seed)); k = mix32(k + lo32(attempt) * 0x85EBCA6B);
        k = mix32(k ^ hi32(attempt) ^ (stream * 0xC2B2AE35))
    draw(t, attempt, stream, R) = (mix32(t * 0x9E3779B1 + key(seed, attempt, stream)) * R) >> 32
an integer in [0, R) formed as a 64-bit product (R < 2^32).  seed is 64 bits (taken mod 2^64) and both halves matter.

PLACEMENT WITH RETRIES ('distance' and 'uniform').  Every token t has a class and a number of slots.  All tokens start
with attempt 0 at the position their draw gives.  One round evaluates all tokens: among the tokens with the same
(class, position) the smallest token index keeps its place (a token that won earlier can lose to a smaller index that
moved in); every other token is a loser of the round.  After each round but the last, every loser increments its attempt
and redraws.  There are `rounds` rounds (default 16); the losers of the last one are UNPLACED and take no part in the
result.  A round without losers changes nothing, and neither does any round after it.  info['rounds_used'] is
min(rounds, 1 + number of rounds that had losers).

model='distance' (stream 1).  c_d = number of edges with j - i = d, n_d = N - d slots (d = 1 .. N-1).  Class d is
COMPLEMENTED iff 2 c_d > n_d: it contributes k_d = n_d - c_d tokens (its holes) instead of c_d.  Tokens are numbered in
ascending d.  In a plain class every placed token at p gives the edge (p, p + d); in a complemented class every p in
[0, n_d) WITHOUT a placed token gives that edge (so an unplaced hole adds an edge).  With no unplaced token the distance
histogram is exactly the input's.  Without the complement the short distances of a Hi-C graph are close to full and the
retries do not converge.

model='uniform' (streams 3 and 4).  m tokens in one class; u = draw(t, a, 3, N), w = draw(t, a, 4, N - 1), w += 1 if
w >= u; the position is the pair (min(u, w), max(u, w)), which is the edge of a placed token.  Unsupported (ValueError) for
N < 2 or 4 m > N (N - 1) when m > 0.

model='degree' (stream 2): the erased configuration model, no retries.  Stub 2e belongs to i and stub 2e+1 to j of edge
e.  The stubs are sorted by (mix32(s * 0x9E3779B1 + key(seed, 0, 2)), s); the sorted stubs 2q and 2q+1 form pair q.  A
pair of one window with itself is a loop and dropped; of equal pairs one is kept (the others are repeats).  So every
window's degree is at most its input degree and the deficits sum to 2 (loops + repeats).

OUTPUT.  The canonical symmetric {0,1} CSR without a diagonal: int32 rowptr [N + 1] and sorted col -- the form
build_raw returns.  info: edges_in (m), edges_out, tokens (distance: sum k_d; uniform: m; degree: the 2m stubs),
unplaced, complemented_classes, loops, repeats, rounds_used.
"""
from __future__ import annotations

from typing import Dict, NamedTuple, Optional

import numpy as np
import scipy.sparse as sp

MODELS = {"distance": 0, "degree": 1, "uniform": 2}   # CGCN_NULL_* in include/chromegcn.h
STREAM_DISTANCE, STREAM_DEGREE, STREAM_UNIFORM_U, STREAM_UNIFORM_W = 1, 2, 3, 4
DEFAULT_ROUNDS = 16
INFO_KEYS = ("edges_in", "edges_out", "tokens", "unplaced", "complemented_classes", "loops", "repeats", "rounds_used")

_M32 = np.uint64(0xFFFFFFFF)


# ----------------------------------------------------------------------------------------------------------------------
# the rule, on the host (numpy / scipy only)
# ----------------------------------------------------------------------------------------------------------------------
def mix32(x):
    x = np.asarray(x, np.uint64) & _M32
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & _M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & _M32
    return x ^ (x >> np.uint64(16))


def key(seed: int, attempt: int, stream: int) -> int:
    seed, attempt = int(seed) & 0xFFFFFFFFFFFFFFFF, int(attempt) & 0xFFFFFFFFFFFFFFFF
    k = int(mix32((seed & 0xFFFFFFFF) ^ 0x9E3779B9))
    k = int(mix32(k ^ (seed >> 32)))
    k = int(mix32((k + (attempt & 0xFFFFFFFF) * 0x85EBCA6B) & 0xFFFFFFFF))
    return int(mix32(k ^ (attempt >> 32) ^ ((int(stream) * 0xC2B2AE35) & 0xFFFFFFFF)))


def draw(t, seed: int, attempt: int, stream: int, R):
    """draw(t, attempt, stream, R) of the module docstring for arrays t and R (or a scalar R)"""
    r = mix32((np.asarray(t, np.uint64) * np.uint64(0x9E3779B1) + np.uint64(key(seed, attempt, stream))) & _M32)
    return ((r * np.asarray(R, np.uint64)) >> np.uint64(32)).astype(np.int64)


def upper_edges(graph):
    """(N, i, j): the edges of the input in storage order (int64 arrays)"""
    n, rowptr, col = _host_csr(graph)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr))
    col = col[:rowptr[-1]].astype(np.int64)
    keep = col > rows
    return n, rows[keep], col[keep]


def _host_csr(graph):
    if sp.issparse(graph):
        a = graph if sp.isspmatrix_csr(graph) else sp.csr_matrix(graph)
        if a.shape[0] != a.shape[1]:
            raise ValueError("the graph must be square, got %s" % (a.shape,))
        return int(a.shape[0]), np.asarray(a.indptr, np.int64), np.asarray(a.indices, np.int64)
    if hasattr(graph, "rowptr") and hasattr(graph, "col"):   # HostCSR, or a ChromGraph (read back)
        rp, ci = graph.rowptr, graph.col
    elif isinstance(graph, (tuple, list)) and len(graph) == 2:
        rp, ci = graph
    else:
        raise TypeError("graph must be a scipy matrix, a HostCSR, a ChromGraph or a (rowptr, col) pair")
    if hasattr(rp, "detach"):
        rp, ci = rp.detach().cpu().numpy(), ci.detach().cpu().numpy()
    rp = np.asarray(rp, np.int64)
    return int(rp.size) - 1, rp, np.asarray(ci, np.int64)


def _place(T: int, pos_shape, code, slots_of, rounds: int):
    """Placement with retries of T tokens.  slots_of(sel, attempt) -> the positions (each of shape pos_shape) of the tokens
    `sel` at `attempt`; code(pos) -> one integer per token that is equal for equal (class, position).  Returns
    (pos, placed mask, rounds_used, unplaced)."""
    att = np.zeros(T, np.int64)
    pos = np.zeros((T,) + tuple(pos_shape), np.int64)
    todo = np.arange(T)
    placed = np.ones(T, bool)
    with_losers = 0
    for r in range(rounds):
        for a in np.unique(att[todo]):
            sel = todo[att[todo] == a]
            pos[sel] = slots_of(sel, int(a))
        k = code(pos)
        order = np.lexsort((np.arange(T), k))
        ks = k[order]
        first = np.ones(T, bool)
        first[1:] = ks[1:] != ks[:-1]
        losers = order[~first]
        if losers.size == 0:
            break
        with_losers += 1
        if r + 1 < rounds:
            att[losers] += 1
            todo = losers
        else:
            placed[losers] = False
    return pos, placed, min(rounds, 1 + with_losers), int((~placed).sum())


def _distance(n, i, j, seed, rounds, info):
    d = j - i
    cd = np.bincount(d, minlength=max(n, 1)).astype(np.int64)[:max(n, 1)]
    nd = n - np.arange(max(n, 1), dtype=np.int64)
    nd[0] = 0
    cd = np.minimum(cd, nd)   # (more than n_d only for an input with repeated entries, which is no canonical CSR)
    comp = 2 * cd > nd
    kd = np.where(comp, nd - cd, cd)
    cls = np.repeat(np.arange(kd.size, dtype=np.int64), kd)
    slots = nd[cls]
    pos, placed, used, unplaced = _place(cls.size, (), lambda pos: cls * np.int64(max(n, 1)) + pos,
                                         lambda sel, a: draw(sel, seed, a, STREAM_DISTANCE, slots[sel]), rounds)
    lo, hi = [], []
    plain = placed & ~comp[cls]
    lo.append(pos[plain])
    hi.append(pos[plain] + cls[plain])
    for dd in np.flatnonzero(comp):
        free = np.ones(nd[dd], bool)
        sel = placed & (cls == dd)
        free[pos[sel]] = False
        p = np.flatnonzero(free)
        lo.append(p)
        hi.append(p + dd)
    info.update(tokens=int(cls.size), unplaced=unplaced, complemented_classes=int(comp.sum()), rounds_used=used)
    return np.concatenate(lo), np.concatenate(hi)


def _uniform(n, i, j, seed, rounds, info):
    m = int(i.size)
    if m and (n < 2 or 4 * m > n * (n - 1)):
        raise ValueError("model 'uniform' is unsupported for N = %d with %d edges (needs N >= 2 and 4 m <= N (N - 1))" % (n, m))

    def slots_of(sel, a):
        u = draw(sel, seed, a, STREAM_UNIFORM_U, n)
        w = draw(sel, seed, a, STREAM_UNIFORM_W, n - 1)
        w = w + (w >= u)
        return np.stack([np.minimum(u, w), np.maximum(u, w)], 1)

    pos, placed, used, unplaced = _place(m, (2,), lambda pos: pos[:, 0] * np.int64(max(n, 1)) + pos[:, 1], slots_of, rounds)
    info.update(tokens=m, unplaced=unplaced, rounds_used=used)
    return pos[placed, 0], pos[placed, 1]


def _degree(n, i, j, seed, info):
    m = int(i.size)
    node = np.empty(2 * m, np.int64)
    node[0::2], node[1::2] = i, j
    s = np.arange(2 * m, dtype=np.int64)
    h = mix32((s.astype(np.uint64) * np.uint64(0x9E3779B1) + np.uint64(key(seed, 0, STREAM_DEGREE))) & _M32)
    order = np.lexsort((s, h))
    u, v = node[order[0::2]], node[order[1::2]]
    lo, hi = np.minimum(u, v), np.maximum(u, v)
    ok = lo != hi
    pairs = np.unique(lo[ok] * np.int64(max(n, 1)) + hi[ok])
    info.update(tokens=2 * m, loops=int((~ok).sum()), repeats=int(ok.sum() - pairs.size), rounds_used=0)
    return pairs // max(n, 1), pairs % max(n, 1)


def null_graph_host(graph, model: str = "distance", seed: int = 0, rounds: int = DEFAULT_ROUNDS, return_info: bool = False):
    """The null graph of `graph` (module docstring) as a canonical float64 scipy CSR of ones; with return_info, (matrix, info).
    graph: a scipy matrix, a HostCSR, a ChromGraph or a (rowptr, col) pair.  Pure numpy / scipy."""
    if model not in MODELS:
        raise ValueError("unknown null model %r (one of %s)" % (model, ", ".join(MODELS)))
    rounds = int(rounds)
    if rounds < 1:
        raise ValueError("rounds must be at least 1")
    n, i, j = upper_edges(graph)
    if np.any(j >= n):
        raise ValueError("column index outside the matrix")
    info = dict.fromkeys(INFO_KEYS, 0)
    info["edges_in"] = int(i.size)
    if model == "distance":
        lo, hi = _distance(n, i, j, seed, rounds, info)
    elif model == "uniform":
        lo, hi = _uniform(n, i, j, seed, rounds, info)
    else:
        lo, hi = _degree(n, i, j, seed, info)
    info["edges_out"] = int(lo.size)
    a = sp.coo_matrix((np.ones(2 * lo.size), (np.concatenate([lo, hi]), np.concatenate([hi, lo]))), shape=(n, n)).tocsr()
    a.sum_duplicates()
    a.sort_indices()
    if a.nnz != 2 * lo.size:
        raise AssertionError("null_graph_host produced a repeated edge")   # the rule cannot: a bug in this file
    a.indptr = a.indptr.astype(np.int32)
    a.indices = a.indices.astype(np.int32)
    return (a, info) if return_info else a


# ----------------------------------------------------------------------------------------------------------------------
# the statistics of the test, on the host (numpy only)
# ----------------------------------------------------------------------------------------------------------------------
def null_statistics(observed, null) -> Dict[str, np.ndarray]:
    """observed [C], null [R, C] -> {'null_mean', 'null_std', 'z', 'p'}, each [C] float64.
    null_std is the population standard deviation (ddof = 0) of the replicates; z = (observed - null_mean) / null_std,
    NaN where null_std is 0; p = (1 + #{null >= observed}) / (R + 1), the one-sided permutation p-value that counts the
    observed graph among its own nulls.  A NaN metric (a label without positives) gives NaN mean, std and z; its
    comparisons are all false, so p is 1 / (R + 1) there -- read p only where observed is finite."""
    observed = np.asarray(observed, np.float64)
    null = np.asarray(null, np.float64)
    if null.ndim != 2 or observed.shape != null.shape[1:]:
        raise ValueError("observed must be [C] and null [R, C]")
    R = null.shape[0]
    if R < 1:
        raise ValueError("at least one replicate is needed")
    mean = null.mean(0)
    std = null.std(0)
    with np.errstate(divide="ignore", invalid="ignore"):
        z = np.where(std > 0, (observed - mean) / np.where(std > 0, std, 1.0), np.nan)
    z = np.where(np.isnan(mean) | np.isnan(observed), np.nan, z)
    p = (1.0 + (null >= observed[None, :]).sum(0)) / (R + 1.0)
    return {"null_mean": mean, "null_std": std, "z": z, "p": p}


class NullGraphTest(NamedTuple):
    """Per metric of multilabel_metrics, [C] float64 arrays; null: {metric: [n_null, C]} with keep_null, else None."""
    observed: Dict[str, np.ndarray]
    null_mean: Dict[str, np.ndarray]
    null_std: Dict[str, np.ndarray]
    z: Dict[str, np.ndarray]
    p: Dict[str, np.ndarray]
    null: Optional[Dict[str, np.ndarray]]
    null_model: str
    n_null: int
    seed: int


# ----------------------------------------------------------------------------------------------------------------------
# the device side
# ----------------------------------------------------------------------------------------------------------------------
SIZES_LEN = 10   # int64: nnz, the eight INFO_KEYS counters (rounds_used raw: rounds that had losers), flags
FLAG_OVERRUN, FLAG_UNSUPPORTED, FLAG_BAD_INDEX = 1, 2, 4


def replicate_seed(seed: int, r: int, c: int, K: int) -> int:
    """the seed of replicate r of chromosome index c out of K"""
    return (int(seed) + int(r) * int(K) + int(c)) & 0xFFFFFFFFFFFFFFFF


def _device_input(graph, dev):
    """(n, rowptr, col, nnz bound, m or None) on the device; m is known when the graph came from the host"""
    import torch
    if isinstance(graph, (tuple, list)) and len(graph) == 2 and torch.is_tensor(graph[0]):
        rp, ci = graph
        if rp.dtype != torch.int32 or ci.dtype != torch.int32 or not rp.is_cuda or not ci.is_cuda:
            raise ValueError("a (rowptr, col) pair must be int32 tensors on the GPU")
        return int(rp.numel()) - 1, rp.contiguous(), ci.contiguous(), int(ci.numel()), None
    if hasattr(graph, "rowptr_t") and torch.is_tensor(graph.rowptr):   # ChromGraph
        return int(graph.n), graph.rowptr.contiguous(), graph.col.contiguous(), int(graph.col.numel()), None
    n, rp, ci = _host_csr(graph)
    nnz = int(rp[-1]) if rp.size else 0
    if nnz >= 2 ** 31 or n >= 2 ** 31 - 1:
        raise ValueError("graph too large for int32 CSR")
    if np.any(ci[:nnz] < 0) or np.any(ci[:nnz] >= n):
        raise ValueError("column index outside the matrix")
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    m = int(np.count_nonzero(ci[:nnz] > rows))
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(dev)
    return n, up(rp), up(ci[:nnz]), nnz, m


def info_from_sizes(sizes, rounds: int, model: str) -> Dict[str, int]:
    """the info dict from the device's counters (one read-back); raises what the host restatement raises"""
    v = [int(x) for x in sizes.tolist()]
    flags = v[9]
    if flags & FLAG_BAD_INDEX:
        raise ValueError("column index outside the matrix")
    if flags & FLAG_UNSUPPORTED:
        raise ValueError("model 'uniform' is unsupported for this graph (needs N >= 2 and 4 m <= N (N - 1))")
    if flags & FLAG_OVERRUN:
        raise RuntimeError("chromegcn_amd.nullgraph: the output capacity was too small")
    info = dict(zip(INFO_KEYS, v[1:9]))
    info["rounds_used"] = 0 if model == "degree" else min(int(rounds), 1 + info["rounds_used"])
    return info


def null_graph(graph, model: str = "distance", seed: int = 0, rounds: int = DEFAULT_ROUNDS, device="cuda",
               return_info: bool = False):
    """null_graph_host on the device (cgcn_null_graph): (rowptr int32 [N + 1], col int32 [>= nnz], sizes int64 [10]) on
    the device, enqueued on the current stream; sizes[0] is nnz.  graph: a scipy matrix or HostCSR (uploaded), a ChromGraph,
    or a (rowptr, col) pair of int32 device tensors (col may be longer than rowptr[N]).  With return_info,
    (rowptr, col, sizes, info) -- reading info is the only host synchronisation, and what raises for a device input that
    'uniform' does not support or that holds a column outside the matrix (a host input raises before anything is launched)."""
    import torch
    from . import _lib
    if model not in MODELS:
        raise ValueError("unknown null model %r (one of %s)" % (model, ", ".join(MODELS)))
    rounds = int(rounds)
    if rounds < 1:
        raise ValueError("rounds must be at least 1")
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("null_graph needs a GPU; null_graph_host is the host restatement")
    n, rp, ci, nnz, m = _device_input(graph, dev)
    if n < 0:
        raise ValueError("rowptr must have N + 1 entries")
    bound = nnz if m is None else m   # an upper bound of the edge count
    if model == "uniform" and m and (n < 2 or 4 * m > n * (n - 1)):
        raise ValueError("model 'uniform' is unsupported for N = %d with %d edges (needs N >= 2 and 4 m <= N (N - 1))" % (n, m))
    # distance: an unplaced hole of a complemented class ADDS an edge; such a class has n_d < 2 c_d, so edges_out < 2 m
    capacity = max(1, (4 if model == "distance" else 2) * bound)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    with torch.cuda.device(dev):
        rowptr = torch.empty(n + 1, dtype=torch.int32, device=dev)
        col = torch.empty(capacity, dtype=torch.int32, device=dev)
        sizes = torch.empty(SIZES_LEN, dtype=torch.int64, device=dev)
        wsp, need = _lib.workspace_for("cgcn_null_graph_workspace_bytes", dev, "null graph N=%d nnz=%d" % (n, nnz),
                                       n=n, nnz=nnz, capacity=capacity, model=MODELS[model])
        _lib.call("cgcn_null_graph", n=n, nnz=nnz, rowptr=rp, col=ci, model=MODELS[model],
                  seed=seed - (1 << 64) if seed >= (1 << 63) else seed, rounds=rounds, capacity=capacity,
                  rowptr_out=rowptr, col_out=col, sizes=sizes, workspace=wsp, workspace_bytes=need)
    if return_info:
        return rowptr, col, sizes, info_from_sizes(sizes, rounds, model)
    return rowptr, col, sizes


def null_chrom_graph(graph, adj_type: str = "hic", model: str = "distance", seed: int = 0, rounds: int = DEFAULT_ROUNDS,
                     device="cuda"):
    """The ChromGraph of process_graph(adj_type, null graph of `graph`): null_graph, then normalize_device_csr -- equal to
    upload(normalize_graph(adj_type, null_graph_host(graph, ...), N)).  adj_type 'hic' or 'both'; 'both' needs the RAW
    matrix as `graph`, because the band is added after the randomisation."""
    from . import graph as G
    if adj_type not in ("hic", "both"):
        raise ValueError("a null graph stands in for the Hi-C matrix: adj_type must be 'hic' or 'both', got %r" % (adj_type,))
    rowptr, col, _ = null_graph(graph, model=model, seed=seed, rounds=rounds, device=device)
    return G.normalize_device_csr(adj_type, int(rowptr.numel()) - 1, rowptr, col, None, device)


def _as_list(x):
    return list(x) if isinstance(x, (list, tuple)) else [x]


METRICS = ("auroc", "aupr", "recall_at_fdr", "average_precision")   # metrics.multilabel_metrics, in its table's order


def strand_probs(model, x_fr, graph):
    """what an evaluation scores: the sigmoid of the strand mean of forward_strands' logits (finetune.py:44,52), [n, C]"""
    import torch
    logits, _ = model.forward_strands(x_fr, graph)
    return torch.sigmoid((logits[0] + logits[1]) * 0.5)


def _pooled_metrics(model, x_frs, graphs, target, nonneg):
    """the flat metric table of the pooled chromosomes ([4 C] and, nonneg, the `bad` word behind it), on the device"""
    import torch
    from . import metrics
    probs = [strand_probs(model, x_fr, g) for x_fr, g in zip(x_frs, graphs)]
    p = probs[0] if len(probs) == 1 else torch.cat(probs, 0)
    flat = metrics._metrics_raw(p, target, 0.5, nonneg=nonneg)
    return flat if nonneg else torch.cat([flat[:-1], flat.new_zeros(1)])


def null_graph_test(model, x_f, x_r, hic, targets, null_model: str = "distance", n_null: int = 100, seed: int = 0,
                    adj_type: str = "hic", keep_null: bool = False, rounds: int = DEFAULT_ROUNDS) -> NullGraphTest:
    """Does `model` gain anything from the Hi-C contacts being the real ones?  Its per-label metrics on the real graphs
    against their distribution over n_null null graphs.

    x_f, x_r: [n, d] features of the forward and the reverse-complement strand; hic: the raw contact matrix (anything
    null_graph takes); targets [n, C] -- one chromosome, or lists of them, pooled like an evaluation split (one metric
    call over the concatenated windows).  Replicate r of chromosome index c out of K uses replicate_seed(seed, r, c, K).
    The probabilities are strand_probs(model, ...), as in evaluation; the model runs in eval mode without autograd and its
    training flag is restored.  No matrix and no prediction visits the host: the graphs are uploaded once, every replicate is
    generated, normalised (normalize_device_csr, which reads back two scalars per graph), run and scored on the device, and
    the metric table [1 + n_null, 4, C] is read back once at the end."""
    import torch
    from . import graph as G
    x_fs, x_rs, hics, tgts = _as_list(x_f), _as_list(x_r), _as_list(hic), _as_list(targets)
    K = len(hics)
    if not (len(x_fs) == len(x_rs) == len(tgts) == K) or K < 1:
        raise ValueError("x_f, x_r, hic and targets must be one chromosome each or lists of one length")
    n_null = int(n_null)
    if n_null < 1:
        raise ValueError("n_null must be at least 1")
    if adj_type not in ("hic", "both"):
        raise ValueError("a null graph stands in for the Hi-C matrix: adj_type must be 'hic' or 'both', got %r" % (adj_type,))
    dev = x_fs[0].device
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            x_frs = [torch.stack([a, b], 0).float().contiguous() for a, b in zip(x_fs, x_rs)]
            tgts = [t.to(dev).float().contiguous() for t in tgts]
            target = tgts[0] if K == 1 else torch.cat(tgts, 0)
            C = int(target.shape[1])
            inputs = [_device_input(h, dev) for h in hics]   # uploaded once
            for n, _, _, _, m in inputs:
                if null_model == "uniform" and m and (n < 2 or 4 * m > n * (n - 1)):
                    raise ValueError("model 'uniform' is unsupported for N = %d with %d edges" % (n, m))
            pairs = [(rp, ci) for _, rp, ci, _, _ in inputs]
            real = [G.normalize_device_csr(adj_type, n, rp, ci, None, dev) for n, rp, ci, _, _ in inputs]

            def run(nonneg):
                table = torch.empty(n_null + 1, 4 * C + 1, dtype=torch.float32, device=dev)
                table[0] = _pooled_metrics(model, x_frs, real, target, nonneg)
                for r in range(n_null):
                    graphs = [null_chrom_graph(pairs[c], adj_type, null_model, replicate_seed(seed, r, c, K), rounds, dev)
                              for c in range(K)]
                    table[1 + r] = _pooled_metrics(model, x_frs, graphs, target, nonneg)
                return table.cpu()   # the one read-back

            table = run(True)
            if bool((table[:, 4 * C].view(torch.int32) != 0).any()):   # a negative or NaN score: the general metric path
                table = run(False)
            host = table[:, :4 * C].numpy().astype(np.float64).reshape(n_null + 1, 4, C)
    finally:
        model.train(was_training)
    out = {k: {} for k in ("observed", "null_mean", "null_std", "z", "p")}
    null = {}
    for q, name in enumerate(METRICS):
        obs, nl = host[0, q], host[1:, q]
        out["observed"][name] = obs
        for k, v in null_statistics(obs, nl).items():
            out[k][name] = v
        null[name] = nl
    return NullGraphTest(null=null if keep_null else None, null_model=null_model, n_null=n_null, seed=int(seed), **out)
