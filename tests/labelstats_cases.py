"""Case builders of the label-statistics tests (test_labelstats_host.py, test_gpu_labelstats.py): numpy / scipy only, nothing
here touches the GPU.  A case is (name, targets float32 [n, C], graph or None); the graph is a scipy sparse matrix (taken as
is), a HostCSR or None.  brute_force is the specification in plain Python loops over dense matrices."""
import functools

import numpy as np
import scipy.sparse as sp

from chromegcn_amd import graph as G
from chromegcn_amd.graph import HostCSR

CS = (1, 63, 64, 65, 103, 128, 129, 256)
NS = (1, 63, 64, 65, 257, 1000)


def bernoulli_targets(n, C, seed, rate=0.05):
    rng = np.random.RandomState(seed)
    return (rng.rand(n, C) < rate).astype(np.float32)


def random_symmetric(n, m, seed, diagonal=False):
    """a {0, 1} symmetric matrix of about 2 m off-diagonal entries, as a raw pickle entry: no diagonal unless asked for"""
    rng = np.random.RandomState(seed)
    if n < 2:
        return sp.csr_matrix((n, n), dtype=np.float64)
    r, c = rng.randint(0, n, m), rng.randint(0, n, m)
    keep = r != c
    a = sp.coo_matrix((np.ones(int(keep.sum())), (r[keep], c[keep])), shape=(n, n)).tocsr()
    a = a + a.T
    a.data[:] = 1.0
    if diagonal:
        a = a + sp.identity(n, format="csr")
    a = sp.csr_matrix(a)
    a.sort_indices()
    return a


def shape_cases():
    """every C of CS crossed with every n of NS: Bernoulli targets (denser for small shapes so that pairs occur), a raw symmetric
    matrix without a diagonal"""
    out = []
    for C in CS:
        for n in NS:
            t = bernoulli_targets(n, C, 17 * C + n, rate=0.3 if n * C < 4000 else 0.05)
            out.append(("shape_C%d_n%d" % (C, n), t, random_symmetric(n, 4 * n, C + 3 * n)))
    return out


def hub_graph(n=4000, hub=7, hub_len=3000, rows=((100, 64), (2000, 65))):
    """non-symmetric pattern: row `hub` holds hub_len entries (the long-row split over all waves, several rounds), two rows
    hold exactly 64 and 65 entries (one full batch; one full batch and one entry), every other row 0 .. 3"""
    rng = np.random.RandomState(5)
    rr, cc = [], []
    for u in range(n):
        k = hub_len if u == hub else dict(rows).get(u, int(rng.randint(0, 4)))
        cols = rng.choice(n - 1, k, replace=False)
        cols = cols + (cols >= u)                       # never the diagonal
        rr.append(np.full(k, u))
        cc.append(cols)
    a = sp.csr_matrix((np.ones(sum(len(c) for c in cc)), (np.concatenate(rr), np.concatenate(cc))), shape=(n, n))
    a.sort_indices()
    lens = np.diff(a.indptr)
    assert lens[hub] == hub_len and all(lens[u] == k for u, k in rows)
    return a


def valued_graph(n, seed):
    """explicit values with 0, 2, 0.5 and a negative one among them, a diagonal with values too: only val > 0 off the diagonal
    counts.  A HostCSR, so that the stored zeros survive."""
    a = random_symmetric(n, 5 * n, seed, diagonal=True)
    rng = np.random.RandomState(seed + 1)
    val = rng.choice(np.array([0.0, 1.0, 2.0, 0.5, -1.0], np.float32), a.nnz)
    assert {0.0, 2.0} <= set(val.tolist())
    return HostCSR(n=n, rowptr=a.indptr.astype(np.int32), col=a.indices.astype(np.int32), val=val, row_scale=None,
                   symmetric=False)


@functools.lru_cache(maxsize=None)
def special_cases():
    out = []
    n, C = 200, 103
    t = bernoulli_targets(n, C, 1)
    t[3] = 0                                            # a window with no label
    t[4] = 1                                            # windows with every label but the empty one (all C: the all_ones case)
    t[199] = 1
    t[:, 50] = 0                                        # a label with no window
    raw = random_symmetric(n, 900, 2)
    out.append(("no_graph", t, None))
    out.append(("identity_only", t, sp.identity(n, format="csr")))
    lil = raw.tolil()
    lil[10, :] = 0
    lil[:, 10] = 0
    lil[10, 10] = 1                                     # a row with no off-diagonal entry (its diagonal is stored)
    no_off = sp.csr_matrix(lil)
    no_off.eliminate_zeros()
    out.append(("row_without_offdiagonal", t, no_off))
    out.append(("raw_scipy", t, raw))
    for kind in ("hic", "both", "constant"):
        out.append(("normalize_" + kind, t, G.normalize_graph(kind, raw, n)))
    out.append(("explicit_values", t, valued_graph(n, 9)))
    rng = np.random.RandomState(4)
    asym = sp.csr_matrix((np.ones(700), (rng.randint(0, n, 700), rng.randint(0, n, 700))), shape=(n, n))
    asym.data[:] = 1.0                                  # duplicates were summed: back to a pattern
    asym.sort_indices()
    assert (abs(asym - asym.T)).nnz > 0
    out.append(("non_symmetric", t, asym))
    last = sp.csr_matrix((np.ones(60), (np.full(60, n - 1), np.arange(60) * 3)), shape=(n, n))
    out.append(("all_in_last_row", t, last))
    ones = np.ones((70, 65), np.float32)                # contact_pairs[a, b] == n_entries for every pair
    out.append(("all_ones", ones, random_symmetric(70, 300, 6)))
    odd = bernoulli_targets(130, 129, 8, rate=0.1)
    pos = odd != 0
    odd[pos] = np.resize(np.array([0.5, -1.0, np.nan, 1.0, 1e-40], np.float32), int(pos.sum()))   # all count as positive
    odd[~pos] = np.resize(np.array([0.0, -0.0], np.float32), int((~pos).sum()))
    out.append(("raw_values", odd, random_symmetric(130, 600, 10)))
    t4 = bernoulli_targets(4000, 103, 11)
    t4[7, :40] = 1                                      # the hub row carries labels of two tiles
    out.append(("hub_rows", t4, hub_graph()))
    return out


@functools.lru_cache(maxsize=None)
def all_cases():
    return shape_cases() + list(special_cases())


def workload_case():
    """the workload's shape: n = 5776, C = 103, 500 000 stored entries"""
    n = 5776
    rng = np.random.RandomState(21)
    keys = rng.choice(n * n, 500000, replace=False)
    a = sp.csr_matrix((np.ones(keys.size), (keys // n, keys % n)), shape=(n, n))
    a.sort_indices()
    assert a.nnz == 500000
    return bernoulli_targets(n, 103, 22), a


def neighbour_entries(graph):
    """[(u, v), ...]: the neighbour entries the graph stores (u != v; val > 0 where it has values), one per stored entry"""
    if isinstance(graph, HostCSR):
        rowptr, col, val = graph.rowptr, graph.col, graph.val
    else:
        a = sp.csr_matrix(graph)
        rowptr, col, val = a.indptr, a.indices, a.data
    out = []
    for u in range(len(rowptr) - 1):
        for p in range(rowptr[u], rowptr[u + 1]):
            v = int(col[p])
            if v != u and (val is None or val[p] > 0):
                out.append((u, v))
    return out


def brute_force(targets, graph):
    """the definitions, literally: dict of int64 arrays"""
    n, C = targets.shape
    pos = targets != 0
    labels = [np.flatnonzero(pos[u]) for u in range(n)]
    out = {"label_count": np.zeros(C, np.int64), "labels_hist": np.zeros(C + 1, np.int64),
           "cooccurrence": np.zeros((C, C), np.int64)}
    for u in range(n):
        out["labels_hist"][len(labels[u])] += 1
        out["label_count"][labels[u]] += 1
        out["cooccurrence"][np.ix_(labels[u], labels[u])] += 1
    if graph is not None:
        out.update(n_entries=np.zeros(1, np.int64), degree_sum=np.zeros(C, np.int64), contact_pairs=np.zeros((C, C), np.int64))
        for u, v in neighbour_entries(graph):
            out["n_entries"][0] += 1
            out["degree_sum"][labels[u]] += 1
            out["contact_pairs"][np.ix_(labels[u], labels[v])] += 1
    return out
