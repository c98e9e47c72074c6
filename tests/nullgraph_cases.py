"""Inputs of the null-graph tests (tests/test_nullgraph_host.py, tests/test_gpu_nullgraph.py) and the host results they
share.  Every builder asserts the properties its case is there for, so a change of a generator cannot hollow a test out."""
import functools

import numpy as np
import scipy.sparse as sp

from chromegcn_amd import nullgraph as NG
from chromegcn_amd import synth

MODELS = ("distance", "degree", "uniform")
SEEDS = (0, 1, 2 ** 32 + 5, 2 ** 63)

# the literal known answer: 8 windows, seed 7.  d = 1: 6 of 7 slots (complemented, one hole); d = 2: 2 of 6 (plain);
# d = 5: 2 of 3 (complemented, one hole); d = 7: 1 of 1 (complemented, no hole: the edge stays)
PINNED_N, PINNED_SEED = 8, 7
PINNED_EDGES = [(0, 1), (0, 2), (0, 5), (0, 7), (1, 2), (1, 3), (2, 3), (2, 7), (3, 4), (4, 5), (5, 6)]
PINNED = {
    "distance": ([(0, 1), (0, 5), (0, 7), (1, 2), (1, 6), (2, 3), (2, 4), (4, 5), (4, 6), (5, 6), (6, 7)],
                 dict(edges_in=11, edges_out=11, tokens=4, unplaced=0, complemented_classes=3, loops=0, repeats=0, rounds_used=1)),
    "degree": ([(0, 2), (0, 3), (0, 4), (0, 7), (1, 2), (1, 6), (2, 5), (3, 4), (3, 7)],
               dict(edges_in=11, edges_out=9, tokens=22, unplaced=0, complemented_classes=0, loops=1, repeats=1, rounds_used=0)),
    "uniform": ([(0, 1), (0, 3), (0, 5), (0, 6), (1, 5), (1, 7), (2, 4), (2, 7), (3, 4), (4, 7), (5, 6)],
                dict(edges_in=11, edges_out=11, tokens=11, unplaced=0, complemented_classes=0, loops=0, repeats=0, rounds_used=3)),
}


def from_edges(n, edges):
    """the symmetric {0,1} CSR of undirected edges (i < j), canonical, no diagonal"""
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    assert np.all(e[:, 0] < e[:, 1]) and np.all(e >= 0) and np.all(e < max(n, 1)) and len({tuple(x) for x in e.tolist()}) == len(e)
    a = sp.coo_matrix((np.ones(2 * len(e)), (np.r_[e[:, 0], e[:, 1]], np.r_[e[:, 1], e[:, 0]])), shape=(n, n)).tocsr()
    a.sort_indices()
    return a


def upper_list(a):
    c = sp.triu(sp.csr_matrix(a), 1).tocoo()
    return sorted(zip(c.row.tolist(), c.col.tolist()))


def distance_hist(a):
    n = a.shape[0]
    c = sp.triu(sp.csr_matrix(a), 1).tocoo()
    return np.bincount(c.col - c.row, minlength=max(n, 1))


def class_facts(a):
    """(c_d, n_d, complemented) per distance"""
    n = a.shape[0]
    cd = distance_hist(a)
    nd = n - np.arange(cd.size)
    nd[0] = 0
    return cd, nd, 2 * cd > nd


def band(n, radius=7):
    return from_edges(n, [(i, i + d) for d in range(1, radius + 1) for i in range(n - d)])


def _pinned():
    return from_edges(PINNED_N, PINNED_EDGES)


def _band40():
    a = band(40)
    cd, nd, comp = class_facts(a)
    assert np.all(comp[1:8]) and np.all(cd[1:8] == nd[1:8]) and not cd[8:].any()   # every class full: complemented, no holes
    return a


def _half():
    # d = 1: c = 10 of n_1 = 20, exactly half: NOT complemented; d = 3: c = 10 of n_3 = 18 = n_3 / 2 + 1: complemented
    a = from_edges(21, [(i, i + 1) for i in range(0, 20, 2)] + [(i, i + 3) for i in range(10)])
    cd, nd, comp = class_facts(a)
    assert 2 * cd[1] == nd[1] and not comp[1] and cd[3] == nd[3] // 2 + 1 and comp[3]
    return a


def _far():
    a = from_edges(12, [(0, 11), (0, 4), (3, 7), (5, 6), (2, 9)])
    assert distance_hist(a)[11] == 1
    return a


def _isolated():
    a = from_edges(30, [(5, 6), (5, 9), (6, 12), (7, 8), (8, 12), (9, 11)])
    assert np.count_nonzero(np.diff(a.indptr) == 0) == 23
    return a


def _crowded():
    # rounds = 1 leaves tokens unplaced in a plain class (d = 1: 20 of 40, exactly half) and in a complemented one
    # (d = 2: 25 of 39, 14 holes)
    a = from_edges(41, [(i, i + 1) for i in range(0, 40, 2)] + [(i, i + 2) for i in range(25)])
    cd, nd, comp = class_facts(a)
    assert not comp[1] and comp[2] and nd[2] - cd[2] == 14
    return a


def _hic300(seed):
    a = synth.contact_graph(300, 6000, seed, "hic_like")
    cd, nd, comp = class_facts(a)
    assert np.any(comp & (cd == nd)) and np.any(comp & (cd < nd)) and np.any(~comp & (cd > 0))
    return a


def _sparse300():
    a = synth.contact_graph(300, 900, 5, "uniform")
    assert a.shape == (300, 300) and 1600 <= a.nnz <= 1800
    return a


def _big5000():
    # several workgroups of every pass: more than 65 536 tokens, and a hub row of more than 1 024 entries
    a = synth.contact_graph(5000, 68000, 9, "uniform").tolil()
    hub = np.arange(1, 3001, 2)
    a[17, hub] = 1.0
    a[hub, 17] = 1.0
    a = sp.csr_matrix(a)
    a.setdiag(0)
    a.eliminate_zeros()
    a.sort_indices()
    assert np.diff(a.indptr).max() > 1024 and 66000 < a.nnz // 2 < 75000 and (a != a.T).nnz == 0
    assert NG.null_graph_host(a, "distance", 0, return_info=True)[1]["tokens"] > 65536
    return a


BUILDERS = {
    "pinned8": _pinned, "band40": _band40, "half": _half, "far": _far, "isolated": _isolated, "crowded": _crowded,
    "n1": lambda: sp.csr_matrix((1, 1)), "n2": lambda: from_edges(2, [(0, 1)]), "empty10": lambda: sp.csr_matrix((10, 10)),
    "hic300_a": lambda: _hic300(3), "hic300_b": lambda: _hic300(6), "sparse300": _sparse300, "big5000": _big5000,
}
SMALL = ("pinned8", "band40", "half", "far", "isolated", "crowded", "n1", "n2", "empty10")
ALL = SMALL + ("hic300_a", "hic300_b", "sparse300", "big5000")
NO_UNIFORM = ("n2",)   # 'uniform' does not support these (tests/test_nullgraph_host.py checks the list)
CASES = [(name, model) for name in ALL for model in MODELS if not (model == "uniform" and name in NO_UNIFORM)]


@functools.lru_cache(maxsize=None)
def graph(name):
    a = sp.csr_matrix(BUILDERS[name]())
    assert (a != a.T).nnz == 0 and a.diagonal().sum() == 0 and a.has_sorted_indices
    return a


def supports(name, model):
    a = graph(name)
    n, m = a.shape[0], a.nnz // 2
    return model != "uniform" or m == 0 or (n >= 2 and 4 * m <= n * (n - 1))


@functools.lru_cache(maxsize=None)
def host(name, model, seed, rounds=NG.DEFAULT_ROUNDS):
    """(matrix, info) of the restatement, computed once per session; callers do not modify it"""
    return NG.null_graph_host(graph(name), model, seed, rounds=rounds, return_info=True)
