"""Planted inputs on which the neighbour gathers are EXACT in fp32, and their integer reference.

Every gather of the library computes  scale_i * sum_k w_ik T[col_k]  (plus an element-wise epilogue in the backward).  Here the
tables T hold small integers stored as float32 (uniform in [-7, 7], drawn per (strand, node, column)) and the stored values
w come from {1, 2, 3} or are implicit ones, so every partial sum of every row is an integer below 2^24 (the longest row has
2 049 entries: 2 049 * 7 * 3 + 15 * 7 < 2^24): the sum is exact in ANY order and under any FMA contraction, and
`sum * row_scale` is one correctly rounded fp32 product that numpy reproduces.  The expected output is therefore known as
numbers, from an int64 CSR x dense product, and the comparison is equality: a dropped, doubled or foreign neighbour, a wrong
slice, strand or row, a window that reads across the strand end or an element never written all change an integer by at
least 1.  Being independent of the summation order, the check freezes neither the cost model nor the butterfly order.

Builders only: nothing here touches the GPU.  tests/test_gather_cases_host.py checks the cases themselves,
tests/test_gpu_gather_exact.py holds the kernels to them.

walk_of_wave / is_super restate the rules of sliced_row_sum / sliced_super_sum (chromegcn_amd/csrc/cgcn_kernels.hip) and
are used only to LABEL planted waves, never to compute an expected value: after a retune of SLICED_COOP_OVERHEAD or
SLICED_SUPER the host test says which cases to re-plant."""
import functools

import numpy as np
import scipy.sparse as sp

from chromegcn_amd import graph as G

SLICED_COOP_OVERHEAD = 3     # cgcn_kernels.hip
SLICED_SUPER = 768
FWD_HUB_ROW = 2048
LONG_ROW = 512
FWD_WAVES = 8                # waves of a k_layer_fwd workgroup (NW of gather_tile)
BAND = G.BAND_RADIUS
EXACT_BOUND = 1 << 24
SD = ((1, 128), (2, 128), (1, 256), (2, 256))


# ---- the two rules, restated ---------------------------------------------------------------------------------------------
def is_super(length):
    return length > SLICED_SUPER


def walk_of_wave(lengths8):
    """'per-row' or 'cooperative' for a wave whose 8 rows have these lengths (a super row walks an empty range there)"""
    ls = [0 if is_super(l) else int(l) for l in lengths8]
    sm, mx = sum(-(-l // 64) for l in ls), max(ls)
    return "per-row" if sm + SLICED_COOP_OVERHEAD >= -(-mx // 8) else "cooperative"


# ---- builders ------------------------------------------------------------------------------------------------------------
def planted_csr(n_rows, n_cols, lengths_by_row, seed, values=None, forced=None):
    """(rowptr int32, col int32, val float32 or None) of a canonical CSR (columns sorted and unique): row r has exactly
    lengths_by_row[r] entries, every row not listed 0-5.  forced: {row: columns that row must hold}.  values: None =
    implicit ones, 'small' = draws from {1, 2, 3}; 'band_plus': the merged CSR of a true 'both' graph (planted_both), whose
    lengths count the stored entries of the merged rows."""
    if values == "band_plus":
        assert n_rows == n_cols and not forced
        h = planted_both(n_rows, tuple(sorted(lengths_by_row.items())), seed)[0]
        return h.rowptr, h.col, h.val
    rng = np.random.RandomState(seed)
    forced = forced or {}
    deg = rng.randint(0, 6, n_rows)
    cand = rng.randint(0, n_cols, (n_rows, 5))
    keep = np.arange(5)[None, :] < deg[:, None]
    planted = np.array(sorted(lengths_by_row), dtype=np.int64)
    keep[planted] = False
    rows = [np.repeat(np.arange(n_rows), keep.sum(1))]
    cols = [cand[keep]]
    for r in planted:
        L, f = int(lengths_by_row[int(r)]), [int(c) for c in forced.get(int(r), ())]
        assert len(f) <= L <= n_cols
        rest = [int(c) for c in rng.permutation(n_cols)[:L + len(f)] if int(c) not in f][:L - len(f)]
        rows.append(np.full(L, r))
        cols.append(np.array(f + rest, dtype=np.int64))
    a = sp.coo_matrix((np.ones(sum(len(c) for c in cols)), (np.concatenate(rows), np.concatenate(cols))),
                      shape=(n_rows, n_cols)).tocsr()     # duplicates of an unlisted row merge: its length stays 0-5
    a.sort_indices()
    val = None
    if values == "small":
        val = rng.randint(1, 4, a.nnz).astype(np.float32)
    else:
        assert values is None
    return a.indptr.astype(np.int32), a.indices.astype(np.int32), val


@functools.lru_cache(maxsize=None)
def planted_both(n, lengths_items, seed, pairs=None):
    """(HostCSR of normalize_graph('both', hic, n), hub rows): hic a planted symmetric {0,1} matrix.  With lengths the rows
    come from saliency_ref.hub_hic (row hubs[k] of the merged graph has lengths[k] stored entries); without, a sparse random
    symmetric matrix with a zero diagonal (small n: rows with and without contacts outside the band)."""
    if lengths_items:
        from saliency_ref import hub_hic
        hic, hubs, _ = hub_hic(n, "both", lengths=tuple(L for _, L in lengths_items), empty_row=False, seed=seed)
    else:
        rng = np.random.RandomState(seed)
        m = 2 * n if pairs is None else pairs
        i, j = rng.randint(0, n, m), rng.randint(0, n, m)
        ok = i != j
        hic = sp.coo_matrix((np.ones(int(ok.sum())), (i[ok], j[ok])), shape=(n, n)).tocsr()
        hic = hic + hic.T
        hic.data[:] = 1.0
        hubs = ()
    return G.normalize_graph("both", hic, n), hubs


def int_table(S, n, d, seed, even=False):
    """[S, n, d] float32 of integers uniform in [-7, 7] (even: even integers in [-6, 6]), independent per element"""
    rng = np.random.RandomState(seed)
    t = rng.randint(-3, 4, (S, n, d)) * 2 if even else rng.randint(-7, 8, (S, n, d))
    return t.astype(np.float32)


def pow2_scale(n, seed):
    """row scales in {0.25, 0.5, 1, 2}: products with integers stay exact (the autograd backward multiplies BEFORE it sums)"""
    return np.float32(2.0) ** np.random.RandomState(seed).randint(-2, 2, n).astype(np.float32)


def inv_len_scale(rowptr):
    """1 / row length as float32 (0 for an empty row): what the normaliser hands the kernels"""
    deg = np.diff(np.asarray(rowptr, np.int64)).astype(np.float64)
    with np.errstate(divide="ignore"):
        r = 1.0 / deg
    r[np.isinf(r)] = 0.0
    return r.astype(np.float32)


# ---- the integer reference -----------------------------------------------------------------------------------------------
def _int_csr(rowptr, col, val, n_cols):
    rowptr, col = np.asarray(rowptr, np.int64), np.asarray(col, np.int64)
    data = np.ones(col.shape[0], np.int64) if val is None else np.asarray(val).astype(np.int64)
    assert val is None or np.array_equal(data, np.asarray(val))
    return sp.csr_matrix((data, col, rowptr), shape=(rowptr.shape[0] - 1, n_cols))


def int_sums(rowptr, col, val, X):
    """[S, n_rows, d] int64: sum_k w_k X[s, col_k, :]"""
    X = np.asarray(X)
    Xi = X.astype(np.int64)
    assert np.array_equal(Xi, X)
    a = _int_csr(rowptr, col, val, X.shape[1])
    return np.stack([np.asarray(a @ Xi[s]) for s in range(X.shape[0])])


def aggregate_ref(rowptr, col, val, row_scale, X):
    """diag(row_scale) Ahat X as the kernels must give it: the int64 sum, then ONE fp32 product per element"""
    out = int_sums(rowptr, col, val, X).astype(np.float32)
    if row_scale is not None:
        out = out * np.asarray(row_scale, np.float32)[None, :, None]
    return out


def bwd_gather_ref(rowptr, col, val, dHs, dXn, gate, keep=None, keep_scale=np.float32(1)):
    """dX = mask * ((1 - g) dXn + sum_k w_k dHs[col_k]) over the list the backward is handed (rowptr, col, val: the CSR of
    Ahat^T); dHs integers, dXn even integers, gate in {0, 0.5, 1}: every operation below is exact in fp32.  keep: bool
    [S, n, d] (dropout_ref.mask) or None."""
    acc = int_sums(rowptr, col, val, dHs).astype(np.float32)
    res = (np.float32(1) - np.asarray(gate, np.float32))[:, :, None] * np.asarray(dXn, np.float32)
    o = res + acc
    if keep is not None:
        o = np.where(keep, o * np.float32(keep_scale), np.float32(0))
    return o.astype(np.float32)


def gate_table(S, n, seed):
    return np.random.RandomState(seed).choice(np.array([0.0, 0.5, 1.0], np.float32), (S, n))


# ---- cases ---------------------------------------------------------------------------------------------------------------
class Case:
    """one planted CSR: arrays, a label for every planted row, and the waves / lengths whose walk the case claims"""

    def __init__(self, name, n_rows, n_cols, lengths, seed, values=None, forced=None, waves=(), notes=None):
        self.name, self.n_rows, self.n_cols, self.lengths, self.values = name, n_rows, n_cols, dict(lengths), values
        self.rowptr, self.col, self.val = planted_csr(n_rows, n_cols, self.lengths, seed, values, forced)
        self.forced = forced or {}
        self.waves = tuple(waves)            # (first row of the wave, 'per-row' | 'cooperative')
        self.labels = dict(notes or {})

    @property
    def deg(self):
        return np.diff(self.rowptr.astype(np.int64))

    def label(self, row):
        return self.labels.get(int(row), "planted" if int(row) in self.lengths else "background (0-5 entries)")

    def __repr__(self):
        return "Case(%s)" % self.name


PER_ROW_LENGTHS = (0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65)
SUPER_LENGTHS = (769, 1024, 1025, 1800, 2049)
NOT_SUPER_LENGTHS = (768,)
PLANTED_N = 2113            # 33 tiles plus one row


def _planted_layout():
    """Without a row_order, wave w of tile t holds rows 64 t + 8 w .. 64 t + 8 w + 7."""
    L, waves, notes = {}, [], {}

    def wave(tile, w, lens, walk, what):
        r0 = 64 * tile + 8 * w
        for k, ln in enumerate(lens):
            L[r0 + k] = ln
            notes[r0 + k] = "%s (tile %d wave %d: %s walk)" % (what, tile, w, walk)
        waves.append((r0, walk))
    # tile 0: the per-row walk around its chunk of 8 and the 64-entry step
    wave(0, 0, (0, 1, 7, 8, 9, 15, 16, 17), "per-row", "per-row lengths")
    wave(0, 1, (63, 64, 65, 60, 60, 60, 60, 60), "per-row", "per-row lengths")
    # tile 1: the cost model's edges, sm + 3 >= ceil(mx / 8), sm = sum ceil(len / 64)
    wave(1, 0, (0, 0, 0, 32, 0, 0, 0, 0), "per-row", "seven empty rows and one of 32")
    wave(1, 1, (0, 0, 0, 0, 0, 33, 0, 0), "cooperative", "seven empty rows and one of 33")
    wave(1, 2, (1, 1, 1, 1, 1, 1, 1, 96), "per-row", "seven rows of 1 and one of 96")
    wave(1, 3, (97, 1, 1, 1, 1, 1, 1, 1), "cooperative", "seven rows of 1 and one of 97")
    wave(1, 4, (200,) * 8, "per-row", "eight rows of 200")
    wave(1, 5, (300, 0, 0, 5, 0, 2, 0, 0), "cooperative", "cooperative wave with empty rows")
    wave(1, 6, (127, 128, 129, 0, 0, 0, 0, 0), "cooperative", "cooperative wave, rows of 127 / 128 / 129")
    # tile 2: two super rows in one tile (769: the last wave's eighth is empty, the seventh holds one entry; 1024: eight
    # full eighths)
    wave(2, 0, (769, 2, 2, 2, 2, 2, 2, 2), "per-row", "two super rows in one tile")
    wave(2, 1, (3, 3, 3, 3, 1024, 3, 3, 3), "per-row", "two super rows in one tile")
    # tile 3: super rows at tile positions 0 and 63 (1025: two empty eighths; 1800: the last eighth holds 8 entries)
    wave(3, 0, (1025, 0, 1, 2, 3, 4, 5, 4), "per-row", "super row at tile position 0")
    wave(3, 7, (4, 5, 4, 3, 2, 1, 0, 1800), "per-row", "super row at tile position 63")
    # tile 4: a super row (2049 > FWD_HUB_ROW: the graph is a hub graph by max_row_len alone) sharing a wave with a
    # cooperative-length row and an empty row
    wave(4, 2, (2049, 300, 0, 3, 3, 3, 3, 3), "cooperative", "super row next to a cooperative-length and an empty row")
    # tile 5: 768 is NOT super
    wave(5, 3, (0, 0, 768, 0, 0, 0, 0, 0), "cooperative", "768 entries: not a super row")
    # tile 33: a super row that is the only row of the last, partial tile
    L[PLANTED_N - 1] = 900
    notes[PLANTED_N - 1] = "super row alone in the last, partial tile"
    return L, waves, notes


@functools.lru_cache(maxsize=None)
def planted_graph(values=None):
    L, waves, notes = _planted_layout()
    forced = {64 * 2: (0, PLANTED_N - 1), 64 * 4 + 16: (0, PLANTED_N - 1)}
    return Case("planted_%s" % (values or "ones"), PLANTED_N, PLANTED_N, L, 17, values, forced, waves, notes)


SMALL_N = (1, 7, 63, 64, 65)


@functools.lru_cache(maxsize=None)
def small_case(n, values=None):
    L = {0: n, n - 1: 0, n // 2: min(n, 9)} if n > 2 else {0: n}
    return Case("small_n%d_%s" % (n, values or "ones"), n, n, L, 100 + n, values)


@functools.lru_cache(maxsize=None)
def index_width_case(n):
    """n = 65 536: the largest graph with a 16-bit index copy, rows that hold columns 32 767 (the largest positive int16),
    32 768 (the first the int16 copy stores as a negative number) and 65 535; n = 65 537: the smallest without a copy."""
    edge = (32767, 32768, 65535) + ((65536,) if n > 65536 else ())
    L = {5: len(edge), 70: 9, 40000: 200, 100: 800, n - 1: len(edge) + 1}
    forced = {5: edge, 70: (32768,), 40000: edge, 100: edge, n - 1: (0,) + edge}
    notes = {5: "only the edge columns", 40000: "cooperative length with the edge columns", 100: "super row with the edge columns",
             n - 1: "last row: column 0 and the edge columns"}
    return Case("index_width_n%d" % n, n, n, L, 7, None, forced, (), notes)


# whole-row kernels: tails around each k_spmm instance's batch (Gather::GU x NPL = 8 entries at S d = 128, 2 at 256, 1 at 512),
# around k_spmm_any's batch of 4 and around the 64-entry chunk
WHOLE_ROW_LENGTHS = tuple(range(0, 21)) + (31, 32, 33, 62, 63, 64, 65, 66, 67, 71, 72, 73, 126, 127, 128, 129, 130, 200)
WHOLE_ROW_N = 300


@functools.lru_cache(maxsize=None)
def whole_row_case(values=None):
    L = {3 + 5 * k: ln for k, ln in enumerate(WHOLE_ROW_LENGTHS)}
    return Case("whole_row_%s" % (values or "ones"), WHOLE_ROW_N, WHOLE_ROW_N, L, 23, values)


# the fused forward's LONG_ROW split (gather_tile): rows of more than 512 entries go to all NW waves in 64-entry chunks
FUSED_N = 1100              # 1100 = 68 * 16 + 12 = 137 * 8 + 4: the last tile is partial for both strand counts
FUSED_LENGTHS = {0: LONG_ROW + 1, 1: LONG_ROW + 1 + 64 * FWD_WAVES,                       # two long rows in tile 0 (16 / S nodes)
                 3: LONG_ROW, 20: LONG_ROW + 64 * FWD_WAVES, 21: LONG_ROW + 2 + 64 * FWD_WAVES,
                 40: LONG_ROW + 64 * 4, 41: LONG_ROW + 1 + 64 * 4, 42: LONG_ROW + 2 + 64 * 4, 60: 1100,
                 FUSED_N - 1: 600}                                                        # the last row of a partial tile


@functools.lru_cache(maxsize=None)
def fused_case(values=None):
    notes = {r: ("long row (LONG_ROW split)" if ln > LONG_ROW else "512 entries: not a long row") for r, ln in FUSED_LENGTHS.items()}
    return Case("fused_%s" % (values or "ones"), FUSED_N, FUSED_N, FUSED_LENGTHS, 29, values, None, (), notes)


# rectangular operators: 20 000 rows are k_spmm's second grid-stride trip (4 096 workgroups of 4 waves)
RECT_SHAPES = ((20000, 300), (300, 5000))


@functools.lru_cache(maxsize=None)
def rect_case(n_rows, n_cols, values=None):
    top = min(n_cols, 300)
    L = {0: top, 7: 64, 8: 65, n_rows // 2: 129, n_rows - 1: top}
    if n_rows > 16384:
        L.update({16383: 63, 16384: 65, 16385: 0, 16390: 200})
    forced = {0: (0, n_cols - 1), n_rows - 1: (0, n_cols - 1)}
    return Case("rect_%dx%d_%s" % (n_rows, n_cols, values or "ones"), n_rows, n_cols, L, 31, values, forced)


def transpose_csr(rowptr, col, val, n_cols):
    """canonical CSR of the transpose (integer values kept)"""
    at = sp.csr_matrix(_int_csr(rowptr, col, val, n_cols).T)
    at.sort_indices()
    return at.indptr.astype(np.int32), at.indices.astype(np.int32), None if val is None else at.data.astype(np.float32)


BAND_N = (1, 2, 7, 8, 15, 31, 32, 33, 64, 65, 257)
BANDPLUS_SMALL_N = (1, 7, 8, 14, 15, 64, 65)
BANDPLUS_HUBS = (200, 900, 1000)     # merged lengths: the unit lists are 15 shorter (885: the last wave's eighth is empty; 985: it holds 89)


def band_host(n):
    return G.normalize_graph("constant", None, n)


def bandplus_host(n):
    """the 'both' graph of the band-plus cases: small n sparse and random; n = 2 113 with hub rows of 200, 900 and 1 000 entries"""
    if n == PLANTED_N:
        return planted_both(n, tuple(enumerate(BANDPLUS_HUBS)), 5)
    return planted_both(n, (), 40 + n)


def bandplus_no_hic(n):
    """A 'both' graph with no Hi-C entry at all.  normalize_graph hands such a graph over with implicit values (it is the
    band); a caller that keeps the explicit unit values gets a band-plus decomposition whose unit-entry list is EMPTY, for
    which graph._register_aux registers a dummy index array.  -> (rowptr, col, val of ones, row_scale)"""
    h = band_host(n)
    return h.rowptr, h.col, np.ones(h.nnz, np.float32), h.row_scale


def edge_rows(n):
    """rows 0 .. 6 and n - 7 .. n - 1: the rows whose band window ends at a strand end"""
    return sorted(set(range(min(7, n))) | set(range(max(0, n - 7), n)))
