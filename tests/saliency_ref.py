"""The adjacency saliency of scripts/visualize.py:29-55 restated on the host, and the graphs and inputs that
tests/test_saliency_ref_host.py and tests/test_gpu_saliency_cases.py share: the dense method (a requires_grad adjacency,
|adj * adj.grad|, row sum, row maximum), the product on a pattern (cgcn_sddmm), the row normalisation on a pattern
(cgcn_saliency_normalize) -- all three in float64 -- and builders of graphs with stated row lengths, so that a stated branch
of k_sddmm / k_saliency_rows (chromegcn_amd/csrc/cgcn_kernels.hip) runs.  Builders only: nothing here touches the GPU.

A "row length" is the number of stored entries of one CSR row of the NORMALISED graph (A-hat: Hi-C + identity, band
included for 'both'); k_sddmm walks a row in chunks of 64 entries and batches of 8 with a clamped tail, k_saliency_rows in
chunks of 64."""
import functools

import numpy as np
import scipy.sparse as sp
import torch

from chromegcn_amd import graph as G
from oracle import chromegcn_oracle as O

ADJ_TYPES = ("hic", "both", "constant", "none")
BAND = G.BAND_RADIUS


# ---- the three float64 statements ----------------------------------------------------------------------------------------
def dense_hidden(orc, adj, x, layers):
    """the gated stack with a dense adjacency (models/ChromeModels.py:37-46): the tensor the classifier head's ReLU reads"""
    h = x
    for k in range(1, layers + 1):
        gc, wk = getattr(orc, "GC%d" % k), getattr(orc, "W%d" % k)
        z = torch.tanh(adj @ (h @ gc.weight) + gc.bias)
        g = torch.sigmoid(wk(z))
        h = (1 - g) * h + g * z
    return h


def dense_saliency(orc, A_dense, x_f, x_r, targets, layers, relu_mask=None, normalize=True):
    """scripts/visualize.py:29-55 as written: the dense adjacency with requires_grad, sigmoid(mean of the strands' logits)
    backpropagated with the targets as the gradient, |adj * adj.grad|, divided by the row sums (1 where 0), then by the row
    maxima (1 where 0).  Runs in the dtype of A_dense (float64 for the reference; float32 to see what fp32 alone does);
    orc must be in that dtype and in eval mode.
    relu_mask: None, or (mask of the forward strand, mask of the reverse strand), bool [n, d]: the head then takes
    h * mask in place of relu(h) -- the derivative of the ReLU is its mask, and an input within fp32 rounding of zero makes
    the mask, not the arithmetic, decide between two saliency maps that differ by percents.
    Returns the [n, n] map as a numpy array."""
    adj = torch.as_tensor(A_dense).detach().clone().requires_grad_(True)
    dt = adj.dtype
    orc.zero_grad()                                                   # visualize.py:33

    def forward(x, mask):
        h = dense_hidden(orc, adj, x.to(dt), layers)
        r = torch.relu(h) if mask is None else h * torch.as_tensor(mask).to(dt)
        return orc.out(orc.batch_norm(r))
    m_f, m_r = (None, None) if relu_mask is None else relu_mask
    pred = (forward(x_f, m_f) + forward(x_r, m_r)) / 2                # visualize.py:37-39
    torch.sigmoid(pred).backward(gradient=targets.to(dt))             # visualize.py:40,47
    adj_grad = torch.abs(adj * adj.grad).detach()                     # visualize.py:49
    if normalize:
        s = adj_grad.sum(1); s[s == 0] = 1                            # visualize.py:50-52
        adj_grad = adj_grad / s.view(-1, 1)
        m, _ = torch.max(adj_grad, 1); m[m == 0] = 1                  # visualize.py:53-55
        adj_grad = adj_grad / m.view(-1, 1)
    return adj_grad.numpy()


def hidden_pair(orc, A_dense, x_f, x_r, layers):
    """(h of the forward strand, h of the reverse strand) as numpy arrays, in the dtype of A_dense"""
    adj = torch.as_tensor(A_dense)
    with torch.no_grad():
        return tuple(dense_hidden(orc, adj, x.to(adj.dtype), layers).numpy() for x in (x_f, x_r))


def rows_of(rowptr):
    rowptr = np.asarray(rowptr, np.int64)
    return np.repeat(np.arange(rowptr.shape[0] - 1), np.diff(rowptr))


def sddmm_ref(rowptr, col, a, b, chunk=1 << 15):
    """out[k] = sum over strands s of <a[s, i, :], b[s, col[k], :]> for every stored entry k of row i, in float64
    (a, b: [S, n, d])"""
    rows, col = rows_of(rowptr), np.asarray(col, np.int64)
    a64, b64 = np.asarray(a, np.float64), np.asarray(b, np.float64)
    out = np.zeros(col.shape[0], np.float64)
    for k0 in range(0, col.shape[0], chunk):
        r, c = rows[k0:k0 + chunk], col[k0:k0 + chunk]
        for s in range(a64.shape[0]):
            out[k0:k0 + chunk] += np.einsum("kd,kd->k", a64[s][r], b64[s][c])
    return out


def normalize_ref(rowptr, val, raw):
    """visualize.py:49-55 on a pattern, in float64 and in the reference's order of operations: v = |val * raw| (val None:
    ones), divided by the row's sum (1 where it is 0), then by the row's maximum of those quotients (1 where it is 0).
    Entries outside the pattern are zeros of the dense matrix: they change neither a sum nor a maximum."""
    rows = rows_of(rowptr)
    n = np.asarray(rowptr).shape[0] - 1
    v = np.abs(np.asarray(raw, np.float64) * (1.0 if val is None else np.asarray(val, np.float64)))
    s = np.zeros(n); np.add.at(s, rows, v); s[s == 0] = 1
    q = v / s[rows]
    m = np.zeros(n); np.maximum.at(m, rows, q); m[m == 0] = 1
    return q / m[rows]


def scaled_error(got, want):
    """max |got - want| / max |want| (1 for an all-zero want): the figure the end-to-end bound is stated in"""
    want = np.asarray(want, np.float64)
    if want.size == 0:
        return 0.0
    scale = float(np.abs(want).max()) or 1.0
    return float(np.abs(np.asarray(got, np.float64) - want).max()) / scale


# ---- patterns with planted row lengths -----------------------------------------------------------------------------------
PLANTED_LENGTHS = (1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 71, 72, 73, 127, 128, 129, 200)
PLANTED_N = 401


@functools.lru_cache(maxsize=None)
def planted_pattern(n=PLANTED_N, lengths=PLANTED_LENGTHS, seed=11):
    """(a, rows): an asymmetric {0,1} matrix with a zero diagonal such that row rows[k] of normalize_graph('hic', a, n) has
    exactly lengths[k] stored entries (its diagonal and lengths[k] - 1 others).  The row of the longest length holds the
    columns 0 and n - 1; the row of length 2 holds column 0; every other row has 0-5 off-diagonal entries."""
    rng = np.random.RandomState(seed)
    rows = tuple(int(r) for r in np.linspace(3, n - 4, len(lengths)).astype(np.int64))
    assert len(set(rows)) == len(lengths)
    longest = int(np.argmax(lengths))
    a = sp.lil_matrix((n, n))
    for i in range(n):
        if i in rows:
            k = rows.index(i)
            want = lengths[k] - 1
            forced = [0, n - 1] if k == longest else ([0] if lengths[k] == 2 else [])
            others = [c for c in rng.permutation(n) if c != i and c not in forced][:want - len(forced)]
            cols = forced + [int(c) for c in others]
        else:
            cols = [int(c) for c in rng.choice(n, rng.randint(0, 6), replace=False) if c != i]
        for c in cols:
            a[i, c] = 1.0
    return sp.csr_matrix(a), rows


def asymmetric_binary(n, density, seed):
    """{0,1}, zero diagonal, a != a.T"""
    a = sp.random(n, n, density, format="lil", random_state=seed)
    a.setdiag(0)
    a = sp.csr_matrix(a); a.eliminate_zeros(); a.data[:] = 1.0
    assert (a != a.T).nnz > 0
    return a


# values with an exact |product| against a power of two, both signs, fractions
VALUE_SET = np.array([-2.0, -0.5, 0.25, 0.75, 1.5, 3.0, -0.375, 1.0])


def asymmetric_valued(n, density, seed, lengths=(), empty_row=None):
    """An asymmetric matrix with negative and fractional values on its stored entries (drawn from VALUE_SET), the diagonal
    stored too; rows 2, 4, 6, ... get exactly lengths[0], lengths[1], ... stored entries and row `empty_row` none at all.
    For host_csr_from_matrix: the values are A itself, there is no row scale."""
    rng = np.random.RandomState(seed)
    a = sp.random(n, n, density, format="lil", random_state=seed)
    a.setdiag(1.0)
    for k, L in enumerate(lengths):
        i = 2 + 2 * k
        a[i, :] = 0
        for c in rng.choice(n, L, replace=False):
            a[i, int(c)] = 1.0
    if empty_row is not None:
        a[empty_row, :] = 0
    a = sp.csr_matrix(a); a.eliminate_zeros(); a.sort_indices()
    a.data[:] = VALUE_SET[rng.randint(0, len(VALUE_SET), a.nnz)]
    assert (abs(a - a.T)).nnz > 0
    return a


HUB_LENGTHS = (63, 64, 65, 128, 200)


@functools.lru_cache(maxsize=None)
def hub_hic(n, adj_type, lengths=HUB_LENGTHS, empty_row=True, seed=5, pairs=None):
    """(hic, hubs, empty): a symmetric {0,1} Hi-C matrix with a zero diagonal (the on-disk contract) over a 1/k background,
    such that row hubs[k] of normalize_graph(adj_type, hic, n) has exactly lengths[k] stored entries -- the diagonal, for
    'both' the band, and neighbours outside both that are no hubs themselves.  empty_row: node `empty` has no contact and
    hic[empty, empty] = -1, which cancels the identity (tests/test_gpu_graph.py): an EMPTY row under 'hic' (row scale 0);
    under 'both' the band remains and only the diagonal goes, which also takes the graph off the band-plus route."""
    rng = np.random.RandomState(seed)
    hubs = tuple(int(h) for h in np.linspace(20, n - 60, len(lengths)).astype(np.int64))
    empty = n - 25 if empty_row else None
    apart = hubs + ((empty,) if empty_row else ())
    assert all(abs(p - q) > 2 * BAND for i, p in enumerate(apart) for q in apart[i + 1:])
    a = O.random_symmetric_graph(n, 4 * n if pairs is None else pairs, seed, hic_like=True).tolil()
    for h in apart:
        a[h, :] = 0; a[:, h] = 0
    base = 1 + (2 * BAND if adj_type == "both" else 0)
    for h, L in zip(hubs, lengths):
        near = set(range(h - BAND, h + BAND + 1)) if adj_type == "both" else {h}
        cand = [c for c in rng.permutation(n) if c not in near and c not in apart]
        for c in cand[:L - base]:
            a[h, int(c)] = 1.0; a[int(c), h] = 1.0
    if empty_row:
        a[empty, empty] = -1.0
    a = sp.csr_matrix(a); a.eliminate_zeros(); a.sort_indices()
    assert (abs(a - a.T)).nnz == 0
    return a, hubs, empty


def row_lengths(rowptr):
    return np.diff(np.asarray(rowptr, np.int64))


# ---- inputs of the row normalisation -------------------------------------------------------------------------------------
def _pow2(v):
    m, _ = np.frexp(np.abs(v))
    return m == 0.5


def craft_raw(rowptr, val, seed, last_chunk_lengths=(64, 65, 129), single=True):
    """(raw float32 [nnz], roles): N(0,1) products of mixed sign on the given pattern, with
      roles['zero']   a row of >= 3 entries whose raw values are all 0 (the output must be exactly 0),
      roles['single'] a row of one entry (the output must be exactly 1),
      roles['last']   for every length in last_chunk_lengths a row of that length whose largest |val * raw| is its LAST
                      entry (the maximum is found in the last 64-entry chunk, for 64 in a full one),
      roles['tie']    a row in which two entries share the largest |val * raw| exactly (both must come out as 1),
      roles['empty']  the rows without entries (nothing to write; listed so that a test can demand one).
    Every role is a row index, or a list of them; a role the pattern has no row for raises (single=False: none is asked
    for -- no row of a 'both' graph is shorter than its band)."""
    rng = np.random.RandomState(seed)
    rowptr = np.asarray(rowptr, np.int64)
    lens = np.diff(rowptr)
    v = None if val is None else np.asarray(val, np.float64)
    raw = rng.randn(int(rowptr[-1])).astype(np.float32)
    raw[raw == 0] = 1.0
    used = set()

    def pick(cond, what):
        for i in np.flatnonzero(cond):
            if int(i) not in used and (v is None or np.all(v[rowptr[i]:rowptr[i + 1]] != 0)):
                used.add(int(i))
                return int(i)
        raise AssertionError("the pattern has no row for the role %r" % what)
    roles = {"empty": [int(i) for i in np.flatnonzero(lens == 0)], "last": []}
    if single:
        roles["single"] = pick(lens == 1, "single")
    for L in last_chunk_lengths:
        i = pick(lens == L, "last %d" % L)
        k = rowptr[i + 1] - 1
        raw[k] = np.float32(64.0 if v is None else 64.0 / v[k]) * (1 if L % 2 else -1)
        roles["last"].append(i)
    i = roles["zero"] = pick(lens >= 3, "zero")
    raw[rowptr[i]:rowptr[i + 1]] = 0.0
    # two equal maxima: positions whose value is a power of two in magnitude, so that val * raw is exact
    for i in np.flatnonzero(lens >= 3):
        k0, k1 = rowptr[i], rowptr[i + 1]
        ok = np.arange(k0, k1) if v is None else k0 + np.flatnonzero(_pow2(v[k0:k1]))
        if int(i) in used or ok.size < 2:
            continue
        p, q = int(ok[0]), int(ok[-1])
        raw[p] = np.float32(32.0 if v is None else 32.0 / v[p])
        raw[q] = np.float32(-32.0 if v is None else -32.0 / v[q])
        used.add(int(i)); roles["tie"] = (int(i), p, q)
        break
    else:
        raise AssertionError("the pattern has no row for the role 'tie'")
    return raw, roles


# ---- end-to-end cases ----------------------------------------------------------------------------------------------------
E2E_MODELS = ((128, 1), (128, 3), (256, 2), (256, 4))      # (d, layers): ring / row-local backward, tap of 1 .. 4 entries
E2E_N = (1, 5, 97, 300)                                    # one node; below the band radius; ragged; hub rows
E2E_C = 7
RELU_MARGIN = 1e-5       # a ReLU input this close to zero may fall on either side in fp32
RELU_FLIPS_MAX = 8       # ... and at most this many entries of one case may


@functools.lru_cache(maxsize=None)
def e2e_hic(adj_type, n):
    """the raw Hi-C matrix of the end-to-end case (None for 'constant' and 'none')"""
    if adj_type in ("constant", "none"):
        return None
    if n == 1:
        return sp.csr_matrix((1, 1))
    if n == 5:
        return O.random_symmetric_graph(5, 6, 3)
    if n == 97:
        a = O.random_symmetric_graph(97, 400, 4).tolil()
        if adj_type == "both":           # no diagonal in row 40: explicit values that are NOT the band-plus form
            a[40, 40] = -1.0
        return sp.csr_matrix(a)
    if n == 300:
        return hub_hic(300, adj_type, empty_row=(adj_type == "hic"))[0]
    raise ValueError(n)


def make_oracle(d, layers, seed, c=E2E_C):
    """float32 oracle with GC weights randn / sqrt(d) * 1.5 (eval mode); .double() of a deep copy is the reference"""
    torch.manual_seed(seed)
    orc = O.GatedGCNOracle(d, c, 0.0, layers).eval()
    with torch.no_grad():
        for k, p in orc.named_parameters():
            if "GC" in k and k.endswith("weight"):
                p.copy_(torch.randn_like(p) / np.sqrt(d) * 1.5)
    return orc


def e2e_seed(adj_type, d, layers, n):
    return 1000 * ADJ_TYPES.index(adj_type) + 100 * E2E_MODELS.index((d, layers)) + E2E_N.index(n)


def e2e_inputs(d, n, seed, c=E2E_C):
    g = torch.Generator().manual_seed(seed)
    x_f, x_r = torch.randn(n, d, generator=g), torch.randn(n, d, generator=g)
    targets = (torch.rand(n, c, generator=g) < 0.3).float()
    return x_f, x_r, targets


def dense_adjacency(adj_type, hic, n):
    """the reference's process_graph(...).to_dense() (fp32 values), as float64"""
    return O.normalized_adjacency(adj_type, hic, n).toarray().astype(np.float64)


def relu_flips(mask_pair, h64_pair):
    """(count, largest |h64|) over the entries where a mask differs from h64 > 0"""
    count, worst = 0, 0.0
    for m, h in zip(mask_pair, h64_pair):
        diff = np.asarray(m, bool) != (h > 0)
        count += int(diff.sum())
        if diff.any():
            worst = max(worst, float(np.abs(h[diff]).max()))
    return count, worst


def check_relu_mask(mask_pair, h64_pair, what):
    """the two conditions under which a test may hand the masks of the code under test to dense_saliency"""
    count, worst = relu_flips(mask_pair, h64_pair)
    assert worst < RELU_MARGIN, ("%s: the FORWARD is wrong, not the saliency: a ReLU input of magnitude %.3g (float64) has "
                                 "the other sign on the device" % (what, worst))
    assert count <= RELU_FLIPS_MAX, "%s: the FORWARD puts %d ReLU inputs on the other side of zero" % (what, count)
    return count


def e2e_case(adj_type, d, layers, n):
    """One row of the end-to-end table: the raw Hi-C matrix, the reference's dense adjacency (float64), the float32 oracle
    and the inputs (x_f, x_r, targets)"""
    seed = e2e_seed(adj_type, d, layers, n)
    hic = e2e_hic(adj_type, n)
    return dict(hic=hic, A=dense_adjacency(adj_type, hic, n), orc=make_oracle(d, layers, seed),
                inputs=e2e_inputs(d, n, 5000 + seed))


ASYM_N = 97
ASYM_KINDS = ("binary", "valued")


def asym_case(kind, d, layers):
    """Operators outside the reference's data contract (A-hat != A-hat^T): 'binary' = normalize_graph('hic', asymmetric a),
    A = diag(row_scale) pattern; 'valued' = host_csr_from_matrix of an asymmetric matrix with negative and fractional
    values, A = the matrix itself.  Returns the HostCSR too."""
    seed = 9000 + 100 * ASYM_KINDS.index(kind) + E2E_MODELS.index((d, layers))
    if kind == "binary":
        h = G.normalize_graph("hic", asymmetric_binary(ASYM_N, 0.05, 7), ASYM_N)
    else:
        h = G.host_csr_from_matrix(asymmetric_valued(ASYM_N, 0.05, 8, lengths=(65,), empty_row=50) * 0.25)
    assert not h.symmetric
    return dict(host=h, A=h.to_scipy().toarray().astype(np.float64), orc=make_oracle(d, layers, seed),
                inputs=e2e_inputs(d, ASYM_N, 5000 + seed))
