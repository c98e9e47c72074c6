"""Records g9_hic_upsample.npz: the reference's step 7 (data/7create_graph_new.py) run on 5 kb records expanded to 1 kb the way
the reference expands them.  Run where the reference is mounted (CHROMEGCN_REFERENCE, as make_golden_hic.py); only data goes
into the file.

Per case c: c{c}_pos1 / _pos2 (int32 [M], file order, multiples of _res) and _count (float64 [M]): the COMPACT records; _norm
(float64 [n_bins] at _res; absent = no vector), _res (5000), _wbp (1000), _ws (int32 [N] window starts, multiples of _wbp),
_edges (hic_edges), _adj (uint8 [N, N]: the dense matrix of create_adj_mat), _tie (1 when survivors with the threshold value were
left out), _inblock (present with _tie: 1 when the cut falls between two children of ONE record), _diag (1 when the children
of one diagonal record are on both sides of the cut).

Path through the reference: the expanded records are written to a text file in the loop order of data/extras/upsample_hic.py
:36-44 (that script hard-codes its input and output directories and runs on import, so its five-line loop -- for every record,
for res_add_a in 0, 1000 .. 4000, for res_add_b in the same, write (A + res_add_a, B + res_add_b, value) -- is restated in
write_expanded below, not imported); then get_normalization_values (:51-65) -> get_contact_edge_pairs (:67-91) ->
get_top_contact_locs (:93-104) -> create_adj_mat (:108-120) with args.resolution = '5' (data/create_data.py:47-55),
total_edges = int(hic_edges / 2.) (:168).  args.norm is non-empty in every case."""
import collections
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from make_golden_hic import load_step7  # noqa: E402

RES, WBP = 5000, 1000
UP = RES // WBP


def make_case(rng, n, n_coarse, m, with_norm):
    """windows on the 1 kb grid; 5 kb records in BOTH orientations, in random file order, each ordered pair once, a share of
    them diagonal and many over bins without a window; small integer counts (ties between blocks); NaN and 0 norm bins"""
    ws = np.sort(rng.choice(n_coarse * UP, n, replace=False)).astype(np.int64)
    a, b = rng.randint(0, n_coarse, m), rng.randint(0, n_coarse, m)
    if n >= 2:   # enough records between bins that hold windows, and diagonal records over such bins
        k = m // 2
        a[:k], b[:k] = ws[rng.randint(0, n, k)] // UP, ws[rng.randint(0, n, k)] // UP
        d = m // 8
        b[k:k + d] = a[k:k + d] = ws[rng.randint(0, n, d)] // UP
    _, first = np.unique(a * n_coarse + b, return_index=True)
    keep = np.sort(first)
    keep = keep[rng.permutation(keep.size)]
    a, b = a[keep], b[keep]
    count = (1 + rng.poisson(2.0, a.size)).astype(np.float64)
    norm = None
    if with_norm:
        norm = 0.5 + rng.random_sample(n_coarse)
        norm[rng.random_sample(n_coarse) < 0.08] = np.nan
        norm[rng.random_sample(n_coarse) < 0.08] = 0.0
        norm[rng.choice(n_coarse, 2, replace=False)] = [np.nan, 0.0]   # both in every vector, the short ones too
    return (a * RES).astype(np.int32), (b * RES).astype(np.int32), count, norm, (ws * WBP).astype(np.int32)


def write_expanded(path, pos1, pos2, count):
    """data/extras/upsample_hic.py:36-44"""
    with open(path, "w") as f:
        for p, q, c in zip(pos1, pos2, count):
            value = repr(float(c))
            for res_add_a in [0, 1000, 2000, 3000, 4000]:
                for res_add_b in [0, 1000, 2000, 3000, 4000]:
                    f.write(str(int(p) + res_add_a) + "\t" + str(int(q) + res_add_b) + "\t" + value + "\n")


def run_reference(step7, tmp, pos1, pos2, count, norm, ws, hic_edges):
    raw = os.path.join(tmp, "chrT_1kb.RAWobserved")
    write_expanded(raw, pos1, pos2, count)
    nv = None
    if norm is not None:
        npath = os.path.join(tmp, "chrT_5kb.Xnorm")
        with open(npath, "w") as f:
            for x in norm:
                f.write("NaN\n" if np.isnan(x) else "%s\n" % repr(float(x)))
        nv = step7.get_normalization_values(npath, "chrT")
    args = types.SimpleNamespace(resolution=str(RES // 1000), norm="X")
    bin_dict = {"chrT": collections.OrderedDict((int(s), {"bin_idx": i}) for i, s in enumerate(ws))}
    total_edges = int(hic_edges / 2.)
    pairs = step7.get_contact_edge_pairs(args, raw, "chrT", nv, None, bin_dict, total_edges)
    top = step7.get_top_contact_locs(pairs, total_edges)
    adj = np.asarray(step7.create_adj_mat(bin_dict, "chrT", top).todense()).astype(np.uint8)
    return adj, len(pairs)


def main():
    from chromegcn_amd import hic
    step7 = load_step7()
    rng = np.random.RandomState(20240917)
    out, c, ties, diags = {}, 0, 0, 0
    shapes = [(1, 6, 30), (7, 8, 60), (7, 12, 90), (211, 150, 1500)]   # windows, 5 kb bins, records drawn
    with tempfile.TemporaryDirectory() as tmp:
        for n, n_coarse, m in shapes:
            for with_norm in (False, True):
                pos1, pos2, count, norm, ws = make_case(rng, n, n_coarse, m, with_norm)
                idx, _, _, v = hic.survivor_values(pos1, pos2, count, norm, RES, ws, window_bp=WBP)
                s = v.size
                for edges in sorted({2 * (s // 2), 2 * (s // 3) + 1, 2 * s, 2 * s + 10, 2}):
                    adj, n_pairs = run_reference(step7, tmp, pos1, pos2, count, norm, ws, edges)
                    assert n_pairs == s, (n_pairs, s)
                    k = int(edges / 2.)
                    tie = diag = 0
                    if 0 < k < s:
                        taken = np.zeros(s, bool)
                        taken[np.argsort(-v, kind="stable")[:k]] = True
                        t = np.sort(v)[::-1][k - 1]
                        tie = int((v == t).sum() > k - (v > t).sum())
                        src = idx // (UP * UP)
                        on_diag = pos1[src] == pos2[src]
                        for r in np.unique(src[on_diag]):
                            diag |= int(taken[src == r].any() and not taken[src == r].all())
                        if tie:   # the cut falls inside a block of equal values: the block of one source record
                            last = np.flatnonzero(taken & (v == t))[-1]
                            inside = last + 1 < s and src[last + 1] == src[last] and not taken[last + 1]
                            out["c%d_inblock" % c] = np.int64(inside)
                    ties += tie
                    diags += diag
                    p = "c%d_" % c
                    out.update({p + "pos1": pos1, p + "pos2": pos2, p + "count": count, p + "res": np.int64(RES),
                                p + "wbp": np.int64(WBP), p + "ws": ws, p + "edges": np.int64(edges),
                                p + "adj": adj, p + "tie": np.int64(tie), p + "diag": np.int64(diag)})
                    if norm is not None:
                        out[p + "norm"] = norm
                    c += 1
    inblock = sum(int(out.get("c%d_inblock" % i, 0)) for i in range(c))
    assert ties >= 4 and inblock >= 4, "fewer than four cases have the threshold inside a block of equal values"
    assert diags >= 2, "fewer than two cases have a diagonal record's children on both sides of the cut"
    out["n_cases"] = np.int64(c)
    path = os.path.join(HERE, "g9_hic_upsample.npz")
    np.savez_compressed(path, **out)
    print("%s: %d cases, %d ties at the threshold (%d inside one record's block), %d diagonal blocks cut, %d bytes"
          % (path, c, ties, inblock, diags, os.path.getsize(path)))


if __name__ == "__main__":
    main()
