"""Records g8_hic_build.npz: the reference's own step 7 (data/7create_graph_new.py) run on small inputs written in its
file formats.  Run where the reference is mounted (CHROMEGCN_REFERENCE, as make_golden.py); only data goes into the file.

Per case c: c{c}_pos1 / _pos2 (int32 [M], file order), _count (float64 [M]), _norm (float64 [n_bins]; absent = no vector),
_res (resolution in bp), _ws (int32 [N] window starts), _edges (hic_edges), _adj (uint8 [N, N]: the dense matrix of
create_adj_mat), _tie (1 when survivors with the threshold value were left out: the tie rule decided the set).

Path through the reference: get_normalization_values (:51-65) -> get_contact_edge_pairs (:67-91) -> get_top_contact_locs
(:93-104) -> create_adj_mat (:108-120), total_edges = int(hic_edges / 2.) (:168).  args.norm is non-empty in every case, so
the early return of the `-norm ''` route (:88-89) is not taken; cases without a vector pass normalization_values=None.
hic_edges < 2 is no case: get_top_contact_locs never reaches `idx == total_edges` for total_edges = 0 and takes everything."""
import collections
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
REF = os.environ.get("CHROMEGCN_REFERENCE")


def load_step7():
    if not REF:
        raise SystemExit("set CHROMEGCN_REFERENCE to the checkout of the reference (QData/ChromeGCN)")
    sys.modules.setdefault("tqdm", types.SimpleNamespace(tqdm=lambda it, **k: it))
    spec = importlib.util.spec_from_file_location("step7", os.path.join(REF, "data", "7create_graph_new.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.tqdm = lambda it, **k: it
    return mod


def make_case(rng, n, n_bins, m, res, with_norm):
    """records in BOTH orientations, in random file order, each ordered pair once, some with pos1 == pos2 and many whose
    ends are not windows; small integer counts (ties); NaN and 0 in the norm vector"""
    ws = np.sort(rng.choice(n_bins, n, replace=False)).astype(np.int64)
    a, b = rng.randint(0, n_bins, m), rng.randint(0, n_bins, m)
    if n >= 2:   # enough records between windows
        k = m // 2
        a[:k], b[:k] = ws[rng.randint(0, n, k)], ws[rng.randint(0, n, k)]
    _, first = np.unique(a * n_bins + b, return_index=True)
    keep = np.sort(first)
    keep = keep[rng.permutation(keep.size)]
    a, b = a[keep], b[keep]
    count = (1 + rng.poisson(2.0, a.size)).astype(np.float64)
    norm = None
    if with_norm:
        norm = 0.5 + rng.random_sample(n_bins)
        norm[rng.random_sample(n_bins) < 0.08] = np.nan
        norm[rng.random_sample(n_bins) < 0.08] = 0.0
    return (a * res).astype(np.int32), (b * res).astype(np.int32), count, norm, (ws * res).astype(np.int32)


def run_reference(step7, tmp, pos1, pos2, count, norm, res, ws, hic_edges):
    raw = os.path.join(tmp, "chrT_1kb.RAWobserved")
    with open(raw, "w") as f:
        for p, q, c in zip(pos1, pos2, count):
            f.write("%d\t%d\t%s\n" % (p, q, repr(float(c))))
    nv = None
    if norm is not None:
        npath = os.path.join(tmp, "chrT_1kb.Xnorm")
        with open(npath, "w") as f:
            for x in norm:
                f.write("NaN\n" if np.isnan(x) else "%s\n" % repr(float(x)))
        nv = step7.get_normalization_values(npath, "chrT")
    args = types.SimpleNamespace(resolution=str(res // 1000), norm="X")
    bin_dict = {"chrT": collections.OrderedDict((int(s), {"bin_idx": i}) for i, s in enumerate(ws))}
    total_edges = int(hic_edges / 2.)
    pairs = step7.get_contact_edge_pairs(args, raw, "chrT", nv, None, bin_dict, total_edges)
    top = step7.get_top_contact_locs(pairs, total_edges)
    return np.asarray(step7.create_adj_mat(bin_dict, "chrT", top).todense()).astype(np.uint8), len(pairs)


def main():
    from chromegcn_amd import hic
    step7 = load_step7()
    rng = np.random.RandomState(20240608)
    out, c, ties = {}, 0, 0
    shapes = [(1, 12, 40, 1000), (7, 30, 160, 1000), (257, 700, 6000, 1000), (7, 30, 160, 5000)]
    with tempfile.TemporaryDirectory() as tmp:
        for n, n_bins, m, res in shapes:
            for with_norm in (False, True):
                pos1, pos2, count, norm, ws = make_case(rng, n, n_bins, m, res, with_norm)
                _, _, _, v = hic.survivor_values(pos1, pos2, count, norm, res, ws)
                s = v.size
                for edges in sorted({2 * (s // 2), 2 * (s // 3) + 1, 2 * s, 2 * s + 10, 2}):
                    adj, n_pairs = run_reference(step7, tmp, pos1, pos2, count, norm, res, ws, edges)
                    assert n_pairs == s, (n_pairs, s)
                    k = int(edges / 2.)
                    tie = 0
                    if 0 < k < s:
                        t = np.sort(v)[::-1][k - 1]
                        tie = int((v == t).sum() > k - (v > t).sum())
                    ties += tie
                    p = "c%d_" % c
                    out.update({p + "pos1": pos1, p + "pos2": pos2, p + "count": count, p + "res": np.int64(res), p + "ws": ws,
                                p + "edges": np.int64(edges), p + "adj": adj, p + "tie": np.int64(tie)})
                    if norm is not None:
                        out[p + "norm"] = norm
                    c += 1
    assert ties >= 4, "no case has a tie straddling the threshold"
    out["n_cases"] = np.int64(c)
    path = os.path.join(HERE, "g8_hic_build.npz")
    np.savez_compressed(path, **out)
    print("%s: %d cases, %d with a tie at the threshold, %d bytes" % (path, c, ties, os.path.getsize(path)))


if __name__ == "__main__":
    main()
