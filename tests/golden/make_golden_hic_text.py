"""Records g10_hic_text.npz: the reference's own step 7 (data/7create_graph_new.py) run on a small TEXT fixture -- a
`RAWobserved` file, a norm file and a windows bed of a few hundred lines.  Run where the reference is mounted
(CHROMEGCN_REFERENCE, as make_golden_hic.py); only data goes into the file.

raw / norm / bed (uint8): the bytes of the three files; chrom, res; per case c: c{c}_edges (hic_edges), c{c}_indptr /
c{c}_indices (the CSR create_adj_mat returns), c{c}_tie (1 when survivors with the threshold value were left out).

Path through the reference: create_bin_dict (:14-47) on the bed -> get_normalization_values (:51-65) on the norm file ->
get_contact_edge_pairs (:67-91) on the text -> get_top_contact_locs (:93-104) -> create_adj_mat (:108-120),
total_edges = int(hic_edges / 2.) (:168); args.norm is non-empty, so the early return of :88-89 is not taken.  The reference
reads positions with int(), so the fixture's are plain digits; its counts come in every spelling float() takes that a dump
can hold (one decimal, integers, exponents, 17 significant digits), small integers mostly, over a norm vector of few distinct
values: ties at the cut.  The bed names a
second chromosome and repeats starts (one line per peak); the norm vector has NaN and 0 bins."""
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

from make_golden_hic import load_step7  # noqa: E402


def make_fixture(rng):
    res, n_bins, n = 1000, 90, 40
    ws = np.sort(rng.choice(n_bins, n, replace=False))
    bed = []
    for chrom, starts in (("chrT", ws), ("chrU", np.sort(rng.choice(n_bins, 12, replace=False)))):
        for s in starts:
            for _ in range(1 + rng.randint(0, 3)):   # one line per peak: starts repeat
                bed.append("%s\t%d\t%d\tassay%d\t0\t.\t%.3f\t%.3f\t%.3f\t%d\n"
                           % (chrom, s * res, s * res + res, rng.randint(0, 9), rng.rand(), rng.rand(), rng.rand(), rng.randint(0, 500)))
    order = rng.permutation(len(bed))            # the bed is not sorted: create_bin_dict sorts
    bed = "".join(bed[i] for i in order)
    a, b = rng.randint(0, n_bins, 420), rng.randint(0, n_bins, 420)
    a[:260], b[:260] = ws[rng.randint(0, n, 260)], ws[rng.randint(0, n, 260)]
    _, first = np.unique(a * n_bins + b, return_index=True)
    keep = np.sort(first)
    a, b = a[keep], b[keep]
    lines = []
    for k, (p, q) in enumerate(zip(a, b)):
        c = 1 + rng.poisson(2.0)
        spell = k % 7
        txt = ("%.1f" % c if spell < 3 else "%d" % c if spell == 3 else "%.1e" % c if spell == 4 else
               "%dE0" % c if spell == 5 else repr(c + rng.rand()) + "1")   # the last: 17 or more digits
        lines.append("%d\t%d\t%s\n" % (p * res, q * res, txt))
    norm = rng.choice([0.5, 1.0, 2.0], n_bins)   # few distinct products: values tie across bins
    norm[rng.random_sample(n_bins) < 0.1] = np.nan
    norm[rng.random_sample(n_bins) < 0.1] = 0.0
    norm_txt = "".join("NaN\n" if np.isnan(x) else "%s\n" % repr(float(x)) for x in norm)
    return "".join(lines), norm_txt, bed, res


def main():
    from chromegcn_amd import hic
    step7 = load_step7()
    rng = np.random.RandomState(20240611)
    raw, norm_txt, bed, res = make_fixture(rng)
    out = {"raw": np.frombuffer(raw.encode(), np.uint8), "norm": np.frombuffer(norm_txt.encode(), np.uint8),
           "bed": np.frombuffer(bed.encode(), np.uint8), "chrom": np.array("chrT"), "res": np.int64(res)}
    ties = 0
    with tempfile.TemporaryDirectory() as tmp:
        paths = {k: os.path.join(tmp, k) for k in ("chrT_1kb.RAWobserved", "chrT_1kb.KRnorm", "windows.bed")}
        for p, txt in zip(paths.values(), (raw, norm_txt, bed)):
            with open(p, "w", newline="") as f:
                f.write(txt)
        args = types.SimpleNamespace(chroms=["chrT", "chrU"], resolution=str(res // 1000), norm="KR")
        bin_dict = step7.create_bin_dict(args, paths["windows.bed"])
        nv = step7.get_normalization_values(paths["chrT_1kb.KRnorm"], "chrT")
        ws = np.array(list(bin_dict["chrT"]), dtype=np.int32)
        p1, p2, cnt, _ = hic.parse_contacts_text_host(raw.encode())
        v = hic.survivor_values(p1, p2, cnt, np.array(nv), res, ws)[3]
        s = v.size
        for c, edges in enumerate(sorted({2 * (s // 2), 2 * (s // 3) + 1, 2 * (s // 5), 2 * s + 10, 2})):
            total_edges = int(edges / 2.)
            pairs = step7.get_contact_edge_pairs(args, paths["chrT_1kb.RAWobserved"], "chrT", nv, None, bin_dict, total_edges)
            assert len(pairs) == s, (len(pairs), s)
            adj = step7.create_adj_mat(bin_dict, "chrT", step7.get_top_contact_locs(pairs, total_edges))
            adj.sort_indices()
            tie = 0
            if 0 < total_edges < s:
                t = np.sort(v)[::-1][total_edges - 1]
                tie = int((v == t).sum() > total_edges - (v > t).sum())
            ties += tie
            out.update({"c%d_edges" % c: np.int64(edges), "c%d_indptr" % c: adj.indptr.astype(np.int32),
                        "c%d_indices" % c: adj.indices.astype(np.int32), "c%d_tie" % c: np.int64(tie)})
        out["n_cases"] = np.int64(c + 1)
        out["n_windows"] = np.int64(len(bin_dict["chrT"]))
    assert ties >= 2, "no case has a tie straddling the threshold"
    path = os.path.join(HERE, "g10_hic_text.npz")
    np.savez_compressed(path, **out)
    print("%s: %d cases, %d with a tie at the threshold, %d lines of text, %d bytes"
          % (path, c + 1, ties, raw.count("\n"), os.path.getsize(path)))


if __name__ == "__main__":
    main()
