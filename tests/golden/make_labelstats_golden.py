"""Writes tests/golden/g14_labelstats.npz: the fixture of tests/test_labelstats_host.py -- what the reference's own
summarize_data (utils/util_methods.py:24-74) prints, the correlation matrix it forms (:48), and the label weights of
scripts/analyze_results.py:246-264, on a small seeded data set of 3 chromosomes, 300 windows and 12 labels.

    targets   uint8 [300, 12]     the label matrix, the chromosomes one after the other
    lengths   int64 [3]           rows per chromosome; chromosomes 0 and 1 are the train split, chromosome 2 the valid split
    rowptr_i, col_i, val_i        chromosome i's raw Hi-C matrix as CSR (symmetric, no diagonal, values 1 and 2)
    summary   fp64 [6]            the six numbers summarize_data prints for train + valid, in its order (mean, median, max
                                  labels per sample; mean, median, max samples per label), parsed from its output: torch prints
                                  four decimals
    pearson   fp64 [12, 12]       np.corrcoef as that function forms it: of the float32 TRAIN label matrix, transposed
    label_neighbor_count, label_count, label_weights   fp64 [12]  the float32 results of the get_label_weights loop over the
                                  three chromosomes
summarize_data is the reference's own function, imported and run under contextlib.redirect_stdout; its input is the data dict
it expects (index lists that count the four vocabulary entries in front, which its [:, 4:] cut removes again).
scripts/analyze_results.py cannot be imported (it parses arguments and loads files from absolute paths at import time), so
its loop (:246-264) is restated below: per chromosome the dense matrix with values above 1 set to 1 (:254-256), per window the
row sum added to the neighbour count, and 1 to the count, of every label the window carries (:258-262), then the quotient (:264).
Data only.

Run from the repository root where the reference is mounted: CHROMEGCN_REFERENCE=<its root> python
tests/golden/make_labelstats_golden.py"""
import contextlib
import io
import os
import re
import sys

import numpy as np
import scipy.sparse as sp
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
LENGTHS = (110, 100, 90)
C = 12
VOCAB = 4   # entries of data['dict']['tgt'] in front of the labels (util_methods.py:46)


def make_inputs():
    rng = np.random.RandomState(14)
    n = sum(LENGTHS)
    rates = np.linspace(0.03, 0.45, C)
    targets = (rng.rand(n, C) < rates[None, :]).astype(np.uint8)
    targets[17] = 1
    empty = np.flatnonzero(targets.sum(axis=1) == 0)       # the reference's index_fill_ refuses a window without a label
    targets[empty, rng.randint(0, C, empty.size)] = 1
    graphs = []
    for k in LENGTHS:
        r, c = rng.randint(0, k, 4 * k), rng.randint(0, k, 4 * k)
        keep = r != c
        a = sp.coo_matrix((np.ones(int(keep.sum())), (r[keep], c[keep])), shape=(k, k)).tocsr()
        a = sp.csr_matrix(a + a.T)          # duplicates and mutual pairs give values 2 and more: clipped by :256
        a.data = np.minimum(a.data, 2.0)
        a.sort_indices()
        graphs.append(a)
    return targets, graphs


def reference_label_weights(targets, graphs):
    """analyze_results.py:246-264 on the three chromosomes"""
    label_neighbor_count = torch.zeros(C)                                    # :247
    label_count = torch.zeros(C)                                             # :248
    at = 0
    for k, a in zip(LENGTHS, graphs):                                        # :250
        chrom_labels = torch.from_numpy(targets[at:at + k].astype(np.float32))   # :252
        dense = torch.from_numpy(a.toarray().astype(np.float32))             # :254-255
        dense[dense > 1] = 1                                                 # :256
        for idx in range(k):                                                 # :258
            nz = chrom_labels[idx].nonzero()                                 # :259
            label_neighbor_count[nz] += dense[idx].sum()                     # :260-261
            label_count[nz] += 1                                             # :262
        at += k
    return label_neighbor_count, label_count, label_neighbor_count.div(label_count)   # :264


def main():
    ref = os.environ.get("CHROMEGCN_REFERENCE")
    if not ref:
        raise SystemExit("set CHROMEGCN_REFERENCE to the root of the reference")
    sys.path.insert(0, ref)
    from utils.util_methods import summarize_data          # the reference

    targets, graphs = make_inputs()
    n_train = LENGTHS[0] + LENGTHS[1]
    as_lists = lambda rows: [(np.flatnonzero(r) + VOCAB).tolist() for r in rows]
    data = {"train": {"tgt": as_lists(targets[:n_train])}, "valid": {"tgt": as_lists(targets[n_train:])},
            "test": {"tgt": []}, "dict": {"tgt": {i: i for i in range(C + VOCAB)}}}
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        summarize_data(data)
    text = buf.getvalue()
    summary = []
    for key in ("Mean Labels Per Sample", "Median Labels Per Sample", "Max Labels Per Sample", "Mean Samples Per Label",
                "Median Samples Per Label", "Max Samples Per Label"):
        m = re.search(re.escape(key) + r": tensor\(([-0-9.e+]+)\)", text)
        summary.append(float(m.group(1)))
    pearson = np.corrcoef(targets[:n_train].astype(np.float32).T)            # util_methods.py:46-48
    nbr, cnt, w = reference_label_weights(targets, graphs)
    out = {"targets": targets, "lengths": np.array(LENGTHS, np.int64), "summary": np.array(summary, np.float64),
           "pearson": pearson.astype(np.float64), "label_neighbor_count": nbr.double().numpy(),
           "label_count": cnt.double().numpy(), "label_weights": w.double().numpy()}
    for i, a in enumerate(graphs):
        out["rowptr_%d" % i], out["col_%d" % i] = a.indptr.astype(np.int32), a.indices.astype(np.int32)
        out["val_%d" % i] = a.data.astype(np.float32)
    print(text)
    path = os.path.join(ROOT, "tests", "golden", "g14_labelstats.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
