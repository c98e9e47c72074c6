"""The per-label table behind the reference's figure of per-label improvement against average Hi-C degree
(scripts/analyze_results.py:97-168, 226-266): two saved prediction sets of the same windows, the chromosomes' graphs and the
number of windows of every chromosome give, per label, both models' metric, the difference b - a and the label's average
degree, and over the labels the paired t-test and the regression of the difference on the degree.  It plots nothing.

--preds-a / --preds-b / --targets: [n, C] matrices, the chromosomes one after the other: .pt (a tensor or array saved with
    torch.save: the reference's epochs/best_test_preds_metrics.pt and best_test_targets_metrics.pt), .npy, or .npz (its
    only array, or the one named after '::', e.g. run.npz::test_preds).  a is the baseline (the CNN), b the GCN.
--lengths: JSON, {"chr3": 12345, ...} or [["chr3", 12345], ...] in the order of the rows.
--graphs: a pickle {chromosome: scipy sparse matrix} (data/7create_graph_new.py:197-202; the raw matrices: taken as they are).
--groups: JSON {"tfbs": [label indices], "hm": [...], "dnase": [...]}.
Written: --out, one .npz -- per metric m of auroc, aupr, recall_at_fdr: m_a, m_b [C], m_diff, m_kept, m_dropped, m_order and
the scalars m_t, m_p, m_slope, m_intercept, m_r, m_p_regress, m_stderr; average_degree [C]; every integer array of the pooled
LabelStats; contact_enrichment and pearson [C, C] -- and --csv, one line per label: label, windows, average_degree, then a, b
and diff of every metric.
--bootstrap B (with --bootstrap-block L): B block-bootstrap replicates over the windows, the chromosomes as strata and both
models under the same weights (chromegcn_amd.bootstrap.bootstrap_compare): m_diff_ci_low, m_diff_ci_high and m_diff_p [C] join
the .npz, and diff_lo, diff_hi (the 95 % interval of b - a) and p (two-sided) the metric's csv columns."""
import argparse
import csv
import json
import os
import pickle
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from chromegcn_amd import labelstats, metrics  # noqa: E402
from chromegcn_amd.compare import compare_labels  # noqa: E402

METRICS = ("auroc", "aupr", "recall_at_fdr")


def load_matrix(spec):
    path, _, key = spec.partition("::")
    if path.endswith(".npy"):
        a = np.load(path, allow_pickle=False)
    elif path.endswith(".npz"):
        z = np.load(path, allow_pickle=False)
        if not key and len(z.files) != 1:
            raise SystemExit("%s holds %s: name one as %s::<array>" % (path, z.files, path))
        a = z[key or z.files[0]]
    else:
        a = torch.load(path, map_location="cpu", weights_only=False)
    a = torch.as_tensor(a)
    if a.dim() != 2:
        raise SystemExit("%s: expected a matrix [n, C], found shape %s" % (spec, tuple(a.shape)))
    return a.float()


def load_lengths(path):
    with open(path) as f:
        d = json.load(f)
    items = list(d.items()) if isinstance(d, dict) else [tuple(x) for x in d]
    return [str(c) for c, _ in items], [int(k) for _, k in items]


def load_graphs(path, names):
    with open(path, "rb") as f:
        graphs = pickle.load(f)
    missing = [c for c in names if c not in graphs]
    if missing:
        raise SystemExit("%s has no graph for %s" % (path, ", ".join(missing)))
    return {c: graphs[c] for c in names}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--preds-a", required=True)
    ap.add_argument("--preds-b", required=True)
    ap.add_argument("--targets", required=True)
    ap.add_argument("--lengths", required=True)
    ap.add_argument("--graphs", required=True)
    ap.add_argument("--groups", default=None)
    ap.add_argument("--bootstrap", type=int, default=0, metavar="B")
    ap.add_argument("--bootstrap-block", type=int, default=50, metavar="L")
    ap.add_argument("--gpu-id", type=int, default=0)
    ap.add_argument("--out", required=True)
    ap.add_argument("--csv", required=True)
    opt = ap.parse_args(argv)
    pa, pb, tg = load_matrix(opt.preds_a), load_matrix(opt.preds_b), load_matrix(opt.targets)
    if pa.shape != tg.shape or pb.shape != tg.shape:
        raise SystemExit("predictions %s, %s and targets %s differ in shape" % (tuple(pa.shape), tuple(pb.shape), tuple(tg.shape)))
    names, lengths = load_lengths(opt.lengths)
    if sum(lengths) != tg.shape[0]:
        raise SystemExit("the lengths sum to %d but there are %d rows" % (sum(lengths), tg.shape[0]))
    graphs = load_graphs(opt.graphs, names)
    groups = None
    if opt.groups:
        with open(opt.groups) as f:
            groups = json.load(f)
    if not torch.cuda.is_available():
        raise SystemExit("tools/analyze_results.py needs a GPU (the HIP path has no CPU fallback)")
    dev = torch.device("cuda", opt.gpu_id)
    torch.cuda.set_device(dev)
    t = tg.to(dev)
    bounds = np.concatenate([[0], np.cumsum(lengths)])
    stats = labelstats.label_stats_split({c: t[bounds[i]:bounds[i + 1]] for i, c in enumerate(names)}, graphs)
    degree = stats.average_degree()
    host = stats.host()
    out = {"average_degree": degree, "contact_enrichment": stats.contact_enrichment(), "pearson": stats.pearson(),
           "n_windows": np.int64(host.n_windows), "chromosomes": np.array(names)}
    for k in ("label_count", "labels_hist", "cooccurrence", "n_entries", "degree_sum", "contact_pairs"):
        out[k] = getattr(host, k)
    per = {}
    for tag, p in (("a", pa), ("b", pb)):
        per[tag] = {k: v.double().cpu().numpy() for k, v in metrics.multilabel_metrics(p.to(dev), t).items()}
    summary = {}
    for m in METRICS:
        r = compare_labels(per["a"][m], per["b"][m], degree, groups)
        out[m + "_a"], out[m + "_b"] = per["a"][m], per["b"][m]
        for k in ("diff", "kept", "dropped", "order"):
            out["%s_%s" % (m, k)] = r[k]
        for k in ("t", "p", "slope", "intercept", "r", "p_regress", "stderr"):
            out["%s_%s" % (m, k)] = np.float64(r[k])
        summary[m] = {k: r[k] for k in ("t", "p", "slope", "r")}
        if groups is not None:
            summary[m]["groups"] = r["groups"]
    boot = None
    if opt.bootstrap > 0:
        from chromegcn_amd.bootstrap import bootstrap_compare
        boot = bootstrap_compare(pb.to(dev), pa.to(dev), t, n_boot=opt.bootstrap, block=opt.bootstrap_block, lengths=lengths,
                                 label_groups=groups)   # differences are b - a
        for m in METRICS:
            out[m + "_diff_ci_low"], out[m + "_diff_ci_high"], out[m + "_diff_p"] = boot.ci_low[m], boot.ci_high[m], boot.p[m]
        summary["bootstrap"] = {k: {f: v[f] for f in ("diff", "ci_low", "ci_high", "p")} for k, v in boot.scalars.items()}
    cols = ("a", "b", "diff") + (("diff_lo", "diff_hi", "p") if boot is not None else ())
    for path in (opt.out, opt.csv):
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez(opt.out, **out)
    with open(opt.csv, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["label", "windows", "average_degree"] + ["%s_%s" % (m, k) for m in METRICS for k in cols])
        for c in range(tg.shape[1]):
            row = [c, int(host.label_count[c]), repr(float(degree[c]))]
            for m in METRICS:
                a, b = float(per["a"][m][c]), float(per["b"][m][c])
                row += [repr(a), repr(b), repr(b - a)]
                if boot is not None:
                    row += [repr(float(boot.ci_low[m][c])), repr(float(boot.ci_high[m][c])), repr(float(boot.p[m][c]))]
            w.writerow(row)
    print(json.dumps({"n": int(tg.shape[0]), "C": int(tg.shape[1]), "chromosomes": len(names), "out": opt.out, "csv": opt.csv,
                      "summary": summary}))


if __name__ == "__main__":
    main()
