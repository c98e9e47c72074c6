"""The null-graph test on the GPU (chromegcn_amd.null_graph_test): does a trained ChromeGCN gain anything from the Hi-C
contacts being the real ones?  Checkpoint, features and graphs in; one .npz out.  It plots nothing.

The inputs are those of `python -m chromegcn_amd.train`: -feat_dir (chrom_feature_dict_<split>.pt) and -graph_root (the graph
pickles) or -hic_contacts (with -adj_type hic: a 'both' graph from a contact cache already holds the band, and the null graph
has to be drawn before it), or -synthetic; -load_gcn is the ChromeGCN checkpoint.  The chromosomes of --split are pooled like
an evaluation.  Written to --out (.npz), for every metric M of auroc, aupr, recall_at_fdr, average_precision:
    M_observed, M_null_mean, M_null_std, M_z, M_p [C] float64;  M_null [n_null, C] with --keep-null
and chroms [K] str, null_model, n_null, seed."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import chromegcn_amd as C  # noqa: E402
from chromegcn_amd import nullgraph, train  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("-feat_dir", type=str, default=None)
    ap.add_argument("-graph_root", type=str, default=None)
    ap.add_argument("-hicsize", type=str, default="500000")
    ap.add_argument("-hicnorm", type=str, default="SQRTVC")
    ap.add_argument("-hic_contacts", type=str, default=None, metavar="DIR")
    ap.add_argument("-hic_upsample", action="store_true")
    ap.add_argument("-hic_compute_norm", action="store_true")
    ap.add_argument("-hic_min_distance", type=int, default=0, metavar="BP")
    ap.add_argument("-hic_expected", action="store_true")
    ap.add_argument("-window_size", type=int, default=1000)
    ap.add_argument("-adj_type", type=str, default="hic", choices=["hic", "both"])
    ap.add_argument("-gcn_layers", type=int, default=2)
    ap.add_argument("-load_gcn", type=str, default=None, help="ChromeGCN checkpoint (without one: a freshly initialised model)")
    ap.add_argument("-synthetic", action="store_true")
    ap.add_argument("-synthetic_chroms", type=str, default="chr21,chr8")
    ap.add_argument("-gpu_id", type=int, default=0)
    ap.add_argument("--split", default="test", choices=["train", "valid", "test"])
    ap.add_argument("--null-model", default="distance", choices=list(nullgraph.MODELS))
    ap.add_argument("--n-null", type=int, default=100)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--keep-null", action="store_true")
    ap.add_argument("--out", required=True)
    opt = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("tools/null_test.py needs a GPU (the HIP path has no CPU fallback)")
    if opt.hic_contacts and opt.adj_type != "hic":
        raise SystemExit("-hic_contacts gives normalised graphs: the null graph of a 'both' graph needs the raw matrix")
    torch.cuda.set_device(opt.gpu_id)
    dev = torch.device("cuda", opt.gpu_id)
    opt.hic_null = None   # the real graphs: the test draws the null graphs itself
    data, graphs = train.load_inputs(opt)
    chroms = data[opt.split]
    if not chroms:
        raise SystemExit("the %s split is empty" % opt.split)
    first = next(iter(chroms.values()))
    d, n_class = first["forward"].shape[1], first["target"].shape[1]
    model = C.ChromeGCN(d, d, n_class, 0.0, True, opt.gcn_layers)
    if opt.load_gcn:
        model.load_state_dict(torch.load(opt.load_gcn, map_location="cpu", weights_only=False)["model"])
    model.to(dev).eval()
    names = list(chroms)
    res = C.null_graph_test(model, [chroms[c]["forward"].float().to(dev) for c in names],
                            [chroms[c]["backward"].float().to(dev) for c in names], [graphs[opt.split][c] for c in names],
                            [chroms[c]["target"].float().to(dev) for c in names], null_model=opt.null_model, n_null=opt.n_null,
                            seed=opt.seed, adj_type=opt.adj_type, keep_null=opt.keep_null)
    out = {"chroms": np.array(names), "null_model": np.array(opt.null_model), "n_null": np.array(opt.n_null),
           "seed": np.array(opt.seed)}
    for m in nullgraph.METRICS:
        for f in ("observed", "null_mean", "null_std", "z", "p"):
            out["%s_%s" % (m, f)] = getattr(res, f)[m]
        if res.null is not None:
            out["%s_null" % m] = res.null[m]
        ok = np.isfinite(res.observed[m])
        print("%-18s observed %.4f  null %.4f +- %.4f  labels with p <= 0.05: %d of %d" % (
            m, np.nanmean(res.observed[m]), np.nanmean(res.null_mean[m]), np.nanmean(res.null_std[m]),
            int((res.p[m][ok] <= 0.05).sum()), int(ok.sum())), flush=True)
    np.savez(opt.out, **out)


if __name__ == "__main__":
    main(sys.argv[1:])
