"""Class-embedding maps (scripts/visualize.py:148-188) on the GPU: checkpoint, features and graphs in; the hidden states of the
single-label windows, their labels and one t-SNE embedding per perplexity out.  It plots nothing.

The inputs are those of `python -m chromegcn_amd.train`: -feat_dir (chrom_feature_dict_<split>.pt) and -graph_root (the graph
pickles) or -hic_contacts, or -synthetic; -load_gcn is the ChromeGCN checkpoint.  Written to --out:
    z.npy [m, d] float32    hidden state of every kept window (both strands averaged), label order then window order
    labels.npy [m] int64    its label;  rows.npy [m] int64: its row in the concatenation of the split's chromosomes
    embedding_p<perplexity>.npy [m, 2] float32, and summary.json (KL, iterations and seconds per perplexity)
The reference's run is --perplexities 5,10,...,65 --max-iter 3000 --patience 500 with at least 200 windows per label."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import chromegcn_amd as C  # noqa: E402
from chromegcn_amd import train  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("-feat_dir", type=str, default=None)
    ap.add_argument("-graph_root", type=str, default=None)
    ap.add_argument("-hicsize", type=str, default="500000")
    ap.add_argument("-hicnorm", type=str, default="SQRTVC")
    ap.add_argument("-hic_contacts", type=str, default=None, metavar="DIR")
    ap.add_argument("-hic_upsample", action="store_true")
    ap.add_argument("-window_size", type=int, default=1000)
    ap.add_argument("-adj_type", type=str, default="hic", choices=["constant", "hic", "both", "none"])
    ap.add_argument("-gcn_layers", type=int, default=2)
    ap.add_argument("-load_gcn", type=str, default=None, help="ChromeGCN checkpoint (without one: a freshly initialised model)")
    ap.add_argument("-synthetic", action="store_true")
    ap.add_argument("-synthetic_chroms", type=str, default="chr21,chr8")
    ap.add_argument("-gpu_id", type=int, default=0)
    ap.add_argument("--split", default="test", choices=["train", "valid", "test"])
    ap.add_argument("--labels", default=None, help="comma-separated label indices to keep (default: all)")
    ap.add_argument("--min-count", type=int, default=200)
    ap.add_argument("--perplexities", default="5,10,15,20,25,30,35,40,45,50,55,60,65")
    ap.add_argument("--max-iter", type=int, default=3000)
    ap.add_argument("--patience", type=int, default=500)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", required=True)
    opt = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("tools/class_map.py needs a GPU (the HIP path has no CPU fallback)")
    torch.cuda.set_device(opt.gpu_id)
    dev = torch.device("cuda", opt.gpu_id)
    data, graphs = train.load_inputs(opt)
    chroms = data[opt.split]
    if not chroms:
        raise SystemExit("no chromosome in the %s split" % opt.split)
    first = next(iter(chroms.values()))
    d, n_class = first["forward"].shape[1], first["target"].shape[1]
    model = C.ChromeGCN(d, d, n_class, 0.0, True, opt.gcn_layers)
    if opt.load_gcn:
        model.load_state_dict(torch.load(opt.load_gcn, map_location="cpu", weights_only=False)["model"])
    model.to(dev).eval()
    xf, xr, adj, tg = [], [], [], []
    for name, f in chroms.items():
        n = f["forward"].shape[0]
        g = graphs[opt.split]
        adj.append(g[name] if isinstance(g, dict) and isinstance(g.get(name), C.ChromGraph)
                   else C.process_graph(opt.adj_type, g, n, name, device=dev))
        xf.append(f["forward"].float().to(dev))
        xr.append(f["backward"].float().to(dev))
        tg.append(f["target"].to(dev))
    labels = None if opt.labels is None else [int(c) for c in opt.labels.split(",")]
    z, lab, rows = C.class_embeddings(model, xf, xr, adj, tg, labels=labels, min_count=opt.min_count)
    if z.shape[0] < 2:
        raise SystemExit("fewer than two single-label windows pass --min-count %d" % opt.min_count)
    os.makedirs(opt.out, exist_ok=True)
    np.save(os.path.join(opt.out, "z.npy"), z.cpu().numpy())
    np.save(os.path.join(opt.out, "labels.npy"), lab.cpu().numpy())
    np.save(os.path.join(opt.out, "rows.npy"), rows.cpu().numpy())
    print("%d windows of %d labels, d = %d" % (z.shape[0], len(torch.unique(lab)), z.shape[1]), flush=True)
    aff = C.TsneAffinities(z)
    summary = []
    for p in (float(s) for s in opt.perplexities.split(",")):
        t0 = time.perf_counter()
        Y, info = C.tsne_embed(aff, perplexity=p, max_iter=opt.max_iter, n_iter_without_progress=opt.patience, seed=opt.seed)
        y = Y.cpu().numpy()
        summary.append({"perplexity": p, "kl_divergence": info["kl_divergence"], "iterations": info["n_iter"] + 1,
                        "seconds": round(time.perf_counter() - t0, 3)})
        np.save(os.path.join(opt.out, "embedding_p%g.npy" % p), y)
        print(json.dumps(summary[-1]), flush=True)
    with open(os.path.join(opt.out, "summary.json"), "w") as f:
        json.dump({"windows": int(z.shape[0]), "d": int(z.shape[1]), "min_count": opt.min_count, "runs": summary}, f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1:])
