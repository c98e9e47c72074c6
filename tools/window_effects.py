"""Variant effects through the Hi-C graph on the GPU (chromegcn_amd.window_effects): checkpoint, features, graphs and a file of
variants in; the reference and alternative probabilities of every reported window out.  It plots nothing.

The inputs are those of `python -m chromegcn_amd.train`: -feat_dir (chrom_feature_dict_<split>.pt) and -graph_root (the graph
pickles) or -hic_contacts, or -synthetic; -load_gcn is the ChromeGCN checkpoint.  --variants is an .npz with
    chrom [M] str        the chromosome of every variant (a key of the split's feature dict)
    window [M] int       its window (row of that chromosome's features)
    alt_f, alt_r [M, d]  the encoder's features of the alternative allele, forward and reverse-complement strand
Written to --out (.npz), rows in the order of the variants file:
    offsets [M + 1] int64, rows [total] int32 (the window of every reported row), ref, alt [total, C] float32
--scope own reports each variant's window alone; contacts adds the windows that have it as a Hi-C neighbour (windows two or
more hops away change too when the model has two layers or more; they are not reported)."""
import argparse
import os
import sys

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
    ap.add_argument("-hic_compute_norm", action="store_true")
    ap.add_argument("-hic_min_distance", type=int, default=0, metavar="BP")
    ap.add_argument("-hic_expected", action="store_true")
    ap.add_argument("-window_size", type=int, default=1000)
    ap.add_argument("-adj_type", type=str, default="hic", choices=["constant", "hic", "both", "none"])
    ap.add_argument("-gcn_layers", type=int, default=2)
    ap.add_argument("-load_gcn", type=str, default=None, help="ChromeGCN checkpoint (without one: a freshly initialised model)")
    ap.add_argument("-synthetic", action="store_true")
    ap.add_argument("-synthetic_chroms", type=str, default="chr21,chr8")
    ap.add_argument("-gpu_id", type=int, default=0)
    ap.add_argument("--split", default="test", choices=["train", "valid", "test"])
    ap.add_argument("--variants", required=True, help=".npz of chrom, window, alt_f, alt_r")
    ap.add_argument("--scope", default="contacts", choices=["own", "contacts"])
    ap.add_argument("--route", default="auto", choices=["auto", "restricted", "composed"])
    ap.add_argument("--out", required=True)
    opt = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("tools/window_effects.py needs a GPU (the HIP path has no CPU fallback)")
    torch.cuda.set_device(opt.gpu_id)
    dev = torch.device("cuda", opt.gpu_id)
    v = np.load(opt.variants, allow_pickle=False)
    chrom_of, window = v["chrom"].astype(str), v["window"].astype(np.int64)
    alt_f, alt_r = torch.from_numpy(v["alt_f"]).float(), torch.from_numpy(v["alt_r"]).float()
    data, graphs = train.load_inputs(opt)
    chroms = data[opt.split]
    missing = sorted(set(chrom_of.tolist()) - set(chroms))
    if missing:
        raise SystemExit("chromosomes %s are not in the %s split" % (missing, opt.split))
    first = next(iter(chroms.values()))
    d, n_class = first["forward"].shape[1], first["target"].shape[1]
    model = C.ChromeGCN(d, d, n_class, 0.0, True, opt.gcn_layers)
    if opt.load_gcn:
        model.load_state_dict(torch.load(opt.load_gcn, map_location="cpu", weights_only=False)["model"])
    model.to(dev).eval()
    M = window.shape[0]
    parts = [None] * M                                     # (rows, ref, alt) per variant, in the file's order
    for name in dict.fromkeys(chrom_of.tolist()):
        f = chroms[name]
        n = f["forward"].shape[0]
        g = graphs[opt.split]
        adj = (g[name] if isinstance(g, dict) and isinstance(g.get(name), C.ChromGraph)
               else C.process_graph(opt.adj_type, g, n, name, device=dev))
        idx = np.flatnonzero(chrom_of == name)
        we = C.window_effects(model, f["forward"].float().to(dev), f["backward"].float().to(dev), adj, window[idx],
                              alt_f[idx].to(dev), alt_r[idx].to(dev), scope=opt.scope, route=opt.route)
        off = we.offsets.cpu().numpy()
        rows, ref, alt = we.rows.cpu().numpy(), we.ref.cpu().numpy(), we.alt.cpu().numpy()
        for k, m in enumerate(idx):
            parts[m] = (rows[off[k]:off[k + 1]], ref[off[k]:off[k + 1]], alt[off[k]:off[k + 1]])
        print("%s: %d variants, %d reported rows" % (name, idx.size, rows.shape[0]), flush=True)
    offsets = np.concatenate([[0], np.cumsum([p[0].shape[0] for p in parts])]).astype(np.int64)
    np.savez(opt.out, offsets=offsets, rows=np.concatenate([p[0] for p in parts]) if M else np.zeros(0, np.int32),
             ref=np.concatenate([p[1] for p in parts]) if M else np.zeros((0, n_class), np.float32),
             alt=np.concatenate([p[2] for p in parts]) if M else np.zeros((0, n_class), np.float32))


if __name__ == "__main__":
    main(sys.argv[1:])
