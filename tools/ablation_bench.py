"""Label-pair edge ablation (chromegcn_amd.label_pair_ablation) on the synthetic chr21-size and chr1-size chromosomes
(C = 103, d = 128, L = 2, GC weights scaled so that ablations matter): full C x C matrix per route, one JSON line each with
the total ms, the us per pair, the pair count and the removed stored entries.

    python tools/ablation_bench.py [--chroms chr21,chr1] [--routes restricted,composed] [--reps 3]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import chromegcn_amd as C  # noqa: E402
from chromegcn_amd import graph as G, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chroms", default="chr21,chr1")
    ap.add_argument("--routes", default="restricted,composed")
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for chrom in args.chroms.split(","):
        feats, hic = synth.synthetic_chromosome(chrom)
        n, d = feats["forward"].shape
        c = feats["target"].shape[1]
        torch.manual_seed(0)
        model = C.ChromeGCN(d, d, c, 0.0, True, 2)
        with torch.no_grad():
            for k in (1, 2):
                getattr(model, "GC%d" % k).weight.copy_(torch.randn(d, d) / np.sqrt(d) * 1.5)
            model.out.weight.mul_(40.0)
        model.to(dev).eval()
        graph = C.process_graph("hic", {chrom: hic}, n, chrom, device=dev)
        x_f, x_r, tg = feats["forward"].to(dev), feats["backward"].to(dev), feats["target"].to(dev)
        # removed stored entries over all pairs (i != j, both label sets non-empty): sum_ij (T^T Ahat T)_ij
        h = G.to_host(graph)
        t = sp.csr_matrix(feats["target"].numpy() != 0, dtype=np.float64)
        rem = (t.T @ (h.ahat().astype(np.float64) @ t)).toarray()
        cnt = np.asarray(t.sum(0)).ravel()
        ok = (cnt[:, None] > 0) & (cnt[None, :] > 0) & ~np.eye(c, dtype=bool)
        pairs, removed = int(ok.sum()), int(rem[ok].sum())
        for route in args.routes.split(","):
            label_pair_ablation_timed = []
            for _ in range(args.reps + 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                m = C.label_pair_ablation(model, x_f, x_r, graph, tg, route=route)
                torch.cuda.synchronize()
                label_pair_ablation_timed.append(time.perf_counter() - t0)
            ms = 1e3 * float(np.median(label_pair_ablation_timed[1:]))
            print(json.dumps({"chrom": chrom, "n": n, "nnz": graph.nnz, "C": c, "route": route, "total_ms": round(ms, 3),
                              "us_per_pair": round(1e3 * ms / max(pairs, 1), 3), "pairs": pairs,
                              "removed_entries": removed, "max_abs_M": float(torch.nan_to_num(m).abs().max())}), flush=True)


if __name__ == "__main__":
    main()
