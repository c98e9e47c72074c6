"""Null graphs (chromegcn_amd.null_graph) against their host restatement (null_graph_host: numpy, this machine's CPU) at
chr21 and chr1 size, for the three synthetic generators and the three models; then one replicate of null_graph_test at each
size split into generate / normalise / forward / metrics (C = 103, d = 128, L = 2).  One JSON line per measurement; the device
time is the median of --reps runs after a warm-up, wall clock around a synchronised region; the host time is one run.

    python tools/nullgraph_bench.py [--chroms chr21,chr1] [--kinds uniform,hic_like,hub] [--reps 5] > profiles/nullgraph_bench.jsonl"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import chromegcn_amd as C  # noqa: E402
from chromegcn_amd import graph as G  # noqa: E402
from chromegcn_amd import metrics, nullgraph, synth  # noqa: E402


def _time(fn, reps):
    ts = []
    for _ in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return round(1e3 * float(np.median(ts[1:] or ts)), 3), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chroms", default="chr21,chr1")
    ap.add_argument("--kinds", default="uniform,hic_like,hub")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for chrom in args.chroms.split(","):
        n = synth.chrom_nodes(chrom)
        for kind in args.kinds.split(","):
            a = synth.contact_graph(n, synth.PAIRS_PER_CHROM, synth.chrom_seed(chrom), kind)
            rp = torch.from_numpy(a.indptr.astype(np.int32)).to(dev)
            ci = torch.from_numpy(a.indices.astype(np.int32)).to(dev)
            for model in nullgraph.MODELS:
                row = {"chrom": chrom, "n": n, "kind": kind, "model": model, "edges": int(a.nnz // 2)}
                t0 = time.perf_counter()
                want, info = nullgraph.null_graph_host(a, model, 7, return_info=True)
                row["host_ms"] = round(1e3 * (time.perf_counter() - t0), 3)
                row["device_ms"], out = _time(lambda: nullgraph.null_graph((rp, ci), model, 7, device=dev), args.reps)
                got = nullgraph.info_from_sizes(out[2], nullgraph.DEFAULT_ROUNDS, model)
                nnz = int(out[2][0])
                row["equal"] = bool(got == info and np.array_equal(out[0].cpu().numpy(), want.indptr)
                                    and np.array_equal(out[1][:nnz].cpu().numpy(), want.indices))
                row["host_over_device"] = round(row["host_ms"] / row["device_ms"], 1)
                row.update({k: info[k] for k in ("tokens", "unplaced", "complemented_classes", "loops", "repeats", "rounds_used",
                                                 "edges_out")})
                print(json.dumps(row), flush=True)
        # one replicate of the test, step by step (the hic_like graph, the distance model)
        feats, _ = synth.synthetic_chromosome(chrom)
        a = synth.contact_graph(n, synth.PAIRS_PER_CHROM, synth.chrom_seed(chrom), "hic_like")
        d, c = feats["forward"].shape[1], feats["target"].shape[1]
        torch.manual_seed(0)
        net = C.ChromeGCN(d, d, c, 0.0, True, 2).to(dev).eval()
        x_fr = torch.stack([feats["forward"], feats["backward"]], 0).to(dev)
        target = feats["target"].to(dev)
        rp = torch.from_numpy(a.indptr.astype(np.int32)).to(dev)
        ci = torch.from_numpy(a.indices.astype(np.int32)).to(dev)
        row = {"chrom": chrom, "n": n, "kind": "hic_like", "model": "distance", "replicate": True, "C": c, "d": d}
        with torch.no_grad():
            row["generate_ms"], raw = _time(lambda: nullgraph.null_graph((rp, ci), "distance", 7, device=dev), args.reps)
            row["normalise_ms"], g = _time(lambda: G.normalize_device_csr("hic", n, raw[0], raw[1], None, dev), args.reps)
            row["forward_ms"], p = _time(lambda: nullgraph.strand_probs(net, x_fr, g), args.reps)
            row["metrics_ms"], _ = _time(lambda: metrics._metrics_raw(p, target, 0.5, nonneg=True), args.reps)
        t0 = time.perf_counter()
        nullgraph.null_graph_host(a, "distance", 7)
        row["generate_host_ms"] = round(1e3 * (time.perf_counter() - t0), 3)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
