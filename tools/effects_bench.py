"""Window effects (chromegcn_amd.window_effects, chromegcn_amd.knockout_map) on the synthetic chr21-size and chr1-size
chromosomes (C = 103, d = 128, L = 2, weights of standard deviation 1 / sqrt(d) so that graph effects matter): restricted
against composed for M variants at random windows, both scopes, and the knock-out map of the whole chromosome.  One JSON line
per measurement; composed is built from the library's existing eval forward only, so it is the baseline.

    python tools/effects_bench.py [--chroms chr21,chr1] [--variants 1,64,4096] [--reps 3] [--knockout-composed chr21]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import chromegcn_amd as C  # noqa: E402
from chromegcn_amd import synth  # noqa: E402


def _time(fn, reps):
    ts = []
    for _ in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts[1:] or ts)), out          # reps = 0: the one run, cold


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chroms", default="chr21,chr1")
    ap.add_argument("--variants", default="1,64,4096")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--knockout-composed", default="chr21", help="chromosomes whose knock-out map is also timed composed")
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
                getattr(model, "GC%d" % k).weight.copy_(torch.randn(d, d) / np.sqrt(d))
                getattr(model, "W%d" % k).weight.copy_(torch.randn(1, d) / np.sqrt(d))
            model.out.weight.copy_(torch.randn(c, d) / np.sqrt(d))
        model.to(dev).eval()
        graph = C.process_graph("hic", {chrom: hic}, n, chrom, device=dev)
        x_f, x_r = feats["forward"].to(dev), feats["backward"].to(dev)
        rng = np.random.RandomState(1)
        for m in (int(v) for v in args.variants.split(",") if v):
            win = rng.randint(0, n, m)
            w = torch.from_numpy(win).to(dev)
            alt_f, alt_r = x_f[w] + torch.randn(m, d, device=dev), x_r[w] + torch.randn(m, d, device=dev)
            for scope in ("own", "contacts"):
                row = {"chrom": chrom, "n": n, "nnz": graph.nnz, "C": c, "d": d, "M": m, "scope": scope}
                res = {}
                for route in ("restricted", "composed"):
                    reps = args.reps if route == "restricted" or m <= 64 else 1
                    row[route + "_ms"], res[route] = _time(
                        lambda: C.window_effects(model, x_f, x_r, graph, win, alt_f, alt_r, scope=scope, route=route), reps)
                    row[route + "_ms"] = round(row[route + "_ms"], 3)
                row["rows"] = int(res["restricted"].rows.numel())
                row["composed_over_restricted"] = round(row["composed_ms"] / row["restricted_ms"], 2)
                row["routes_apart"] = float((res["restricted"].alt - res["composed"].alt).abs().max())
                row["max_effect"] = float((res["restricted"].alt - res["restricted"].ref).abs().max())
                print(json.dumps(row), flush=True)
                del res
        row = {"chrom": chrom, "n": n, "nnz": graph.nnz, "C": c, "d": d, "knockout_map": True}
        row["restricted_ms"], km = _time(lambda: C.knockout_map(model, x_f, x_r, graph), 1)
        row["restricted_ms"] = round(row["restricted_ms"], 3)
        row["max_entry"] = float(km.max())
        if chrom in args.knockout_composed.split(","):
            row["composed_ms"], kc = _time(lambda: C.knockout_map(model, x_f, x_r, graph, route="composed"), 0)
            row["composed_ms"] = round(row["composed_ms"], 3)
            row["composed_over_restricted"] = round(row["composed_ms"] / row["restricted_ms"], 2)
            row["routes_apart"] = float((km - kc).abs().max())
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
