"""Times the label statistics on the GPU (chromegcn_amd.labelstats, csrc/cgcn_labelstats.hip) against their numpy / scipy
restatement on the same machine; fails without a GPU.

Two sizes, C = 103 labels, targets Bernoulli(0.05), the package's synthetic graphs (chromegcn_amd.synth: 250 000 uniform pairs
per chromosome, as 'hic' ChromGraphs already on the device):
  chr21    one chromosome, 5 776 windows
  genome   the 22 chromosomes of the synthetic genome, pooled with label_stats_split
Per size:
  device_ms   device time of label_stats / label_stats_split, graphs and targets resident (the packing, the window pass and
              the graph pass of every chromosome, the zeroing memsets): --reps samples, each a pair of device events around
              --calls back-to-back calls, after a warm call
  host_s      wall time of label_stats_host / label_stats_split_host on numpy targets and HostCSR graphs, best of --host-reps
  equal       the device integers equal the host's (checked once, outside the timing)
Appends one JSON line per size to --out (default profiles/labelstats_bench.jsonl) and prints it."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from chromegcn_amd import graph as G  # noqa: E402
from chromegcn_amd import labelstats, synth  # noqa: E402

FIELDS = ("label_count", "labels_hist", "cooccurrence", "n_entries", "degree_sum", "contact_pairs")


def timed(fn, reps, calls):
    """ms per call by device events: `reps` samples of `calls` back-to-back calls, after a warm call"""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(round(a.elapsed_time(b) / calls, 4))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="chr21,genome")
    ap.add_argument("--labels", type=int, default=synth.N_LABELS)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "labelstats_bench.jsonl"))
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/labelstats_bench.py needs a GPU")
    dev = torch.device("cuda")
    for size in opt.sizes.split(","):
        chroms = ["chr21"] if size == "chr21" else list(synth.HG19_LEN)[:22]
        hosts, targets = [], []
        for c in chroms:
            n = synth.chrom_nodes(c)
            hosts.append(G.normalize_graph("hic", synth.contact_graph(n, synth.PAIRS_PER_CHROM, synth.chrom_seed(c)), n))
            rng = np.random.RandomState(1000 + synth.chrom_seed(c))
            targets.append((rng.rand(n, opt.labels) < 0.05).astype(np.float32))
        graphs = [G.upload(h, dev) for h in hosts]
        tdev = [torch.from_numpy(t).to(dev) for t in targets]
        run = (lambda: labelstats.label_stats(tdev[0], graphs[0])) if len(chroms) == 1 else \
            (lambda: labelstats.label_stats_split(tdev, graphs))
        line = {"size": size, "chromosomes": len(chroms), "n": int(sum(t.shape[0] for t in targets)), "C": opt.labels,
                "stored_entries": int(sum(h.nnz for h in hosts)), "reps": opt.reps, "calls_per_sample": opt.calls}
        line["device_ms"] = timed(run, opt.reps, opt.calls)
        best, want = None, None
        for _ in range(opt.host_reps):
            t0 = time.perf_counter()
            want = labelstats.label_stats_split_host(targets, hosts)
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        line["host_s"] = round(best, 3)
        got = run().host()
        line["equal"] = bool(all(np.array_equal(getattr(got, k), getattr(want, k)) for k in FIELDS))
        print(json.dumps(line), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
        with open(opt.out, "a") as f:
            f.write(json.dumps(line) + "\n")
        del graphs, tdev


if __name__ == "__main__":
    main()
