"""Times the thresholded multi-label counts on the GPU (chromegcn_amd.thresholds, csrc/cgcn_threshold.hip); fails without one.

Per size (default: the whole-genome training split, 242 908 x 103, and a chr21-size split, 5 776 x 103 -- the sizes of
profiles/curves_bench.jsonl; sigmoid of normal logits, sparse positives that lean to the high scores) and a grid of --grid
thresholds shared by all labels (27: the grid of scripts/analyze_results.py:63):
  counts_ms       device time of threshold_counts (the zeroing launch and the counting launch): --reps samples, each a pair
                  of device events around --calls back-to-back calls, after a warm call
  bytes_read      what the call has to read: probs and targets once, the thresholds ([T, C] fp32)
  gbps            bytes_read over the median of counts_ms
  stream_floor_ms bytes_read over 6.3 TB/s, the achievable HBM rate
  passes          cgcn_debug_threshold_route: 1 = every histogram in LDS, the rows streamed once
  metrics_ms      metrics.multilabel_metrics on the same tensors in the same run (the sort-based ranking metrics), same clock
  host_s          wall time of threshold_metrics_host (numpy) on the same arrays, the device-to-host copy not included
Appends one JSON line per size to --out (default profiles/threshold_bench.jsonl) and prints it."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from chromegcn_amd import _lib, metrics, thresholds  # noqa: E402
from tools.thresholds import REFERENCE_GRID  # noqa: E402

HBM_BYTES_PER_S = 6.3e12


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
    ap.add_argument("--sizes", default="242908x103,5776x103")
    ap.add_argument("--grid", type=int, default=27, help="number of thresholds (27: the reference's grid)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--host", type=int, default=1, help="0: skip the numpy restatement")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "threshold_bench.jsonl"))
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/threshold_bench.py needs a GPU")
    dev = torch.device("cuda")
    T = opt.grid
    grid = np.asarray(REFERENCE_GRID if T == 27 else np.linspace(0.0, 1.0, T + 2)[1:-1], dtype=np.float32)
    for size in opt.sizes.split(","):
        n, C = (int(v) for v in size.split("x"))
        g = torch.Generator(device=dev).manual_seed(n + C)
        logits = torch.randn(n, C, device=dev, generator=g)
        p = torch.sigmoid(logits)
        t = (torch.rand(n, C, device=dev, generator=g) < 0.1 * torch.sigmoid(logits + 0.5)).float()
        del logits
        line = {"n": n, "C": C, "T": T, "reps": opt.reps, "calls_per_sample": opt.calls,
                "passes": sum(_lib.query("cgcn_debug_threshold_route", n=n, C=C, T=min(64, T - t0)) for t0 in range(0, T, 64)),
                "bytes_read": 2 * n * C * 4 + T * C * 4}
        line["counts_ms"] = timed(lambda: thresholds.threshold_counts(p, t, grid), opt.reps, opt.calls)
        med = statistics.median(line["counts_ms"])
        line["gbps"] = round(line["bytes_read"] / (med * 1e-3) / 1e9, 1)
        line["stream_floor_ms"] = round(line["bytes_read"] / HBM_BYTES_PER_S * 1e3, 4)
        line["metrics_ms"] = timed(lambda: metrics.multilabel_metrics(p, t), opt.reps, max(1, opt.calls // 4))
        if opt.host:
            ph, th_ = p.cpu().numpy(), t.cpu().numpy()
            t0 = time.perf_counter()
            thresholds.threshold_metrics_host(ph, th_, grid)
            line["host_s"] = round(time.perf_counter() - t0, 3)
        print(json.dumps(line), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
        with open(opt.out, "a") as f:
            f.write(json.dumps(line) + "\n")
        del p, t


if __name__ == "__main__":
    main()
