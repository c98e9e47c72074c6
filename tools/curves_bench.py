"""Times the per-label ROC / precision-recall curves and cutoffs on the GPU (chromegcn_amd.curves, the curve kernels of
csrc/cgcn_metrics.hip); fails without one.

Per size (default: the whole-genome training split, 242 908 x 103, and a chr21-size split, 5 776 x 103; sigmoid of normal
logits, 5 % positives that lean to the high scores): every sample is a host clock around --calls back-to-back calls that end
in a device synchronise, divided by their number; --reps samples after a warm call.
  roc_ms, roc_keep_ms   roc_curves with and without drop_intermediate: cgcn_curves_count, the read of offsets[C], the
                        allocation of the outputs, cgcn_curves_fill and the float64 ratios
  roc_points_ms         the same without the ratios: count, the read, fill
  pr_ms, pr_points_ms   pr_curves, and the same without the ratios
  cutoffs_ms            cgcn_curves_cutoff alone, on the filled ROC curves
  metrics_ms            metrics.multilabel_metrics on the same tensors: the same pack and sort, then four scalars per label --
                        the difference to roc_points_ms is the price of writing the curves out
  sklearn_s             where scikit-learn imports: roc_curve + precision_recall_curve per label on the host (the reference's
                        loop, utils/metrics.py:255-303), one pass, the device-to-host copy of both matrices included
  *_bytes               algorithmic bytes: sort = pack + 4 radix passes; curves = the two scans of
                        the sorted keys, the points written and read, the outputs
Appends one JSON line per size to --out (default profiles/curves_bench.jsonl) and prints it."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from chromegcn_amd import curves, metrics  # noqa: E402


def timed(fn, reps, calls):
    """ms per call: `reps` samples of `calls` back-to-back calls and one synchronise, after a warm call"""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        out.append(round((time.perf_counter() - t0) * 1e3 / calls, 4))
    return out


def algorithmic_bytes(n, C, points, kept):
    """bytes the launches have to move, from the shapes: items = n C elements, `points` curve points, `kept` output points"""
    items = n * C
    sort = items * 12 + 4 * items * 12          # pack: two fp32 reads, one key write; a radix pass: two reads, one write
    scan = 2 * items * 4 + points * 8           # k_curves_runs and k_curves_points read the keys; the points (position, tps) out
    keep = 2 * points * 8                       # k_curves_keep_count and k_curves_fill read them
    fill = kept * 12 + kept * 4                 # tps, fps, thresholds out; the key behind every threshold
    return {"sort_bytes": sort, "curves_bytes": scan + keep + fill}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="242908x103,5776x103")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--sklearn", type=int, default=1, help="0: skip the host loop")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "curves_bench.jsonl"))
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/curves_bench.py needs a GPU")
    dev = torch.device("cuda")
    for size in opt.sizes.split(","):
        n, C = (int(v) for v in size.split("x"))
        g = torch.Generator(device=dev).manual_seed(n + C)
        logits = torch.randn(n, C, device=dev, generator=g)
        p = torch.sigmoid(logits)
        t = (torch.rand(n, C, device=dev, generator=g) < 0.1 * torch.sigmoid(logits + 0.5)).float()
        roc = curves.roc_curves(p, t)
        keep = curves.roc_curves(p, t, drop_intermediate=False)
        line = {"n": n, "C": C, "points": int(keep.tps.numel()) - C, "roc_kept_points": int(roc.tps.numel()),
                "reps": opt.reps, "calls_per_sample": opt.calls}
        line.update(algorithmic_bytes(n, C, line["points"], line["roc_kept_points"]))
        line["roc_ms"] = timed(lambda: curves.roc_curves(p, t), opt.reps, opt.calls)
        line["roc_keep_ms"] = timed(lambda: curves.roc_curves(p, t, drop_intermediate=False), opt.reps, opt.calls)
        line["roc_points_ms"] = timed(lambda: curves._curves_raw("roc", p, t, True), opt.reps, opt.calls)
        line["pr_ms"] = timed(lambda: curves.pr_curves(p, t), opt.reps, opt.calls)
        line["pr_points_ms"] = timed(lambda: curves._curves_raw("pr", p, t, False), opt.reps, opt.calls)
        line["cutoffs_ms"] = timed(lambda: curves.cutoffs_of(roc), opt.reps, opt.calls)
        line["metrics_ms"] = timed(lambda: metrics.multilabel_metrics(p, t), opt.reps, opt.calls)
        if opt.sklearn:
            try:
                from sklearn.metrics import precision_recall_curve, roc_curve
            except ImportError:
                roc_curve = None
            if roc_curve is not None:
                t0 = time.perf_counter()
                ph, th = p.cpu().numpy(), t.cpu().numpy()
                for c in range(C):
                    roc_curve(th[:, c], ph[:, c])
                    precision_recall_curve(th[:, c], ph[:, c])
                line["sklearn_s"] = round(time.perf_counter() - t0, 3)
        print(json.dumps(line), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
        with open(opt.out, "a") as f:
            f.write(json.dumps(line) + "\n")
        del p, t, roc, keep, logits


if __name__ == "__main__":
    main()
