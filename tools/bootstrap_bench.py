"""The three stages of chromegcn_amd.bootstrap at evaluation size, one JSON line per (n, block): the sort, the weights and
the walk, each the median of --reps runs after a warm-up, device events around the stage's own launches (no host copy inside
the window); the walk also as element visits per second (B * C * n visits).  Scores come from a fixed generator: targets with
a per-label rate, logits = noise + a per-label shift on the positives, through the sigmoid.  For --host-reps replicates the
numpy restatement (weighted_sums_host) and scikit-learn with sample_weight (roc_auc_score, average_precision_score and the
area under precision_recall_curve) are timed on the same replicates of the first 8 labels on this machine's CPU and scaled to
B replicates of C labels: printed as measured, not as a claim.  The device sums of those replicates are compared with the restatement's ('equal').

    python tools/bootstrap_bench.py [--sizes 45000,250000] [--blocks 1,50] [--C 103] [--B 1000] [--reps 10] \\
        > profiles/bootstrap_bench.jsonl"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from chromegcn_amd import _lib  # noqa: E402
from chromegcn_amd import bootstrap as B  # noqa: E402


def generate(n, C, seed=0):
    rng = np.random.default_rng(seed)
    rate = rng.uniform(0.005, 0.2, C)
    shift = rng.uniform(0.5, 2.5, C)
    t = (rng.random((n, C)) < rate[None, :]).astype(np.float32)
    s = (1.0 / (1.0 + np.exp(-(rng.normal(size=(n, C)) - 2.0 + t * shift[None, :])))).astype(np.float32)
    return s, t


def _events(fn, reps):
    """median milliseconds of fn() over `reps` runs after one warm-up, by device events; and its last result"""
    ms = []
    for i in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        if i:
            ms.append(a.elapsed_time(b))
    return float(np.median(ms)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="45000,250000")
    ap.add_argument("--blocks", default="1,50")
    ap.add_argument("--C", type=int, default=103)
    ap.add_argument("--B", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bootstrap_bench.py needs a GPU")
    dev = torch.device("cuda:0")
    C, nb = args.C, args.B
    for n in (int(x) for x in args.sizes.split(",")):
        s, t = generate(n, C)
        p_d, t_d = torch.from_numpy(s).to(dev), torch.from_numpy(t).to(dev)
        sort_ms, srt = _events(lambda: B._sort(p_d, t_d), args.reps)
        for block in (int(x) for x in args.blocks.split(",")):
            row = {"n": n, "C": C, "B": nb, "block": block, "sort_ms": round(sort_ms, 3)}
            batch = min(B.batch_replicates(n), (nb + 63) // 64 * 64)
            row["batch"] = batch
            blk, off_dev, n_strata, draws = B._rule_setup(n, block, None, dev)
            out, flags = B._new_out(batch, C, dev)
            # one batch of weights and its walk, timed apart; a run of B replicates is ceil(B / batch) of each
            w_ms, tile = _events(lambda: B._rule_tile(n, 0, batch, off_dev, n_strata, blk, draws, 0, flags, dev), args.reps)
            q = ctypes.c_double(0.5)
            walk_ms, _ = _events(lambda: _lib.call("cgcn_bootstrap_sums", n=n, C=C, R=batch, order=srt.order, tile=tile,
                                                   fdr_cutoff=q, out=out), args.reps)
            scale = nb / batch
            row["weights_ms_per_batch"], row["walk_ms_per_batch"] = round(w_ms, 3), round(walk_ms, 3)
            row["weights_ms"], row["walk_ms"] = round(w_ms * scale, 3), round(walk_ms * scale, 3)
            row["walk_visits_per_s"] = float("%.4g" % (batch * C * n / (walk_ms * 1e-3)))
            row["max_weight"] = int(tile.max())
            t0 = time.perf_counter()
            res = B.bootstrap_metrics(p_d, t_d, n_boot=nb, block=block)
            row["bootstrap_metrics_s"] = round(time.perf_counter() - t0, 3)   # end to end, host statistics included
            row["meanAUC"] = [round(res.scalars["meanAUC"][k], 5) for k in ("point", "ci_low", "ci_high")]
            # the host side, for --host-reps replicates of the first 8 labels, scaled to B replicates of C labels
            hr, hc = args.host_reps, min(C, 8)
            if hr > 0:
                W = B.bootstrap_weights_host(n, hr, 0, block)
                t0 = time.perf_counter()
                want = B.weighted_sums_host(s[:, :hc], t[:, :hc], W)
                row["restatement_s_scaled"] = round((time.perf_counter() - t0) * (nb / hr) * (C / hc), 1)
                got = B._read(out, batch, C)
                row["equal"] = bool(all(np.array_equal(got[k][:hr, :hc], want[k]) for k in ("A", "P", "TOT", "F")) and all(
                    np.allclose(got[k][:hr, :hc], want[k], rtol=(n + 4) * 2.0 ** -52, atol=0) for k in ("S_ap", "S_pr")))
                from sklearn.metrics import auc, average_precision_score, precision_recall_curve, roc_auc_score
                t0 = time.perf_counter()
                for r in range(hr):   # the same replicates and labels, the three calls the restatement is tested against
                    for c in range(hc):
                        if 0 < t[:, c].sum() < n:
                            roc_auc_score(t[:, c], s[:, c], sample_weight=W[r])
                            average_precision_score(t[:, c], s[:, c], sample_weight=W[r])
                            auc(*precision_recall_curve(t[:, c], s[:, c], sample_weight=W[r])[1::-1])
                row["sklearn_s_scaled"] = round((time.perf_counter() - t0) * (nb / hr) * (C / hc), 1)
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
