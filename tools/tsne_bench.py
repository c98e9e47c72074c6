"""Times exact t-SNE on the GPU (chromegcn_amd.tsne, csrc/cgcn_tsne.hip); fails without one.

Per point count (default 5 000 and 20 000; d = 128, clustered synthetic z):
Every sample is a host clock around --calls (or --iters) back-to-back calls that end in a device synchronise, divided by
their number; --reps samples after a warm one.
  sqdist_ms           cgcn_tsne_sqdist;
  affinities_ms       per perplexity: the perplexity search (cgcn_tsne_affinities) and the symmetrisation;
  iteration_ms        one iteration (Z pass, total, gradient pass, update) with and without the KL, from a start that has
                      left the exaggeration stage;
  gradient_call_ms    one cgcn_tsne_gradient call: ALL THREE of its launches (Z pass, total, gradient pass), and
                      gradient_call_p_bytes_per_s = n * pitch * 4 bytes of P over that time, against the measured copy rate
                      of 6.29 TB/s.  The Z pass and the total are inside the time, so the figure is a lower bound of the
                      gradient pass's own rate, which this tool does not isolate;
  embed_s          one tsne_embed of --max-iter iterations end to end, and its final KL;
  sklearn_s        where scikit-learn imports, at the point counts of --sklearn-sizes: TSNE(n_components=2, perplexity=p) --
                   the reference's own Barnes-Hut call, scripts/visualize.py:176, with --max-iter iterations -- on this
                   machine's CPU for one perplexity.
Appends one JSON line per point count to --out (default profiles/tsne_bench.jsonl) and prints them."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from chromegcn_amd import tsne  # noqa: E402

COPY_BYTES_PER_S = 6.29e12


def clustered(n, d, k=12, seed=0):
    rng = np.random.RandomState(seed)
    centres = rng.standard_normal((k, d)) * 1.5
    return (centres[rng.randint(0, k, n)] + rng.standard_normal((n, d))).astype(np.float32)


def timed(fn, reps, calls=1):
    """ms per call: `reps` samples of `calls` back-to-back calls and one synchronise, after a warm call"""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3 / calls)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="5000,20000")
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--perplexities", default="5,30,65")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200, help="iterations per timed sample")
    ap.add_argument("--calls", type=int, default=20, help="sqdist / search / symmetrise calls per timed sample")
    ap.add_argument("--max-iter", type=int, default=1000)
    ap.add_argument("--sklearn-sizes", default="5000",
                    help="point counts at which scikit-learn's Barnes-Hut TSNE is timed on the host too (minutes each; '' = none)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "tsne_bench.jsonl"))
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/tsne_bench.py needs a GPU")
    dev = torch.device("cuda")
    perps = [float(p) for p in opt.perplexities.split(",")]
    for n in (int(s) for s in opt.sizes.split(",")):
        x = clustered(n, opt.d)
        z = torch.from_numpy(x).to(dev)
        sq_ms = timed(lambda: tsne.sqdist(z), opt.reps, opt.calls)
        aff = tsne.TsneAffinities(z)
        aff_ms = {}
        for p in perps:
            search = timed(lambda: tsne.affinities(aff.D, p), opt.reps, opt.calls)
            C, _ = tsne.affinities(aff.D, p)
            sym = timed(lambda: tsne.symmetrize(C, aff.ws, out=C), opt.reps, opt.calls)   # (repeated in place: the pass is timed)
            aff_ms["%g" % p] = {"search": [round(t, 3) for t in search], "symmetrize": [round(t, 3) for t in sym]}
            del C
        t0 = time.perf_counter()
        Y, info = tsne.tsne_embed(aff, perplexity=perps[len(perps) // 2], max_iter=opt.max_iter)
        torch.cuda.synchronize()
        embed_s = time.perf_counter() - t0
        P = aff.joint(perps[len(perps) // 2])
        grad, upd, gains = torch.empty_like(Y), torch.zeros_like(Y), torch.ones_like(Y)
        rec = torch.zeros(4, device=dev, dtype=torch.float64)
        lr = info["learning_rate"]

        def iterate(want, y):
            for _ in range(opt.iters):
                tsne.kl_gradient(P, y, 1.0, grad, want, aff.ws)
                tsne.update_step(y, upd, gains, grad, 0.8, lr, want, rec, aff.ws)
        it_ms = [t / opt.iters for t in timed(lambda: iterate(False, Y.clone()), opt.reps)]
        it_kl_ms = [t / opt.iters for t in timed(lambda: iterate(True, Y.clone()), opt.reps)]

        def gradients():
            for _ in range(opt.iters):
                tsne.kl_gradient(P, Y, 1.0, grad, False, aff.ws)
        call_ms = [t / opt.iters for t in timed(gradients, opt.reps)]
        p_bytes = n * tsne._pitch(n) * 4
        rate = p_bytes / (statistics.median(call_ms) * 1e-3)
        line = {"n": n, "d": opt.d, "sqdist_ms": [round(t, 3) for t in sq_ms], "affinities_ms": aff_ms,
                "iteration_ms": [round(t, 4) for t in it_ms], "iteration_with_kl_ms": [round(t, 4) for t in it_kl_ms],
                "gradient_call_ms": [round(t, 4) for t in call_ms], "p_bytes": p_bytes,
                "gradient_call_p_bytes_per_s": round(rate, -8),
                "gradient_call_over_copy_rate": round(rate / COPY_BYTES_PER_S, 3), "embed_s": round(embed_s, 3),
                "embed_iterations": info["n_iter"] + 1, "embed_kl": round(info["kl_divergence"], 5),
                "calls_per_sample": opt.calls, "iterations_per_sample": opt.iters}
        if n in [int(v) for v in opt.sklearn_sizes.split(",") if v]:
            try:
                from sklearn.manifold import TSNE
            except ImportError:
                TSNE = None
            if TSNE is not None:
                t0 = time.perf_counter()
                sk = TSNE(n_components=2, perplexity=perps[len(perps) // 2], max_iter=opt.max_iter).fit(x)
                line["sklearn_s"] = round(time.perf_counter() - t0, 2)
                line["sklearn_kl"] = round(float(sk.kl_divergence_), 5)
        print(json.dumps(line), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
        with open(opt.out, "a") as f:
            f.write(json.dumps(line) + "\n")
        del aff, P, z


if __name__ == "__main__":
    main()
