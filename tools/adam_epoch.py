#!/usr/bin/env python3
"""Train-epoch time of the synthetic GM12878-shaped genome (the 16 train chromosomes of tools/epoch_bench.py, d = 128,
two layers, dropout 0.2) with three optimizers:
    sgd         SGD(lr 0.25, momentum 0.9, wd 1e-6): the fused SGD step, the whole split as one HIP graph (bench.py's headline)
    adam_eager  Adam(betas (0.9, 0.98), lr 1e-3), the reference's default: a captured fwd+bwd graph per chromosome, then
                torch's own Adam step from the host
    adam_fused  Adam(..., fused=True): cgcn_adam_step inside the graphs, the whole split as one HIP graph
Each form runs in a child process of its own under a time limit; one JSON line per form, then a summary line.
Reporting tool, not part of the product."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = ("sgd", "adam_eager", "adam_fused")


def child(form, epochs, d, layers):
    sys.path.insert(0, ROOT)
    import torch
    import chromegcn_amd as C
    from chromegcn_amd import synth
    from chromegcn_amd.finetune import GCNStage
    dev = torch.device("cuda")
    torch.manual_seed(0)
    model = C.ChromeGCN(d, d, synth.N_LABELS, 0.2, True, layers).to(dev)
    if form == "sgd":
        opt = torch.optim.SGD(model.parameters(), lr=0.25, momentum=0.9, weight_decay=1e-6)
    else:
        opt = torch.optim.Adam(model.parameters(), betas=(0.9, 0.98), lr=1e-3, fused=(form == "adam_fused") or None)
    stage = GCNStage(model, opt, "hic", dev)
    names = [c for c in synth.HG19_LEN if synth.split_of(c) == "train"]
    for c in names:
        feats, hic = synth.synthetic_chromosome(c, d=d)
        stage.add_chromosome(c, feats, hic)
    times = []
    for e in range(epochs + 1):   # epoch 0 captures
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, _, loss = stage.run_split("train", names, to_cpu=False)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    kinds = sorted({k[1] for k in stage._graphs})
    print(json.dumps({"form": form, "train_epoch_ms_min": min(times[1:]) * 1e3,
                      "train_epoch_ms_median": statistics.median(times[1:]) * 1e3, "epochs": epochs,
                      "chromosomes": len(names), "windows": sum(stage.chroms[c].n for c in names), "graphs": kinds,
                      "fused_step": stage._fused, "last_loss": loss}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per form")
    ap.add_argument("--child", choices=FORMS, default=None)
    args = ap.parse_args()
    if args.child:
        child(args.child, args.epochs, args.d, args.layers)
        return
    res = {}
    for form in FORMS:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", form, "--epochs", str(args.epochs), "--d", str(args.d),
               "--layers", str(args.layers)]
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=args.timeout)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            raise SystemExit("adam_epoch: form %s exited with %d" % (form, r.returncode))
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
        print(line, flush=True)
        res[form] = json.loads(line)
    print(json.dumps({"summary": {f: round(res[f]["train_epoch_ms_min"], 3) for f in FORMS},
                      "fused_minus_sgd_ms": res["adam_fused"]["train_epoch_ms_min"] - res["sgd"]["train_epoch_ms_min"],
                      "eager_over_fused": res["adam_eager"]["train_epoch_ms_min"] / res["adam_fused"]["train_epoch_ms_min"]}))


if __name__ == "__main__":
    main()
