"""Per-workgroup timestamps of the feature-sliced gathers (tuning tool): where a launch's time goes between workgroup start,
the descriptor chain (order -> rowptr -> col), the first table line, the walk and the store -- launched alone on a hot L2 and
inside the replayed genome epoch.  Needs a -DSLICED_TIMING build loaded through CHROMEGCN_LIB:
  CGCN_EXTRA_FLAGS="-DSLICED_TIMING" python -c "from chromegcn_amd import _build; _build.build_library(out='variants/libcgcn_slt.so')"
  CHROMEGCN_LIB=$PWD/variants/libcgcn_slt.so python tools/sliced_stamps.py [--label TEXT] [chromosome ...]
(-DSLICED_TIMING -DSLICED_WARM_WGS=0: the same table without the first-touch warming.)
Default chromosomes: the smallest, a mean-size and the largest of the train split.

Per launch: grid, span = last store - first start, and for the workgroups that start with the launch (within 1 us of its first
start: the first round) and for the later ones the medians of
  chain  = start -> order / rowptr returned      col   = -> first chunk of column indices returned
  line   = -> that chunk's table lines returned   walk  = -> walk done      store = -> store done
Every stamp waits for the memory operations in flight, so the first chunk is serialised: a timing build is slower than the
product and its differences, not its totals, are the result.  In the epoch the table holds the LAST launch that matches
(n, kernel): for k_aggregate_sliced the second layer's, for k_bwd_sliced the first layer's (which carries the riders and the
next chromosome's aggregation); --grid G selects the launch of G workgroups instead."""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import chromegcn_amd as C
from chromegcn_amd import _lib, graph as G, synth
from chromegcn_amd.finetune import GCNStage

SL_WGS = 8192
P = _lib.ptr


def report(raw, what, n, kind, grid=0):
    """read the table left by the launches since the last call, print it, clear it and keep the selection"""
    buf = np.zeros(SL_WGS * 8, dtype=np.uint64)
    assert raw.cgcn_debug_sliced_stamps(buf.ctypes.data_as(ctypes.c_void_p), n, kind, grid) == 0
    t = buf.reshape(SL_WGS, 8).astype(np.int64)
    t = t[t[:, 0] > 0]
    if not len(t):
        print("%-44s no matching launch" % what)
        return
    t = t[t[:, 7] == t[np.argmax(t[:, 0]), 7]]   # (an earlier matching launch of another grid size leaves its higher slots behind)
    t0 = t[:, 0].min()
    span = (t[:, 5].max() - t0) / 100.0
    first = (t[:, 0] - t0) <= 100
    line = "%-44s grid %5d  wgs %5d  span %6.2f us  last start %6.2f" % (what, int(t[0, 7]), len(t), span, (t[:, 0].max() - t0) / 100.0)
    for nm, sel in (("first round", first), ("later", ~first)):
        v = t[sel]
        if not len(v):
            continue
        w = v[(v[:, 2] > 0) & (v[:, 3] > 0)]   # thread 0's row was not empty
        med = lambda a: float(np.median(a)) / 100.0 if len(a) else float("nan")
        line += "\n    %-11s %5d wgs: chain %5.2f  col %5.2f  line %5.2f  walk %6.2f  store %5.2f  | whole %6.2f us" % (
            nm, len(v), med(v[:, 1] - v[:, 0]), med(w[:, 2] - w[:, 1]), med(w[:, 3] - w[:, 2]), med(w[:, 4] - w[:, 3]),
            med(v[:, 5] - v[:, 4]), med(v[:, 5] - v[:, 0]))
    print(line)
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("names", nargs="*")
    ap.add_argument("--label", default="")
    ap.add_argument("--grid", type=int, default=0)
    ap.add_argument("--epochs", type=int, default=4)
    args = ap.parse_args()
    dev = torch.device("cuda")
    lib = _lib.load()
    raw = ctypes.CDLL(os.environ["CHROMEGCN_LIB"])
    raw.cgcn_debug_sliced_stamps.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    d, S = 128, 2
    torch.manual_seed(0)
    model = C.ChromeGCN(d, d, synth.N_LABELS, 0.2, True, 2).to(dev)
    opt = torch.optim.SGD(model.parameters(), lr=0.25, momentum=0.9, weight_decay=1e-6)
    stage = GCNStage(model, opt, "hic", dev, hip_graphs=True, input_grad=True, cache_input_aggregation=False)
    train = [c for c in synth.HG19_LEN if synth.split_of(c) == "train"]
    for nm in train:
        feats, hic = synth.synthetic_chromosome(nm, d=d)
        stage.add_chromosome(nm, feats, hic)
    by_n = sorted(train, key=synth.chrom_nodes)
    mean_n = sum(synth.chrom_nodes(c) for c in train) / len(train)
    names = args.names or [by_n[0], min(train, key=lambda c: abs(synth.chrom_nodes(c) - mean_n)), by_n[-1]]
    print("# %s  (100 MHz stamps; medians over workgroups, us)" % (args.label or os.path.basename(os.environ["CHROMEGCN_LIB"])))
    for _ in range(3):   # capture and warm the epoch graph
        stage.run_split("train", train, to_cpu=False)
    torch.cuda.synchronize()
    for nm in names:
        g = stage.chroms[nm].graph
        n = g.n
        # launched alone, hot: the same launch five times on the same table
        x, h = torch.randn(S, n, d, device=dev), torch.empty(S, n, d, device=dev)
        raw.cgcn_debug_sliced_stamps(None, n, 0, 0)
        lib.cgcn_debug_set_fwd_split_bytes(0)   # the sliced route at every size
        for _ in range(5):
            _lib.check(lib.cgcn_spmm(_lib.stream_ptr(), n, n, S, d, P(g.rowptr), P(g.col), P(g.val), P(g.row_scale), P(x), P(h),
                                     G.aux_ptr(g.col)), "cgcn_spmm")
        torch.cuda.synchronize()
        lib.cgcn_debug_set_fwd_split_bytes(-1)
        report(raw, "%s n=%d k_aggregate_sliced alone, hot" % (nm, n), n, 1)
        z = torch.zeros(S, n, d, device=dev)
        W, wg, gate = torch.zeros(d, d, device=dev), torch.zeros(d, device=dev), torch.rand(S, n, device=dev)
        dW, db, dwg, dcg = (torch.zeros(k, device=dev) for k in (d * d, d, d, 1))
        wsb = lib.cgcn_layer_bwd_workspace_bytes(n, S, d)
        ws = torch.zeros(wsb, dtype=torch.uint8, device=dev)
        for _ in range(5):   # phase 2 of the layer backward alone: the gather with the second-stage sums riding
            _lib.check(lib.cgcn_debug_layer_bwd_phases(_lib.stream_ptr(), n, S, d, P(g.rowptr_t), P(g.col_t), P(g.val_t), P(g.row_scale), P(z), P(z),
                                                       P(z), P(gate), P(W), P(wg), P(x), None, P(h), P(x), P(dW), P(db), P(dwg), P(dcg), 0, 0.0,
                                                       None, 0, None, P(ws), wsb, 2, G.aux_ptr(g.col_t)), "cgcn_debug_layer_bwd_phases")
        torch.cuda.synchronize()
        report(raw, "%s n=%d k_bwd_sliced alone, hot" % (nm, n), n, 0, args.grid)
        for kind, kname in ((0, "k_aggregate_sliced"), (1, "k_bwd_sliced")):
            raw.cgcn_debug_sliced_stamps(None, n, kind, args.grid)
            for _ in range(args.epochs):
                stage.run_split("train", train, to_cpu=False)
            torch.cuda.synchronize()
            report(raw, "%s n=%d %s in the epoch" % (nm, n, kname), n, 0, 0)
    raw.cgcn_debug_sliced_stamps(None, 0, 0, 0)


if __name__ == "__main__":
    main()
