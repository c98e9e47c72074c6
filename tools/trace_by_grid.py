#!/usr/bin/env python3
"""Reads the kernel trace of one `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python bench.py ...` run:
hand-written launches and their summed kernel time per epoch, every kernel's calls per epoch and mean time, the two gathers by
grid size (the first layer's backward gather carries the SGD riders and, with it, the companion aggregation: its grid differs
from the last layer's), and the k_bwd_sliced launches that end a chromosome's step.  python tools/trace_by_grid.py DIR
(profiles/co_aggregation_ab.txt)."""
import csv, glob, os, sys
from collections import defaultdict
d = sys.argv[1]
f = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)[0]
rows = list(csv.DictReader(open(f)))
gcols = [c for c in rows[0] if c.startswith("Grid_Size")]
wcols = [c for c in rows[0] if c.startswith("Workgroup_Size")]
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
def short(n):
    n = n.split("(")[0].strip()
    return n[5:] if n.startswith("void ") else n
hand = [r for r in rows if short(r["Kernel_Name"]).startswith("k_")]
dur = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
heads = sum(1 for r in hand if short(r["Kernel_Name"]).startswith("k_head_fused"))
epochs = heads / 16.0
print("trace:", f.split("/")[-1], "hand-written dispatches", len(hand), "head launches", heads, "-> epochs", epochs)
by = defaultdict(list)
for r in hand:
    by[short(r["Kernel_Name"]).split("<")[0]].append(dur(r))
print("per epoch: hand-written launches %.1f, sum of their kernel time %.1f us" % (len(hand) / epochs, sum(map(dur, hand)) / epochs))
for k, v in sorted(by.items(), key=lambda kv: -sum(kv[1])):
    print("  %-28s calls/epoch %6.1f  avg %8.2f us  total/epoch %9.1f us" % (k, len(v) / epochs, sum(v) / len(v), sum(v) / epochs))
# the gathers by grid size (workgroups): the layer-1 backward gather carries the SGD riders (and the companion), so its grid differs
for name in ("k_bwd_sliced", "k_aggregate_sliced"):
    g = defaultdict(list)
    sel = [r for r in hand if short(r["Kernel_Name"]).startswith(name)]
    for r in sel:
        wg = 1
        for gc, wc in zip(gcols, wcols):
            wg *= max(1, int(r[gc]) // max(1, int(r[wc])))
        g[wg].append(dur(r))
    print(name, "by workgroups in the grid (calls over the whole trace, avg us):")
    for wg, v in sorted(g.items()):
        print("   %7d wg  calls %5d  avg %8.2f" % (wg, len(v), sum(v) / len(v)))
    if name == "k_aggregate_sliced":
        ev, od = [dur(r) for r in sel[0::2]], [dur(r) for r in sel[1::2]]
        print("   in launch order: even-indexed avg %.2f us (%d), odd-indexed avg %.2f us (%d)" % (sum(ev) / len(ev), len(ev), sum(od) / max(1, len(od)), len(od)))
# pairs: a k_bwd_sliced directly followed by a k_aggregate_sliced (parent: layer-1 gather + the next chromosome's aggregation)
names = [short(r["Kernel_Name"]).split("<")[0] for r in hand]
pair_b, pair_a, gap = [], [], []
for i in range(len(hand) - 1):
    if names[i] == "k_bwd_sliced" and names[i + 1] == "k_aggregate_sliced":
        pair_b.append(dur(hand[i])); pair_a.append(dur(hand[i + 1]))
        gap.append((int(hand[i + 1]["Start_Timestamp"]) - int(hand[i]["End_Timestamp"])) / 1e3)
if pair_b:
    k = len(pair_b)
    print("k_bwd_sliced -> k_aggregate_sliced pairs: %d; avg bwd %.2f + agg %.2f us, gap between them %.2f us, end-to-end %.2f us"
          % (k, sum(pair_b) / k, sum(pair_a) / k, sum(gap) / k, (sum(pair_b) + sum(pair_a) + sum(gap)) / k))
# layer-1 gathers: the k_bwd_sliced launches followed by something else than k_bwd_rowlocal (i.e. the last launch of a step)
last = [dur(hand[i]) for i in range(len(hand) - 1) if names[i] == "k_bwd_sliced" and not names[i + 1].startswith("k_bwd_rowlocal")]
if last:
    print("k_bwd_sliced as the last launch of a step: %d, avg %.2f us" % (len(last), sum(last) / len(last)))
