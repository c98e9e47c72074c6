"""Aggregate peak analysis of one chromosome's Hi-C contacts (chromegcn_amd/pileup.py): a `.cghic` contact cache or contact
text plus a list of pixel centres in, the pile-up as an `.npz` and one text matrix of the mean per group out.  It plots nothing.

    python tools/hic_apa.py chr21.cghic --chrom chr21 --bedpe loops.bedpe --out out/chr21.apa
    python tools/hic_apa.py chr21.cghic --chrom chr21 --call-loops --out out/chr21.apa
    python tools/hic_apa.py chr21.cghic --chrom chr21 --graph chr21.hic.cgcsr --saliency sal.npy --quantiles 4 --out out/chr21.apa

The centres are ONE of: --bedpe (the lines of --chrom; the centre is the pair of bins that hold the two start positions),
--call-loops (the loops called from the records by chromegcn_amd/loops.py with --norm, --peak and --loop-window), or --graph (a
`.cgcsr` graph cache over the windows the contact cache stores: one centre per stored entry above the diagonal).  With --graph,
--saliency is a `.npy` with one value per stored entry and --quantiles Q groups the edges by its quantiles; --distances a,b,c
(bins) groups by distance instead; --shift BINS moves every centre along the diagonal (the same-distance control).
Writes <out>.npz (Pileup.save) and <out>.group<g>.txt, and prints P2LL, P2M and ZscoreLL per group.
--host runs the numpy restatement instead of the GPU."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from chromegcn_amd import hic, loops, pileup  # noqa: E402


def bedpe_centres(path, chrom, res):
    """(i, j) of the BEDPE lines whose two chromosomes are `chrom`"""
    i, j = [], []
    with open(path) as f:
        for ln in f:
            t = ln.split()
            if len(t) < 5 or ln.startswith("#") or t[0] != chrom or t[3] != chrom:
                continue
            i.append(int(t[1]) // res)
            j.append(int(t[4]) // res)
    return np.asarray(i, dtype=np.int64), np.asarray(j, dtype=np.int64)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("contacts", help="a .cghic contact cache, or contact text (pos1 pos2 count per line)")
    ap.add_argument("--chrom", required=True, help="the chromosome's name (in --bedpe and in the output)")
    ap.add_argument("--bedpe", default=None, help="centres: a BEDPE file")
    ap.add_argument("--call-loops", action="store_true", help="centres: the loops called from the records")
    ap.add_argument("--graph", default=None, help="centres: the entries above the diagonal of a .cgcsr graph cache")
    ap.add_argument("--saliency", default=None, help="--graph: a .npy with one value per stored entry")
    ap.add_argument("--quantiles", type=int, default=0, metavar="Q", help="--saliency: group the edges by Q quantiles of it")
    ap.add_argument("--distances", default=None, metavar="A,B,C", help="group the centres by distance: ascending edges in bins")
    ap.add_argument("--shift", type=int, default=0, metavar="BINS", help="move every centre along the diagonal: the control")
    ap.add_argument("--res", type=int, default=10000, help="bin size")
    ap.add_argument("--norm", default="VC", help="RAW, KR, VC, SQRTVC (computed from the records), or a name stored in the cache")
    ap.add_argument("--value", default="oe", choices=pileup.VALUES)
    ap.add_argument("--window", type=int, default=None, help="the window half-width w (bins), at most 10")
    ap.add_argument("--corner", type=int, default=None, help="the corner width (bins)")
    ap.add_argument("--min-dist", type=int, default=None, help="the least distance of a centre (bins), at least 2 w")
    ap.add_argument("--max-distance", type=int, default=pileup.MAX_DISTANCE_BP, help="the largest distance of a centre, bp")
    ap.add_argument("--peak", type=int, default=None, help="--call-loops: the peak half-width p (bins)")
    ap.add_argument("--loop-window", type=int, default=None, help="--call-loops: the window half-width of the caller (bins)")
    ap.add_argument("--out", required=True, help="the output prefix")
    ap.add_argument("--host", action="store_true", help="the numpy restatement instead of the GPU")
    opt = ap.parse_args(argv)
    if (opt.bedpe is not None) + bool(opt.call_loops) + (opt.graph is not None) != 1:
        raise SystemExit("give exactly one of --bedpe, --call-loops and --graph")
    if (opt.saliency is not None or opt.quantiles) and (opt.graph is None or opt.saliency is None or opt.quantiles < 1):
        raise SystemExit("--saliency and --quantiles go together and with --graph")
    if opt.quantiles and opt.distances:
        raise SystemExit("group by --quantiles or by --distances, not both")
    c = hic.load_contacts_cache(opt.contacts) if opt.contacts.endswith(".cghic") else hic.load_contacts_text(opt.contacts)
    norm = None if opt.norm == "RAW" else opt.norm
    if norm is not None and norm in c.norms and c.resolution_bp == opt.res:
        norm = c.norms[norm]
    elif norm is not None and norm not in ("KR", "VC", "SQRTVC"):
        raise SystemExit("%s holds no %r vector at %d bp (has: %s at %d bp)"
                         % (opt.contacts, norm, opt.res, ", ".join(sorted(c.norms)) or "none", c.resolution_bp))
    rule = dict(value=opt.value, w=opt.window, corner=opt.corner, min_dist=opt.min_dist, max_distance_bp=opt.max_distance)
    pileup.pileup_rule(opt.res, **rule)
    dev = None
    if not opt.host:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("tools/hic_apa.py needs a GPU (or --host: the numpy restatement)")
        dev = hic.HicContacts.from_host(c)
    group, G = None, 1
    if opt.bedpe is not None:
        ci, cj = bedpe_centres(opt.bedpe, opt.chrom, opt.res)
    elif opt.call_loops:
        lr = dict(max_distance_bp=opt.max_distance)
        lr.update({k: v for k, v in (("p", opt.peak), ("w", opt.loop_window)) if v is not None})
        found = (loops.loops_host(c.pos1, c.pos2, c.count, norm, opt.res, "auto", **lr) if opt.host
                 else dev.loops(norm, opt.res, "auto", **lr))
        ci, cj = found.peak_i, found.peak_j
    else:
        from chromegcn_amd import graph
        if c.window_start is None:
            raise SystemExit("%s holds no window list: --graph needs the windows of the graph's rows" % opt.contacts)
        ci, cj, entry = pileup.centres_of_graph(graph.load_csr_cache(opt.graph), c.window_start, opt.res)
        if opt.quantiles:
            sal = np.load(opt.saliency).ravel()
            if entry.size and sal.size <= int(entry.max()):
                raise SystemExit("%s has %d values but the graph has more stored entries" % (opt.saliency, sal.size))
            group, G = pileup.quantile_groups(sal[entry], opt.quantiles), opt.quantiles
    if opt.distances:
        edges = [int(x) for x in opt.distances.split(",")]
        group, G = pileup.distance_groups(ci, cj, edges), len(edges) - 1
    if opt.shift:
        ci, cj = pileup.shifted_centres(ci, cj, opt.shift)
    if opt.host:
        p = pileup.pileup_host(c.pos1, c.pos2, c.count, (ci, cj), group, G, norm, opt.res, "auto", **rule)
    else:
        p = dev.pileup((ci, cj), group, G, norm, opt.res, "auto", **rule)
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    p.save(opt.out + ".npz")
    s = p.scores()
    for g in range(G):
        np.savetxt("%s.group%d.txt" % (opt.out, g), p.mean[g], fmt="%.10g")
        print("group %d: %d centres, P2LL %.4g, P2M %.4g, ZscoreLL %.4g" % (g, p.kept[g], s["P2LL"][g], s["P2M"][g], s["ZscoreLL"][g]))
    print("%d centres given, skipped: %s; %s.npz" % (len(ci), ", ".join("%s %d" % kv for kv in p.skipped.items()), opt.out))


if __name__ == "__main__":
    main(sys.argv[1:])
