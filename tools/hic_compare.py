"""How alike two Hi-C contact maps of one chromosome are (chromegcn_amd/mapcompare.py): two `.cghic` contact caches or contact
text files in, the stratum-adjusted correlation coefficient per smoothing half-width as an `.npz` each and one text table of
rho per distance out.  It plots nothing.

    python tools/hic_compare.py gm12878/chr21.cghic k562/chr21.cghic --chrom chr21 --res 40000 --h 0,1,2,5 --out out/chr21.scc

Writes <out>.h<H>.npz (MapComparison.save) per half-width and <out>.txt: one line per distance with the cells and rho of every
half-width.  --host runs the numpy restatement instead of the GPU."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from chromegcn_amd import hic, mapcompare  # noqa: E402


def _load(path):
    return hic.load_contacts_cache(path) if path.endswith(".cghic") else hic.load_contacts_text(path)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("contacts_a", help="a .cghic contact cache, or contact text (pos1 pos2 count per line)")
    ap.add_argument("contacts_b", help="the second map, the same way")
    ap.add_argument("--chrom", required=True, help="the chromosome's name (in the output)")
    ap.add_argument("--res", type=int, default=40000, help="bin size")
    ap.add_argument("--h", default="5", metavar="H[,H...]", help="the smoothing half-widths (bins), each at most 20")
    ap.add_argument("--norm", default="RAW", help="RAW (the observed counts), KR, VC or SQRTVC (computed from each map's records)")
    ap.add_argument("--max-distance", type=int, default=mapcompare.MAX_DISTANCE_BP, help="the largest compared distance, bp")
    ap.add_argument("--min-dist", type=int, default=1, help="the least compared distance (bins)")
    ap.add_argument("--out", required=True, help="the output prefix")
    ap.add_argument("--host", action="store_true", help="the numpy restatement instead of the GPU")
    opt = ap.parse_args(argv)
    if opt.norm not in ("RAW", "KR", "VC", "SQRTVC"):
        raise SystemExit("--norm is one of RAW, KR, VC, SQRTVC")
    try:
        hs = [int(x) for x in opt.h.split(",")]
        for v in hs:
            mapcompare.scc_rule(opt.res, 0, v, opt.max_distance, opt.min_dist)
    except ValueError as e:
        raise SystemExit("tools/hic_compare.py: %s" % e)
    a, b = _load(opt.contacts_a), _load(opt.contacts_b)
    kw = dict(norm=None if opt.norm == "RAW" else opt.norm, resolution_bp=opt.res, h=hs, max_distance_bp=opt.max_distance,
              min_dist=opt.min_dist)
    if opt.host:
        found = mapcompare.map_scc_host((a.pos1, a.pos2, a.count), (b.pos1, b.pos2, b.count), **kw)
    else:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("tools/hic_compare.py needs a GPU (or --host: the numpy restatement)")
        found = hic.HicContacts.from_host(a).scc(hic.HicContacts.from_host(b), **kw)
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    for v, r in zip(hs, found):
        r.save("%s.h%d.npz" % (opt.out, v))
        print("%s h=%d: SCC %.6f over %d strata, %d of %d bins valid" % (opt.chrom, v, r.scc, r.n_strata, int(r.valid.sum()), r.valid.size))
    with open(opt.out + ".txt", "w") as f:
        f.write("# %s at %d bp, norm %s; distance_bins" % (opt.chrom, opt.res, opt.norm)
                + "".join("\tcells_h%d\trho_h%d" % (v, v) for v in hs) + "\n")
        for d in range(max([r.rho.size for r in found] or [0])):
            f.write("%d" % d + "".join("\t%d\t%.10g" % (r.cells[d], r.rho[d]) for r in found) + "\n")
    print("%s.txt" % opt.out)


if __name__ == "__main__":
    main(sys.argv[1:])
