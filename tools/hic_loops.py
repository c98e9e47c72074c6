"""Chromatin loops of one chromosome's Hi-C contacts (chromegcn_amd/loops.py): a `.cghic` contact cache or contact text in, a
BEDPE of the loops out.  It plots nothing.

    python tools/hic_loops.py chr21.cghic --chrom chr21 --res 10000 --out out/chr21.loops.bedpe

The records are binned to --res, balanced by --norm (VC by default; RAW = none; a name the cache stores is taken from it when its
vector is at --res), scored against the expected vector computed from the records with that norm, and called by the rule of the
module's docstring.  One line per loop: chrom, start and end of the two peak bins, the observed count, the four local expected
values (donut, lower-left, horizontal, vertical), the centroid (bp, bp), the radius (bp) and the number of pixels.
--host runs the numpy restatement instead of the GPU."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from chromegcn_amd import hic, loops  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("contacts", help="a .cghic contact cache, or contact text (pos1 pos2 count per line)")
    ap.add_argument("--chrom", required=True, help="the chromosome's name in the output")
    ap.add_argument("--res", type=int, default=10000, help="bin size; 5000, 10000 and 25000 have default half-widths")
    ap.add_argument("--norm", default="VC", help="RAW, KR, VC, SQRTVC (computed from the records), or a name stored in the cache")
    ap.add_argument("--peak", type=int, default=None, help="the peak half-width p (bins)")
    ap.add_argument("--window", type=int, default=None, help="the window half-width w (bins), at most 10")
    ap.add_argument("--max-distance", type=int, default=loops.MAX_DISTANCE_BP, help="the largest distance of a pixel, bp")
    ap.add_argument("--fdr", type=float, default=loops.FDR)
    ap.add_argument("--cluster-radius", type=int, default=loops.CLUSTER_RADIUS_BP, help="bp")
    ap.add_argument("--min-cluster-pixels", type=int, default=1)
    ap.add_argument("--out", required=True, help="the BEDPE file")
    ap.add_argument("--host", action="store_true", help="the numpy restatement instead of the GPU")
    opt = ap.parse_args(argv)
    c = hic.load_contacts_cache(opt.contacts) if opt.contacts.endswith(".cghic") else hic.load_contacts_text(opt.contacts)
    norm = None if opt.norm == "RAW" else opt.norm
    if norm is not None and norm in c.norms and c.resolution_bp == opt.res:
        norm = c.norms[norm]
    elif norm is not None and norm not in ("KR", "VC", "SQRTVC"):
        raise SystemExit("%s holds no %r vector at %d bp (has: %s at %d bp)"
                         % (opt.contacts, norm, opt.res, ", ".join(sorted(c.norms)) or "none", c.resolution_bp))
    rule = dict(max_distance_bp=opt.max_distance, fdr=opt.fdr, cluster_radius_bp=opt.cluster_radius,
                min_cluster_pixels=opt.min_cluster_pixels)
    rule.update({k: v for k, v in (("p", opt.peak), ("w", opt.window)) if v is not None})
    if opt.host:
        found = loops.loops_host(c.pos1, c.pos2, c.count, norm, opt.res, "auto", **rule)
    else:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("tools/hic_loops.py needs a GPU (or --host: the numpy restatement)")
        found = hic.HicContacts.from_host(c).loops(norm, opt.res, "auto", **rule)
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as f:
        f.write(found.to_bedpe(opt.chrom))
    print("%d loops from %d candidates, %d enriched pixels, %d after the ratios: %s"
          % (len(found), found.info["candidates"], found.info["enriched"], found.info["kept_after_ratios"], opt.out))


if __name__ == "__main__":
    main(sys.argv[1:])
