"""Insulation scores and domains of one chromosome's Hi-C contacts (chromegcn_amd/insulation.py): a `.cghic` contact cache or
contact text in, a bedGraph of the log2 insulation score per window size and a BED of the domains out.  It plots nothing.

    python tools/hic_domains.py chr21.cghic --chrom chr21 --res 10000 --windows 100000,250000 --out-prefix out/chr21

The records are binned to --res, balanced by --norm (VC by default: it cannot fail to converge; RAW = none; a name the cache
stores is taken from it when its vector is at --res) and scored at every window of --windows (bp, multiples of --res).  Written:
  <prefix>.w<WINDOW>.log2.bedGraph   chrom, start, end, log2(score / mean) of the junction left of the bin, defined bins only
  <prefix>.domains.bed               chrom, start, end, domain index, strength of the boundary that opens it (0 for the first),
                                     from the boundaries of --domain-window (default: the first window)
--host runs the numpy restatement instead of the GPU."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from chromegcn_amd import hic, insulation  # noqa: E402


def write_outputs(ins, chrom, prefix, domain_window_bp):
    res, n = ins.resolution_bp, ins.n
    paths = []
    for k, wbp in enumerate(ins.windows_bp):
        path = "%s.w%d.log2.bedGraph" % (prefix, wbp)
        with open(path, "w") as f:
            for b in np.flatnonzero(ins.defined[k]).tolist():
                f.write("%s\t%d\t%d\t%.6f\n" % (chrom, b * res, (b + 1) * res, ins.log2[k, b]))
        paths.append(path)
    k = ins.index_of(domain_window_bp)
    edges = [0] + ins.boundaries[k].tolist() + [n]
    strength = [0.0] + ins.strength[k].tolist()
    path = prefix + ".domains.bed"
    with open(path, "w") as f:
        d = 0
        for a, b, s in zip(edges[:-1], edges[1:], strength):
            if b > a:   # a boundary at bin 0 opens no domain of its own
                f.write("%s\t%d\t%d\tdomain%d\t%.6f\n" % (chrom, a * res, b * res, d, s))
            d += 1
    return paths + [path]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("contacts", help="a .cghic contact cache, or contact text (pos1 pos2 count per line)")
    ap.add_argument("--chrom", required=True, help="the chromosome's name in the output")
    ap.add_argument("--res", type=int, default=10000, help="bin size of the insulation score")
    ap.add_argument("--windows", default="100000,250000", help="window sizes in bp, ascending, at most 8")
    ap.add_argument("--norm", default="VC", help="RAW, KR, VC, SQRTVC (computed from the records), or a name stored in the cache")
    ap.add_argument("--min-strength", type=float, default=insulation.MIN_STRENGTH)
    ap.add_argument("--min-valid-share", type=float, default=insulation.MIN_VALID_SHARE)
    ap.add_argument("--span", type=int, default=None, help="boundary neighbourhood in bins (default: each window's own size)")
    ap.add_argument("--domain-window", type=int, default=None, help="the window (bp) whose boundaries make the domains")
    ap.add_argument("--out-prefix", required=True)
    ap.add_argument("--host", action="store_true", help="the numpy restatement instead of the GPU")
    opt = ap.parse_args(argv)
    wbp = [int(x) for x in opt.windows.split(",")]
    if opt.contacts.endswith(".cghic"):
        c = hic.load_contacts_cache(opt.contacts)
    else:
        c = hic.load_contacts_text(opt.contacts)
    norm = None if opt.norm == "RAW" else opt.norm
    if norm is not None and norm in c.norms and c.resolution_bp == opt.res:
        norm = c.norms[norm]
    elif norm is not None and norm not in ("KR", "VC", "SQRTVC"):
        raise SystemExit("%s holds no %r vector at %d bp (has: %s at %d bp)"
                         % (opt.contacts, norm, opt.res, ", ".join(sorted(c.norms)) or "none", c.resolution_bp))
    rule = dict(min_strength=opt.min_strength, min_valid_share=opt.min_valid_share, span=opt.span)
    if opt.host:
        ins = insulation.insulation_host(c.pos1, c.pos2, c.count, norm, opt.res, wbp, **rule)
    else:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("tools/hic_domains.py needs a GPU (or --host: the numpy restatement)")
        ins = hic.HicContacts.from_host(c).insulation(norm, opt.res, wbp, **rule)
    os.makedirs(os.path.dirname(os.path.abspath(opt.out_prefix)), exist_ok=True)
    for k, w in enumerate(ins.windows_bp):
        print("window %d bp: %d of %d bins defined, %d boundaries" % (w, int(ins.defined[k].sum()), ins.n, ins.boundaries[k].size))
    for path in write_outputs(ins, opt.chrom, opt.out_prefix, wbp[0] if opt.domain_window is None else opt.domain_window):
        print(path)


if __name__ == "__main__":
    main(sys.argv[1:])
