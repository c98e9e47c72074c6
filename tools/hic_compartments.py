"""A/B compartments of one chromosome's Hi-C contacts (chromegcn_amd/compartments.py): a `.cghic` contact cache or contact text
in, a bedGraph of the leading eigenvector of the O/E Pearson map (`E1`) out, and optionally the Pearson map.  It plots nothing.

    python tools/hic_compartments.py chr21.cghic --chrom chr21 --res 100000 --out-prefix out/chr21 [--pearson] [--orient x.bedGraph]

The records are binned to --res and balanced by --norm (VC by default: it cannot fail to converge; RAW = none; a name the cache
stores is taken from it when its vector is at --res).  Written:
  <prefix>.E1.bedGraph     chrom, start, end, E1 of the bin, the bins with a value only (A > 0, B < 0)
  <prefix>.E<k>.bedGraph   the further vectors of --n-eigs
  <prefix>.pearson.npy     with --pearson: the m x m Pearson map over the kept bins; <prefix>.keep.npy: their bin numbers
--orient: a bedGraph (chrom, start, end, value) whose values, added up per bin, orient every vector (a peak or gene density:
A is the side that carries it); without it the entry of largest |E| is positive.  --host runs the numpy restatement instead of
the GPU."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from chromegcn_amd import compartments, hic  # noqa: E402


def read_orient(path, chrom, res, n):
    """the values of a bedGraph's rows of `chrom` added up per bin of their start: float64 [n]"""
    out = np.zeros(n)
    with open(path) as f:
        for ln in f:
            p = ln.split()
            if len(p) >= 4 and p[0] == chrom and 0 <= int(p[1]) // res < n:
                out[int(p[1]) // res] += float(p[3])
    return out


def write_outputs(comp, chrom, prefix, pearson=False):
    res, paths = comp.resolution_bp, []
    for k in range(comp.E.shape[0]):
        path = "%s.E%d.bedGraph" % (prefix, k + 1)
        with open(path, "w") as f:
            for b in np.flatnonzero(~np.isnan(comp.E[k])).tolist():
                f.write("%s\t%d\t%d\t%.9g\n" % (chrom, b * res, (b + 1) * res, comp.E[k, b]))
        paths.append(path)
    if pearson and comp.pearson is not None:
        C = comp.pearson
        np.save(prefix + ".pearson.npy", C if isinstance(C, np.ndarray) else C.cpu().numpy())
        np.save(prefix + ".keep.npy", comp.keep)
        paths += [prefix + ".pearson.npy", prefix + ".keep.npy"]
    return paths


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("contacts", help="a .cghic contact cache, or contact text (pos1 pos2 count per line)")
    ap.add_argument("--chrom", required=True, help="the chromosome's name in the output")
    ap.add_argument("--res", type=int, default=compartments.RESOLUTION_BP, help="bin size of the compartment call")
    ap.add_argument("--norm", default="VC", help="RAW, KR, VC, SQRTVC (computed from the records), or a name stored in the cache")
    ap.add_argument("--n-eigs", type=int, default=1)
    ap.add_argument("--ignore-diags", type=int, default=compartments.IGNORE_DIAGS)
    ap.add_argument("--tol", type=float, default=compartments.TOL)
    ap.add_argument("--max-iter", type=int, default=compartments.MAX_ITER)
    ap.add_argument("--orient", default=None, help="a bedGraph whose per-bin sums orient the vectors")
    ap.add_argument("--pearson", action="store_true", help="also write the Pearson map as .npy")
    ap.add_argument("--out-prefix", required=True)
    ap.add_argument("--host", action="store_true", help="the numpy restatement instead of the GPU")
    opt = ap.parse_args(argv)
    c = hic.load_contacts_cache(opt.contacts) if opt.contacts.endswith(".cghic") else hic.load_contacts_text(opt.contacts)
    norm = None if opt.norm == "RAW" else opt.norm
    if norm is not None and norm in c.norms and c.resolution_bp == opt.res:
        norm = c.norms[norm]
    elif norm is not None and norm not in ("KR", "VC", "SQRTVC"):
        raise SystemExit("%s holds no %r vector at %d bp (has: %s at %d bp)"
                         % (opt.contacts, norm, opt.res, ", ".join(sorted(c.norms)) or "none", c.resolution_bp))
    rule = dict(n_eigs=opt.n_eigs, ignore_diags=opt.ignore_diags, tol=opt.tol, max_iter=opt.max_iter)
    if opt.host:
        comp = compartments.compartments_host(c.pos1, c.pos2, c.count, norm, opt.res, **rule)
    else:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("tools/hic_compartments.py needs a GPU (or --host: the numpy restatement)")
        comp = hic.HicContacts.from_host(c).compartments(norm, opt.res, **rule)
    if opt.orient:
        comp = comp.oriented(read_orient(opt.orient, opt.chrom, opt.res, comp.n))
    os.makedirs(os.path.dirname(os.path.abspath(opt.out_prefix)), exist_ok=True)
    call = comp.compartment_of_bin
    print("%d of %d bins kept, %d called, A share %.3f, %d flat rows" % (comp.keep.size, comp.n, int(np.count_nonzero(call)),
                                                                          comp.a_share(), comp.info["flat_rows"]))
    for k in range(comp.E.shape[0]):
        print("E%d: converged %s after %d steps, eigenvalue %.6g, residual %.3g" % (
            k + 1, comp.info["converged"][k], comp.info["iterations"][k], comp.info["eigenvalue"][k], comp.info["residual"][k]))
    for path in write_outputs(comp, opt.chrom, opt.out_prefix, opt.pearson):
        print(path)


if __name__ == "__main__":
    main(sys.argv[1:])
