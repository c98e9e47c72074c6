"""Times the insulation pass (chromegcn_amd/insulation.py, csrc/cgcn_insulation.hip) on the GPU against its numpy restatement;
fails without a GPU.

For chr21- and chr1-size synthetic contacts (synth.raw_contacts: 1 kb records, `hic_like` distances), binned to --res, windows
--windows (bp), records resident on the device; device stages are the median of --reps calls after a warm one, host clock
around the call and a device synchronise:
  * aggregate_ms: the contact matrix at --res (hicnorm.aggregate_contacts; needed once per resolution, kept by HicContacts);
  * sums_raw_ms / sums_vc_ms: cgcn_hicinsul_sums alone, without a vector and with the records' VC vector;
  * terms: the matrix entries the kernel adds, summed over the bins (the entries inside every bin's largest diamond), and
    sums_*_gbytes_s = terms x (12 bytes of column and value, + 8 of the column's norm bin with a vector) / the kernel time:
    the gather rate to hold against the gather numbers of DESIGN.md section 7;
  * rule_ms: the read-back of S, VC and the vector plus insulation_from_sums on the host;
  * insulation_ms: HicContacts.insulation end to end with the matrix resident (caches of the result cleared);
  * host_matrix_ms, host_sums_ms, host_rule_ms: contact_matrix_host, diamond_sums_host and insulation_from_sums on this
    machine's CPU in the same run (one call each), and whether the device sums equal the host's bit for bit (integer counts).
Prints one JSON line per chromosome and appends the lines to --out (default: profiles/insulation_bench.jsonl; '' = nowhere)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import scipy.sparse as sp
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from chromegcn_amd import hic, hicmap, hicnorm, insulation, synth  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def host_ms(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--chroms", default="chr21,chr1")
    ap.add_argument("--res", type=int, default=10000)
    ap.add_argument("--windows", default="100000,250000,500000")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-host", action="store_true", help="skip the CPU restatement")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "insulation_bench.jsonl"))
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/insulation_bench.py needs a GPU")
    dev = torch.device("cuda")
    wbp = [int(x) for x in opt.windows.split(",")]
    w = insulation.windows_in_bins(wbp, opt.res)
    lines = []
    for chrom in opt.chroms.split(","):
        r = synth.raw_contacts(chrom)
        c = hic.HicContacts(r["pos1"], r["pos2"], r["count"], dev)
        agg = timed(lambda: hicnorm.aggregate_contacts(c.pos1, c.pos2, c.count, opt.res), opt.reps)
        A = c.contact_matrix(opt.res)
        vc = c.norm_vector("VC", opt.res)
        sums_raw = timed(lambda: insulation.diamond_sums(A, None, w), opt.reps)
        sums_vc = timed(lambda: insulation.diamond_sums(A, vc, w), opt.reps)
        S = insulation.diamond_sums(A, None, w)
        valid = hicmap.valid_bins(A.vc.cpu().numpy(), None)
        rule = timed(lambda: insulation.insulation_from_sums(S.cpu().numpy(), hicmap.valid_bins(A.vc.cpu().numpy(), vc.cpu().numpy()), w),
                     opt.reps)

        def end_to_end():
            c._insulations.clear()
            return c.insulation("VC", opt.res, wbp)

        total = timed(end_to_end, opt.reps)
        ins = end_to_end()
        host = A.to_host()
        pattern = sp.csr_matrix((np.ones_like(host.data), host.indices, host.indptr), shape=host.shape)
        terms = int(insulation.diamond_sums_host(pattern, None, w[-1:]).sum())
        ln = {"chrom": chrom, "M": c.M, "resolution_bp": opt.res, "n_bins": A.n, "nnz": A.nnz, "windows_bp": wbp, "terms": terms,
              "aggregate_ms": round(agg, 3), "sums_raw_ms": round(sums_raw, 3), "sums_vc_ms": round(sums_vc, 3),
              "sums_raw_gbytes_s": round(terms * 12 / (sums_raw * 1e-3) / 1e9, 2),
              "sums_vc_gbytes_s": round(terms * 20 / (sums_vc * 1e-3) / 1e9, 2),
              "rule_ms": round(rule, 3), "insulation_ms": round(total, 3), "boundaries": [int(b.size) for b in ins.boundaries]}
        if not opt.no_host:
            Ah, t_mat = host_ms(lambda: hicnorm.contact_matrix_host(r["pos1"], r["pos2"], r["count"], opt.res))
            Sh, t_sums = host_ms(lambda: insulation.diamond_sums_host(Ah, None, w))
            _, t_rule = host_ms(lambda: insulation.insulation_from_sums(Sh, valid, w))
            ln.update(host_matrix_ms=round(t_mat, 1), host_sums_ms=round(t_sums, 1), host_rule_ms=round(t_rule, 1),
                      sums_bit_equal=bool(np.array_equal(S.cpu().numpy(), Sh)))
        lines.append(ln)
        print(json.dumps(ln), flush=True)
    if opt.out:
        os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
        with open(opt.out, "a") as f:
            f.write("".join(json.dumps(ln) + "\n" for ln in lines))


if __name__ == "__main__":
    main()
