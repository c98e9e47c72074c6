"""Times the Hi-C norm vectors computed from the contact records (chromegcn_amd/hicnorm.py, csrc/cgcn_hicnorm.hip) on the GPU;
fails without one.

For chr21- and chr1-size synthetic contacts (synth.raw_contacts, the record sets of tools/hic_build_bench.py), records
resident on the device:
  * aggregate_ms: records -> symmetric fp64 CSR with VC and the row counts (cgcn_hicnorm_count, the read-back of the sizes,
    cgcn_hicnorm_fill), median of --reps calls after a warm one, host clock around the call and a device synchronise;
  * vc_ms: the VC vector from the aggregated matrix;
  * kr_ms: Knight-Ruiz at tol 1e-6 from the aggregated matrix, with its products, outer updates and host read-backs, and
    kr_ms_per_product; spmv_ms: one product alone;
  * host_*_ms: the numpy / scipy restatement on the same records on this machine's CPU, in the same run (one call each).
Prints one JSON line per chromosome and appends the lines to --out (default: profiles/hic_norm_bench.jsonl; '' = nowhere).
--kr-only CHROM runs one aggregation and one KR call and nothing else.  The tool does not start a profiler itself (a process
that has the GPU open does not spawn another one around itself): profiles/hic_norm_kernel_stats.csv is
`rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 tools/hic_norm_bench.py --kr-only chr21`, a run of
its own, whose `*kernel_stats.csv` is copied there."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from chromegcn_amd import hic, hicnorm, synth  # noqa: E402


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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tol", type=float, default=1e-6)
    ap.add_argument("--no-host", action="store_true", help="skip the CPU restatement")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "hic_norm_bench.jsonl"))
    ap.add_argument("--kr-only", default=None, metavar="CHROM")
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/hic_norm_bench.py needs a GPU")
    dev = torch.device("cuda")
    if opt.kr_only:
        r = synth.raw_contacts(opt.kr_only)
        c = hic.HicContacts(r["pos1"], r["pos2"], r["count"], dev)
        _, info = c.norm_vector("KR", r["resolution_bp"], tol=opt.tol, return_info=True)
        torch.cuda.synchronize()
        print(json.dumps({"chrom": opt.kr_only, "kr": info}))
        return
    lines = []
    for chrom in opt.chroms.split(","):
        r = synth.raw_contacts(chrom)
        res = r["resolution_bp"]
        c = hic.HicContacts(r["pos1"], r["pos2"], r["count"], dev)
        agg_ms = timed(lambda: hicnorm.aggregate_contacts(c.pos1, c.pos2, c.count, res), opt.reps)
        a = c.contact_matrix(res)
        vc_ms = timed(lambda: hicnorm.vector_from_matrix(a, "VC"), opt.reps)
        y = torch.empty(a.n, dtype=torch.float64, device=dev)
        spmv_ms = timed(lambda: hicnorm.spmv(a, x=a.vc, p=a.vc, out=y), opt.reps)
        kr_ms = timed(lambda: hicnorm.kr_balance_device(a, tol=opt.tol), opt.reps)
        _, info = hicnorm.kr_balance_device(a, tol=opt.tol)
        ln = {"chrom": chrom, "M": c.M, "n_bins": a.n, "nnz": a.nnz, "tol": opt.tol, "aggregate_ms": round(agg_ms, 3),
              "vc_ms": round(vc_ms, 3), "spmv_ms": round(spmv_ms, 4), "kr_ms": round(kr_ms, 3), "kr": info,
              "kr_ms_per_product": round(kr_ms / max(info["mvp"], 1), 4)}
        if not opt.no_host:
            ah, t_agg = host_ms(lambda: hicnorm.contact_matrix_host(r["pos1"], r["pos2"], r["count"], res))
            _, t_vc = host_ms(lambda: hicnorm._vector_from_stats_host("VC", hicnorm._row_stats_host(ah)[0]))
            (_, ih), t_kr = host_ms(lambda: hicnorm.kr_balance_host(ah, tol=opt.tol))
            ln.update(host_aggregate_ms=round(t_agg, 1), host_vc_ms=round(t_vc, 1), host_kr_ms=round(t_kr, 1), host_kr=ih,
                      host_kr_ms_per_product=round(t_kr / max(ih["mvp"], 1), 3))
        lines.append(ln)
        print(json.dumps(ln), flush=True)
    if opt.out:
        os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
        with open(opt.out, "a") as f:
            f.write("".join(json.dumps(ln) + "\n" for ln in lines))


if __name__ == "__main__":
    main()
