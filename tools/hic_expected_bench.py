"""Times the distance sums, the expected vector and the distance-aware graph build (chromegcn_amd/hicdist.py,
csrc/cgcn_hicdist.hip, the *_dist passes of csrc/cgcn_hic.hip) on the GPU; fails without one.

For chr21- and chr1-size synthetic contacts (synth.raw_contacts, the record sets of tools/hic_build_bench.py), records
resident on the device, median of --reps calls after a warm one, host clock around the call and a device synchronise:
  * sums_raw_ms / sums_vector_ms: distance_sums without a norm vector and with the records' own one (caches cleared before
    every call: one or two launches of cgcn_hicdist_sums and their read-backs);
  * expected_ms: expected_vector end to end (the sums, the read-back of 2 n_bins doubles, expected_from_sums on the host, the
    upload), with w_max and the number of whole-range windows;
  * build_plain_ms: build_raw of the records with their norm vector at --hic-edges, as it was; build_oe_gap_ms: the same call
    with the expected vector of that norm vector (computed before, as in a sweep) and min_distance_bp = --gap;
    build_oe_first_ms: the same with expected="auto", which computes the vector inside the call; build_gap_ms: the gap alone, with the norm vector; survivors with and
    without the gap;
  * host_sums_ms, host_expected_from_sums_ms: the numpy restatements on this machine's CPU in the same run (one call each).
Prints one JSON line per chromosome and appends the lines to --out (default: profiles/hic_expected_bench.jsonl; '' = nowhere)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from chromegcn_amd import hic, hicdist, synth  # noqa: E402


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
    ap.add_argument("--hic-edges", type=int, default=500000)
    ap.add_argument("--gap", type=int, default=20000, help="min_distance_bp of the distance-aware build")
    ap.add_argument("--no-host", action="store_true", help="skip the CPU restatement")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "hic_expected_bench.jsonl"))
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/hic_expected_bench.py needs a GPU")
    dev = torch.device("cuda")
    lines = []
    for chrom in opt.chroms.split(","):
        r = synth.raw_contacts(chrom)
        res, ws = r["resolution_bp"], r["window_start"]
        c = hic.HicContacts(r["pos1"], r["pos2"], r["count"], dev)
        nv = torch.from_numpy(r["norm"]).to(dev)

        def fresh(fn):
            c._dist_sums.clear()
            c._expected.clear()
            return fn()

        sums_raw = timed(lambda: fresh(lambda: c.distance_sums(None, res)), opt.reps)
        sums_vec = timed(lambda: c.distance_sums(nv, res), opt.reps)   # a caller's vector is never kept
        exp_ms = timed(lambda: fresh(lambda: c.expected_vector(None, res)), opt.reps)
        ex, info = fresh(lambda: c.expected_vector(None, res, return_info=True))
        plain = timed(lambda: c.build_raw(nv, res, ws, opt.hic_edges), opt.reps)
        first = timed(lambda: c.build_raw(nv, res, ws, opt.hic_edges, expected="auto", min_distance_bp=opt.gap), opt.reps)
        ex_nv = c.expected_vector(nv, res)
        oe = timed(lambda: c.build_raw(nv, res, ws, opt.hic_edges, expected=ex_nv, min_distance_bp=opt.gap), opt.reps)
        gap_only = timed(lambda: c.build_raw(nv, res, ws, opt.hic_edges, min_distance_bp=opt.gap), opt.reps)
        ln = {"chrom": chrom, "M": c.M, "n_bins": int(ex.numel()), "hic_edges": opt.hic_edges, "gap_bp": opt.gap,
              "sums_raw_ms": round(sums_raw, 3), "sums_vector_ms": round(sums_vec, 3), "expected_ms": round(exp_ms, 3),
              "expected": info, "build_plain_ms": round(plain, 3), "build_gap_ms": round(gap_only, 3),
              "build_oe_gap_ms": round(oe, 3), "build_oe_first_ms": round(first, 3), "survivors": c.survivors(ws),
              "survivors_gap": c.survivors(ws, min_distance_bp=opt.gap)}
        if not opt.no_host:
            (raw, act), t_sums = host_ms(lambda: hicdist.distance_sums_host(r["pos1"], r["pos2"], r["count"], r["norm"], res))
            _, t_exp = host_ms(lambda: hicdist.expected_from_sums(raw, act))
            ln.update(host_sums_ms=round(t_sums, 1), host_expected_from_sums_ms=round(t_exp, 1))
        lines.append(ln)
        print(json.dumps(ln), flush=True)
    if opt.out:
        os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
        with open(opt.out, "a") as f:
            f.write("".join(json.dumps(ln) + "\n" for ln in lines))


if __name__ == "__main__":
    main()
