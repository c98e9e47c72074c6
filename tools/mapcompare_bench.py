"""Times the map comparison (chromegcn_amd/mapcompare.py, csrc/cgcn_mapcompare.hip) on the GPU against the numpy restatement;
fails without a GPU.

For chr21- and chr1-size synthetic contacts (synth.raw_contacts, two seeds: two maps of one shape), at --cases resolution:h pairs
(default 40000:5 and 10000:20), observed counts (norm = None), the default reach of 5 Mb.  Device stages are the median of --reps
calls after a warm one, between two device events on the current stream:
  * band_ms: hicmap.device_band of both maps (cgcn_hicloops_band with the zero fill of the band);
  * smooth_ms: cgcn_mapcmp_smooth of both maps; smooth_gbs = 2 maps x (n x width + (D + 1) x ld) x 8 B / smooth_ms, the bytes the
    kernel must move (the halo re-reads hit a cache and are not counted); smooth_gadds = the fp64 additions the kernel performs
    (per tile of 32 x 32 cells: (32 + 2 h) x 32 row sums and 32 x 32 column sums of 2 h + 1 terms each) / smooth_ms;
  * sums_ms: both passes of cgcn_mapcmp_sums with their folds, nothing read back;
  * scc_ms: HicContacts.scc end to end with the matrices resident (bands, validity, smoothing, sums, the read-backs, scores);
  * host_smooth_ms, host_sums_ms, host_scc_ms: smooth_strata_host (both maps), stratum_sums_host and map_scc_host on this machine's
    CPU (one call each), and whether the device's strata and sums equal them bit for bit.
Prints one JSON line per chromosome and case and appends the lines to --out (default: profiles/mapcompare_bench.jsonl; '' =
nowhere)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from chromegcn_amd import hic, hicmap, mapcompare, synth  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        out.append(t0.elapsed_time(t1))
    return statistics.median(out)


def host_ms(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--chroms", default="chr21,chr1")
    ap.add_argument("--cases", default="40000:5,10000:20", help="resolution_bp:h pairs")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-host", action="store_true", help="skip the CPU restatement")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "mapcompare_bench.jsonl"))
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/mapcompare_bench.py needs a GPU")
    dev = torch.device("cuda")
    lines = []
    same = lambda a, b: bool(np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64)))  # noqa: E731
    for chrom in opt.chroms.split(","):
        recs = [synth.raw_contacts(chrom), synth.raw_contacts(chrom, seed=synth.chrom_seed(chrom) + 7001)]
        maps = [hic.HicContacts(r["pos1"], r["pos2"], r["count"], dev) for r in recs]
        for case in opt.cases.split(","):
            res, h = (int(x) for x in case.split(":"))
            n = max(m.contact_matrix(res).n for m in maps)
            A, B = (m.contact_matrix(res, n) for m in maps)
            r = mapcompare.scc_rule(res, n, h)
            D, ld = r.max_dist, mapcompare.leading_dim(n)
            band_ms = timed(lambda: (hicmap.device_band(A, r.width), hicmap.device_band(B, r.width)), opt.reps)
            ba, bb = hicmap.device_band(A, r.width), hicmap.device_band(B, r.width)
            smooth_ms = timed(lambda: (mapcompare.smooth_strata(ba, None, h, D), mapcompare.smooth_strata(bb, None, h, D)), opt.reps)
            Sa, Sb = mapcompare.smooth_strata(ba, None, h, D), mapcompare.smooth_strata(bb, None, h, D)
            valid = mapcompare.valid_bins_device(A.vc, None) & mapcompare.valid_bins_device(B.vc, None)
            sums_ms = timed(lambda: mapcompare.stratum_sums_device(Sa, Sb, valid, n, r.min_dist), opt.reps)
            scc_ms = timed(lambda: maps[0].scc(maps[1], resolution_bp=res, h=h), opt.reps)
            got = maps[0].scc(maps[1], resolution_bp=res, h=h)
            tiles = -(-ld // 32) * -(-(32 + D) // 32)
            adds = tiles * ((32 + 2 * h) * 32 + 32 * 32) * (2 * h + 1) * 2
            ln = {"chrom": chrom, "resolution_bp": res, "h": h, "n_bins": n, "D": D, "width": r.width, "nnz": [A.nnz, B.nnz],
                  "band_ms": round(band_ms, 3), "smooth_ms": round(smooth_ms, 3),
                  "smooth_gbs": round(2 * (n * r.width + (D + 1) * ld) * 8 / smooth_ms / 1e6, 1),
                  "smooth_gadds": round(adds / smooth_ms / 1e6, 1), "sums_ms": round(sums_ms, 3),
                  "sums_gbs": round(2 * 2 * (D + 1) * ld * 8 / sums_ms / 1e6, 1), "scc_ms": round(scc_ms, 3),
                  "scc": round(got.scc, 6), "strata": got.n_strata}
            if not opt.no_host:
                ha, hb = (hicmap.band_host(M.to_host(), r.width) for M in (A, B))
                (hSa, hSb), t_smooth = host_ms(lambda: (mapcompare.smooth_strata_host(ha, None, h, D),
                                                        mapcompare.smooth_strata_host(hb, None, h, D)))
                want, t_sums = host_ms(lambda: mapcompare.stratum_sums_host(hSa, hSb, got.valid, n, r.min_dist))
                _, t_all = host_ms(lambda: mapcompare.map_scc_host(*[(q["pos1"], q["pos2"], q["count"]) for q in recs],
                                                                   resolution_bp=res, h=h))
                ln.update(host_smooth_ms=round(t_smooth, 1), host_sums_ms=round(t_sums, 1), host_scc_ms=round(t_all, 1),
                          strata_equal=same(Sa.cpu().numpy(), hSa) and same(Sb.cpu().numpy(), hSb),
                          sums_equal=all(same(getattr(got.sums, k), getattr(want, k)) for k in mapcompare.StratumSums._fields))
            lines.append(ln)
            print(json.dumps(ln), flush=True)
    if opt.out:
        os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
        with open(opt.out, "a") as f:
            f.write("".join(json.dumps(ln) + "\n" for ln in lines))


if __name__ == "__main__":
    main()
