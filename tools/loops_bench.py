"""Times the loop passes (chromegcn_amd/loops.py, csrc/cgcn_loops.hip) on the GPU against the numpy restatement; fails without
a GPU.

For chr21- and chr1-size synthetic contacts (synth.raw_contacts), binned to --res, with the records' VC vector and "auto"
expected vector and the default rule of that resolution; device stages are the median of --reps calls after a warm one, host
clock around the call and a device synchronise:
  * band_ms: cgcn_hicloops_band with the zero fill of the band;
  * pass1_ms: cgcn_hicloops_pass1 with the zero fill of the histograms and of the packed records; pixels = n (D + 1), and
    pass1_bound_ms = pixels x cells x 5 LDS cycles / 64 lanes / (256 CUs x 2.4 GHz): two 8-byte reads at 2 cycles and one byte
    read at 1 cycle per wavefront and visited cell, cells = (2 w + 1)^2 - (2 p + 1)^2;
  * pass2_ms: cgcn_hicloops_count, the read-back of the count, cgcn_hicloops_write and the read-back of the list;
  * host_part_ms: the read-back of the histograms, loop_thresholds and loops_from_pixels;
  * loops_ms: HicContacts.loops end to end with the matrix and the vectors resident (the cache of results cleared);
  * host_lambdas_ms, host_hist_ms, host_pixels_ms: loop_lambdas_host, loop_histograms_host and enriched_pixels_host on this
    machine's CPU (one call each), and whether the device's histograms and pixel list equal them exactly.
Prints one JSON line per chromosome and appends the lines to --out (default: profiles/loops_bench.jsonl; '' = nowhere)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from chromegcn_amd import hic, hicmap, loops, synth  # noqa: E402


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
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-host", action="store_true", help="skip the CPU restatement")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "loops_bench.jsonl"))
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/loops_bench.py needs a GPU")
    dev = torch.device("cuda")
    lines = []
    for chrom in opt.chroms.split(","):
        rec = synth.raw_contacts(chrom)
        c = hic.HicContacts(rec["pos1"], rec["pos2"], rec["count"], dev)
        A = c.contact_matrix(opt.res)
        r = loops.loop_rule(opt.res, A.n)
        t = loops.chunk_boundaries(r.K)
        vc = c.norm_vector("VC", opt.res, n_bins=A.n)
        ex = c.expected_vector("VC", opt.res, n_bins=A.n)
        band_ms = timed(lambda: hicmap.device_band(A, r.width), opt.reps)
        band = hicmap.device_band(A, r.width)
        pass1_ms = timed(lambda: loops.loop_histograms(band, A.vc, vc, ex, r, t), opt.reps)
        hist, flags, _ = loops.loop_histograms(band, A.vc, vc, ex, r, t)
        thr = loops.loop_thresholds(hist.cpu().numpy(), r.fdr, t)
        pass2_ms = timed(lambda: loops.enriched_pixels(band, A.vc, vc, ex, r, flags, thr), opt.reps)
        pix = loops.enriched_pixels(band, A.vc, vc, ex, r, flags, thr)
        host_part, host_part_ms = host_ms(lambda: loops.loops_from_pixels(
            pix, r.res, A.n, r.ratios, r.radius_bins * r.res, r.min_cluster_pixels, t,
            {"thresholds": loops.loop_thresholds(hist.cpu().numpy(), r.fdr, t)}))

        def end_to_end():
            c._loops.clear()
            return c.loops("VC", opt.res, "auto", n_bins=A.n)

        loops_ms = timed(end_to_end, opt.reps)
        pixels, cells = A.n * (r.D + 1), (2 * r.w + 1) ** 2 - (2 * r.p + 1) ** 2
        ln = {"chrom": chrom, "M": c.M, "resolution_bp": opt.res, "n_bins": A.n, "nnz": A.nnz, "p": r.p, "w": r.w, "D": r.D,
              "pixels": pixels, "candidates": int(hist[0].sum().item()), "enriched": int(pix.i.size), "loops": len(host_part),
              "band_ms": round(band_ms, 3), "pass1_ms": round(pass1_ms, 3),
              "pass1_bound_ms": round(pixels * cells * 5 / 64 / (256 * 2.4e9) * 1e3, 4),
              "pass2_ms": round(pass2_ms, 3), "host_part_ms": round(host_part_ms, 1), "loops_ms": round(loops_ms, 3)}
        if not opt.no_host:
            host = A.to_host()
            hband = hicmap.band_host(host, r.width)
            nv, exh = vc.cpu().numpy(), ex.cpu().numpy()
            (lam, cand), t_lam = host_ms(lambda: loops.loop_lambdas_host(hband, np.asarray(host.sum(axis=1)).ravel(), nv, exh, r.p,
                                                                         r.w, r.D, r.ignore_diags, r.min_dist))
            hh, t_hist = host_ms(lambda: loops.loop_histograms_host(hband, lam, cand, t, r.W - 1))
            hp, t_pix = host_ms(lambda: loops.enriched_pixels_host(hband, lam, cand, thr, t, r.W - 1))
            ln.update(host_lambdas_ms=round(t_lam, 1), host_hist_ms=round(t_hist, 1), host_pixels_ms=round(t_pix, 1),
                      hist_equal=bool(np.array_equal(hist.cpu().numpy(), hh)),
                      pixels_equal=bool(np.array_equal(pix.i, hp.i) and np.array_equal(pix.j, hp.j)
                                        and np.array_equal(pix.lam, hp.lam)))
        lines.append(ln)
        print(json.dumps(ln), flush=True)
    if opt.out:
        os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
        with open(opt.out, "a") as f:
            f.write("".join(json.dumps(ln) + "\n" for ln in lines))


if __name__ == "__main__":
    main()
