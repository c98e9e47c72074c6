"""Times every stage of the A/B compartment call (chromegcn_amd/compartments.py) on the device against the host's
np.corrcoef + np.linalg.eigh, on a synthetic chr1-shaped checkerboard map at 100 kb (n = 2493) and 50 kb (n = 4986), and reports
the achieved fp64 rate of the Pearson-map kernel.  It needs a GPU and fails without one.

    python tools/compartment_bench.py [--res 100000,50000] [--reps 50] [--steps 1000] [--no-host] [--json out.json]

How the numbers are taken: every shape is warmed up once; a stage is timed with device events around `reps` back-to-back
calls and the median of five such windows is reported, the in-place stage (O/E rows) once on copies made before its one window
opens; the power iteration is timed over `steps` enqueued steps (no read-back inside the window); `end_to_end_s` is a host
clock around HicContacts.compartments from resident records to the oriented result, device synchronised, aggregation and every
read-back included.  corr_needed_tflops is m^2 (m + 1) operations (2 m per element of the upper triangle with the diagonal,
what the symmetric product needs) over the kernel's time; corr_executed_tflops counts what the 64 x 64 tiles execute, padding
included.  MI355X's public fp64 peak is 78.6 TFLOP/s, vector and matrix alike.  The host figures are one run each of
np.corrcoef on the device's O/E map and np.linalg.eigh on the result."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from chromegcn_amd import compartments as CP  # noqa: E402
from chromegcn_amd import hic, hicmap  # noqa: E402

CHR1_BP = 249250621
FP64_PEAK_TFLOPS = 78.6


def checkerboard(n, res, seed=0):
    """records of a chr1-shaped map: compartments in runs of ~3 Mb, Poisson(2000 / (1 + d) * (1.6 | 0.6) + 0.5)"""
    rng = np.random.default_rng(seed)
    run = max(4, int(3e6) // res)
    comp = np.repeat(np.where(rng.random(-(-n // run)) < 0.5, 1, -1), run)[:n]
    a, b = np.triu_indices(n)
    c = rng.poisson(2000.0 / (1.0 + (b - a)) * np.where(comp[a] == comp[b], 1.6, 0.6) + 0.5).astype(np.float64)
    k = c > 0
    return (a[k] * res).astype(np.int32), (b[k] * res).astype(np.int32), c[k], comp


def timed(torch, fn, reps, windows=5):
    """seconds per call of fn(i), i = 0 .. reps - 1: device events around a window of `reps` calls, the median of `windows`"""
    out = []
    for _ in range(windows):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for i in range(reps):
            fn(i)
        stop.record()
        torch.cuda.synchronize()
        out.append(start.elapsed_time(stop) / 1e3 / reps)
    return float(np.median(out))


def bench_one(torch, res, reps, steps, host):
    n = -(-CHR1_BP // res)
    p1, p2, cnt, planted = checkerboard(n, res)
    hc = hic.HicContacts(p1, p2, cnt, "cuda")
    out = {"resolution_bp": res, "n_bins": n, "records": int(p1.size)}
    t0 = time.perf_counter()
    A = hc.contact_matrix(res, n)
    nv = hc.norm_vector("VC", res, n)
    torch.cuda.synchronize()
    out["aggregate_and_vc_s"] = time.perf_counter() - t0
    valid = hicmap.valid_bins(A.vc.cpu().numpy(), nv.cpu().numpy())
    keep, _ = CP.kept_bins(valid, res)
    m = int(keep.size)
    out["m"] = m
    B = CP.balanced_dense(A, nv, keep)                                   # warm-up of every stage, and the inputs of the next
    dsum = CP.dist_sums(B, keep, n)
    e = CP.expected_from_dist_sums(dsum.cpu().numpy(), CP.pair_counts(valid))
    e_dev = torch.from_numpy(e).to("cuda")
    Z = B.clone()
    CP.oe_rows(Z, keep, e_dev)
    C = CP.pearson(Z)
    v = torch.from_numpy(CP.start_vector(m)).to("cuda")
    y, w, rec = CP.power_step(C, v)
    out["dense_s"] = timed(torch, lambda i: CP.balanced_dense(A, nv, keep), reps)
    out["dist_sums_s"] = timed(torch, lambda i: CP.dist_sums(B, keep, n), reps)
    copies = [B.clone() for _ in range(min(reps, 16))]                   # M -> Z in place: one window only, each call on its own copy
    out["oe_rows_s"] = timed(torch, lambda i: CP.oe_rows(copies[i], keep, e_dev), len(copies), windows=1)
    del copies
    out["corr_s"] = timed(torch, lambda i: CP.pearson(Z), reps)
    tiles = -(-m // 64)
    out["corr_needed_tflops"] = m * m * (m + 1) / out["corr_s"] / 1e12
    out["corr_executed_tflops"] = tiles * (tiles + 1) // 2 * 64 * 64 * 2 * (-(-m // 16) * 16) / out["corr_s"] / 1e12
    out["corr_needed_share_of_fp64_peak"] = out["corr_needed_tflops"] / FP64_PEAK_TFLOPS
    bufs = [v.clone(), w]
    out["step_s"] = timed(torch, lambda i: CP.power_step(C, bufs[i & 1], None, y, bufs[1 - (i & 1)], rec), steps)
    out["step_matrix_gbytes_per_s"] = 8.0 * m * m / out["step_s"] / 1e9
    hc._compartments.clear()
    t0 = time.perf_counter()
    comp = hc.compartments("VC", res, n_bins=n, orient=planted.astype(np.float64))
    torch.cuda.synchronize()
    out["end_to_end_s"] = time.perf_counter() - t0
    out["iterations"], out["converged"], out["host_syncs"] = comp.info["iterations"], comp.info["converged"], comp.info["host_syncs"]
    out["planted_recovered"] = float(np.mean(comp.compartment_of_bin[keep] == planted[keep]))
    if host:
        M = B.clone()
        CP.oe_rows(M, keep, e_dev, stages=1)
        Mh = M.cpu().numpy()[:, :m]
        t0 = time.perf_counter()
        Ch = np.corrcoef(Mh)
        out["host_corrcoef_s"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        lam, V = np.linalg.eigh(Ch)
        out["host_eigh_s"] = time.perf_counter() - t0
        u = V[:, -1]
        g = comp.E[0, keep]
        out["max_abs_diff_to_eigh"] = float(np.nanmax(np.abs(g - (u if float(u @ np.nan_to_num(g)) >= 0 else -u))))
        out["lambda2_over_lambda1"] = float(lam[-2] / lam[-1])
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--res", default="100000,50000")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--no-host", action="store_true", help="skip np.corrcoef + np.linalg.eigh")
    ap.add_argument("--json", default=None, help="also write the results to this file")
    opt = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/compartment_bench.py needs a GPU: a CPU run says nothing about the device")
    results = [bench_one(torch, int(r), opt.reps, opt.steps, not opt.no_host) for r in opt.res.split(",")]
    for r in results:
        print(json.dumps(r))
    if opt.json:
        with open(opt.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1:])
