"""Times the pile-up passes (chromegcn_amd/pileup.py, csrc/cgcn_pileup.hip) on the GPU against the numpy restatement; fails
without a GPU.

For chr21- and chr1-size synthetic contacts (synth.raw_contacts), binned to --res, with the records' VC vector and "auto"
expected vector, value = "oe" and the default rule of that resolution (w = 10 at 10 kb).  The centres are the --centres
records of the largest counts among those at a legal distance, one group unless --groups: what a top-K graph's edges look like.
Device stages are the median of --reps calls after a warm one, host clock around the call and a device synchronise:
  * band_ms: cgcn_hicloops_band with the zero fill of the band;
  * values_ms: cgcn_pileup_values;
  * keep_ms: the keep test, the stable sort and the read-back of the sizes (torch);
  * slices_ms: cgcn_pileup_slices alone, workspace and slice table resident; slices_gbs = M x (2 w + 1)^2 x 8 B / slices_ms,
    the rate of the value reads the pass asks for (most of them hit a cache: neighbouring offsets and centres share lines);
  * fold_ms: cgcn_pileup_fold alone;
  * sums_ms: pileup_sums end to end (keep, table upload, slices, fold, read-back of P and N);
  * host_values_ms, host_sums_ms: value_band_host and pileup_sums_host on this machine's CPU (one call each), and whether the
    device's value band, P and N equal them bit for bit.
Prints one JSON line per chromosome and appends the lines to --out (default: profiles/pileup_bench.jsonl; '' = nowhere)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from chromegcn_amd import _lib, hic, hicmap, pileup, synth  # noqa: E402


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
    ap.add_argument("--centres", type=int, default=500000)
    ap.add_argument("--groups", type=int, default=1, help="distance quantile groups of the centres")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-host", action="store_true", help="skip the CPU restatement")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "pileup_bench.jsonl"))
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/pileup_bench.py needs a GPU")
    dev = torch.device("cuda")
    lines = []
    for chrom in opt.chroms.split(","):
        rec = synth.raw_contacts(chrom)
        c = hic.HicContacts(rec["pos1"], rec["pos2"], rec["count"], dev)
        A = c.contact_matrix(opt.res)
        G = opt.groups
        r = pileup.pileup_rule(opt.res, A.n, G)
        vc = c.norm_vector("VC", opt.res, n_bins=A.n)
        ex = c.expected_vector("VC", opt.res, n_bins=A.n)
        # the centres: the records of the largest counts at a legal distance, in record order
        b1, b2 = (c.pos1 // opt.res).long(), (c.pos2 // opt.res).long()
        d = (b2 - b1).abs()
        score = torch.where((d >= r.min_dist) & (d <= r.max_dist), c.count, torch.full_like(c.count, -1.0))
        top = torch.sort(torch.topk(score, min(opt.centres, c.M)).indices).values
        top = top[score[top] > 0]
        ci, cj = b1[top].contiguous(), b2[top].contiguous()
        group = None if G == 1 else torch.from_numpy(pileup.quantile_groups(d[top].cpu().numpy(), G)).to(dev)
        M = int(ci.numel())
        band_ms = timed(lambda: hicmap.device_band(A, r.width), opt.reps)
        band = hicmap.device_band(A, r.width)
        values_ms = timed(lambda: pileup.value_band(band, A.vc, vc, ex, r), opt.reps)
        vb = pileup.value_band(band, A.vc, vc, ex, r)
        g = torch.zeros_like(ci) if group is None else group
        keep_ms = timed(lambda: pileup.keep_centres(ci, cj, g, G, A.n, r), opt.reps)
        i, j, kept, skipped = pileup.keep_centres(ci, cj, g, G, A.n, r)
        slice_off, group_off = pileup.slice_table(kept)
        ns = slice_off.size - 1
        wsp, need = _lib.workspace_for("cgcn_pileup_workspace_bytes", dev, "pile-up bench", n_slices=ns, w=r.w)
        so, go = torch.from_numpy(slice_off).to(dev), torch.from_numpy(group_off).to(dev)
        P = torch.empty(G, r.S, r.S, dtype=torch.float64, device=dev)
        N = torch.empty(G, r.S, r.S, dtype=torch.int64, device=dev)
        slices_ms = timed(lambda: _lib.call("cgcn_pileup_slices", n=A.n, width=r.width, vband=vb, w=r.w, n_slices=ns, slice_off=so,
                                            n_centres=int(i.numel()), ci=i, cj=j, workspace=wsp, workspace_bytes=need), opt.reps)
        fold_ms = timed(lambda: _lib.call("cgcn_pileup_fold", n_groups=G, w=r.w, n_slices=ns, group_off=go, workspace=wsp,
                                          workspace_bytes=need, P=P, N=N), opt.reps)
        sums_ms = timed(lambda: pileup.pileup_sums(vb, ci, cj, group, G, r), opt.reps)
        got = pileup.pileup_sums(vb, ci, cj, group, G, r)
        K = int(kept.sum())
        s = got.scores()
        ln = {"chrom": chrom, "M": c.M, "resolution_bp": opt.res, "n_bins": A.n, "nnz": A.nnz, "w": r.w, "width": r.width,
              "centres": M, "kept": K, "groups": G, "slices": ns, "band_ms": round(band_ms, 3), "values_ms": round(values_ms, 3),
              "values_gbs": round(2 * A.n * r.width * 8 / values_ms / 1e6, 1), "keep_ms": round(keep_ms, 3),
              "slices_ms": round(slices_ms, 3), "slices_gbs": round(K * r.S * r.S * 8 / slices_ms / 1e6, 1),
              "fold_ms": round(fold_ms, 3), "sums_ms": round(sums_ms, 3), "P2LL": round(float(s["P2LL"][0]), 4),
              "P2M": round(float(s["P2M"][0]), 4)}
        if not opt.no_host:
            host = A.to_host()
            hband = hicmap.band_host(host, r.width)
            nv, exh = vc.cpu().numpy(), ex.cpu().numpy()
            hvb, t_vb = host_ms(lambda: pileup.value_band_host(hband, np.asarray(host.sum(axis=1)).ravel(), nv, exh, r))
            hci, hcj, hg = ci.cpu().numpy(), cj.cpu().numpy(), None if group is None else group.cpu().numpy()
            want, t_sums = host_ms(lambda: pileup.pileup_sums_host(hvb, hci, hcj, hg, G, r))
            same = lambda a, b: bool(np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64)))  # noqa: E731
            ln.update(host_values_ms=round(t_vb, 1), host_sums_ms=round(t_sums, 1), values_equal=same(vb.cpu().numpy(), hvb),
                      sums_equal=same(got.sum, want.sum) and bool(np.array_equal(got.count, want.count)))
        lines.append(ln)
        print(json.dumps(ln), flush=True)
    if opt.out:
        os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
        with open(opt.out, "a") as f:
            f.write("".join(json.dumps(ln) + "\n" for ln in lines))


if __name__ == "__main__":
    main()
