"""Times the top-K Hi-C contact graph build (chromegcn_amd/hic.py, csrc/cgcn_hic.hip) on the GPU; fails without one.

For chr21- and chr1-size synthetic contacts (synth.raw_contacts), hic_edges 250 k / 500 k / 1 M, with and without the norm
vector:
  * device_ms: cgcn_hic_build with the contacts resident, median of --reps calls after a warm one, each timed with a host
    clock around the call and a device synchronise (the normaliser that follows it is timed apart: normalise_ms);
  * host_ms: build_hic_graph_host on the same arrays on this machine's CPU (one call);
  * filter pass: 16 B x M over the time of ONE filter pass (cgcn_hic_count: the survivor count pass, the same kernel the
    build runs twice), beside a plain device copy of the same 16 B x M timed in the same run.
Prints one JSON line per configuration and a closing table; --out FILE also writes the lines there."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from chromegcn_amd import _lib, graph as G, hic, synth  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--chroms", default="chr21,chr1")
    ap.add_argument("--edges", default="250000,500000,1000000")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-host", action="store_true", help="skip the CPU baseline")
    ap.add_argument("--out", default=None)
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/hic_build_bench.py needs a GPU")
    if opt.reps < 5:
        raise SystemExit("--reps must be at least 5")
    dev = torch.device("cuda")
    lines = []
    for chrom in opt.chroms.split(","):
        r = synth.raw_contacts(chrom)
        c = hic.HicContacts(r["pos1"], r["pos2"], r["count"], dev)
        ws, res = r["window_start"], r["resolution_bp"]
        s = c.survivors(ws)
        nbytes = 16 * c.M
        # one filter pass, and a plain copy of as many bytes
        need = _lib.query("cgcn_hic_workspace_bytes", M=c.M, N=int(ws.size), capacity=0, K=0)
        wsp, cnt = torch.empty(need, dtype=torch.uint8, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
        filter_ms = timed(lambda: _lib.call("cgcn_hic_count", M=c.M, pos1=c.pos1, pos2=c.pos2, window_start=c._ws_dev,
                                            N=int(ws.size), workspace=wsp, workspace_bytes=need, n_survivors=cnt), opt.reps)
        src, dst = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev), torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
        copy_ms = timed(lambda: dst.copy_(src), opt.reps)   # reads nbytes / 2 and writes nbytes / 2: nbytes moved
        del src, dst
        for use_norm in (False, True):
            norm = r["norm"] if use_norm else None
            for edges in [int(e) for e in opt.edges.split(",")]:
                device_ms = timed(lambda: c.build_raw(norm, res, ws, edges), opt.reps)
                rowptr, col, sizes = c.build_raw(norm, res, ws, edges)
                normalise_ms = timed(lambda: G.normalize_device_csr("hic", int(ws.size), rowptr, col, None, dev), opt.reps)
                host_ms = None
                if not opt.no_host:
                    t0 = time.perf_counter()
                    a = hic.build_hic_graph_host(r["pos1"], r["pos2"], r["count"], norm, res, ws, edges)
                    host_ms = (time.perf_counter() - t0) * 1e3
                    assert int(sizes[0]) == a.nnz
                lines.append({"chrom": chrom, "M": c.M, "N": int(ws.size), "survivors": s, "hic_edges": edges, "norm": use_norm,
                              "nnz": int(sizes[0]), "device_ms": round(device_ms, 3), "normalise_ms": round(normalise_ms, 3),
                              "host_ms": None if host_ms is None else round(host_ms, 1),
                              "speedup": None if host_ms is None else round(host_ms / device_ms, 1),
                              "filter_pass_ms": round(filter_ms, 3), "filter_GBps": round(nbytes / filter_ms / 1e6, 1),
                              "copy_ms": round(copy_ms, 3), "copy_GBps": round(nbytes / copy_ms / 1e6, 1)})
                print(json.dumps(lines[-1]), flush=True)
    print("\n| chrom | M | survivors | hic_edges | norm | device ms | host ms | x | filter GB/s | copy GB/s |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for ln in lines:
        print("| %(chrom)s | %(M)d | %(survivors)d | %(hic_edges)d | %(norm)s | %(device_ms).3f | %(host_ms)s | %(speedup)s | "
              "%(filter_GBps).1f | %(copy_GBps).1f |" % ln)
    if opt.out:
        os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
        with open(opt.out, "w") as f:
            f.write("".join(json.dumps(ln) + "\n" for ln in lines))


if __name__ == "__main__":
    main()
