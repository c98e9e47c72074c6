"""Times the top-K Hi-C contact graph build (chromegcn_amd/hic.py, csrc/cgcn_hic.hip) on the GPU; fails without one.

For chr21- and chr1-size synthetic contacts (synth.raw_contacts), hic_edges 250 k / 500 k / 1 M, with and without the norm
vector:
  * device_ms: cgcn_hic_build with the contacts resident, median of --reps calls after a warm one, each timed with a host
    clock around the call and a device synchronise (the normaliser that follows it is timed apart: normalise_ms);
  * host_ms: build_hic_graph_host on the same arrays on this machine's CPU (one call);
  * filter pass: 16 B x M over the time of ONE filter pass (cgcn_hic_count: the survivor count pass, the same kernel the
    build runs twice), beside a plain device copy of the same 16 B x M timed in the same run.
--resolution-bp 5000 times records coarser than the 1 kb windows instead (synth.raw_contacts_coarse), in one process:
  * device_ms: cgcn_hic_build_up on the compact records (window_bp = 1000);
  * expanded_device_ms (with its fastest and slowest call): cgcn_hic_build on the expand_contacts_host arrays of the same
    chromosome -- the same graph, which the tool asserts;
  * host_ms: build_hic_graph_host(window_bp = 1000) on the compact records;
  * one counting pass in ns per record read: the expanding filter on the compact records (up = 5), and on the expanded arrays
    the binary-search filter (cgcn_hic_count) beside the bitmap + rank filter at up = 1 (cgcn_hic_count_up).
Prints one JSON line per configuration and a closing table; --out FILE also writes the lines there (--append: adds them)."""
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


def timings(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def timed(fn, reps):
    return statistics.median(timings(fn, reps))


def coarse(opt, dev, kw):
    """the --resolution-bp rows: records coarser than the windows"""
    res, wbp, lines = opt.resolution_bp, 1000, []
    for chrom in opt.chroms.split(","):
        r = synth.raw_contacts_coarse(chrom, res, wbp, **kw)
        ws = r["window_start"]
        n, bins = int(ws.size), int(ws[-1]) // wbp + 1
        c = hic.HicContacts(r["pos1"], r["pos2"], r["count"], dev)
        e = hic.HicContacts(*hic.expand_contacts_host(r["pos1"], r["pos2"], r["count"], res, wbp), dev)
        s = c.survivors(ws, res, wbp)
        assert s == e.survivors(ws)
        cnt = torch.zeros(1, dtype=torch.int64, device=dev)

        def count_up(x, resolution):
            need = _lib.query("cgcn_hic_up_workspace_bytes", M=x.M, N=n, capacity=0, K=0, resolution_bp=resolution, window_bp=wbp,
                              n_window_bins=bins)
            wsp = torch.empty(need, dtype=torch.uint8, device=dev)
            return timed(lambda: _lib.call("cgcn_hic_count_up", M=x.M, pos1=x.pos1, pos2=x.pos2, window_start=x._ws_dev, N=n,
                                           resolution_bp=resolution, window_bp=wbp, n_window_bins=bins, workspace=wsp,
                                           workspace_bytes=need, n_survivors=cnt), opt.reps)

        need = _lib.query("cgcn_hic_workspace_bytes", M=e.M, N=n, capacity=0, K=0)
        wsp = torch.empty(need, dtype=torch.uint8, device=dev)
        search_ms = timed(lambda: _lib.call("cgcn_hic_count", M=e.M, pos1=e.pos1, pos2=e.pos2, window_start=e._ws_dev, N=n,
                                            workspace=wsp, workspace_bytes=need, n_survivors=cnt), opt.reps)
        del wsp
        up_ms, up1_ms = count_up(c, res), count_up(e, wbp)
        for use_norm in (False, True):
            norm = r["norm"] if use_norm else None
            for edges in [int(x) for x in opt.edges.split(",")]:
                device_ms = timed(lambda: c.build_raw(norm, res, ws, edges, window_bp=wbp), opt.reps)
                expanded = timings(lambda: e.build_raw(norm, res, ws, edges), opt.reps)
                got, want = c.build_raw(norm, res, ws, edges, window_bp=wbp), e.build_raw(norm, res, ws, edges)
                nnz = int(got[2][0])
                assert torch.equal(got[2], want[2]) and torch.equal(got[0], want[0]) and torch.equal(got[1][:nnz], want[1][:nnz])
                host_ms = None
                if not opt.no_host:
                    t0 = time.perf_counter()
                    a = hic.build_hic_graph_host(r["pos1"], r["pos2"], r["count"], norm, res, ws, edges, window_bp=wbp)
                    host_ms = (time.perf_counter() - t0) * 1e3
                    assert nnz == a.nnz
                lines.append({"chrom": chrom, "resolution_bp": res, "window_bp": wbp, "M": c.M, "M_expanded": e.M, "N": n,
                              "survivors": s, "hic_edges": edges, "norm": use_norm, "nnz": nnz, "device_ms": round(device_ms, 3),
                              "expanded_device_ms": round(statistics.median(expanded), 3),
                              "expanded_device_min_ms": round(min(expanded), 3), "expanded_device_max_ms": round(max(expanded), 3),
                              "host_ms": None if host_ms is None else round(host_ms, 1),
                              "count_up_pass_ms": round(up_ms, 3), "count_up_ns_per_record": round(up_ms * 1e6 / c.M, 4),
                              "expanded_search_pass_ms": round(search_ms, 3),
                              "expanded_search_ns_per_record": round(search_ms * 1e6 / e.M, 4),
                              "expanded_bitmap_pass_ms": round(up1_ms, 3),
                              "expanded_bitmap_ns_per_record": round(up1_ms * 1e6 / e.M, 4)})
                print(json.dumps(lines[-1]), flush=True)
    print("\n| chrom | M | M expanded | survivors | hic_edges | norm | compact ms | expanded ms (min .. max) | host ms |")
    print("|---|---|---|---|---|---|---|---|---|")
    for ln in lines:
        print("| %(chrom)s | %(M)d | %(M_expanded)d | %(survivors)d | %(hic_edges)d | %(norm)s | %(device_ms).3f | "
              "%(expanded_device_ms).3f (%(expanded_device_min_ms).3f .. %(expanded_device_max_ms).3f) | %(host_ms)s |" % ln)
    return lines


def write(opt, lines):
    if opt.out:
        os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
        with open(opt.out, "a" if opt.append else "w") as f:
            f.write("".join(json.dumps(ln) + "\n" for ln in lines))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--chroms", default="chr21,chr1")
    ap.add_argument("--edges", default="250000,500000,1000000")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-host", action="store_true", help="skip the CPU baseline")
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true", help="add the lines to --out instead of replacing it")
    ap.add_argument("--resolution-bp", type=int, default=1000, help="records coarser than the 1 kb windows (5000: K562)")
    ap.add_argument("--background-per-bin", type=float, default=None, help="synth.raw_contacts' density (default: its own)")
    ap.add_argument("--peak-pairs-per-window", type=float, default=None)
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/hic_build_bench.py needs a GPU")
    if opt.reps < 5:
        raise SystemExit("--reps must be at least 5")
    dev = torch.device("cuda")
    kw = {k: v for k, v in (("background_per_bin", opt.background_per_bin), ("peak_pairs_per_window", opt.peak_pairs_per_window))
          if v is not None}
    if opt.resolution_bp != 1000:
        return write(opt, coarse(opt, dev, kw))
    lines = []
    for chrom in opt.chroms.split(","):
        r = synth.raw_contacts(chrom, **kw)
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
    write(opt, lines)


if __name__ == "__main__":
    main()
