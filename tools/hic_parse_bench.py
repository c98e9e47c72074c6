"""Times contact text -> device-resident records (chromegcn_amd.hic.contacts_from_text, csrc/cgcn_text.hip) on the GPU; fails
without one.

Per chromosome size (synth.raw_contacts written as a Juicer dump, %d<TAB>%d<TAB>%.1f, into --dir and read once so that it
sits in the page cache):
  (a) host_s: hic.load_contacts_text (numpy.loadtxt) of the file on this machine's CPU, --host-reps runs;
  (b) device_s: contacts_from_text end to end, --reps runs after a warm one, and once more with a device sync behind every
      stage: file read, host-to-device copy (what the read did not hide), count pass, parse pass, slow-line patch;
      parse_pass_ms: cgcn_text_parse alone on the resident text, median of --reps calls;
  (c) copy_ms: a plain device copy_ of the same byte count, the floor of the parse pass.
Appends one JSON line per size to --out (default profiles/hic_parse_bench.jsonl) and prints them."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from chromegcn_amd import _lib, hic, synth  # noqa: E402


def write_juicer(path, r, block=1 << 20):
    with open(path, "wb") as f:
        for lo in range(0, r["pos1"].size, block):
            rows = zip(r["pos1"][lo:lo + block].tolist(), r["pos2"][lo:lo + block].tolist(), r["count"][lo:lo + block].tolist())
            f.write("".join("%d\t%d\t%.1f\n" % row for row in rows).encode())


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--chroms", default="chr21,chr1")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--dir", default=None, help="where the text files are written (default: a temporary directory)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "hic_parse_bench.jsonl"))
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/hic_parse_bench.py needs a GPU")
    import tempfile
    dev = torch.device("cuda")
    with tempfile.TemporaryDirectory(dir=opt.dir) as tmp:
        for chrom in opt.chroms.split(","):
            r = synth.raw_contacts(chrom)
            path = os.path.join(tmp, "%s_1kb.RAWobserved" % chrom)
            write_juicer(path, r)
            n = os.path.getsize(path)
            with open(path, "rb") as f:   # into the page cache
                while f.read(1 << 24):
                    pass
            print("%s: %d lines, %d bytes" % (chrom, r["pos1"].size, n), flush=True)
            c = hic.contacts_from_text(path, device=dev)   # the warm one; checked against the arrays the text was written from
            assert c.M == r["pos1"].size and c.text_info["slow_lines"].size == 0 and c.text_info["parse_calls"] == 1
            assert np.array_equal(c.pos1.cpu().numpy(), r["pos1"]) and np.array_equal(c.pos2.cpu().numpy(), r["pos2"])
            assert np.array_equal(c.count.cpu().numpy(), r["count"])
            del c
            device_s = []
            for _ in range(opt.reps):
                t0 = time.perf_counter()
                c = hic.contacts_from_text(path, device=dev)
                torch.cuda.synchronize()
                device_s.append(time.perf_counter() - t0)
                del c
            stages = {}
            hic.contacts_from_text(path, device=dev, timings=stages)
            # the parse pass alone, on the resident text, and a copy of as many bytes
            text = torch.from_numpy(np.fromfile(path, dtype=np.uint8)).to(dev)
            m = r["pos1"].size
            need = _lib.query("cgcn_text_workspace_bytes", n_bytes=n)
            wsp = torch.empty(need, dtype=torch.uint8, device=dev)
            p1, p2 = torch.empty(m, dtype=torch.int32, device=dev), torch.empty(m, dtype=torch.int32, device=dev)
            cnt, flags = torch.empty(m, dtype=torch.float64, device=dev), torch.empty((1024, 3), dtype=torch.int64, device=dev)
            totals = torch.zeros(2, dtype=torch.int64, device=dev)

            def timed(fn):
                fn()
                torch.cuda.synchronize()
                out = []
                for _ in range(opt.reps):
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    out.append((time.perf_counter() - t0) * 1e3)
                return out

            parse_ms = timed(lambda: _lib.call("cgcn_text_parse", text=text, n_bytes=n, M=m, pos1_out=p1, pos2_out=p2, count_out=cnt,
                                               flags=flags, flag_capacity=1024, flag_totals=totals, workspace=wsp,
                                               workspace_bytes=need))
            dst = torch.empty_like(text)
            copy_ms = timed(lambda: dst.copy_(text))
            del text, dst, p1, p2, cnt, wsp
            host_s = []
            for _ in range(opt.host_reps):
                t0 = time.perf_counter()
                h = hic.load_contacts_text(path)
                host_s.append(time.perf_counter() - t0)
            assert h.M == m
            line = {"chrom": chrom, "lines": int(m), "bytes": int(n), "host_loadtxt_s": [round(x, 3) for x in host_s],
                    "device_end_to_end_s": [round(x, 4) for x in device_s],
                    "stages_s": {k: round(v, 5) for k, v in stages.items()},
                    "parse_pass_ms": [round(x, 3) for x in parse_ms], "copy_ms": [round(x, 3) for x in copy_ms],
                    "parse_over_copy": round(statistics.median(parse_ms) / statistics.median(copy_ms), 2),
                    "slowest_device_over_fastest_host": round(max(device_s) / min(host_s), 4),
                    "kept": max(device_s) < min(host_s)}
            print(json.dumps(line), flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
            with open(opt.out, "a") as f:
                f.write(json.dumps(line) + "\n")
            os.remove(path)


if __name__ == "__main__":
    main()
