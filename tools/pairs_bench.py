"""Times read-pair text -> contact records (chromegcn_amd.pairs.ReadPairs, csrc/cgcn_pairs.hip) on the GPU; fails without one.

Per size (synth.read_pairs over chr1 ... chr22 at their hg19 lengths, written in blocks of 10^6 lines with a seed each into
--dir and read once so that it sits in the page cache):
  (a) host_s: bin_read_pairs_host + pairs_to_contacts_host of every chromosome on this machine's CPU, --host-reps runs;
  (b) device_s: ReadPairs.from_text + contacts_all() end to end, --reps runs after a warm one, and once more with a device
      sync behind every stage: file read, host-to-device copy (what the read did not hide), cgcn_pairs_parse (parse and
      compaction are one call), host patch, cgcn_pairs_reduce (sort and run-length are one call);
      parse_call_ms: cgcn_pairs_parse alone on one resident chunk of --chunk-bytes, median of --reps calls;
  (c) copy_ms: a plain device copy_ of that chunk's byte count.
The warm run is checked against the host's result.  Appends one JSON line per size to --out (default
profiles/pairs_bench.jsonl) and prints them."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from chromegcn_amd import _lib, pairs, synth  # noqa: E402

SIZES = {c: n for c, n in synth.HG19_LEN.items()}
CHROMS = list(SIZES)


def write_pairs(path, n_lines, block=1000000):
    with open(path, "wb") as f:
        for k, lo in enumerate(range(0, n_lines, block)):
            f.write(synth.read_pairs(SIZES, min(block, n_lines - lo), 100 + k))


def host_run(path):
    with open(path, "rb") as f:
        data = f.read()
    hp = pairs.bin_read_pairs_host(data, chroms=CHROMS)
    return hp, {c: hp.contacts(c) for c in CHROMS}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lines", default="4000000,16000000", help="comma-separated file sizes in lines")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--chunk-bytes", type=int, default=32 << 20)
    ap.add_argument("--dir", default=None, help="where the text files are written (default: a temporary directory)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "pairs_bench.jsonl"))
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/pairs_bench.py needs a GPU")
    import tempfile
    dev = torch.device("cuda")
    with tempfile.TemporaryDirectory(dir=opt.dir) as tmp:
        for n_lines in [int(x) for x in opt.lines.split(",")]:
            path = os.path.join(tmp, "synthetic_%d_allValidPairs.txt" % n_lines)
            write_pairs(path, n_lines)
            n = os.path.getsize(path)
            with open(path, "rb") as f:   # into the page cache
                while f.read(1 << 24):
                    pass
            print("%d lines, %d bytes" % (n_lines, n), flush=True)

            def device_run(timings=None):
                rp = pairs.ReadPairs.from_text(path, chroms=CHROMS, device=dev, chunk_bytes=opt.chunk_bytes, timings=timings)
                recs = rp.contacts_all(timings)
                torch.cuda.synchronize()
                return rp, recs

            rp, recs = device_run()   # the warm one; checked against the host below
            device_s = []
            for _ in range(opt.reps):
                t0 = time.perf_counter()
                device_run()
                device_s.append(time.perf_counter() - t0)
            stages = {}
            device_run(stages)
            host_s = []
            for _ in range(opt.host_reps):
                t0 = time.perf_counter()
                hp, want = host_run(path)
                host_s.append(time.perf_counter() - t0)
            assert pairs.same_info(rp.info, hp.info)
            for c in CHROMS:
                assert np.array_equal(recs[c].pos1.cpu().numpy(), want[c][0]) and np.array_equal(recs[c].pos2.cpu().numpy(), want[c][1])
                assert np.array_equal(recs[c].count.cpu().numpy(), want[c][2])
            records, kept, calls = sum(r.M for r in recs.values()), rp.info["kept"], rp.info["parse_calls"]
            del rp, recs, hp, want
            # cgcn_pairs_parse alone on one resident chunk of whole lines, and a copy of as many bytes
            with open(path, "rb") as f:
                head = f.read(min(n, opt.chunk_bytes))
            head = head[:head.rfind(b"\n") + 1]
            nb = len(head)
            text = torch.frombuffer(bytearray(head), dtype=torch.uint8).to(dev)
            table = np.zeros((len(CHROMS), 16), np.uint8)
            for k, nm in enumerate(CHROMS):
                table[k, :len(nm)] = np.frombuffer(nm.encode(), np.uint8)
                table[k, 15] = len(nm)
            names = torch.from_numpy(table).to(dev)
            need = _lib.query("cgcn_pairs_parse_workspace_bytes", n_bytes=nb)
            wsp = torch.empty(need, dtype=torch.uint8, device=dev)
            keys = torch.empty(nb // 9 + 1, dtype=torch.int64, device=dev)
            flags = torch.empty((1024, 4), dtype=torch.int64, device=dev)
            totals = torch.zeros((2, 8), dtype=torch.int64, device=dev)

            def parse():
                totals.zero_()
                _lib.call("cgcn_pairs_parse", text=text, n_bytes=nb, byte_base=0, names=names, n_chroms=len(CHROMS),
                          resolution_bp=1000, binning=0, min_diff=10, keys=keys, key_capacity=keys.numel(), flags=flags,
                          flag_capacity=1024, totals=totals[0], chunk_totals=totals[1], workspace=wsp, workspace_bytes=need)

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

            parse_ms = timed(parse)
            dst = torch.empty_like(text)
            copy_ms = timed(lambda: dst.copy_(text))
            del text, dst, keys, wsp
            line = {"lines": n_lines, "bytes": int(n), "kept_pairs": int(kept), "records": int(records), "parse_calls": int(calls),
                    "chunk_bytes": int(opt.chunk_bytes), "host_s": [round(x, 3) for x in host_s],
                    "device_end_to_end_s": [round(x, 4) for x in device_s],
                    "stages_s": {k: round(v, 5) for k, v in stages.items()},
                    "parse_call_bytes": nb, "parse_call_ms": [round(x, 3) for x in parse_ms],
                    "copy_ms": [round(x, 3) for x in copy_ms],
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
