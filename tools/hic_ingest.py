"""Turns a Juicer directory into the contact caches `python -m chromegcn_amd.train -hic_contacts DIR` loads; needs a GPU.

Walks the reference's layout (data/7create_graph_new.py:145, :174-175):
    <hic_root>/<cell>_combined/<res>kb_resolution_intrachromosomal/<chrom>/MAPQGE30/<chrom>_<res>kb.RAWobserved
plus the `<chrom>_<res>kb.{KR,VC,SQRTVC}norm` files that exist beside it, and a windows bed (chrom<TAB>start<TAB>...: the
chromosome's windows with peaks, create_bin_dict :14-47).  Per chromosome the contact text is parsed on the device
(chromegcn_amd.hic.contacts_from_text), the norm vectors -- one value per bin -- on the host, and
`<out>/<chrom>.cghic` is written (hic.save_contacts_cache).  Prints one JSON line per chromosome.
--compute-norms KR,VC,SQRTVC also computes those vectors from the records on the device (chromegcn_amd/hicnorm.py) and
stores them as cKR / cVC / cSQRTVC -- names Juicer's files never take -- so that `-hicnorm cKR` finds them; the line then
carries what the KR run reports.  A KR that did not converge is not stored.
--compute-expected RAW,KR,VC,SQRTVC also computes the expected vectors of those kinds from the records on the device
(chromegcn_amd/hicdist.py; KR, VC, SQRTVC: with the vector computed from the records) and stores them beside the norm vectors
as eRAW / eKR / eVC / eSQRTVC: the cache's named-vector section takes any name of at most 16 bytes, so files already written
stay readable and a reader that does not know these names sees four more vectors.  `graphs_from_contact_caches(...,
expected="eKR")` scores with a stored one.
--pairs FILE [--pairs-binning floor|nearest] starts one step earlier, for data that has no Juicer output: FILE is a HiC-Pro
`allValidPairs` file (one line per read pair); its pairs are binned at --resolution-kb and turned into contact records on the
device (chromegcn_amd/pairs.py) for every chromosome of --chroms, and the same caches are written.  --hic-root and --cell are
not needed then; there are no norm files, so --compute-norms is what gives a pairs file its vectors."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from chromegcn_amd import hic  # noqa: E402

NORMS = ("KR", "VC", "SQRTVC")
EXPECTED = ("RAW",) + NORMS


def expected_vectors(c, kinds, res):
    """{'e' + kind: the expected vector of the records} (a KR that did not converge is left out)"""
    from chromegcn_amd.hicnorm import HicNormError
    out = {}
    for kind in kinds:
        try:
            out["e" + kind] = c.expected_vector(None if kind == "RAW" else kind, res).cpu().numpy()
        except HicNormError:
            pass
    return out


def chrom_dir(hic_root, cell, res_kb, chrom):
    return os.path.join(hic_root, "%s_combined" % cell, "%skb_resolution_intrachromosomal" % res_kb, chrom, "MAPQGE30")


def ingest(hic_root, cell, res_kb, bed, chroms, out, device="cuda", chunk_bytes=None, compute_norms=(), compute_expected=()):
    """writes <out>/<chrom>.cghic for every chromosome of `chroms`; returns one dict per chromosome"""
    windows = hic.windows_from_bed(bed, chroms)
    os.makedirs(out, exist_ok=True)
    kw = {} if chunk_bytes is None else {"chunk_bytes": int(chunk_bytes)}
    lines = []
    for chrom in chroms:
        d = chrom_dir(hic_root, cell, res_kb, chrom)
        raw = os.path.join(d, "%s_%skb.RAWobserved" % (chrom, res_kb))
        if not os.path.exists(raw):
            raise SystemExit("%s is missing" % raw)
        t0 = time.perf_counter()
        c = hic.contacts_from_text(raw, device=device, **kw)
        norms = {}
        for name in NORMS:
            p = os.path.join(d, "%s_%skb.%snorm" % (chrom, res_kb, name))
            if os.path.exists(p):
                norms[name] = np.loadtxt(p, dtype=np.float64, ndmin=1)
        computed = {}
        for name in compute_norms:
            v, info = c.norm_vector(name, int(res_kb) * 1000, return_info=True)
            if name == "KR":
                computed["KR"] = info
            if info.get("converged", True):
                norms["c" + name] = v.cpu().numpy()
        norms.update(expected_vectors(c, compute_expected, int(res_kb) * 1000))
        path = hic.contact_cache_path(out, chrom)
        hic.save_contacts_cache(path, c.to_host(norms=norms, resolution_bp=int(res_kb) * 1000, window_start=windows[chrom]))
        lines.append({"chrom": chrom, "records": c.M, "text_bytes": c.text_info["n_bytes"],
                      "host_parsed_lines": int(c.text_info["slow_lines"].size), "windows": int(windows[chrom].size),
                      "norms": sorted(norms), "cache": path, "seconds": round(time.perf_counter() - t0, 3),
                      **({"kr": computed["KR"]} if "KR" in computed else {})})
        print(json.dumps(lines[-1]), flush=True)
    return lines


def ingest_pairs(pairs_file, res_kb, bed, chroms, out, binning="nearest", device="cuda", chunk_bytes=None, compute_norms=(),
                 compute_expected=()):
    """writes <out>/<chrom>.cghic for every chromosome of `chroms` from a read-pair file; returns one dict per chromosome"""
    from chromegcn_amd.pairs import ReadPairs
    windows = hic.windows_from_bed(bed, chroms)
    os.makedirs(out, exist_ok=True)
    res = int(res_kb) * 1000
    kw = {} if chunk_bytes is None else {"chunk_bytes": int(chunk_bytes)}
    t0 = time.perf_counter()
    rp = ReadPairs.from_text(pairs_file, chroms=chroms, resolution_bp=res, binning=binning, device=device, **kw)
    records = rp.contacts_all()
    t_parse = time.perf_counter() - t0
    lines = []
    for chrom in chroms:
        t0 = time.perf_counter()
        c, norms, computed = records[chrom], {}, {}
        for name in compute_norms:
            v, info = c.norm_vector(name, res, return_info=True)
            if name == "KR":
                computed["KR"] = info
            if info.get("converged", True):
                norms["c" + name] = v.cpu().numpy()
        norms.update(expected_vectors(c, compute_expected, res))
        path = hic.contact_cache_path(out, chrom)
        hic.save_contacts_cache(path, c.to_host(norms=norms, resolution_bp=res, window_start=windows[chrom]))
        lines.append({"chrom": chrom, "records": c.M, "kept_pairs": rp.info["kept_per_chrom"][chrom],
                      "host_parsed_lines": rp.info["slow"], "windows": int(windows[chrom].size), "norms": sorted(norms),
                      "cache": path, "seconds": round(time.perf_counter() - t0 + (t_parse if not lines else 0.0), 3),
                      **({"kr": computed["KR"]} if "KR" in computed else {})})
        print(json.dumps(lines[-1]), flush=True)
    print(json.dumps({"pairs": {k: v for k, v in rp.info.items() if k not in ("slow_lines", "kept_per_chrom")}}), flush=True)
    return lines


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--hic-root")
    ap.add_argument("--cell", help="the cell type: <hic_root>/<cell>_combined")
    ap.add_argument("--pairs", help="a HiC-Pro allValidPairs file, instead of --hic-root and --cell")
    ap.add_argument("--pairs-binning", choices=("floor", "nearest"), default="nearest",
                    help="nearest: the reference's round(pos, -3) at any resolution; floor: Juicer's bins")
    ap.add_argument("--resolution-kb", default="1")
    ap.add_argument("--bed", required=True, help="the windows bed (windows.bed or chipseq_windows.bed of the reference)")
    ap.add_argument("--chroms", required=True, help="comma-separated")
    ap.add_argument("--out", required=True, help="the directory of the caches (train's -hic_contacts)")
    ap.add_argument("--chunk-bytes", type=int, default=None)
    ap.add_argument("--compute-norms", default="", help="comma-separated subset of KR,VC,SQRTVC: stored as cKR, cVC, cSQRTVC")
    ap.add_argument("--compute-expected", default="", help="comma-separated subset of RAW,KR,VC,SQRTVC: stored as eRAW, eKR, ...")
    opt = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/hic_ingest.py needs a GPU")
    kinds = [k for k in opt.compute_norms.split(",") if k]
    if any(k not in NORMS for k in kinds):
        raise SystemExit("--compute-norms takes a subset of %s" % ",".join(NORMS))
    expected = [k for k in opt.compute_expected.split(",") if k]
    if any(k not in EXPECTED for k in expected):
        raise SystemExit("--compute-expected takes a subset of %s" % ",".join(EXPECTED))
    if opt.pairs:
        return ingest_pairs(opt.pairs, opt.resolution_kb, opt.bed, opt.chroms.split(","), opt.out, binning=opt.pairs_binning,
                            chunk_bytes=opt.chunk_bytes, compute_norms=kinds, compute_expected=expected)
    if not opt.hic_root or not opt.cell:
        raise SystemExit("--hic-root and --cell are needed unless --pairs is given")
    return ingest(opt.hic_root, opt.cell, opt.resolution_kb, opt.bed, opt.chroms.split(","), opt.out, chunk_bytes=opt.chunk_bytes,
                  compute_norms=kinds, compute_expected=expected)


if __name__ == "__main__":
    main()
