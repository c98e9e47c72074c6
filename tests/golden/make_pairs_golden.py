"""Records g13_pairs.npz: the reference's own pairs step (data/eqtl_data/HiChIP.py) run on a small HiC-Pro-shaped fixture.  Run
where the reference is mounted (CHROMEGCN_REFERENCE, as make_golden_hic.py); only data goes into the file.

input (uint8): the bytes of the pairs file; chroms: the table the tests use (the reference has none: it writes a file for every
chromosome name it meets); files: the names of the chromosomes the reference wrote a file for; out_<name> (uint8): the bytes
of its `<name>.allValidPairs` -- `p1 TAB p2 TAB |p2 - p1| CR LF` per kept pair, in input order.

The script is run as it is, as a program, in a temporary directory that holds the fixture under the input name the script
hard-codes.  The fixture has every residue class around the ties (x499 / x500 / x501 over even and odd thousands), position 0,
pos1 > pos2, pairs that fall into one bin, inter-chromosomal pairs, chromosomes outside the table, 8, 9, 12 and 13 columns,
heavy duplicates, and a few positions in spellings int() takes (blanks, `+`, `_`)."""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
REF = os.environ.get("CHROMEGCN_REFERENCE")
INPUT_NAME = "GSM2705062_HCASMC_HiChIP_H3K27ac_B1T1_allValidPairs.txt"   # data/eqtl_data/HiChIP.py:9
CHROMS = ["chr1", "chr2", "chrX"]
TAILS = ["\t+\t212", "\t-\t212\t0-1", "\t+\t212\tHIC_chr1_7\tHIC_chr1_9\t42\t42", "\t-\t88\tHIC_chr2_70\tHIC_chr2_9\t42\t7\t1-0"]


def make_fixture(rng):
    lines = []

    def add(c1, a, c2, b):
        name = "SRR5831489.%d" % (len(lines) + 1) + ":%d" % rng.randint(1101, 2679) * rng.randint(0, 3)
        lines.append("%s\t%s\t%s\t%s\t%s\t%s%s" % (name, c1, a, "+-"[rng.randint(0, 2)], c2, b, TAILS[rng.randint(0, len(TAILS))]))

    for th in (0, 1, 2, 3, 10, 11, 248999, 249000):           # the ties: even and odd thousands
        for r in (0, 1, 499, 500, 501, 999):
            x = th * 1000 + r
            add("chr1", x, "chr1", 50000000 + th * 1000)
            add("chr2", 123456789, "chr2", x)
            add("chrX", x, "chrX", x + (500 if r < 500 else 1))   # one bin, or neighbours, by the tie alone
    hot = [(CHROMS[rng.randint(0, 3)], rng.randint(0, 90000) * 1000 + rng.randint(0, 1000), rng.randint(0, 90000) * 1000)
           for _ in range(25)]
    for _ in range(2600):
        u = rng.rand()
        if u < 0.35:                                          # heavy duplicates, either order
            c, a, b = hot[rng.randint(0, len(hot))]
            b = b + rng.randint(0, 1000)
            a, b = (a, b) if rng.rand() < 0.5 else (b, a)
            add(c, a, c, b)
        elif u < 0.5:                                         # inter-chromosomal
            add(CHROMS[rng.randint(0, 3)], rng.randint(0, 10 ** 8), ["chr3", "chr1", "chrM", "chr2"][rng.randint(0, 4)] + "_x" * rng.randint(0, 2),
                rng.randint(0, 10 ** 8))
        elif u < 0.6:                                         # a chromosome outside the table
            c = ["chr3", "chrM", "chrUn_gl000220"][rng.randint(0, 3)]
            a = rng.randint(0, 10 ** 7)
            add(c, a, c, a + rng.randint(0, 40000))
        else:
            c = CHROMS[rng.randint(0, 3)]
            a = rng.randint(0, 150000000)
            d = int(10 ** (rng.rand() * 7))                   # from 1 bp: many pairs fall into one bin
            add(c, a, c, a + d if rng.rand() < 0.5 else max(0, a - d))
    for a, b in ((" 1499", "77500"), ("+2500", "1_000_499"), ("3500 ", " +12_345 "), ("007", "0")):
        add("chr1", a, "chr1", b)
    order = rng.permutation(len(lines))
    text = "".join(lines[i] + "\n" for i in order)
    return text[:-1]                                          # the last line ends with nothing


def main():
    if not REF:
        raise SystemExit("set CHROMEGCN_REFERENCE to the checkout of the reference (QData/ChromeGCN)")
    text = make_fixture(np.random.RandomState(20240713))
    out = {"input": np.frombuffer(text.encode(), np.uint8), "chroms": np.array(CHROMS)}
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, INPUT_NAME), "w", newline="") as f:
            f.write(text)
        subprocess.run([sys.executable, os.path.join(REF, "data", "eqtl_data", "HiChIP.py")], cwd=tmp, check=True)
        files = sorted(n[:-len(".allValidPairs")] for n in os.listdir(tmp) if n.endswith(".allValidPairs"))
        for name in files:
            with open(os.path.join(tmp, name + ".allValidPairs"), "rb") as f:
                out["out_" + name] = np.frombuffer(f.read(), np.uint8)
    out["files"] = np.array(files)
    assert set(CHROMS) < set(files), files
    path = os.path.join(HERE, "g13_pairs.npz")
    np.savez_compressed(path, **out)
    print("%s: %d lines, %d output files (%s), %d bytes" % (path, text.count("\n") + 1, len(files), ", ".join(files), os.path.getsize(path)))


if __name__ == "__main__":
    main()
