"""Lines and files of read-pair text (HiC-Pro `allValidPairs`) for tests/test_pairs_host.py and tests/test_gpu_pairs.py: every
shape of the fast and the slow form, malformed lines, the rule written out once more with str methods and Python's own int()
and round(), the generator of the mixed file, and the dense files whose 4 KiB tiles hold more line starts than one round of the
parse kernel hands out."""
import random

import numpy as np

LINE_MAX, NAME_MAX = 256, 15
TILE, ROUND, TILE_KEYS = 4096, 256, 416      # cgcn_pairs.hip: PAIRS_TILE bytes per workgroup, PAIRS_THREADS line starts per round
CHROMS = ("chr1", "chr2", "chr10", "chrX", "c", "chr_fifteen_byt")          # 1 and 15 bytes among them
OTHER_NAMES = ("chrM", "chrUn_gl000220", "chr", "chr11", "CHR1", "chr1 ")     # same-chromosome pairs outside the table
# positions the fast form takes, and spellings int() takes that it does not
FAST_POS = ["0", "5", "007", "499", "500", "501", "1499", "1500", "1501", "2500", "2147480999", "0000000005", "249250621"]
SLOW_POS = [" 12", "12 ", "+12", "1_000", "00000000012", " +1_5 ", "-0", "3500 ", "\x0b77", "0_0"]
TAILS = ["", "\t+", "\t+\t212", "\t-\t212\tHIC_chr1_7", "\t+\t212\tHIC_chr1_7\tHIC_chr1_9\t42\t42",
         "\t+\t212\tHIC_chr1_7\tHIC_chr1_9\t42\t42\t0-0", "\t\t\t\t"]               # 6, 7, 8, 9, 12, 13 and 10 columns
# (what is wrong, the line); {c} is a chromosome of the table
MALFORMED = [("five fields", "n\t{c}\t5\t+\t{c}"), ("one field", "n"), ("blanks only", "   "), ("not a number", "n\t{c}\tx\t+\t{c}\t5000"),
             ("not a number, second", "n\t{c}\t5\t+\t{c}\t5e3"), ("negative", "n\t{c}\t-5\t+\t{c}\t5000"),
             ("a fraction", "n\t{c}\t1.5\t+\t{c}\t5000"), ("empty position", "n\t{c}\t\t+\t{c}\t5000"),
             ("empty last position", "n\t{c}\t5\t+\t{c}\t"), ("a quote", 'n\t{c}\t5\t+\t{c}\t5000\t"q"'),
             ("a quote in the name", '"n"\t{c}\t5\t+\t{c}\t5000'), ("a lone CR", "n\t{c}\t5\r\t+\t{c}\t5000"),
             ("2^31", "n\t{c}\t2147483648\t+\t{c}\t5000"), ("twenty digits", "n\t{c}\t99999999999999999999\t+\t{c}\t5"),
             ("hex", "n\t{c}\t0x10\t+\t{c}\t5000"), ("malformed on a chromosome outside the table", "n\tchrM\tx\t+\tchrM\t5"),
             ("a long line with a bad position", "n" * 300 + "\t{c}\tx\t+\t{c}\t5000")]
# fast to look at, but the NEAREST bin at 1000 is 2^31 or more
MALFORMED_NEAREST_1000 = ("binned position 2^31", "n\t{c}\t2147483600\t+\t{c}\t5000")


def is_fast(line: bytes) -> bool:
    """the fast form of the rule's `Classes of line`, written out with bytes methods (binned positions aside)"""
    f = line.split(b"\t")
    if len(line) > LINE_MAX or len(f) < 6 or b'"' in line or b"\r" in line:
        return False
    return all(1 <= len(x) <= 10 and x.isdigit() and x.isascii() and int(x) < 2 ** 31 for x in (f[2], f[5])) \
        and all(1 <= len(x) <= NAME_MAX for x in (f[1], f[4]))


def python_bin(x: int, res: int, binning: str) -> int:
    if binning == "floor":
        return x - x % res
    if res == 1000:
        return round(x, -3)                           # the reference's own call
    q, r = divmod(x, res)
    return (q if 2 * r < res else q + 1 if 2 * r > res else q + (q & 1)) * res


def python_rule(lines, chroms=CHROMS, res=1000, binning="nearest", min_diff=10):
    """What the reference's statements make of `lines` (bytes, no terminators): ({chrom: [(p1, p2), ...] in input order}, the
    totals, the slow line numbers).  Malformed lines must not be among them."""
    out = {c: [] for c in chroms}
    tot = dict.fromkeys(("lines", "empty", "kept", "inter_chrom", "other_chrom", "too_close"), 0)
    slow = []
    for k, ln in enumerate(lines):
        tot["lines"] += 1
        if not ln:
            tot["empty"] += 1
            continue
        if not is_fast(ln):
            slow.append(k)
        row = ln.decode("latin-1").split("\t")
        if row[1] != row[4]:
            tot["inter_chrom"] += 1
            continue
        p1, p2 = python_bin(int(row[2]), res, binning), python_bin(int(row[5]), res, binning)
        if row[1] not in out:
            tot["other_chrom"] += 1
        elif abs(p2 - p1) > min_diff:
            out[row[1]].append((p1, p2))
            tot["kept"] += 1
        else:
            tot["too_close"] += 1
    return out, tot, slow


def _read_name(rng, length=None):
    n = rng.randint(0, 60) if length is None else length
    return "".join(rng.choices("SRR0123456789.:_-/ ", k=n))


def tie_lines(chrom="chr1"):
    """every residue class around the ties, x499 / x500 / x501 over even and odd thousands, position 0, both orders"""
    out = []
    for th in (0, 1, 2, 3, 10, 11, 2147482, 2147483):
        for r in (0, 1, 499, 500, 501, 999):
            x = th * 1000 + r
            if x < 2147483500:
                out.append("t%d\t%s\t%d\t+\t%s\t%d\t-\t100" % (x, chrom, x, chrom, 777000 + (x % 7) * 1000))
                out.append("u%d\t%s\t%d\t+\t%s\t%d\t-\t100" % (x, chrom, 12345678, chrom, x))
    return [ln.encode() for ln in out]


def mixed_lines(n, seed, chroms=CHROMS, slow_share=0.006, max_pos=2147480999, empty_share=0.002):
    """n valid lines (bytes, no terminators) of every fast shape and -- a `slow_share` of them -- every slow shape: the
    shortest legal line (9 bytes) to LINE_MAX bytes and a few of LINE_MAX + 1 (slow), 6 to 13 columns, kept pairs in both
    orders, pairs in one bin, heavy duplicates, inter-chromosomal pairs (some with positions int() would refuse: the
    reference never looks), chromosomes outside the table, names of 1 and 15 bytes, empty lines."""
    rng = random.Random(seed)
    hot = [(rng.choice(chroms), rng.randint(0, 2000) * 1000 + rng.randint(0, 999), rng.randint(0, 2000) * 1000) for _ in range(40)]
    out = []
    while len(out) < n:
        u = rng.random()
        if u < empty_share:
            out.append(b"")
            continue
        slow = rng.random() < slow_share
        c1 = c2 = rng.choice(chroms)
        k = rng.random()
        if k < 0.12:
            c2 = rng.choice([c for c in chroms + OTHER_NAMES if c != c1])
        elif k < 0.18:
            c1 = c2 = rng.choice(OTHER_NAMES)
        if rng.random() < 0.3:
            c, a, b = rng.choice(hot)                                 # heavy duplicates
            if c1 == c2 and c1 in chroms:
                c1 = c2 = c
            b += rng.randint(0, 999)
        else:
            a = rng.randint(0, max_pos) if rng.random() < 0.1 else rng.randint(0, 50000000)
            d = int(10 ** (rng.random() * 7.5))                        # separations from 1 bp: some pairs fall into one bin
            b = min(max_pos, a + d) if rng.random() < 0.5 else max(0, a - d)
        pa, pb = str(a), str(b)
        if rng.random() < 0.03:
            pa = rng.choice(FAST_POS)
        if rng.random() < 0.03:
            pb = rng.choice(FAST_POS)
        name, tail = _read_name(rng), rng.choice(TAILS)
        if slow:
            kind = rng.randrange(6)
            if kind == 0:
                pa = rng.choice(SLOW_POS)
            elif kind == 1:
                pb = rng.choice(SLOW_POS)
            elif kind == 2:
                c1 = c2 = rng.choice(["chr_sixteen_bytes", "", "chromosome_of_a_long_name"])
            elif kind == 3 and c1 != c2:
                pa = rng.choice(["x", "", "1.5", "-3"])              # inter-chromosomal: the positions are never read
            elif kind == 4:
                name = _read_name(rng, rng.randint(300, 700))
        line = "%s\t%s\t%s\t+\t%s\t%s%s" % (name, c1, pa, c2, pb, tail)
        if slow and kind == 5:
            line = "%s\t%s\t%s\t+\t%s\t%s%s" % (_read_name(rng, max(0, len(name) + LINE_MAX + 1 - len(line))), c1, pa, c2, pb, tail)
        elif not slow and rng.random() < 0.02 and len(line) <= LINE_MAX:
            pad = LINE_MAX - rng.randrange(3) - len(line)            # to the bound or just below it
            line = "%s\t%s\t%s\t+\t%s\t%s%s" % (name + _read_name(rng, max(0, pad)), c1, pa, c2, pb, tail)
        elif not slow and rng.random() < 0.01:
            line = "\t%s\t%d\t\t%s\t%d" % (c1, a % 10, c2, b % 10) if rng.random() < 0.5 else "\tc\t%d\t\tc\t%d" % (a % 10, b % 10)
        out.append(line.encode())
    return out


def join_lines(lines, seed=None, crlf_share=0.0, final_terminator=True) -> bytes:
    """the lines as a file: LF, or (a `crlf_share` of them, seeded) CR LF; the last line without a terminator if asked"""
    rng = random.Random(seed)
    parts = []
    for k, ln in enumerate(lines):
        parts.append(ln)
        if k + 1 < len(lines) or final_terminator:
            parts.append(b"\r\n" if crlf_share and rng.random() < crlf_share else b"\n")
    return b"".join(parts)


def arrays(pairs):
    """[(p1, p2), ...] -> two int32 vectors"""
    a = np.array(pairs, dtype=np.int64).reshape(-1, 2)
    return a[:, 0].astype(np.int32), a[:, 1].astype(np.int32)


# ----------------------------------------------------------------------------------------------
# dense files: lines so short that a tile's line starts need several rounds of 256
# ----------------------------------------------------------------------------------------------
DENSE_RULE = dict(chroms=["c"], min_diff=-1, resolution_bp=8)     # what dense_kept is parsed with: every line is kept
BAD_SHORT = b"\tc\t1"                                               # three fields: malformed


def tile_ranks(data: bytes):
    """for every line start of `data` (byte 0 and every byte behind an LF), in line order: (its 4 KiB tile, its place among
    the line starts of that tile, 0-based).  Line k of the file is entry k."""
    buf = np.frombuffer(data, np.uint8)
    starts = np.concatenate([np.zeros(1, np.int64), np.flatnonzero(buf == 10) + 1])
    starts = starts[starts < buf.size]
    tile = starts // TILE
    return tile, np.arange(starts.size) - np.searchsorted(tile, tile)


def dense_kept(n=60000, seed=1):
    """n lines of the shortest kept form, `TAB c TAB d TAB TAB c TAB d LF` = 10 bytes (DENSE_RULE keeps every one of them):
    4096 = 6 mod 10, so the tiles start at five phases of a line and every fifth tile starts on a line start and holds 410"""
    rng = random.Random(seed)
    return [b"\tc\t%d\t\tc\t%d" % (rng.randrange(10), rng.randrange(10)) for _ in range(n)]


def dense_mixed(n=40000, seed=2, slow_every=211):
    """n short lines of every class at the default min_diff with chroms=["c"]: kept, too close, inter-chromosomal, outside the
    table, empty; every `slow_every`-th line is a slow one (a blank inside int()), kept and too close in turn"""
    rng = random.Random(seed)
    out = []
    for k in range(n):
        if k % slow_every == slow_every - 1:
            out.append(b"\tc\t 1\t\tc\t%d" % (7000 + k if (k // slow_every) % 2 else 2))
            continue
        u = rng.random()
        if u < 0.45:
            a, b = rng.randrange(10), 1000 * rng.randint(1, 99) + rng.randrange(10)
            out.append(b"\tc\t%d\t\tc\t%d" % ((a, b) if rng.random() < 0.5 else (b, a)))
        elif u < 0.6:
            out.append(b"\tc\t%d\t\tc\t%d" % (rng.randrange(10), rng.randrange(10)))
        elif u < 0.75:
            out.append(b"\tc\t1\t\td\t2")
        elif u < 0.85:
            out.append(b"\td\t1\t\td\t2")
        else:
            out.append(b"")
    return out
