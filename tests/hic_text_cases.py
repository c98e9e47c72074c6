"""Lines and files of Hi-C contact text for tests/test_hic_text_host.py and tests/test_gpu_hic_text.py: every shape of the fast
and the slow form, malformed lines, the fast form written out once more with `re`, Python's own parse of a list of lines, and
the generators of the mixed and the Juicer-style file."""
import random
import re

import numpy as np

from chromegcn_amd import hic

LINE_MAX = 64

# every shape of F3 the fast form has: sign, point, exponent, leading and trailing zeros, 15 digits, |e| = 22
FAST_F3 = ["0", "7", "42", "+42", "-42", "007", "1.0", "1.5", "-1.5", "+0.25", "123456789012345", "12345678.9012345",
           "0.000123456789012345", "000000000000000000001", "1.00000000000000000000000", "100000000000000.0", "1e0", "1E0",
           "1e22", "1E+22", "1e-22", "-1e-22", "123456789012345e22", "123456789012345e-22", "1.5e23", "0.001e-19",
           "0.001e25", "12345.678e-19", "9007199254740.99", "0.0", "-0.0", "0e0", "0.000", "-0", "5e-0", "5e+00000000000000022",
           "5e-00022", "999999999999999", "0.999999999999999", "99999999999.9999e-5", "1234.5000e3", "10.50", "3.0e-1"]
# every shape the rule calls slow (float() takes it; the device does not)
SLOW_F3 = ["1234567890123456", "0.1234567890123456", "1.2345678901234567", "10000000000000000", "1e23", "1e-23", "1.5e-22",
           "12345e-27", "0e23", "nan", "NaN", "inf", "-inf", "Infinity", " 1.5", "1.5 ", "1.", ".5", "5.e3", "1_0", "1e400",
           "1e-400", "2.2250738585072014e-308", "0.30000000000000004", "1e0000000000000000000023",
           # an integer part that is a multiple of 2^64, with a fraction: a 64-bit significand that wraps reads it as 0.5 / 0.25
           "18446744073709551616.5", "36893488147419103232.25", "18446744073709551616", "18446744073709551616.0e-3",
           "-184467440737095516160.5", "10000000000000000.5", "1234567890123456.0"]
SLOW_POS = ["1e3", "12.0", " 5", "5 ", "-5", "+5", "12345678901e-1", "1_000", "2.5"]
FAST_POS = ["0", "5", "007", "2147483647", "0000000005", "249250000"]
MALFORMED = [b"", b"#comment", b"# a\tb\tc", b"1\t2", b"1\t2\t3\t4", b"1 2 3", b"a\tb\tc", b"1\t2\t", b"\t2\t3", b"1\t\t3",
             b"1\t2\tx", b"1\t2\t1e", b"1\t2\t--1", b"1\t2\t1.5.2", b"2147483648\t2\t3", b"nan\t2\t3", b"inf\t2\t3",
             b"1\t1e10\t3", b"1\t2\t0x10", b"1\t2\t3\t", b"\t\t", b"1\t2\t3" + b"0" * 80 + b"x"]


def rule_is_fast(line: bytes) -> bool:
    """the fast form of the rule, written out with `re` and integer arithmetic"""
    f = line.split(b"\t")
    if len(line) > LINE_MAX or len(f) != 3:
        return False
    for x in f[:2]:
        if not re.fullmatch(rb"[0-9]{1,10}", x) or int(x) >= 2 ** 31:
            return False
    m = re.fullmatch(rb"[+-]?([0-9]+)(?:\.([0-9]+))?(?:[eE]([+-]?[0-9]+))?", f[2])
    if not m:
        return False
    frac = (m.group(2) or b"").rstrip(b"0")
    return len((m.group(1) + frac).lstrip(b"0")) <= 15 and abs(int(m.group(3) or 0) - len(frac)) <= 22


def python_fields(lines):
    """(pos1, pos2, count as int64 bit patterns) by int(float(.)) / float(.), the reference's own calls (:74-76)"""
    f = [ln.split(b"\t") for ln in lines]
    return (np.array([int(float(x[0])) for x in f], np.int64), np.array([int(float(x[1])) for x in f], np.int64),
            np.array([float(x[2]) for x in f], np.float64).view(np.int64))


def assert_parses_like_python(lines, data, got=None):
    """parse_contacts_text_host(data) (or `got`) == Python's calls on `lines`; its slow set == the rule's"""
    p1, p2, c, slow = got if got is not None else hic.parse_contacts_text_host(data)
    w1, w2, wc = python_fields(lines)
    assert p1.dtype == np.int32 and p2.dtype == np.int32 and c.dtype == np.float64 and slow.dtype == np.int64
    assert np.array_equal(p1, w1) and np.array_equal(p2, w2)
    bad = np.flatnonzero(c.view(np.int64) != wc)
    assert bad.size == 0, [(lines[i], c[i]) for i in bad[:5]]
    assert slow.tolist() == [i for i, ln in enumerate(lines) if not rule_is_fast(ln)]
    return slow


def _digits(rng, k, first_nonzero=True):
    s = "".join(rng.choice("0123456789") for _ in range(k))
    return (rng.choice("123456789") + s[1:]) if first_nonzero and k else s


def random_f3(rng, slow):
    """one count field: a fast one, or (slow=True) one of the slow kinds"""
    if slow:
        k = rng.randrange(5)
        if k == 0:
            return _digits(rng, rng.randint(16, 20))
        if k == 1:
            return repr(rng.random() * 10 ** rng.randint(-5, 5)) + rng.choice("123456789") * 3
        if k == 2:
            return "%se%s%d" % (_digits(rng, rng.randint(1, 5)), rng.choice(["", "+", "-"]), rng.randint(40, 300))
        if k == 3:
            return rng.choice(SLOW_F3)
        return rng.choice([" %s", "%s "]) % ("%.1f" % (rng.random() * 100))
    k = rng.randrange(6)
    if k == 0:
        return "%.1f" % (rng.random() * 10 ** rng.randint(0, 5))
    if k == 1:
        return str(rng.randint(0, 10 ** rng.randint(1, 15) - 1))
    nd = rng.randint(1, 15)
    cut = rng.randint(1, nd) if k != 5 else 0
    digs = _digits(rng, nd)
    ip, fp = (digs[:cut], digs[cut:]) if cut else ("0", digs)
    body = rng.choice(["", "+", "-"]) + "0" * rng.randint(0, 3) + ip + ("." + fp + "0" * rng.randint(0, 4) if fp else "")
    if k in (2, 5):
        return body
    # an exponent that keeps |e| <= 22: e = ex - (digits of fp without its trailing zeros)
    kept = len(fp.rstrip("0"))
    ex = rng.randint(-22 + kept, 22 + kept)
    return "%s%s%s%d" % (body, rng.choice("eE"), "+" if ex >= 0 and rng.random() < 0.5 else "", ex)


def mixed_lines(n, seed, slow_share=0.008):
    """n valid lines of every fast shape and (a `slow_share` of them) every slow shape, 5 to LINE_MAX bytes long without the LF
    (6 bytes with it), the longest padded up to LINE_MAX with zeros that do not change the value; a few one byte longer
    (slow)"""
    rng = random.Random(seed)
    out = []
    for i in range(n):
        slow = rng.random() < slow_share
        kind = rng.randrange(8)
        if kind == 0 and not slow:
            out.append(b"%d\t%d\t%d" % (rng.randint(0, 9), rng.randint(0, 9), rng.randint(0, 9)))   # the shortest
            continue
        a = rng.choice(FAST_POS) if rng.random() < 0.05 else str(rng.randint(0, 249250) * 1000)
        b = rng.choice(FAST_POS) if rng.random() < 0.05 else str(rng.randint(0, 249250) * 1000)
        if slow and rng.random() < 0.2:
            a = rng.choice(SLOW_POS)
        f3 = random_f3(rng, slow and rng.random() < 0.8)
        line = "%s\t%s\t%s" % (a, b, f3)
        if kind == 1 and "e" not in f3.lower() and f3.strip() == f3 and f3[0] in "+-0123456789" and "n" not in f3 and "_" not in f3 \
                and not f3.endswith(".") and len(line) + 4 <= LINE_MAX:
            pad = LINE_MAX + (1 if slow else -rng.randrange(3)) - len(line)   # to the bound or just below it (one beyond: slow)
            line += ("" if "." in f3 else ".") + "0" * (pad - (0 if "." in f3 else 1))
        out.append(line.encode())
    return out


def dense_lines(n=100000, slow_every=1000, seed=3):
    """n lines of the shortest form, `d TAB d TAB d` (6 bytes with the LF: two or three line starts in every 16 bytes, 682 or
    683 in a 4 KiB tile), every `slow_every`-th one the slow line `1 TAB 2 TAB 1e23`"""
    rng = random.Random(seed)
    return [b"1\t2\t1e23" if k % slow_every == slow_every - 1 else
            b"%d\t%d\t%d" % (rng.randrange(10), rng.randrange(10), rng.randrange(10)) for k in range(n)]


def juicer_text(pos1, pos2, count) -> bytes:
    """a Juicer `RAWobserved` dump of the records: %d<TAB>%d<TAB>%.1f"""
    rows = np.char.add(np.char.add(np.char.add(pos1.astype(str), "\t"), np.char.add(pos2.astype(str), "\t")),
                       np.char.mod("%.1f", count))
    return ("\n".join(rows.tolist()) + "\n").encode()
