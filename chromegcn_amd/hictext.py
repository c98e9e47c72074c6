"""Contact TEXT (a Juicer `RAWobserved` dump, which the reference's data/7create_graph_new.py reads with int() and float(),
:71-76) becomes records by one rule, restated by parse_contacts_text_host and run on the device by HicContacts.from_text
(parse_contacts_text below; csrc/cgcn_text.hip):
  * a file is a sequence of lines, each ended by LF or CR LF, the last one possibly by nothing (a CR belongs to the terminator
    only in front of an LF); record r is the r-th line; the empty piece behind a final terminator is no line; a line is
    F1 TAB F2 TAB F3;
  * FAST: at most TEXT_LINE_MAX = 64 bytes without the terminator; F1, F2 one to ten decimal digits below 2^31; F3 is
    [+-]? digits [. digits]? ([eE] [+-]? digits)?; its digits without leading zeros and without trailing zeros of the fraction
    are at most 15 and form the integer w < 10^15 < 2^53; e = exponent - (fraction digits that remain in w), |e| <= 22; the
    value is float(w) * 10^e (e >= 0) or float(w) / 10^-e, negated behind '-': one correctly rounded operation on two exact
    operands, so it IS float(F3);
  * SLOW: not fast, but int(float(F1)), int(float(F2)) and float(F3) accept the fields and the positions fit int32 (16 or more
    digits, |e| > 22, nan, inf, 1e3 as a position, blanks around a field, a line beyond the bound): parsed by exactly those
    calls, on the host in both paths; 17-digit normalised dumps are of this kind throughout: load_contacts_text reads
    those faster;
  * MALFORMED: everything else (an empty line, a field count other than three, a '#' comment, a field float() rejects):
    ValueError naming the first such line, 1-based, the same text from both paths."""
import time

import numpy as np
import torch

from ._textio import TextSource, _text_bytes, _text_lines, lap_timer, staging

TEXT_LINE_MAX = 64   # include/chromegcn.h: CGCN_TEXT_LINE_MAX
TEXT_SLOW, TEXT_MALFORMED = 1, 2
_P10 = np.array([float("1e%d" % k) for k in range(23)])           # the 23 powers of ten that are exact in fp64
_P10U = np.array([10 ** k for k in range(16)], dtype=np.uint64)


def _malformed(record: int) -> ValueError:
    return ValueError("contact text: line %d is not `pos1<TAB>pos2<TAB>count`" % (record + 1))


def _slow_line(raw: bytes):
    """(pos1, pos2, count) of one line without its terminator by Python's own int(float(.)) and float(.); None = malformed"""
    f = raw.split(b"\t")
    if len(f) != 3:
        return None
    try:
        a, b, v = int(float(f[0])), int(float(f[1])), float(f[2])
    except (ValueError, OverflowError):
        return None
    if not (-2 ** 31 <= a < 2 ** 31 and -2 ** 31 <= b < 2 ** 31):
        return None
    return a, b, v


def _text_fast(buf, start, end):
    """The fast form, all lines at once, one byte of every line per step (the walk of cgcn_text.hip's text_parse_line):
    (fast bool [M], pos1 int64 [M], pos2 int64 [M], count float64 [M]); the last three mean nothing where fast is False."""
    n, m_lines = buf.size, start.size
    bufp = np.concatenate([buf, np.zeros(1, np.uint8)])

    def at(p):
        return bufp[np.minimum(p, n)].astype(np.int64)

    ok = (end - start >= 1) & (end - start <= TEXT_LINE_MAX)
    p = start.copy()
    pos = []
    for _ in range(2):   # one to ten digits below 2^31, then the TAB
        x, nd, run = np.zeros(m_lines, np.int64), np.zeros(m_lines, np.int64), ok.copy()
        for _ in range(11):
            d = at(p) - 48
            run = run & (p < end) & (d >= 0) & (d <= 9)
            if not run.any():
                break
            x = np.where(run, x * 10 + d, x)
            nd += run
            p += run
        ok &= (nd >= 1) & (nd <= 10) & (x < 2 ** 31) & (p < end) & (at(p) == 9)
        p += 1
        pos.append(x)
    c = at(p)
    sign = ok & (p < end) & ((c == 43) | (c == 45))
    neg = sign & (c == 45)
    p += sign
    st = np.ones(m_lines, np.int8)   # 1 integer digits, 2 fraction digits, 3 behind [eE], 4 exponent digits
    w = np.zeros(m_lines, np.uint64)
    nsig, nint, nfr, fr, z, ex, nex = (np.zeros(m_lines, np.int64) for _ in range(7))
    eneg = np.zeros(m_lines, bool)
    for _ in range(TEXT_LINE_MAX):
        act = ok & (p < end)
        if not act.any():
            break
        c = at(p)
        d = c - 48
        isd = (d >= 0) & (d <= 9)
        du = np.where(isd, d, 0).astype(np.uint64)
        is_e = (c | 32) == 101
        in1, in2, in3, in4 = act & (st == 1), act & (st == 2), act & (st == 3), act & (st == 4)
        # integer part: leading zeros do not count
        dig = in1 & isd
        grow = dig & ((nsig > 0) | (d != 0))
        nsig += grow
        w = np.where(grow & (nsig <= 15), w * np.uint64(10) + du, w)   # never beyond 15 digits: w does not wrap
        nint += dig
        # fraction: zeros wait in z until a digit follows them
        dig2 = in2 & isd
        nfr += dig2
        nz = dig2 & (d != 0)
        first = nz & (nsig == 0)
        more = nz & (nsig > 0)
        nsig = np.where(first, 1, np.where(more, nsig + z + 1, nsig))
        w = np.where(first, du, np.where(more & (nsig <= 15), w * _P10U[np.minimum(z + 1, 15)] + du, w))
        fr += np.where(nz, z + 1, 0)
        z = np.where(nz, 0, z + (dig2 & (d == 0)))
        # exponent
        esign = in3 & ((c == 43) | (c == 45))
        eneg |= esign & (c == 45)
        dig4 = (in3 | in4) & isd
        ex = np.where(dig4 & (ex < 10000), ex * 10 + d, ex)
        nex += dig4
        # what ends a part
        end1, end2 = in1 & ~isd, in2 & ~isd
        to2 = end1 & (nint >= 1) & (c == 46)
        to3 = (end1 & (nint >= 1) & is_e) | (end2 & (nfr >= 1) & is_e)
        ok &= ~((end1 & ~to2 & ~to3) | (end2 & ~to3) | (in3 & ~esign & ~isd) | (in4 & ~isd))
        st = np.where(to2, 2, np.where(to3, 3, np.where(esign | dig4, 4, st))).astype(np.int8)
        p += act
    ok &= np.where(st == 1, nint >= 1, np.where(st == 2, nfr >= 1, nex >= 1))
    e = np.where(eneg, -ex, ex) - fr
    ok &= (nsig <= 15) & (e >= -22) & (e <= 22)
    mant = w.astype(np.float64)   # exact: w < 10^15
    with np.errstate(all="ignore"):
        val = np.where(e >= 0, mant * _P10[np.clip(e, 0, 22)], mant / _P10[np.clip(-e, 0, 22)])   # one rounding
    return ok, pos[0], pos[1], np.where(neg, -val, val)


def parse_contacts_text_host(data):
    """The rule of the module docstring on bytes (bytes, bytearray, memoryview or a uint8 vector): (pos1 int32 [M], pos2 int32
    [M], count float64 [M], slow_lines int64: the 0-based records that are SLOW, ascending).  Fast lines are parsed by the
    walk the device kernel does, every other line by int(float(.)) and float(.); ValueError at the first malformed line."""
    buf = _text_bytes(data)
    start, end = _text_lines(buf)
    fast, a, b, v = _text_fast(buf, start, end)
    pos1, pos2, count = a.astype(np.int32), b.astype(np.int32), np.ascontiguousarray(v, dtype=np.float64)
    slow = np.flatnonzero(~fast)
    for r in slow.tolist():
        rec = _slow_line(buf[start[r]:end[r]].tobytes())
        if rec is None:
            raise _malformed(r)
        pos1[r], pos2[r], count[r] = rec
    return pos1, pos2, count, slow.astype(np.int64)


# ----------------------------------------------------------------------------------------------
# device parse
# ----------------------------------------------------------------------------------------------
def _stage_text(src: TextSource, text, chunk_bytes) -> float:
    """Copy the bytes of `src` into the device buffer `text`, chunk by chunk through the two pinned buffers: chunk k + 1 is
    read while chunk k is on its way.  Returns the seconds spent reading."""
    pinned, busy, t_read = staging(text.device, chunk_bytes), [None, None], 0.0
    off, k = 0, 0
    while off < src.n:
        if busy[k] is not None:
            busy[k].synchronize()
        want = min(chunk_bytes, src.n - off)
        t0 = time.perf_counter()
        src.read_into(memoryview(pinned[k].numpy()), want)
        t_read += time.perf_counter() - t0
        text[off:off + want].copy_(pinned[k][:want], non_blocking=True)
        busy[k] = torch.cuda.Event()
        busy[k].record()
        off, k = off + want, k ^ 1
    for e in busy:
        if e is not None:
            e.synchronize()   # the buffers are shared with the next call
    return t_read


def parse_contacts_text(cls, path_or_bytes, device, chunk_bytes, flag_capacity, timings):
    """HicContacts.from_text (its docstring); cls: the class of the result"""
    from . import _lib
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("HicContacts.from_text needs a GPU; parse_contacts_text_host is the CPU path")
    if int(chunk_bytes) < 1 or int(flag_capacity) < 0:
        raise ValueError("chunk_bytes must be positive and flag_capacity non-negative")
    src = TextSource(path_or_bytes)
    n = src.n
    lap = lap_timer(timings, device)
    try:
        with torch.cuda.device(device):
            text = torch.empty(max(n, 1), dtype=torch.uint8, device=device)
            t_read = _stage_text(src, text, int(chunk_bytes))
            staged = lap()
            if staged is not None:
                timings["read"], timings["h2d"] = t_read, staged - t_read
            wsp, need = _lib.workspace_for("cgcn_text_workspace_bytes", device, "contact text, %d bytes" % n, n_bytes=n)
            out = torch.zeros(1, dtype=torch.int64, device=device)
            _lib.call("cgcn_text_count", text=text, n_bytes=n, workspace=wsp, workspace_bytes=need, n_records=out)
            m = int(out.item())
            lap("count")
            if m >= 2 ** 31:
                raise ValueError("contact text: %d records, more than 2^31 - 1" % m)
            pos1 = torch.empty(m, dtype=torch.int32, device=device)
            pos2 = torch.empty(m, dtype=torch.int32, device=device)
            count = torch.empty(m, dtype=torch.float64, device=device)
            cap, calls = int(flag_capacity), 0
            while True:
                flags = torch.empty((max(cap, 1), 3), dtype=torch.int64, device=device)
                totals = torch.zeros(2, dtype=torch.int64, device=device)
                _lib.call("cgcn_text_parse", text=text, n_bytes=n, M=m, pos1_out=pos1, pos2_out=pos2, count_out=count,
                          flags=flags, flag_capacity=cap, flag_totals=totals, workspace=wsp, workspace_bytes=need)
                calls += 1
                flagged = int(totals.sum().item())
                if flagged <= cap:
                    break
                if calls == 2:
                    raise RuntimeError("chromegcn_amd: cgcn_text_parse reported %d flagged lines for a capacity of %d" % (flagged, cap))
                cap = flagged   # once more, with room for every one of them
            lap("parse")
            fl = flags[:flagged].cpu().numpy()
            del text, flags, wsp
            fl = fl[np.argsort(fl[:, 0], kind="stable")]
            if flagged:
                recs = []
                for r, off, _ in fl.tolist():   # ascending records: the first line that fails is the first malformed one
                    rec = _slow_line(src.line_at(off))
                    if rec is None:
                        raise _malformed(r)
                    recs.append(rec)
                idx = torch.from_numpy(fl[:, 0].copy()).to(device)
                pos1.index_copy_(0, idx, torch.tensor([x[0] for x in recs], dtype=torch.int32).to(device))
                pos2.index_copy_(0, idx, torch.tensor([x[1] for x in recs], dtype=torch.int32).to(device))
                count.index_copy_(0, idx, torch.tensor([x[2] for x in recs], dtype=torch.float64).to(device))
            lap("patch")
    finally:
        src.close()
    c = cls(pos1, pos2, count, device)
    c.text_info = {"n_bytes": int(n), "slow_lines": fl[:, 0].astype(np.int64), "parse_calls": calls}
    return c
