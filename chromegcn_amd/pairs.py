"""Contact records from read-pair text (a HiC-Pro `allValidPairs` file: one line per read pair) on the device
(csrc/cgcn_pairs.hip), with a host restatement in numpy / plain Python.  This is the step in front of
chromegcn_amd.hic: the reference's third data source (HCASMC HiChIP, data/eqtl_data/) exists only as pairs, and its own step
for them, data/eqtl_data/HiChIP.py:8-24, is a csv.DictReader loop that reopens an output file for every line it keeps.

THE RULE (include/chromegcn.h states it above cgcn_pairs_parse_workspace_bytes; the two move together).
Lines.  A line ends with LF or CR LF; the last line may end with nothing.  An empty line is skipped, as csv.DictReader skips
  it.  A line has at least six TAB-separated fields (read name, chr1, pos1, strand1, chr2, pos2, strand2, fragment size, ...);
  fields 2, 3, 5 and 6 are used and the rest are ignored.  Line numbers count every line, empty ones included.
Parameters.  chroms: 1 to 64 names of 1 to 15 bytes each; the default is chr1 ... chr22 and chrX (DEFAULT_CHROMS).
  resolution_bp >= 8.  binning: "nearest" is the reference's round(int(pos), -3) generalised -- with
  q, r = divmod(pos, resolution_bp): q when 2 r < res, q + 1 when 2 r > res, the even one of the two on a tie; times
  resolution_bp.  "floor" is pos - pos % resolution_bp, the binning of Juicer's dumps and of data/7create_graph_old.py:89
  (with 5000 it gives K562-style records that go with window_bp=1000).  min_diff, default 10: a pair is kept iff
  |p2 - p1| > min_diff on the binned positions.
Fate of a pair.  Field 2 != field 5: dropped, counted as inter_chrom (the reference does not look at its positions, nor do
  we).  Otherwise both positions are read and binned; a name that is not in chroms: dropped, other_chrom; a pair that fails
  min_diff: dropped, too_close; else kept.
Classes of line.  FAST (decided and parsed on the device): at most 256 bytes, six or more fields, fields 3 and 6 one to ten
  plain digits below 2^31, fields 2 and 5 of 1 to 15 bytes, no `"` byte and no lone CR.  SLOW: not fast, but the reference's
  statements accept it (blanks, `+` or `_` inside int(), a longer line, a longer name); the device lists it and _host_line
  below, which follows the reference statement by statement, decides it.  MALFORMED: everything else -- fewer than six fields,
  a position int() refuses, a negative position, a binned position >= 2^31, a `"` byte, a lone CR: ValueError naming the first
  such line, the same text from the host and the device path.  (Positions are read with int() on the field's bytes: digits and
  blanks outside ASCII, which int() of a str would take, are malformed here.)

Stage A, binned pairs: the kept pairs in input order -- ReadPairs.binned(chrom) is the reference's `<chrom>.allValidPairs`
without its third column, which is |pos2 - pos1|.  Stage B, contact records: per chromosome one record for every distinct
unordered bin pair, pos1 = the lower binned position, pos2 = the higher, count = the number of kept pairs (fp64), sorted by
(pos1, pos2).  The reference stops at stage A: it never aggregates pairs into counts, and its third column is the distance, not
a count.  Stage B is this project's definition.  It is the one Juicer's `dump observed` would give for the same pairs."""
import time
from dataclasses import dataclass, field
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import hic
from ._textio import TextSource, _text_bytes, _text_lines, lap_adder, staging

DEFAULT_CHROMS = tuple(["chr%d" % k for k in range(1, 23)] + ["chrX"])
LINE_MAX, NAME_MAX, MAX_CHROMS = 256, 15, 64   # include/chromegcn.h: CGCN_PAIRS_LINE_MAX, _NAME_MAX, _MAX_CHROMS
BINNINGS = {"nearest": 0, "floor": 1}          # CGCN_PAIRS_NEAREST, CGCN_PAIRS_FLOOR
TOTALS = ("lines", "empty", "kept", "inter_chrom", "other_chrom", "too_close", "slow", "malformed")   # CGCN_PAIRS_T_*
_KEPT, _INTER, _OTHER, _CLOSE, _BAD = "kept", "inter_chrom", "other_chrom", "too_close", "malformed"


def _malformed(line: int) -> ValueError:
    return ValueError("read pairs: line %d is not `name<TAB>chr1<TAB>pos1<TAB>strand1<TAB>chr2<TAB>pos2...`" % (line + 1))


def _check_rule(chroms, resolution_bp, binning):
    names = [c.encode() if isinstance(c, str) else bytes(c) for c in chroms]
    if not 1 <= len(names) <= MAX_CHROMS:
        raise ValueError("chroms must hold 1 to %d names" % MAX_CHROMS)
    for nm in names:
        if not 1 <= len(nm) <= NAME_MAX or any(b in nm for b in b"\t\n\r\"\0"):
            raise ValueError("chromosome name %r: 1 to %d bytes, no TAB, LF, CR, quote or NUL" % (nm, NAME_MAX))
    if len(set(names)) != len(names):
        raise ValueError("chroms holds a name twice")
    if int(resolution_bp) < 8:
        raise ValueError("resolution_bp must be 8 or more")
    if binning not in BINNINGS:
        raise ValueError("binning must be 'nearest' or 'floor'")
    return names


def bin_position(pos, resolution_bp: int, binning: str = "nearest"):
    """the binned position of `pos` (an int, or an int64 array): the module docstring's `binning`"""
    res = int(resolution_bp)
    if isinstance(pos, np.ndarray):
        q, r = np.divmod(pos.astype(np.int64), res)
        if binning == "nearest":
            q = q + ((2 * r > res) | ((2 * r == res) & (q % 2 == 1)))
        return q * res
    q, r = divmod(int(pos), res)
    if binning == "nearest" and (2 * r > res or (2 * r == res and q % 2 == 1)):
        q += 1
    return q * res


def _host_line(raw: bytes, index: Dict[bytes, int], res: int, binning: str, min_diff: int):
    """One line without its terminator by the reference's statements (data/eqtl_data/HiChIP.py:11-24): (fate, chromosome
    index, p1, p2); the last three mean something for a kept pair only."""
    if b'"' in raw or b"\r" in raw:
        return _BAD, -1, 0, 0
    f = raw.split(b"\t")                               # csv.DictReader(delimiter='\t')
    if len(f) < 6:
        return _BAD, -1, 0, 0
    if f[1] != f[4]:                                   # if row['chr_reads1']==row['chr_reads2']:
        return _INTER, -1, 0, 0
    try:
        x1, x2 = int(f[2]), int(f[5])                  # int(row['pos_reads1']), int(row['pos_reads2'])
    except ValueError:
        return _BAD, -1, 0, 0
    if x1 < 0 or x2 < 0:
        return _BAD, -1, 0, 0
    p1, p2 = bin_position(x1, res, binning), bin_position(x2, res, binning)   # round(., -3)
    if p1 >= 2 ** 31 or p2 >= 2 ** 31:
        return _BAD, -1, 0, 0
    c = index.get(f[1])
    if c is None:
        return _OTHER, -1, p1, p2
    if abs(p2 - p1) <= min_diff:                       # if posDiff>10:
        return _CLOSE, c, p1, p2
    return _KEPT, c, p1, p2


def _pack_name(nm: bytes):
    """a name as the kernel's table holds it: 16 bytes -- the name, zeros, its length in byte 15 -- as two uint64"""
    b = np.frombuffer(nm.ljust(15, b"\0") + bytes([len(nm)]), dtype="<u8")
    return int(b[0]), int(b[1])


def _fast_lines(buf, start, end, names, res, binning, min_diff):
    """The FAST decision and the fate of every fast line, all lines at once (the walk of cgcn_pairs.hip's pairs_parse_line):
    (fast bool [L], fate int8 [L] -- an index into TOTALS --, chromosome int64 [L], p1 int64 [L], p2 int64 [L])."""
    n, n_lines = buf.size, start.size
    bufp = np.concatenate([buf, np.zeros(1, np.uint8)])

    def at(p):
        return bufp[np.minimum(p, n)].astype(np.int64)

    special = np.concatenate([np.zeros(1, np.int64), np.cumsum((buf == 34) | (buf == 13), dtype=np.int64)])
    tabs = np.flatnonzero(buf == 9)
    k0 = np.searchsorted(tabs, start)
    ntabs = np.searchsorted(tabs, end) - k0
    tabp = np.concatenate([tabs, np.full(6, n, np.int64)])
    t = [tabp[k0 + j] for j in range(6)]
    t[5] = np.where(ntabs >= 6, t[5], end)
    length = end - start
    ok = (length >= 1) & (length <= LINE_MAX) & (ntabs >= 5) & (special[end] == special[start])
    fields = {2: (t[0] + 1, t[1]), 3: (t[1] + 1, t[2]), 5: (t[3] + 1, t[4]), 6: (t[4] + 1, t[5])}
    val = {}
    for f in (3, 6):   # one to ten plain digits below 2^31
        a, b = fields[f]
        nd = b - a
        good = ok & (nd >= 1) & (nd <= 10)
        x = np.zeros(n_lines, np.int64)
        for k in range(10):
            act = good & (k < nd)
            if not act.any():
                break
            d = at(a + k) - 48
            good &= ~act | ((d >= 0) & (d <= 9))
            x = np.where(act, x * 10 + np.clip(d, 0, 9), x)
        ok = good & (x < 2 ** 31)
        val[f] = x
    packed = {}
    for f in (2, 5):   # 1 to 15 bytes, packed as the kernel packs them
        a, b = fields[f]
        ln = b - a
        ok &= (ln >= 1) & (ln <= NAME_MAX)
        lo, hi = np.zeros(n_lines, np.uint64), np.zeros(n_lines, np.uint64)
        for k in range(NAME_MAX):
            act = ok & (k < ln)
            if not act.any():
                break
            c = np.where(act, at(a + k), 0).astype(np.uint64) << np.uint64(8 * (k & 7))
            if k < 8:
                lo |= c
            else:
                hi |= c
        packed[f] = (lo, hi | (np.where(ok, ln, 0).astype(np.uint64) << np.uint64(56)))
    same = (packed[2][0] == packed[5][0]) & (packed[2][1] == packed[5][1])
    p1, p2 = bin_position(val[3], res, binning), bin_position(val[6], res, binning)
    ok &= ~same | ((p1 < 2 ** 31) & (p2 < 2 ** 31))          # a binned position beyond int32 is the host's to report
    chrom = np.full(n_lines, -1, np.int64)
    for c, nm in enumerate(names):
        lo, hi = _pack_name(nm)
        chrom = np.where((packed[2][0] == np.uint64(lo)) & (packed[2][1] == np.uint64(hi)), c, chrom)
    fate = np.where(~same, 3, np.where(chrom < 0, 4, np.where(np.abs(p2 - p1) <= min_diff, 5, 2))).astype(np.int8)
    fate = np.where(length == 0, 1, fate).astype(np.int8)
    return ok, fate, chrom, p1, p2


@dataclass
class HostPairs:
    """bin_read_pairs_host's result: the kept pairs in input order"""
    chroms: tuple
    resolution_bp: int
    chrom: np.ndarray      # int64 [kept]: index into chroms
    pos1: np.ndarray       # int32 [kept]
    pos2: np.ndarray       # int32 [kept]
    info: dict = field(default_factory=dict)

    def binned(self, chrom):
        m = self.chrom == self.chroms.index(chrom)
        return self.pos1[m], self.pos2[m]

    def contacts(self, chrom):
        return pairs_to_contacts_host(*self.binned(chrom), self.resolution_bp)


def _info(totals, per_chrom, chroms, slow_lines, n_bytes, parse_calls=None):
    d = {k: int(totals[k]) for k in TOTALS[:6]}
    d["slow"], d["malformed"] = int(len(slow_lines)), 0
    d["kept_per_chrom"] = {c if isinstance(c, str) else bytes(c).decode("latin-1"): int(v) for c, v in zip(chroms, per_chrom)}
    d["slow_lines"] = np.asarray(slow_lines, dtype=np.int64)
    d["n_bytes"] = int(n_bytes)
    if parse_calls is not None:
        d["parse_calls"] = int(parse_calls)
    return d


def same_info(a: dict, b: dict) -> bool:
    """two `info` dicts agree on everything both hold (parse_calls is the device path's alone)"""
    keys = (set(a) & set(b)) - {"slow_lines"}
    return all(a[k] == b[k] for k in keys) and np.array_equal(a["slow_lines"], b["slow_lines"])


def bin_read_pairs_host(data, chroms: Sequence = DEFAULT_CHROMS, resolution_bp: int = 1000, binning: str = "nearest",
                        min_diff: int = 10, vectorised: bool = True, block_bytes: int = 64 << 20) -> HostPairs:
    """Stage A on the host, from bytes (bytes, bytearray, memoryview or a uint8 vector).  vectorised: the fast lines are
    decided and parsed by numpy, the walk the kernel does, in blocks of whole lines of about `block_bytes`, and the others by
    _host_line; otherwise every line goes through _host_line, the reference statement by statement (slow: a Python loop), and
    numpy only says which lines count as slow.  Either way the result is the same, `info` included; ValueError at the first
    malformed line."""
    names = _check_rule(chroms, resolution_bp, binning)
    res, min_diff = int(resolution_bp), int(min_diff)
    index = {nm: k for k, nm in enumerate(names)}
    buf = _text_bytes(data)
    totals = dict.fromkeys(TOTALS, 0)
    out_c, out_1, out_2, slow_lines = [], [], [], []
    off, line0 = 0, 0
    while off < buf.size:
        stop = min(buf.size, off + int(block_bytes))
        if stop < buf.size:
            lf = np.flatnonzero(buf[off:stop] == 10)
            if lf.size:
                stop = off + int(lf[-1]) + 1
            else:
                more = np.flatnonzero(buf[stop:] == 10)
                stop = stop + int(more[0]) + 1 if more.size else buf.size
        blk = buf[off:stop]
        start, end = _text_lines(blk)
        fast, fate, chrom, p1, p2 = _fast_lines(blk, start, end, names, res, binning, min_diff)
        fast = fast | (end == start)
        for r in np.flatnonzero(~fast if vectorised else end > start).tolist():
            what, c, a, b = _host_line(blk[start[r]:end[r]].tobytes(), index, res, binning, min_diff)
            if what == _BAD:
                raise _malformed(line0 + r)
            fate[r], chrom[r], p1[r], p2[r] = TOTALS.index(what), c, a, b
            if not fast[r]:
                slow_lines.append(line0 + r)
        counts = np.bincount(fate, minlength=8)
        for k in range(1, 6):
            totals[TOTALS[k]] += int(counts[k])
        totals["lines"] += int(start.size)
        kept = fate == 2
        out_c.append(chrom[kept])
        out_1.append(p1[kept].astype(np.int32))
        out_2.append(p2[kept].astype(np.int32))
        off, line0 = stop, line0 + int(start.size)
    chrom = np.concatenate(out_c) if out_c else np.zeros(0, np.int64)
    pos1 = np.concatenate(out_1) if out_1 else np.zeros(0, np.int32)
    pos2 = np.concatenate(out_2) if out_2 else np.zeros(0, np.int32)
    per = np.bincount(chrom, minlength=len(names))
    return HostPairs(tuple(chroms), res, chrom, pos1, pos2, _info(totals, per, chroms, slow_lines, buf.size))


def pairs_to_contacts_host(pos1, pos2, resolution_bp: int):
    """Stage B on the host: (pos1 int32, pos2 int32, count float64) of one chromosome's binned pairs -- one record per
    distinct unordered pair, the lower position first, count = the number of pairs, sorted by (pos1, pos2)."""
    a, b = np.asarray(pos1).astype(np.int64), np.asarray(pos2).astype(np.int64)
    res = int(resolution_bp)
    if a.shape != b.shape or a.ndim != 1:
        raise ValueError("pos1 and pos2 must be vectors of one length")
    if a.size and ((a % res).any() or (b % res).any() or min(a.min(), b.min()) < 0):
        raise ValueError("binned positions must be non-negative multiples of resolution_bp")
    key, cnt = np.unique((np.minimum(a, b) << 32) | np.maximum(a, b), return_counts=True)
    return (key >> 32).astype(np.int32), (key & 0xFFFFFFFF).astype(np.int32), cnt.astype(np.float64)


# ----------------------------------------------------------------------------------------------
# device path
# ----------------------------------------------------------------------------------------------
class _LineChunks:
    """The bytes of a TextSource as chunks of whole lines of at most `chunk_bytes`, staged in turn in the two pinned buffers
    of _textio.staging (a line longer than that travels alone, in a buffer of its own).  next() -> (uint8 host tensor,
    byte offset of its first byte in the source) or None."""

    def __init__(self, src: TextSource, chunk_bytes, device):
        self.pinned, self.k = staging(device, chunk_bytes), 0
        self.src, self.chunk = src, chunk_bytes
        self.base = 0         # source offset of the next chunk's first byte
        self.carry = b""      # the piece behind the last LF of the chunk before
        self.seconds = 0.0    # spent reading

    @staticmethod
    def _last_lf(view, total):
        hi = total
        while hi > 0:
            lo = max(0, hi - 65536)
            k = bytes(view[lo:hi]).rfind(b"\n")
            if k >= 0:
                return lo + k
            hi = lo
        return -1

    def next(self):
        t0 = time.perf_counter()
        buf = self.pinned[self.k]
        self.k ^= 1
        view = memoryview(buf.numpy())
        have = len(self.carry)
        view[:have] = self.carry
        src = self.src
        want = min(self.chunk - have, src.n - src.off)
        src.read_into(view[have:], want)
        total = have + want
        if total == 0:
            return None
        out = buf
        if src.off == src.n:
            cut = total
        else:
            cut = self._last_lf(view, total) + 1
            if cut == 0:   # a line longer than a chunk: it travels alone, up to and with its LF
                big = bytearray(view[:total])
                while src.off < src.n:
                    want = min(self.chunk, src.n - src.off)
                    piece = bytearray(want)
                    src.read_into(memoryview(piece), want)
                    k = piece.find(b"\n")
                    if k >= 0:
                        big += piece[:k + 1]
                        self.carry = bytes(piece[k + 1:])
                        break
                    big += piece
                else:
                    self.carry = b""
                self.seconds += time.perf_counter() - t0
                base, self.base = self.base, self.base + len(big)
                return torch.frombuffer(big, dtype=torch.uint8), base
        self.carry = bytes(view[cut:total])
        self.seconds += time.perf_counter() - t0
        base, self.base = self.base, self.base + cut
        return out[:cut], base


class ReadPairs:
    """The kept pairs of a read-pair file resident on the device as 64-bit keys in input order (stage A), and the contact
    records made of them (stage B, computed once when first asked for).  `info`: the totals of the module docstring (lines,
    empty, kept, inter_chrom, other_chrom, too_close; slow = the lines the host parsed; malformed = 0), kept_per_chrom,
    slow_lines (int64 line numbers, 0-based), n_bytes, parse_calls."""

    def __init__(self, keys, chroms, resolution_bp, info):
        self.keys = keys                      # int64 [kept]: chromosome << 57 | lo << 29 | hi << 1 | swapped
        self.chroms = tuple(chroms)
        self.resolution_bp = int(resolution_bp)
        self.info = info
        self.device = keys.device
        self._records = None                  # (pos1, pos2, count, offsets as a list)

    @classmethod
    def from_text(cls, path_or_bytes, chroms: Sequence = DEFAULT_CHROMS, resolution_bp: int = 1000, binning: str = "nearest",
                  min_diff: int = 10, device="cuda", chunk_bytes: int = 32 << 20, flag_capacity: int = 1 << 16,
                  timings: Optional[dict] = None) -> "ReadPairs":
        """Stage A of a path, or of bytes / bytearray / memoryview, by the rule of the module docstring.  The text goes
        through the pinned staging buffers HicContacts.from_text uses in chunks of whole lines of at most `chunk_bytes`; one chunk of
        text is resident at a time and the keys (8 bytes per kept pair) are what stays, so a 30 GB file does not need 30 GB
        of device memory.  Per chunk: copy, cgcn_pairs_parse (a second call when more than `flag_capacity` lines of the chunk
        are not fast), then the next chunk is read while the device works, and one read-back of the running totals.  The
        lines the device lists are parsed by _host_line and merged in at their input positions.  timings: a dict that
        receives the seconds of every stage, with a device sync behind each (read, h2d, parse, patch)."""
        from . import _lib
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("ReadPairs.from_text needs a GPU; bin_read_pairs_host is the CPU path")
        names = _check_rule(chroms, resolution_bp, binning)
        res, min_diff, chunk_bytes = int(resolution_bp), int(min_diff), int(chunk_bytes)
        if chunk_bytes < 1 or int(flag_capacity) < 0:
            raise ValueError("chunk_bytes must be positive and flag_capacity non-negative")
        index = {nm: k for k, nm in enumerate(names)}
        src = TextSource(path_or_bytes)
        n = src.n
        tm = dict.fromkeys(("read", "h2d", "parse", "patch"), 0.0)
        lap = lap_adder(tm, timings is not None, device)

        table = np.zeros((len(names), 16), np.uint8)
        for k, nm in enumerate(names):
            table[k, :len(nm)] = np.frombuffer(nm, np.uint8)
            table[k, 15] = len(nm)
        host_totals = dict.fromkeys(TOTALS, 0)     # the fates of the lines the host parsed
        slow_lines, slow_rank, slow_key = [], [], []
        calls = 0
        chunks = _LineChunks(src, chunk_bytes, device)
        try:
            with torch.cuda.device(device):
                names_dev = torch.from_numpy(table).to(device)
                text = torch.empty(chunk_bytes, dtype=torch.uint8, device=device)
                wsp, need = _lib.workspace_for("cgcn_pairs_parse_workspace_bytes", device,
                                               "read pairs, chunks of %d bytes" % chunk_bytes, n_bytes=chunk_bytes)
                totals = torch.zeros((2, 8), dtype=torch.int64, device=device)   # running | this chunk's
                before = np.zeros(8, np.int64)
                keys = torch.empty(max(1, min(n, chunk_bytes) // 9 + 1), dtype=torch.int64, device=device)
                cap = int(flag_capacity)
                flags = torch.empty((max(cap, 1), 4), dtype=torch.int64, device=device)
                nxt = chunks.next()
                while nxt is not None:
                    (chunk, base), nb = nxt, int(nxt[0].numel())
                    t0 = time.perf_counter()
                    tx, ws_c, need_c = text, wsp, need
                    if nb > chunk_bytes:            # a single line longer than a chunk
                        tx = torch.empty(nb, dtype=torch.uint8, device=device)
                        ws_c, need_c = _lib.workspace_for("cgcn_pairs_parse_workspace_bytes", device,
                                                          "read pairs, a line of %d bytes" % nb, n_bytes=nb)
                    tx[:nb].copy_(chunk, non_blocking=True)
                    lap("h2d", t0)
                    kept0 = int(before[2])
                    if kept0 + nb // 9 + 1 > keys.numel():   # a kept line has ten bytes, the last one nine
                        grown = torch.empty(max(2 * keys.numel(), kept0 + nb // 9 + 1), dtype=torch.int64, device=device)
                        grown[:kept0] = keys[:kept0]
                        keys = grown
                    t0 = time.perf_counter()
                    first = True
                    for attempt in range(2):
                        _lib.call("cgcn_pairs_parse", text=tx, n_bytes=nb, byte_base=base, names=names_dev, n_chroms=len(names),
                                  resolution_bp=res, binning=BINNINGS[binning], min_diff=min_diff, keys=keys,
                                  key_capacity=keys.numel(), flags=flags, flag_capacity=cap, totals=totals[0],
                                  chunk_totals=totals[1], workspace=ws_c, workspace_bytes=need_c)
                        calls += 1
                        if first:
                            lap("parse", t0)
                            t0 = time.perf_counter()
                            nxt = chunks.next()     # read while the device works
                            tm["read"] += time.perf_counter() - t0
                            t0, first = time.perf_counter(), False
                        tot = totals.cpu().numpy()
                        flagged = int(tot[1, 6] + tot[1, 7])
                        if flagged <= cap:
                            break
                        if attempt:
                            raise RuntimeError("chromegcn_amd: cgcn_pairs_parse reported %d flagged lines for a capacity of %d"
                                               % (flagged, cap))
                        cap = flagged               # once more, with room for every one of them
                        flags = torch.empty((cap, 4), dtype=torch.int64, device=device)
                        totals[0].copy_(torch.from_numpy(before))
                    lap("parse", t0)
                    if int(tot[0, 2]) > keys.numel():
                        raise RuntimeError("chromegcn_amd: cgcn_pairs_parse kept more pairs than a chunk of %d bytes can hold" % nb)
                    before = tot[0].copy()
                    t0 = time.perf_counter()
                    if flagged:
                        fl = flags[:flagged].cpu().numpy()
                        fl = fl[np.argsort(fl[:, 0], kind="stable")]
                        for line, off, _, rank in fl.tolist():   # ascending lines: the first that fails is the first malformed
                            what, c, a, b = _host_line(src.line_at(off), index, res, binning, min_diff)
                            if what == _BAD:
                                raise _malformed(line)
                            host_totals[what] += 1
                            slow_lines.append(line)
                            if what == _KEPT:
                                lo, hi = min(a, b) // res, max(a, b) // res
                                slow_rank.append(rank)
                                slow_key.append((c << 57) | (lo << 29) | (hi << 1) | int(a > b))
                    lap("patch", t0)
                t0 = time.perf_counter()
                n_fast = int(before[2])
                keys = keys[:n_fast]
                if slow_key:   # the host's pairs, each in front of the device's key of the same rank
                    at = torch.tensor(slow_rank, dtype=torch.int64) + torch.arange(len(slow_rank), dtype=torch.int64)
                    merged = torch.empty(n_fast + len(slow_key), dtype=torch.int64, device=device)
                    mask = torch.zeros(merged.numel(), dtype=torch.bool, device=device)
                    at = at.to(device)
                    mask[at] = True
                    merged[at] = torch.tensor(slow_key, dtype=torch.int64).to(device)
                    merged[~mask] = keys
                    keys = merged
                else:
                    keys = keys.clone()             # the capacity beyond the kept pairs is released
                per = torch.bincount(keys >> 57, minlength=len(names)).cpu().numpy() if keys.numel() else np.zeros(len(names), np.int64)
                lap("patch", t0)
        finally:
            src.close()
        tm["read"] = chunks.seconds
        totals_all = {k: int(before[i]) + host_totals[k] for i, k in enumerate(TOTALS)}
        if timings is not None:
            timings.update(tm)
        return cls(keys, chroms, res, _info(totals_all, per, chroms, slow_lines, n, calls))

    def _index(self, chrom) -> int:
        try:
            return self.chroms.index(chrom)
        except ValueError:
            raise KeyError("%r is not one of this file's chromosomes" % (chrom,)) from None

    def binned(self, chrom):
        """(pos1, pos2) int32 device vectors of the chromosome's kept pairs in input order: the reference's
        `<chrom>.allValidPairs` without its third column, which is |pos2 - pos1|"""
        k = self.keys[(self.keys >> 57) == self._index(chrom)]
        lo, hi, swapped = (k >> 29) & 0xFFFFFFF, (k >> 1) & 0xFFFFFFF, (k & 1).bool()
        p1, p2 = torch.where(swapped, hi, lo), torch.where(swapped, lo, hi)
        return (p1 * self.resolution_bp).to(torch.int32), (p2 * self.resolution_bp).to(torch.int32)

    def _reduce(self, timings=None):
        if self._records is None:
            from . import _lib
            n, nc = int(self.keys.numel()), len(self.chroms)
            t0 = time.perf_counter()
            with torch.cuda.device(self.device):
                wsp, need = _lib.workspace_for("cgcn_pairs_reduce_workspace_bytes", self.device, "read pairs, %d keys" % n, n_keys=n)
                pos1 = torch.empty(max(n, 1), dtype=torch.int32, device=self.device)
                pos2 = torch.empty(max(n, 1), dtype=torch.int32, device=self.device)
                count = torch.empty(max(n, 1), dtype=torch.float64, device=self.device)
                meta = torch.zeros(nc + 2, dtype=torch.int64, device=self.device)   # offsets [nc + 1] | the record count
                _lib.call("cgcn_pairs_reduce", n_keys=n, keys=self.keys, n_chroms=nc, resolution_bp=self.resolution_bp,
                          pos1_out=pos1, pos2_out=pos2, count_out=count, chrom_offsets=meta, n_records=meta[nc + 1:],
                          workspace=wsp, workspace_bytes=need)
                m = meta.cpu().tolist()
            r = m[nc + 1]
            self._records = (pos1[:r].clone(), pos2[:r].clone(), count[:r].clone(), m[:nc + 1])
            if timings is not None:
                timings["reduce"] = time.perf_counter() - t0
        return self._records

    def contacts(self, chrom) -> "hic.HicContacts":
        """the chromosome's contact records (stage B) as a HicContacts: norm_vector, build and to_host work on it"""
        pos1, pos2, count, off = self._reduce()
        c = self._index(chrom)
        return hic.HicContacts(pos1[off[c]:off[c + 1]], pos2[off[c]:off[c + 1]], count[off[c]:off[c + 1]], self.device)

    def contacts_all(self, timings=None) -> Dict[str, "hic.HicContacts"]:
        self._reduce(timings)
        return {c: self.contacts(c) for c in self.chroms}
