"""What the two text readers (hictext: contact text, pairs: read-pair text) share on the host: bytes as a uint8 vector, the
line table, a source over a path or a memoryview, the two pinned staging buffers and the stage timers."""
import os
import time

import numpy as np
import torch


def _text_bytes(data) -> np.ndarray:
    if isinstance(data, np.ndarray):
        if data.dtype != np.uint8 or data.ndim != 1:
            raise TypeError("contact text as an array must be a uint8 vector")
        return np.ascontiguousarray(data)
    return np.frombuffer(data, dtype=np.uint8)


def _text_lines(buf):
    """(start, end) int64 [M] of every line: its first byte and the byte behind its last (terminator excluded)"""
    n = buf.size
    lf = np.flatnonzero(buf == 10)
    start = np.concatenate([np.zeros(1, np.int64), lf + 1])
    start = start[start < n]
    end = np.concatenate([lf, np.full(1, n, np.int64)])[:start.size]
    cr = (end < n) & (end > start) & (buf[np.maximum(end - 1, 0)] == 13)
    return start, end - cr


def _find_lf(mem, off: int) -> int:
    """index of the first LF at or behind `off` in a byte memoryview, or its length - 1"""
    step = 4096
    for lo in range(off, len(mem), step):
        k = bytes(mem[lo:lo + step]).find(b"\n")
        if k >= 0:
            return lo + k
    return len(mem) - 1


_staging = {}   # (device, chunk_bytes) -> the two pinned staging buffers of from_text (release_text_staging frees them)


def staging(device, chunk_bytes):
    """the two pinned buffers of `chunk_bytes` for `device`: made on first use, replaced when either changes"""
    key = (device, chunk_bytes)
    if key not in _staging:
        _staging.clear()
        _staging[key] = [torch.empty(chunk_bytes, dtype=torch.uint8, pin_memory=True) for _ in range(2)]
    return _staging[key]


def release_text_staging():
    """Free the two pinned staging buffers HicContacts.from_text keeps between calls (2 x chunk_bytes of page-locked host
    memory, 64 MiB at the default; kept because pinning costs more than a chunk's copy, replaced when chunk_bytes or the
    device changes)."""
    _staging.clear()


class TextSource:
    """The n bytes of a path, or of bytes / bytearray / memoryview: read front to back with read_into, and line by line at
    known offsets with line_at.  A path is opened when first read; close() closes it."""

    def __init__(self, path_or_bytes):
        self.is_path = isinstance(path_or_bytes, (str, os.PathLike))
        self.path = path_or_bytes if self.is_path else None
        self.mem = None if self.is_path else memoryview(path_or_bytes).cast("B")
        self.n = os.path.getsize(path_or_bytes) if self.is_path else len(self.mem)
        self.off = 0            # bytes read_into has taken
        self._raw = self._lines = None

    def read_into(self, view, want):
        """the next `want` bytes into the byte memoryview `view`"""
        if self.is_path:
            if self._raw is None:
                self._raw = open(self.path, "rb", buffering=0)
            got = 0
            while got < want:
                r = self._raw.readinto(view[got:want])
                if not r:
                    raise ValueError("%s ended after %d of %d bytes" % (self.path, self.off + got, self.n))
                got += r
        else:
            view[:want] = self.mem[self.off:self.off + want]
        self.off += want

    def line_at(self, off) -> bytes:
        """the line that starts at byte `off`, without its terminator"""
        if self.is_path:
            if self._lines is None:
                self._lines = open(self.path, "rb")
            self._lines.seek(off)
            raw = self._lines.readline()
        else:
            raw = bytes(self.mem[off:_find_lf(self.mem, off) + 1])
        return raw[:-2] if raw.endswith(b"\r\n") else raw[:-1] if raw.endswith(b"\n") else raw

    def close(self):
        for f in (self._raw, self._lines):
            if f is not None:
                f.close()
        self._raw = self._lines = None


def lap_timer(timings, device):
    """lap(name) -> the seconds since the lap before (or since now), with a device sync in front, kept as timings[name]:
    a stage that runs again overwrites its time.  lap() only measures.  Without a `timings` dict it does nothing: None."""
    t = [time.perf_counter()]

    def lap(name=None):
        if timings is None:
            return None
        torch.cuda.synchronize(device)
        t.append(time.perf_counter())
        if name is not None:
            timings[name] = t[-1] - t[-2]
        return t[-1] - t[-2]

    return lap


def lap_adder(totals, enabled, device):
    """lap(name, t0): totals[name] += the seconds since t0, with a device sync in front; does nothing unless `enabled`"""
    def lap(name, t0):
        if enabled:
            torch.cuda.synchronize(device)
            totals[name] += time.perf_counter() - t0

    return lap
