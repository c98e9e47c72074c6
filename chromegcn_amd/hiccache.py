"""Contact records of one chromosome on the host: the plain numpy text loader, the windows bed, and the flat binary
`.cghic` cache that `chromegcn_amd.train -hic_contacts` reads (hic.graphs_from_contact_caches)."""
from __future__ import annotations

import csv
import os
from dataclasses import dataclass, field
from typing import Dict, Optional

import numpy as np


@dataclass
class HostContacts:
    pos1: np.ndarray                 # int32 [M]
    pos2: np.ndarray                 # int32 [M]
    count: np.ndarray                # float64 [M]
    norms: Dict[str, np.ndarray] = field(default_factory=dict)   # name ('KR', 'VC', 'SQRTVC') -> float64 [n_bins]
    resolution_bp: int = 1000
    window_start: Optional[np.ndarray] = None   # int32 [N]: the chromosome's windows with peaks, when known

    @property
    def M(self) -> int:
        return int(self.pos1.shape[0])


def load_contacts_text(raw_path: str, norm_paths: Optional[Dict[str, str]] = None, resolution_bp: int = 1000,
                       window_start=None) -> HostContacts:
    """Parse a `RAWobserved` file (`start_pos1<TAB>start_pos2<TAB>count` per line) and its norm files (one value per line,
    'NaN' allowed) once, with numpy.  Slow and simple on purpose: the result goes into the binary cache."""
    from .hic import _windows
    raw = np.loadtxt(raw_path, dtype=np.float64, delimiter="\t", ndmin=2)
    if raw.size == 0:
        raw = raw.reshape(0, 3)
    if raw.shape[1] != 3:
        raise ValueError("%s: expected three columns, found %d" % (raw_path, raw.shape[1]))
    norms = {name: np.loadtxt(p, dtype=np.float64, ndmin=1) for name, p in (norm_paths or {}).items()}
    return HostContacts(raw[:, 0].astype(np.int32), raw[:, 1].astype(np.int32), np.ascontiguousarray(raw[:, 2]), norms,
                        int(resolution_bp), None if window_start is None else _windows(window_start))


def windows_from_bed(path: str, chroms) -> Dict[str, np.ndarray]:
    """{chrom: int32 window starts, ascending} of a windows bed (chrom<TAB>start<TAB>...): create_bin_dict of
    data/7create_graph_new.py:14-47 -- the distinct start positions of every chromosome of `chroms`; a window's node index
    is its rank.  Host only."""
    starts = {c: set() for c in chroms}
    with open(path, newline="") as f:
        for row in csv.reader(f, delimiter="\t"):
            if row and row[0] in starts:
                starts[row[0]].add(int(row[1]))
    return {c: np.array(sorted(s), dtype=np.int32) for c, s in starts.items()}


_MAGIC = b"CGHIC01\0"


def save_contacts_cache(path: str, c: HostContacts):
    """Flat little-endian file: magic, int64 header [M, n_norms, resolution_bp, N or -1], pos1 int32[M], pos2 int32[M],
    count fp64[M], per norm vector (name 16 bytes, int64 n_bins, fp64[n_bins]), window_start int32[N]."""
    n = -1 if c.window_start is None else int(c.window_start.shape[0])
    with open(path, "wb") as f:
        f.write(_MAGIC)
        f.write(np.array([c.M, len(c.norms), c.resolution_bp, n], dtype="<i8").tobytes())
        f.write(np.ascontiguousarray(c.pos1, dtype="<i4").tobytes())
        f.write(np.ascontiguousarray(c.pos2, dtype="<i4").tobytes())
        f.write(np.ascontiguousarray(c.count, dtype="<f8").tobytes())
        for name, v in c.norms.items():
            b = name.encode()
            if not 0 < len(b) <= 16:
                raise ValueError("norm name %r does not fit 16 bytes" % name)
            f.write(b.ljust(16, b"\0"))
            f.write(np.array([v.shape[0]], dtype="<i8").tobytes())
            f.write(np.ascontiguousarray(v, dtype="<f8").tobytes())
        if n >= 0:
            f.write(np.ascontiguousarray(c.window_start, dtype="<i4").tobytes())


def load_contacts_cache(path: str) -> HostContacts:
    from .hic import _windows

    def take(f, dtype, k):
        raw = f.read(np.dtype(dtype).itemsize * k)
        if len(raw) != np.dtype(dtype).itemsize * k:
            raise ValueError("%s is truncated" % path)
        return np.frombuffer(raw, dtype=dtype).copy()

    with open(path, "rb") as f:
        if f.read(8) != _MAGIC:
            raise ValueError("%s is not a chromegcn contact cache" % path)
        m, n_norms, res, n = take(f, "<i8", 4).tolist()
        if m < 0 or n_norms < 0 or res < 1 or n < -1:
            raise ValueError("%s is corrupt" % path)
        pos1, pos2, count = take(f, "<i4", m), take(f, "<i4", m), take(f, "<f8", m)
        norms = {}
        for _ in range(n_norms):
            name = f.read(16).rstrip(b"\0").decode()
            norms[name] = take(f, "<f8", int(take(f, "<i8", 1)[0]))
        ws = None if n < 0 else _windows(take(f, "<i4", n))
    return HostContacts(pos1, pos2, count, norms, int(res), ws)


def contact_cache_path(root: str, chrom: str) -> str:
    return os.path.join(root, "%s.cghic" % chrom)
