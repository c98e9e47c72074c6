"""What every analysis of one chromosome's balanced Hi-C map does before its own rule starts (insulation, compartments, loops,
pile-ups): the records and a norm name become (matrix, norm vector, expected vector); a bin is valid or not; a CSR gives its
upper band; a device vector or band is checked before a kernel reads it.  csrc/cgcn_hicmap.hpp is the device side.  Nothing
here knows an analysis: this module imports hicnorm and hicdist and none of the modules that import it.  The norm vector "as
rule 1 reads it" is hicnorm.clean_norm, one level down, because hicdist reads it too."""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp
import torch

from . import hicdist, hicnorm

MAX_ELEMS = 1 << 28   # elements of a band (csrc: LP_MAX_PIXELS, PU_MAX_ELEMS)


# ----------------------------------------------------------------------------------------------
# records -> (matrix, norm vector, expected vector) on the host
# ----------------------------------------------------------------------------------------------
def auto_expected(expected) -> bool:
    """whether an analysis' `expected` asks for the vector computed from the records; any string but "auto" is an error"""
    if isinstance(expected, str) and expected != "auto":
        raise ValueError("expected=%r is neither a vector nor 'auto'" % (expected,))
    return isinstance(expected, str)


def matrix_host(pos1, pos2, count, resolution_bp, n_bins=None):
    """(A, vc): hicnorm.contact_matrix_host's CSR of the records at resolution_bp and its row sums.  The first half of
    resolve_host, for a caller whose size guard needs A's bins before the vectors are computed."""
    A = hicnorm.contact_matrix_host(pos1, pos2, count, int(resolution_bp), n_bins)
    return A, np.asarray(A.sum(axis=1)).ravel()


def vectors_host(pos1, pos2, count, n, norm, resolution_bp, n_bins=None, norm_args=None, expected=None, expected_args=None):
    """(norm vector or None, expected vector or None) for the map of n bins.  norm: None, a vector, or 'KR' / 'VC' / 'SQRTVC'
    (computed from the records with norm_args; HicNormError for a KR that did not converge).  expected: None (the analysis
    reads no expected vector: none is computed), a vector, or "auto": hicdist.expected_from_sums with expected_args of the
    distance sums under this norm added in the DEVICE's order (hicdist.distance_sums_device_order_host), that is
    HicContacts.expected_vector to the last bit."""
    res = int(resolution_bp)
    norm = hicnorm.resolve_norm_host(pos1, pos2, count, norm, res, n_bins, norm_args)
    if auto_expected(expected):
        sums = hicdist.distance_sums_device_order_host(pos1, pos2, count, norm, res, n)
        expected = hicdist.expected_from_sums(*sums, **(expected_args or {}))
    return norm, expected


def resolve_host(pos1, pos2, count, norm, resolution_bp, n_bins=None, norm_args=None, expected=None, expected_args=None):
    """(A, vc, norm vector or None, expected vector or None): matrix_host, then vectors_host at A's bins"""
    A, vc = matrix_host(pos1, pos2, count, resolution_bp, n_bins)
    return (A, vc) + vectors_host(pos1, pos2, count, A.shape[0], norm, resolution_bp, n_bins, norm_args, expected, expected_args)


# ----------------------------------------------------------------------------------------------
# bins
# ----------------------------------------------------------------------------------------------
def valid_bins(vc, norm):
    """valid[b] from the row sums and the norm vector: VC[b] > 0 and nv[b] finite (None: every bin in contact is valid)"""
    vc = np.asarray(vc, dtype=np.float64).ravel()
    return (vc > 0) if norm is None else (vc > 0) & np.isfinite(hicnorm.clean_norm(norm, vc.size))


def bins_of_band_host(vc, norm, n):
    """(valid bool [n], nv float64 [n]: all ones without a vector) of the n bins of a host band and its row sums vc"""
    vc = np.asarray(vc, dtype=np.float64).ravel()
    if vc.size != n:
        raise ValueError("vc has %d bins but the band has %d" % (vc.size, n))
    return valid_bins(vc, norm), np.ones(n) if norm is None else hicnorm.clean_norm(norm, n)


# ----------------------------------------------------------------------------------------------
# graphs
# ----------------------------------------------------------------------------------------------
def csr_of(graph_or_csr):
    """(rowptr int64 [N + 1], col int64 [nnz], nnz) on the host of a graph: a ChromGraph, a scipy matrix, or (rowptr, col[, nnz])
    tensors or arrays"""
    g = graph_or_csr
    if sp.issparse(g):
        g = sp.csr_matrix(g)
        rowptr, col = g.indptr, g.indices
    elif isinstance(g, (tuple, list)):
        rowptr, col = g[0], g[1]
    else:
        rowptr, col = g.rowptr, g.col
    if torch.is_tensor(rowptr):
        rowptr, col = rowptr.cpu().numpy(), col.cpu().numpy()
    rowptr = np.asarray(rowptr, dtype=np.int64)
    nnz = int(rowptr[-1]) if rowptr.size else 0
    return rowptr, np.asarray(col, dtype=np.int64)[:nnz], nnz


def edge_rows(graph_or_csr, n_windows, what):
    """(row int64 [nnz], col int64 [nnz], nnz): the two windows of every stored entry of a graph (csr_of's inputs), which must
    have n_windows windows, the length of the per-window vector named `what`"""
    rowptr, col, nnz = csr_of(graph_or_csr)
    if n_windows != rowptr.size - 1:
        raise ValueError("the graph has %d windows but %s has %d" % (rowptr.size - 1, what, n_windows))
    return np.repeat(np.arange(n_windows, dtype=np.int64), np.diff(rowptr)), col, nnz


# ----------------------------------------------------------------------------------------------
# bands
# ----------------------------------------------------------------------------------------------
def band_host(A, width) -> np.ndarray:
    """band float64 [n, width], band[i, d] = A[i, i + d] (0 beyond the matrix), from anything scipy makes a CSR of"""
    width = int(width)
    if width < 1:
        raise ValueError("the band is at least one distance wide")
    coo = sp.csr_matrix(A, dtype=np.float64).tocoo()
    band = np.zeros((coo.shape[0], width))
    d = coo.col.astype(np.int64) - coo.row
    k = (d >= 0) & (d < width)
    band[coo.row[k], d[k]] = coo.data[k]
    return band


def device_band(A: hicnorm.DeviceContactMatrix, width) -> torch.Tensor:
    """band float64 [n, width] on the device, band[i, d] = A[i, i + d] (cgcn_hicloops_band: enqueue only)"""
    from . import _lib
    width = int(width)
    if width < 1:
        raise ValueError("the band is at least one distance wide")
    dev = A.rowptr.device
    band = torch.zeros(A.n, width, dtype=torch.float64, device=dev)
    if A.n:
        with torch.cuda.device(dev):
            _lib.call("cgcn_hicloops_band", n=A.n, rowptr=A.rowptr, col=A.col, val=A.val, width=width, band=band)
    return band


def device_vector(v, dev, what, optional=False):
    """v, a non-empty contiguous float64 vector on dev (None passes when optional), or the ValueError that names it"""
    if v is None and optional:
        return None
    if not (torch.is_tensor(v) and v.device == dev and v.dtype == torch.float64 and v.is_contiguous() and v.ndim == 1
            and v.numel() > 0):
        raise ValueError("%s must be a non-empty contiguous float64 vector on the matrix's device" % what)
    return v


def check_band(band, vc, min_width, distances=None, what="band"):
    """(n, width) of a device band that a kernel may read: contiguous float64 [n, >= min_width], at most 2^28 elements over
    `distances` distances (None: its width), and, unless vc is None, row sums vc of its n bins on its device"""
    n, width = int(band.shape[0]), int(band.shape[1])
    if band.dtype != torch.float64 or not band.is_contiguous() or width < min_width:
        raise ValueError("the %s must be contiguous float64 [n, >= %d]" % (what, min_width))
    distances = width if distances is None else distances
    if n * distances > MAX_ELEMS:
        raise ValueError("%d bins x %d distances are more than 2^28 band elements" % (n, distances))
    if vc is not None:
        device_vector(vc, band.device, "vc")
        if int(vc.numel()) != n:
            raise ValueError("vc has %d bins but the band has %d" % (int(vc.numel()), n))
    return n, width


def expected_reach(n_ex, n, reach, what):
    """an expected vector of n_ex entries must hold the own distance of everything that reads it: min(n, reach) entries, reach
    the largest distance + 1 of the `what` ("pixels", "centres")"""
    if n_ex < min(n, reach):
        raise ValueError("the expected vector has %d entries but the %s reach distance %d" % (n_ex, what, min(n, reach) - 1))


def expected_at_host(ex, n, size, reach, what) -> np.ndarray:
    """the expected vector at `size` distances on the host (0 beyond its length), checked by expected_reach"""
    given = np.asarray(ex, dtype=np.float64).ravel()
    expected_reach(given.size, n, reach, what)
    out = np.zeros(size)
    out[:min(size, given.size)] = given[:size]
    return out
