"""The diamond sums on the device (csrc/cgcn_insulation.hip) against insulation.diamond_sums_host fed the device matrix read
back, so that the comparison does not lean on the aggregation; HicContacts.insulation against insulation_host on contact
maps with planted domains; the domain-restricted device build against the host builder.  Integer sums are compared bit for
bit, fractional ones within the bound of a reordered sum of non-negative terms, graphs exactly (indptr and indices).
Sizes: a wavefront owns a bin and its lanes stride over the window's rows, so the bin counts and the windows sit on both
sides of 64; one row is longer than a workgroup; 70 001 bins are far more than one round of the grid's wavefronts."""
import functools

import numpy as np
import pytest
import torch

from chromegcn_amd import HicContacts, build_hic_graph_host, hicnorm, insulation

import insulation_cases as IC
from test_insulation_host import DOMAIN_BP, DOMAINS, explicit_vectors

pytestmark = pytest.mark.gpu
DEV = "cuda"
ONE, EIGHT = (64,), (1, 2, 5, 63, 64, 65, 300, 1000)   # lane trips either side of 64; 300 and 1000 exceed n of every small case


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


@functools.lru_cache(maxsize=None)
def device_matrix(name):
    """(HicContacts, its device matrix, the matrix read back) of a hicnorm case"""
    c = IC.case(name)
    hc = HicContacts(c["pos1"], c["pos2"], c["count"], DEV)
    A = hc.contact_matrix(c["res"], c["n_bins"])
    return hc, A, A.to_host()


def check_sums(name, windows, with_norm, inf=False):
    c = IC.case(name)
    _, A, host = device_matrix(name)
    norm = IC.noisy_norm(c["n_bins"], 40 + c["n_bins"], inf) if with_norm else None
    nv = None if norm is None else torch.from_numpy(norm).to(DEV)
    ref = insulation.diamond_sums_host(host, norm, windows)
    got = insulation.diamond_sums(A, nv, windows)
    again = insulation.diamond_sums(A, nv, windows)
    got, again = got.cpu().numpy(), again.cpu().numpy()
    assert same_bits(got, again)                      # no order that scheduling could change
    exact = not with_norm and bool(np.all(host.data == np.floor(host.data)))
    IC.assert_sums_close(got, ref, None if exact else IC.term_counts(host, norm, windows), exact)
    assert np.all(got[:, 0] == 0)
    return got


@pytest.mark.parametrize("with_norm", [False, True])
@pytest.mark.parametrize("windows", [ONE, EIGHT], ids=["one", "eight"])
@pytest.mark.parametrize("name", ["n1", "n2", "n63", "n64", "n65", "fullrow", "n257_frac"])
def test_diamond_sums(name, windows, with_norm):
    got = check_sums(name, windows, with_norm)
    if IC.case(name)["n_bins"] > 2 and not with_norm:
        assert np.all(got[:, 1:].sum(axis=1) > 0)


def test_diamond_sums_with_every_kind_of_bad_norm_entry():
    """n63: 63 bins, four of them empty; the vector is a bin short and holds NaN, 0 and +inf"""
    norm = IC.noisy_norm(63, 40 + 63, inf=True)
    assert norm.size == 62 and np.isnan(norm).any() and (norm == 0).any() and np.isinf(norm).any()
    check_sums("n63", EIGHT, True, inf=True)


@pytest.mark.parametrize("windows", [(1,), (63,), (65,), (63, 64, 65)])
def test_single_windows_either_side_of_a_wavefront(windows):
    check_sums("n257_frac", windows, True)
    check_sums("n65", windows, False)


def test_large_grid():
    got = check_sums("n70001", (10, 50), False)    # integer counts: bit-equal
    assert np.count_nonzero(got[1]) > 69000


def test_norm_shorter_than_the_matrix_and_window_checks():
    _, A, host = device_matrix("n65")
    nv = np.full(30, 2.0)
    got = insulation.diamond_sums(A, torch.from_numpy(nv).to(DEV), (5,)).cpu().numpy()
    assert np.array_equal(got, insulation.diamond_sums_host(host, nv, (5,)))   # powers of two: exact
    assert np.all(got[0, 30 + 5:] == 0) and got[0, :30].sum() > 0              # the bins beyond the vector read as +inf
    for bad in ([], [0], [3, 3], list(range(1, 10))):
        with pytest.raises(ValueError):
            insulation.diamond_sums(A, None, bad)
    with pytest.raises(ValueError):
        insulation.diamond_sums(A, nv, (5,))       # a host vector


@pytest.mark.parametrize("name", IC.INTEGER_PLANTED)
def test_insulation_end_to_end_on_planted_domains(name):
    c, want = IC.planted_case(name), IC.planted_host(name)
    hc = HicContacts(c["pos1"], c["pos2"], c["count"], DEV)
    got = hc.insulation(None, IC.RES, [w * IC.RES for w in IC.RECOVERY_WINDOWS], n_bins=c["n_bins"], min_strength=IC.RECOVERY_STRENGTH)
    assert got.windows == want.windows == IC.RECOVERY_WINDOWS and got.sums.is_cuda
    assert same_bits(got.sums.cpu().numpy(), want.sums)
    assert np.array_equal(got.valid, want.valid) and np.array_equal(got.log2, want.log2, equal_nan=True)
    for k in range(len(IC.RECOVERY_WINDOWS)):
        assert got.boundaries[k].tolist() == want.boundaries[k].tolist() == c["starts"].tolist()
        assert np.array_equal(got.strength[k], want.strength[k])
        assert np.array_equal(got.domain_of_bin(k), want.domain_of_bin(k))
    assert hc.insulation(None, IC.RES, [w * IC.RES for w in IC.RECOVERY_WINDOWS], n_bins=c["n_bins"],
                         min_strength=IC.RECOVERY_STRENGTH) is got     # kept per argument tuple
    dom, bp = hc.domains(IC.RECOVERY_WINDOWS[0] * IC.RES, norm=None, resolution_bp=IC.RES, n_bins=c["n_bins"],
                         min_strength=IC.RECOVERY_STRENGTH)
    assert bp == IC.RES and dom.dtype == np.int32 and np.array_equal(dom, want.domain_of_bin(0))


def test_insulation_fractional_counts_and_named_norm():
    c, want = IC.planted_case("n400_frac"), IC.planted_host("n400_frac")
    hc = HicContacts(c["pos1"], c["pos2"], c["count"], DEV)
    wbp = [w * IC.RES for w in IC.RECOVERY_WINDOWS]
    got = hc.insulation(None, IC.RES, wbp, n_bins=c["n_bins"], min_strength=IC.RECOVERY_STRENGTH)
    host = hc.contact_matrix(IC.RES, c["n_bins"]).to_host()
    IC.assert_sums_close(got.sums.cpu().numpy(), want.sums, IC.term_counts(host, None, IC.RECOVERY_WINDOWS), exact=False)
    for k in range(len(IC.RECOVERY_WINDOWS)):
        assert got.boundaries[k].tolist() == c["starts"].tolist()
    vc = hc.insulation("VC", IC.RES, wbp, n_bins=c["n_bins"], min_strength=IC.RECOVERY_STRENGTH)
    vc_host = insulation.insulation_host(c["pos1"], c["pos2"], c["count"], "VC", IC.RES, wbp, n_bins=c["n_bins"],
                                         min_strength=IC.RECOVERY_STRENGTH)
    assert np.array_equal(vc.valid, vc_host.valid) and np.array_equal(vc.defined, vc_host.defined)
    np.testing.assert_allclose(vc.sums.cpu().numpy(), vc_host.sums, rtol=1e-12, atol=0)   # the VC vectors themselves differ in the last bits
    for k in range(len(IC.RECOVERY_WINDOWS)):
        assert vc.boundaries[k].tolist() == vc_host.boundaries[k].tolist()


@pytest.mark.parametrize("scoring", ["raw", "vc_oe"])
def test_device_build_within_domains(scoring):
    c, ws = IC.graph_case()
    hc = HicContacts(c["pos1"], c["pos2"], c["count"], DEV)
    norm, ex = (None, None) if scoring == "raw" else ("VC", "auto")
    want = build_hic_graph_host(c["pos1"], c["pos2"], c["count"], norm, c["res"], ws, IC.GRAPH_EDGES, min_distance_bp=2000,
                                expected=ex, domains=(DOMAINS, DOMAIN_BP))
    g, raw = hc.build(norm, c["res"], ws, IC.GRAPH_EDGES, return_raw=True, min_distance_bp=2000, expected=ex,
                      domains=(DOMAINS, DOMAIN_BP))
    assert raw.nnz > 100 and np.array_equal(raw.indptr, want.indptr) and np.array_equal(raw.indices, want.indices)
    dom = insulation.domain_of_windows(ws, DOMAINS, DOMAIN_BP)        # the vector ends before the last windows: -1 there
    assert (dom < 0).any() and insulation.domain_edge_share(raw, dom) == (raw.nnz, raw.nnz)
    full = np.concatenate([DOMAINS, [9, 9]]).astype(np.int32)         # every bin in a domain: the self loops count too
    g = hc.build(norm, c["res"], ws, IC.GRAPH_EDGES, min_distance_bp=2000, expected=ex, domains=(full, DOMAIN_BP))
    assert insulation.domain_edge_share(g, insulation.domain_of_windows(ws, full, DOMAIN_BP)) == (g.nnz, g.nnz)
    free = hc.build(norm, c["res"], ws, IC.GRAPH_EDGES, min_distance_bp=2000, expected=ex)
    same, nnz = insulation.domain_edge_share(free, insulation.domain_of_windows(ws, full, DOMAIN_BP))
    assert ws.size < same < nnz == free.nnz
    if scoring == "vc_oe":   # the vectors come from ALL records: the pre-filtered records with explicit vectors give the same graph
        nv, ev = explicit_vectors(c)
        keep = insulation.same_domain_host(c["pos1"], c["pos2"], DOMAINS, DOMAIN_BP)
        pre = build_hic_graph_host(c["pos1"][keep], c["pos2"][keep], c["count"][keep], hicnorm.pad_vector(nv, int(ws[-1]) // c["res"] + 1),
                                   c["res"], ws, IC.GRAPH_EDGES, min_distance_bp=2000, expected=ev)
        assert np.array_equal(raw.indptr, pre.indptr) and np.array_equal(raw.indices, pre.indices)


def test_graphs_from_contact_caches_within_domains(tmp_path):
    from chromegcn_amd import hic
    p = IC.planted_case("n257")
    pw = (np.arange(0, 257, 2) * IC.RES).astype(np.int32)
    hic.save_contacts_cache(hic.contact_cache_path(str(tmp_path), "chrT"), hic.HostContacts(p["pos1"], p["pos2"], p["count"], {}, IC.RES, pw))
    kw = dict(window_bp=10 * IC.RES, norm=None, resolution_bp=IC.RES, min_strength=IC.RECOVERY_STRENGTH)
    report = {}
    g = hic.graphs_from_contact_caches(str(tmp_path), ["chrT"], 600, "", domains=kw, domain_report=report)["chrT"]
    dom = np.searchsorted(p["starts"], np.arange(257), side="right").astype(np.int32)
    want = HicContacts(p["pos1"], p["pos2"], p["count"], DEV).build(None, IC.RES, pw, 600, domains=(dom, IC.RES))
    assert g.nnz == want.nnz and torch.equal(g.rowptr, want.rowptr) and torch.equal(g.col[:g.nnz], want.col[:g.nnz])
    free = build_hic_graph_host(p["pos1"], p["pos2"], p["count"], None, IC.RES, pw, 600)
    assert report == {"chrT": (3,) + insulation.domain_edge_share(free, dom[pw // IC.RES])}
    plain = hic.graphs_from_contact_caches(str(tmp_path), ["chrT"], 600, "")["chrT"]     # the default: as it was
    assert plain.nnz == free.nnz + pw.size


def test_within_domains_keeps_file_order_and_domains_from_the_records():
    c, ws = IC.graph_case()
    hc = HicContacts(c["pos1"], c["pos2"], c["count"], DEV)
    keep = insulation.same_domain_host(c["pos1"], c["pos2"], DOMAINS, DOMAIN_BP)
    sel = hc.within_domains(DOMAINS, DOMAIN_BP)
    assert 0 < sel.M == int(keep.sum()) < hc.M
    assert np.array_equal(sel.pos1.cpu().numpy(), c["pos1"][keep]) and np.array_equal(sel.pos2.cpu().numpy(), c["pos2"][keep])
    assert np.array_equal(sel.count.cpu().numpy(), c["count"][keep])
    with pytest.raises(ValueError):
        hc.build_raw(None, c["res"], ws, IC.GRAPH_EDGES, domains=(DOMAINS, 1500))
    p = IC.planted_case("n257")
    pw = (np.arange(0, 257, 2) * IC.RES).astype(np.int32)
    kw = dict(window_bp=10 * IC.RES, norm=None, resolution_bp=IC.RES, min_strength=IC.RECOVERY_STRENGTH)
    _, raw = HicContacts(p["pos1"], p["pos2"], p["count"], DEV).build(None, IC.RES, pw, 600, return_raw=True, domains=kw)
    want = build_hic_graph_host(p["pos1"], p["pos2"], p["count"], None, IC.RES, pw, 600, domains=kw)
    assert raw.nnz > 0 and np.array_equal(raw.indptr, want.indptr) and np.array_equal(raw.indices, want.indices)
