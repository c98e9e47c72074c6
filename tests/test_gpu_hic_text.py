"""Hi-C contact text parsed on the device (csrc/cgcn_text.hip, HicContacts.from_text) against parse_contacts_text_host, which
tests/test_hic_text_host.py ties to Python's int() / float() and to the reference's step 7.  Every comparison is exact: pos1,
pos2 identical, count as int64 bit patterns, the set of host-parsed lines identical."""
import os
import sys

import numpy as np
import pytest
import torch

from chromegcn_amd import hic, synth

from hic_text_cases import FAST_F3, SLOW_F3, assert_parses_like_python, dense_lines, juicer_text, mixed_lines

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(c):
    """(pos1, pos2, count as int64 bit patterns) of a HicContacts or of parse_contacts_text_host's result"""
    if isinstance(c, hic.HicContacts):
        return c.pos1.cpu().numpy(), c.pos2.cpu().numpy(), c.count.cpu().numpy().view(np.int64)
    return c[0], c[1], c[2].view(np.int64)


def assert_same_records(c, want, what=""):
    got, exp = bits(c), bits(want)
    assert got[0].dtype == np.int32 and got[1].dtype == np.int32 and c.count.dtype == torch.float64, what
    for g, w in zip(got, exp):
        assert g.shape == w.shape and np.array_equal(g, w), what
    if not isinstance(want, hic.HicContacts):
        assert np.array_equal(c.text_info["slow_lines"], want[3]), what


@pytest.fixture(scope="module")
def juicer():
    """a Juicer-style dump at chr21 size, its host parse and its device parse: made once, never changed"""
    r = synth.raw_contacts("chr21")
    data = juicer_text(r["pos1"], r["pos2"], r["count"])
    return r, data, hic.parse_contacts_text_host(data), hic.contacts_from_text(data, device=DEV)


@pytest.fixture(scope="module")
def mixed():
    """about 200 k lines of every fast and slow shape, 6 bytes to the line bound (and one beyond), under 1 % slow"""
    lines = mixed_lines(200000, 11)
    data = b"\n".join(lines) + b"\n"
    return lines, data, hic.parse_contacts_text_host(data)


@pytest.mark.timeout(600)
def test_juicer_file_at_chr21_size_is_parsed_by_the_kernel_alone(juicer):
    r, data, host, c = juicer
    assert host[3].size == 0 and c.text_info["slow_lines"].size == 0 and c.text_info["parse_calls"] == 1
    assert c.M == r["pos1"].size > 3000000 and c.text_info["n_bytes"] == len(data)
    assert_same_records(c, host, "juicer")
    assert np.array_equal(bits(c)[0], r["pos1"]) and np.array_equal(bits(c)[2], r["count"].view(np.int64))


@pytest.mark.timeout(600)
def test_mixed_file_of_every_shape_and_length(mixed, tmp_path):
    lines, data, host = mixed
    lengths = np.array([len(ln) for ln in lines])
    assert lengths.min() == 5 and lengths.max() == 65 and (lengths == 64).sum() > 100     # without the LF
    assert 0 < host[3].size <= 0.01 * len(lines)
    path = tmp_path / "chrT_1kb.RAWobserved"
    path.write_bytes(data)
    for src in (data, str(path), bytearray(data)):
        c = hic.contacts_from_text(src, device=DEV)
        assert c.M == len(lines) and c.text_info["parse_calls"] == 1
        assert_same_records(c, host, type(src))


@pytest.mark.timeout(600)
def test_small_staging_chunks_give_the_same_records(mixed, tmp_path):
    lines, data, host = mixed
    path = tmp_path / "chrT_1kb.RAWobserved"
    path.write_bytes(data)
    part = data[:data.index(b"\n", 300000)]                                       # some whole lines, the last without its LF
    for src, chunk in ((str(path), 40961), (data, 65537), (part, 4099)):           # no multiple of a tile, a line or 16
        want = host if src is not part else hic.parse_contacts_text_host(part)
        assert_same_records(hic.contacts_from_text(src, device=DEV, chunk_bytes=chunk), want, chunk)


@pytest.mark.timeout(600)
def test_flag_list_that_overflows_is_fetched_by_a_second_call(mixed):
    lines, data, host = mixed
    assert host[3].size > 100
    c = hic.contacts_from_text(data, device=DEV, flag_capacity=7)
    assert c.text_info["parse_calls"] == 2
    assert_same_records(c, host, "capacity 7")
    c = hic.contacts_from_text(data, device=DEV, flag_capacity=0)
    assert c.text_info["parse_calls"] == 2
    assert_same_records(c, host, "capacity 0")
    c = hic.contacts_from_text(data, device=DEV, flag_capacity=int(host[3].size))      # exactly enough
    assert c.text_info["parse_calls"] == 1
    assert_same_records(c, host, "exact capacity")


def test_every_listed_shape_against_python_itself():
    """the device result against int() / float() directly, not through the host restatement: a fault the two walks share
    (a significand that wraps 64 bits) shows here"""
    lines = [("%d\t%d\t%s" % (1000 * k, 2147483647 - k, f3)).encode() for k, f3 in enumerate(FAST_F3 + SLOW_F3)]
    data = b"\n".join(lines) + b"\n"
    c = hic.contacts_from_text(data, device=DEV)
    p1, p2, cnt = bits(c)
    assert_parses_like_python(lines, data, got=(p1, p2, cnt.view(np.float64), c.text_info["slow_lines"]))
    assert c.text_info["slow_lines"].tolist() == list(range(len(FAST_F3), len(lines)))


def test_a_file_of_six_byte_lines_has_two_or_three_line_starts_in_every_lane():
    """k_text_starts reads 16 bytes per lane: in a file of 6-byte lines every lane of every tile holds two or three line
    starts and a tile 682 or 683, five times what the Juicer and the mixed files reach.  Against Python's own int() and
    float(), with room for every slow line and with a flag list that overflows."""
    lines = dense_lines()
    data = b"\n".join(lines) + b"\n"
    starts = np.concatenate([[0], np.flatnonzero(np.frombuffer(data, np.uint8) == 10)[:-1] + 1])
    per_lane, per_tile = np.bincount(starts // 16)[:-1], np.bincount(starts // 4096)[:-1]
    assert starts.size == len(lines) == 100000 and per_lane.min() == 2 and per_lane.max() == 3
    assert per_tile.min() == 682 and per_tile.max() == 683
    n_slow = sum(ln == b"1\t2\t1e23" for ln in lines)
    assert n_slow == 100
    for cap, calls in ((1 << 16, 1), (n_slow - 1, 2), (7, 2)):
        c = hic.contacts_from_text(data, device=DEV, flag_capacity=cap)
        assert c.M == len(lines) and c.text_info["parse_calls"] == calls, cap
        p1, p2, cnt = bits(c)
        slow = assert_parses_like_python(lines, data, got=(p1, p2, cnt.view(np.float64), c.text_info["slow_lines"]))
        assert slow.tolist() == list(range(999, 100000, 1000))
    assert_same_records(c, hic.parse_contacts_text_host(data), "dense")


def test_empty_file_single_line_and_crlf(mixed):
    lines, _, _ = mixed
    for data in (b"", b"1000\t2000\t3.5", b"1000\t2000\t3.5\n", b"1000\t2000\t3.5\r\n", b"7\t8\t9\r", b"1\t2\t1e400\n3\t4\t5"):
        assert_same_records(hic.contacts_from_text(data, device=DEV), hic.parse_contacts_text_host(data), data)
    few = lines[:20000]
    for data in (b"\r\n".join(few) + b"\r\n", b"\r\n".join(few), b"\n".join(few)):
        want = hic.parse_contacts_text_host(data)
        assert want[0].size == len(few)
        assert_same_records(hic.contacts_from_text(data, device=DEV), want, data[-2:])
    # a line whose LF is the last byte of a 4096-byte tile, the first of the next one, or near either
    for pad in range(4090, 4101):
        body, size, k = [], 0, 0
        while size + 40 < pad:
            body.append(b"%d\t%d\t%d.5\n" % (k * 1000, k * 1000 + 1000, k))
            size += len(body[-1])
            k += 1
        last = b"5\t6\t" + b"0" * (pad - size - 5) + b"\n"          # ends exactly at byte `pad`
        data = b"".join(body) + last + b"123000\t456000\t-7.25e-3\n9\t9\t9"
        assert len(last) <= 65 and data[pad - 1:pad] == b"\n"
        assert_same_records(hic.contacts_from_text(data, device=DEV), hic.parse_contacts_text_host(data), pad)


@pytest.mark.timeout(600)
def test_two_parses_are_bitwise_equal(juicer, mixed):
    _, data, _, first = juicer
    assert_same_records(hic.contacts_from_text(data, device=DEV), first, "juicer again")
    _, data, _ = mixed
    a, b = hic.contacts_from_text(data, device=DEV), hic.contacts_from_text(data, device=DEV)
    assert_same_records(a, b, "mixed again")
    assert np.array_equal(a.text_info["slow_lines"], b.text_info["slow_lines"])


def test_malformed_lines_raise_the_hosts_message(mixed, tmp_path):
    lines, _, _ = mixed
    good = lines[:5000]
    cases = [(7, b""), (0, b"#comment"), (4999, b"1\t2"), (300, b"1\t2\t3\t4"), (1234, b"a\tb\tc"), (4000, b"1\t2\tnan\t"),
             (2500, b"1\t2\t3" + b"0" * 80 + b"x"), (2501, b"nan\t2\t3"), (17, b"\t\t")]
    for k, bad in cases:
        body = good[:k] + [bad] + good[k:]
        for data in (b"\n".join(body) + b"\n", b"\n".join(body + [b"#later", b""]) + b"\n"):   # alone, and the first of several
            with pytest.raises(ValueError) as host:
                hic.parse_contacts_text_host(data)
            assert str(host.value) == "contact text: line %d is not `pos1<TAB>pos2<TAB>count`" % (k + 1)
            with pytest.raises(ValueError) as dev:
                hic.contacts_from_text(data, device=DEV, flag_capacity=3)
            assert str(dev.value) == str(host.value), (k, bad)
    path = tmp_path / "bad.RAWobserved"
    path.write_bytes(b"1\t2\t3\n4\t5\n")
    with pytest.raises(ValueError, match="contact text: line 2 is not"):
        hic.contacts_from_text(str(path), device=DEV)


@pytest.mark.timeout(600)
def test_text_to_graph_equals_arrays_to_graph(juicer):
    r, _, _, c = juicer
    ref = hic.HicContacts(r["pos1"], r["pos2"], r["count"], DEV)
    for norm, edges in ((None, 500000), (r["norm"], 250000)):
        got = c.build(norm, 1000, r["window_start"], edges)
        want = ref.build(norm, 1000, r["window_start"], edges)
        assert got.n == want.n and got.nnz == want.nnz > 200000
        assert torch.equal(got.rowptr, want.rowptr) and torch.equal(got.col, want.col)
    h = c.to_host(norms={"KR": r["norm"]}, resolution_bp=1000, window_start=r["window_start"])
    assert isinstance(h, hic.HostContacts) and h.M == c.M and np.array_equal(h.count, r["count"]) and h.resolution_bp == 1000


@pytest.mark.timeout(600)
def test_hic_ingest_writes_the_caches_train_loads(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import hic_ingest
    finally:
        sys.path.pop(0)
    root, out, recs, bed = tmp_path / "hic", tmp_path / "caches", {}, []
    for chrom in ("chr21", "chr22"):
        r = recs[chrom] = synth.raw_contacts(chrom, background_per_bin=2.0, peak_pairs_per_window=20.0)
        d = hic_ingest.chrom_dir(str(root), "GM12878", "1", chrom)
        os.makedirs(d)
        with open(os.path.join(d, "%s_1kb.RAWobserved" % chrom), "wb") as f:
            f.write(juicer_text(r["pos1"], r["pos2"], r["count"]))
        with open(os.path.join(d, "%s_1kb.KRnorm" % chrom), "w") as f:
            f.write("".join("NaN\n" if np.isnan(x) else "%r\n" % float(x) for x in r["norm"]))
        bed += ["%s\t%d\t%d\tpeak\n" % (chrom, s, s + 1000) for s in r["window_start"][::-1]] * 2
    (tmp_path / "windows.bed").write_text("".join(bed))
    lines = hic_ingest.main(["--hic-root", str(root), "--cell", "GM12878", "--bed", str(tmp_path / "windows.bed"),
                             "--chroms", "chr21,chr22", "--out", str(out), "--chunk-bytes", "1000003"])
    assert [ln["chrom"] for ln in lines] == ["chr21", "chr22"] and all(ln["host_parsed_lines"] == 0 and ln["norms"] == ["KR"]
                                                                         for ln in lines)
    for hicnorm in ("", "KR"):
        graphs = hic.graphs_from_contact_caches(str(out), ["chr21", "chr22"], 100000, hicnorm, device=DEV)
        for chrom, r in recs.items():
            want = hic.build_hic_graph(r["pos1"], r["pos2"], r["count"], r["norm"] if hicnorm else None, 1000, r["window_start"],
                                       100000, device=DEV)
            g = graphs[chrom]
            assert g.n == want.n == r["window_start"].size and g.nnz == want.nnz > 50000
            assert torch.equal(g.rowptr, want.rowptr) and torch.equal(g.col, want.col)
            assert torch.equal(g.row_scale.view(torch.int32), want.row_scale.view(torch.int32))
