"""Read-pair text on the device (csrc/cgcn_pairs.hip, chromegcn_amd.pairs.ReadPairs) against bin_read_pairs_host and
pairs_to_contacts_host, which tests/test_pairs_host.py ties to the reference's own output, to Python's int() and round() and to
a Counter.  Every comparison is exact: int32 arrays equal, counts as int64 bit patterns, `info` equal."""
import os
import sys

import numpy as np
import pytest
import torch

from chromegcn_amd import ReadPairs, bin_read_pairs_host, build_hic_graph_host, hic, pairs, synth

import pairs_cases as PC

pytestmark = pytest.mark.gpu
DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))


def assert_same(rp, hp, what=""):
    """the device result against the host restatement: binned pairs, records and info"""
    assert pairs.same_info(rp.info, hp.info), (what, {k: v for k, v in rp.info.items() if k != "slow_lines"}, hp.info)
    assert rp.keys.dtype == torch.int64 and rp.keys.numel() == hp.info["kept"]
    for c in hp.chroms:
        g1, g2 = rp.binned(c)
        w1, w2 = hp.binned(c)
        assert g1.dtype == torch.int32 and g2.dtype == torch.int32
        assert np.array_equal(g1.cpu().numpy(), w1) and np.array_equal(g2.cpu().numpy(), w2), (what, c)
        rec, want = rp.contacts(c), hp.contacts(c)
        assert isinstance(rec, hic.HicContacts) and rec.pos1.dtype == torch.int32 and rec.count.dtype == torch.float64
        assert np.array_equal(rec.pos1.cpu().numpy(), want[0]) and np.array_equal(rec.pos2.cpu().numpy(), want[1]), (what, c)
        assert np.array_equal(rec.count.cpu().numpy().view(np.int64), want[2].view(np.int64)), (what, c)


@pytest.fixture(scope="module")
def mixed():
    """about 200 k lines of every fast and slow shape with CR LF and LF mixed and no terminator at the end, and the host's
    parse of them: made once, never changed"""
    lines = PC.mixed_lines(200000, 11) + PC.tie_lines()
    data = PC.join_lines(lines, 3, 0.3, final_terminator=False)
    return lines, data, bin_read_pairs_host(data, chroms=PC.CHROMS)


@pytest.fixture(scope="module")
def mixed_dev(mixed):
    return ReadPairs.from_text(mixed[1], chroms=PC.CHROMS, device=DEV)


def test_golden_file_matches_the_reference_line_for_line():
    g = np.load(os.path.join(HERE, "golden", "g13_pairs.npz"))
    chroms = [str(c) for c in g["chroms"]]
    rp = ReadPairs.from_text(g["input"].tobytes(), chroms=chroms, device=DEV)
    for c in chroms:
        rows = [ln.split(b"\t") for ln in g["out_" + c].tobytes().split(b"\r\n")[:-1]]
        p1, p2 = rp.binned(c)
        assert p1.cpu().tolist() == [int(r[0]) for r in rows] and p2.cpu().tolist() == [int(r[1]) for r in rows], c
        assert all(int(r[2]) == abs(int(r[1]) - int(r[0])) for r in rows)
    assert sum(rp.info["kept_per_chrom"].values()) == rp.info["kept"] > 1000
    assert_same(rp, bin_read_pairs_host(g["input"].tobytes(), chroms=chroms), "golden")


def test_mixed_file_of_every_shape_and_length(mixed, mixed_dev, tmp_path):
    lines, data, host = mixed
    lengths = np.array([len(ln) for ln in lines])
    assert lengths.min() == 0 and (lengths == 9).sum() > 100 and (lengths == 256).sum() > 100 and (lengths == 257).sum() > 10
    assert 0 < host.info["slow"] <= 0.01 * len(lines) and host.info["lines"] == len(lines)
    assert data.count(b"\r\n") > 10000 and data.count(b"\n") > data.count(b"\r\n") + 10000 and not data.endswith(b"\n")
    assert min(host.info[k] for k in ("empty", "kept", "inter_chrom", "other_chrom", "too_close")) > 100
    assert mixed_dev.info["parse_calls"] == 1 and mixed_dev.info["n_bytes"] == len(data)
    assert_same(mixed_dev, host, "bytes")
    path = tmp_path / "sample_allValidPairs.txt"
    path.write_bytes(data)
    for src in (str(path), bytearray(data)):
        rp = ReadPairs.from_text(src, chroms=PC.CHROMS, device=DEV)
        assert rp.info["parse_calls"] == 1 and torch.equal(rp.keys, mixed_dev.keys), type(src)
        assert pairs.same_info(rp.info, host.info)
    fast = PC.join_lines([ln for ln in lines if PC.is_fast(ln)])
    rp = ReadPairs.from_text(fast, chroms=PC.CHROMS, device=DEV)
    assert rp.info["slow"] == 0 and rp.info["parse_calls"] == 1
    assert_same(rp, bin_read_pairs_host(fast, chroms=PC.CHROMS), "fast lines only")


def test_small_staging_chunks_give_the_same_keys_in_the_same_order(mixed, mixed_dev, tmp_path):
    lines, data, host = mixed
    path = tmp_path / "sample_allValidPairs.txt"
    path.write_bytes(data)
    for src, chunk in ((str(path), 40961), (data, 65537), (str(path), 4096 * 3)):    # lines cross tile and chunk edges
        rp = ReadPairs.from_text(src, chroms=PC.CHROMS, device=DEV, chunk_bytes=chunk)
        assert rp.info["parse_calls"] >= len(data) // chunk and torch.equal(rp.keys, mixed_dev.keys), chunk
        assert pairs.same_info(rp.info, host.info), chunk
    part = data[:data.index(b"\n", 150000) + 1]
    want = bin_read_pairs_host(part, chroms=PC.CHROMS)
    first = ReadPairs.from_text(part, chroms=PC.CHROMS, device=DEV)
    assert_same(first, want, "part")
    for chunk in (4099, 700, 64):          # down to chunks that hold a single line, and lines longer than a chunk
        rp = ReadPairs.from_text(part, chroms=PC.CHROMS, device=DEV, chunk_bytes=chunk)
        assert torch.equal(rp.keys, first.keys) and pairs.same_info(rp.info, want.info), chunk


def test_lines_that_end_around_a_tile_edge():
    """a line whose LF is the last byte of a 4096-byte tile, the first of the next one, or near either; and one that starts in
    the last bytes of a tile"""
    for pad in range(4090, 4101):
        body, size, k = [], 0, 0
        while size + 200 < pad:
            body.append(b"r%d\tchr1\t%d\t+\tchr1\t%d\t-\t99\n" % (k, k * 1000, k * 3000 + 5000))
            size += len(body[-1])
            k += 1
        tail = b"\tchr2\t1500\t+\tchr2\t99500\n"
        last = b"x" * (pad - size - len(tail)) + tail                                # ends exactly at byte `pad`
        data = b"".join(body) + last + b"after\tchr2\t123456\t-\tchr2\t7\t+\t1\r\nend\tchrX\t9\t+\tchrX\t99999"
        assert data[pad - 1:pad] == b"\n" and 100 < len(last) <= 256
        assert_same(ReadPairs.from_text(data, chroms=PC.CHROMS, device=DEV), bin_read_pairs_host(data, chroms=PC.CHROMS), pad)


@pytest.mark.parametrize("binning", ["nearest", "floor"])
def test_both_binnings_at_three_resolutions(mixed, binning):
    data = PC.join_lines(mixed[0][:40000], 5, 0.1)
    for res in (1000, 5000, 2500):
        want = bin_read_pairs_host(data, chroms=PC.CHROMS, resolution_bp=res, binning=binning)
        assert want.info["kept"] > 10000
        assert_same(ReadPairs.from_text(data, chroms=PC.CHROMS, resolution_bp=res, binning=binning, device=DEV), want, res)


def test_min_diff_and_name_tables(mixed):
    data = PC.join_lines(mixed[0][:40000])
    kept = []
    for md in (-1, 0, 10, 5000):          # -1 keeps the pairs that fall into one bin; 0 and 10 agree at 1 kb bins
        want = bin_read_pairs_host(data, chroms=PC.CHROMS, min_diff=md)
        assert_same(ReadPairs.from_text(data, chroms=PC.CHROMS, min_diff=md, device=DEV), want, md)
        kept.append(want.info["kept"])
    assert kept[0] > kept[1] == kept[2] > kept[3] > 0
    want = bin_read_pairs_host(data, chroms=PC.CHROMS, min_diff=10, resolution_bp=8)
    assert kept[0] > want.info["kept"] > kept[1]
    assert_same(ReadPairs.from_text(data, chroms=PC.CHROMS, min_diff=10, resolution_bp=8, device=DEV), want, "8 bp bins")
    one = bin_read_pairs_host(data, chroms=["chr2"])
    assert one.info["other_chrom"] > one.info["kept"] > 1000
    assert_same(ReadPairs.from_text(data, chroms=["chr2"], device=DEV), one, "one name")
    names = ["k%d" % k for k in range(63)] + ["chr_fifteen_byt"]
    data = PC.join_lines(PC.mixed_lines(30000, 5, chroms=tuple(names)))
    many = bin_read_pairs_host(data, chroms=names)
    assert min(many.info["kept_per_chrom"].values()) > 50
    assert_same(ReadPairs.from_text(data, chroms=names, device=DEV), many, "64 names")
    gaps = bin_read_pairs_host(data, chroms=names[::7])               # most chromosomes of the table without a pair
    assert_same(ReadPairs.from_text(data, chroms=names[::7] + ["absent"], device=DEV),
                bin_read_pairs_host(data, chroms=names[::7] + ["absent"]), "gaps")
    assert gaps.info["other_chrom"] > gaps.info["kept"]


def test_no_pair_one_pair_many_times_and_all_distinct():
    data = b"".join(b"r%d\tchr1\t%d\t+\tchr2\t%d\t-\n" % (k, k * 1000, k * 2000) for k in range(5000))
    rp = ReadPairs.from_text(data, device=DEV)
    assert rp.info["inter_chrom"] == 5000 and rp.info["kept"] == 0 and rp.keys.numel() == 0
    recs = rp.contacts_all()
    assert list(recs) == list(pairs.DEFAULT_CHROMS) and all(isinstance(c, hic.HicContacts) and c.M == 0 for c in recs.values())
    assert ReadPairs.from_text(b"", device=DEV).contacts("chr1").M == 0
    data = b"".join(b"r%d\tchr7\t%d\t+\tchr7\t%d\t-\n" % ((k, 5000499, 7000500) if k % 2 else (k, 7000001, 4999500))
                    for k in range(100000))
    c = ReadPairs.from_text(data, device=DEV).contacts("chr7")
    assert (c.pos1.tolist(), c.pos2.tolist(), c.count.tolist()) == ([5000000], [7000000], [100000.0])
    data = b"".join(b"r%d\tchrX\t%d\t+\tchrX\t%d\t-\n" % (k, (k % 300) * 1000 + 7, (300 + k // 300) * 1000 + 7) for k in range(60000))
    rp = ReadPairs.from_text(data, device=DEV)
    assert rp.contacts("chrX").M == 60000 and bool((rp.contacts("chrX").count == 1.0).all())
    assert_same(rp, bin_read_pairs_host(data), "all distinct")


def test_flag_list_that_overflows_is_fetched_by_a_second_call(mixed):
    lines = [ln for ln in mixed[0][:30000] if PC.is_fast(ln)]
    slow = [("s%d\tchr1\t %d\t+\tchr1\t%d_000" % (k, 1000 * k, 7 + k)).encode() for k in range(50)]
    for k, ln in enumerate(slow):
        lines.insert(500 * k + 3, ln)
    data = PC.join_lines(lines)
    want = bin_read_pairs_host(data, chroms=PC.CHROMS)
    assert want.info["slow"] == 50
    rp = ReadPairs.from_text(data, chroms=PC.CHROMS, device=DEV, flag_capacity=4)
    assert rp.info["parse_calls"] == 2
    assert_same(rp, want, "capacity 4")
    rp = ReadPairs.from_text(data, chroms=PC.CHROMS, device=DEV, flag_capacity=50)
    assert rp.info["parse_calls"] == 1
    assert_same(rp, want, "exact capacity")
    rp = ReadPairs.from_text(data, chroms=PC.CHROMS, device=DEV, flag_capacity=0, chunk_bytes=1 << 20)
    assert_same(rp, want, "capacity 0, several chunks")


def test_tiles_of_410_kept_lines_take_two_rounds():
    """every tile of dense_kept holds 409 or 410 line starts, all kept: the second round of k_pairs_starts<true> ranks its
    kept lines behind the 256 of the first, k_pairs_compact copies more than 256 keys of a tile"""
    data = PC.join_lines(PC.dense_kept())
    tile, rank = PC.tile_ranks(data)
    assert np.bincount(tile).max() == 410 and rank.max() == 409 > PC.ROUND
    want = bin_read_pairs_host(data, **PC.DENSE_RULE)
    assert want.info["kept"] == want.info["lines"] == 60000
    rp = ReadPairs.from_text(data, device=DEV, **PC.DENSE_RULE)
    assert rp.info["parse_calls"] == 1
    assert_same(rp, want, "dense kept")
    for chunk in (4096 * 5, 4099):                                   # chunks of 2048 and of 409 whole lines: each starts on a line start
        again = ReadPairs.from_text(data, device=DEV, chunk_bytes=chunk, **PC.DENSE_RULE)
        assert torch.equal(again.keys, rp.keys) and pairs.same_info(again.info, want.info), chunk


@pytest.mark.parametrize("data,starts", [(b"\n" * 20000, 4096), (b"\r\n" * 10000, 2048)], ids=["lf", "crlf"])
def test_a_text_of_line_ends_alone(data, starts):
    """4096 (2048) line starts in a tile, every line empty: 16 (8) rounds"""
    assert np.bincount(PC.tile_ranks(data)[0]).max() == starts
    want = bin_read_pairs_host(data, chroms=["c"])
    rp = ReadPairs.from_text(data, chroms=["c"], device=DEV)
    assert rp.info["lines"] == rp.info["empty"] == data.count(b"\n") and rp.keys.numel() == 0 and rp.info["slow"] == 0
    assert_same(rp, want, starts)


def test_dense_lines_of_every_class_with_slow_lines_in_late_rounds():
    lines = PC.dense_mixed()
    data = PC.join_lines(lines)
    tile, rank = PC.tile_ranks(data)
    want = bin_read_pairs_host(data, chroms=["c"])
    late = [k for k in want.info["slow_lines"].tolist() if rank[k] >= PC.ROUND]
    assert np.bincount(tile).min() > PC.ROUND and len(late) >= 10 and want.info["slow"] > 100
    rp = ReadPairs.from_text(data, chroms=["c"], device=DEV)
    assert rp.info["parse_calls"] == 1
    assert_same(rp, want, "default capacity")
    for kw in (dict(flag_capacity=4), dict(flag_capacity=0), dict(chunk_bytes=4099)):
        again = ReadPairs.from_text(data, chroms=["c"], device=DEV, **kw)
        assert again.keys.dtype == torch.int64 and torch.equal(again.keys, rp.keys), kw          # the same bits in the same order
        assert_same(again, want, kw)
    assert ReadPairs.from_text(data, chroms=["c"], device=DEV, flag_capacity=4).info["parse_calls"] == 2


def test_a_malformed_line_in_a_late_round_raises_the_hosts_message():
    good = PC.dense_kept(6000)
    for k in (300, 2048 + 350):
        data = PC.join_lines(good[:k] + [PC.BAD_SHORT] + good[k:] + [b"also\tbad"])
        tile, rank = PC.tile_ranks(data)
        assert rank[k] >= 300
        with pytest.raises(ValueError) as host:
            bin_read_pairs_host(data, **PC.DENSE_RULE)
        assert str(host.value).startswith("read pairs: line %d is not" % (k + 1))
        for cap in (1 << 16, 1):
            with pytest.raises(ValueError) as dev:
                ReadPairs.from_text(data, device=DEV, flag_capacity=cap, **PC.DENSE_RULE)
            assert str(dev.value) == str(host.value), (k, cap)


def test_two_runs_are_bitwise_equal(mixed, mixed_dev):
    again = ReadPairs.from_text(mixed[1], chroms=PC.CHROMS, device=DEV)
    assert torch.equal(again.keys, mixed_dev.keys) and pairs.same_info(again.info, mixed_dev.info)
    for c in PC.CHROMS:
        a, b = again.contacts(c), mixed_dev.contacts(c)
        assert torch.equal(a.pos1, b.pos1) and torch.equal(a.pos2, b.pos2)
        assert torch.equal(a.count.view(torch.int64), b.count.view(torch.int64))


def test_pairs_to_graph_end_to_end():
    """synthetic pairs at chr21 scale -> records -> VC vector -> top-K graph, against the host chain on the host's records"""
    res = 1000
    data = synth.read_pairs({"chr21": synth.HG19_LEN["chr21"], "chr22": 12000000}, 500000, 21)
    rp = ReadPairs.from_text(data, device=DEV)
    hp = bin_read_pairs_host(data)
    assert 200000 < hp.info["kept_per_chrom"]["chr21"] < 300000 and hp.info["inter_chrom"] > 10000
    p1, p2, cnt = hp.contacts("chr21")
    assert cnt.max() >= 2 and p1.size > 150000
    rng = np.random.default_rng(5)
    n_bins = -(-synth.HG19_LEN["chr21"] // res)
    ws = (np.sort(rng.choice(n_bins, n_bins // 4, replace=False)) * res).astype(np.int32)
    want = build_hic_graph_host(p1, p2, cnt, "VC", res, ws, 8000)
    c = rp.contacts("chr21")
    nv = c.norm_vector("VC", res)
    rowptr, col, sizes = c.build_raw("VC", res, ws, 8000)
    nnz = int(sizes[0].item())
    print("records %d, survivors %d, nnz %d, host nnz %d" % (c.M, int(sizes[1].item()), nnz, want.nnz))
    assert int(sizes[1].item()) > 4000 and nnz == want.nnz > 0 and nv.numel() > 0
    assert np.array_equal(rowptr.cpu().numpy(), want.indptr) and np.array_equal(col[:nnz].cpu().numpy(), want.indices)


def test_malformed_lines_raise_the_hosts_message(mixed, tmp_path):
    good = [ln for ln in mixed[0][:5000]]
    cases = [(k, ln.format(c="chr2").encode()) for k, (_, ln) in zip((7, 0, 4999, 300, 1234, 4000, 2500, 2501, 17, 99, 1, 2, 3, 4,
                                                                     5, 6, 8), PC.MALFORMED)]
    cases.append((77, PC.MALFORMED_NEAREST_1000[1].format(c="chr2").encode()))
    assert len(cases) == len(PC.MALFORMED) + 1
    for k, bad in cases:
        body = good[:k] + [bad] + good[k:]
        data = PC.join_lines(body + [b"also\tbad"])
        with pytest.raises(ValueError) as host:
            bin_read_pairs_host(data, chroms=PC.CHROMS)
        assert str(host.value).startswith("read pairs: line %d is not" % (k + 1))
        with pytest.raises(ValueError) as dev:
            ReadPairs.from_text(data, chroms=PC.CHROMS, device=DEV, flag_capacity=3)
        assert str(dev.value) == str(host.value), (k, bad)
    path = tmp_path / "bad_allValidPairs.txt"
    path.write_bytes(b"a\tchr1\t5\t+\tchr1\t9000\nb\tchr1\t5\n")
    with pytest.raises(ValueError, match="read pairs: line 2 is not"):
        ReadPairs.from_text(str(path), device=DEV)
    with pytest.raises(ValueError, match="resolution_bp"):
        ReadPairs.from_text(b"", resolution_bp=4, device=DEV)


def test_hic_ingest_turns_a_pairs_file_into_the_caches_train_loads(tmp_path):
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
    try:
        import hic_ingest
    finally:
        sys.path.pop(0)
    sizes = {"chr21": 3000000, "chr22": 2000000}
    data = synth.read_pairs(sizes, 60000, 4)
    (tmp_path / "pairs.txt").write_bytes(data)
    bed = ["%s\t%d\t%d\tpeak\n" % (c, s, s + 5000) for c, n in sizes.items() for s in range(0, n, 10000)]
    (tmp_path / "windows.bed").write_text("".join(bed))
    out = tmp_path / "caches"
    lines = hic_ingest.main(["--pairs", str(tmp_path / "pairs.txt"), "--pairs-binning", "floor", "--resolution-kb", "5",
                             "--bed", str(tmp_path / "windows.bed"), "--chroms", "chr21,chr22", "--out", str(out),
                             "--compute-norms", "VC"])
    assert [ln["chrom"] for ln in lines] == ["chr21", "chr22"] and all(ln["norms"] == ["cVC"] for ln in lines)
    hp = bin_read_pairs_host(data, chroms=["chr21", "chr22"], resolution_bp=5000, binning="floor")
    for chrom in sizes:
        h = hic.load_contacts_cache(hic.contact_cache_path(str(out), chrom))
        want = hp.contacts(chrom)
        assert h.resolution_bp == 5000 and np.array_equal(h.pos1, want[0]) and np.array_equal(h.pos2, want[1])
        assert np.array_equal(h.count, want[2]) and h.window_start.size == sizes[chrom] // 10000
    graphs = hic.graphs_from_contact_caches(str(out), list(sizes), 2000, "cVC", device=DEV)
    assert all(graphs[c].n == sizes[c] // 10000 and graphs[c].nnz > 0 for c in sizes)
