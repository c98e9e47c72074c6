"""The host restatement of the read-pair rule (chromegcn_amd/pairs.py: bin_read_pairs_host, pairs_to_contacts_host) against the
reference's own output (tests/golden/g13_pairs.npz: data/eqtl_data/HiChIP.py run as it is), against Python's int() and round(),
and against a Counter.  No GPU."""
import collections
import os

import numpy as np
import pytest

from chromegcn_amd import bin_read_pairs_host, hic, pairs, pairs_to_contacts_host, synth
from chromegcn_amd.pairs import bin_position

import pairs_cases as PC

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(HERE, "golden", "g13_pairs.npz"))
    return g, g["input"].tobytes(), [str(c) for c in g["chroms"]], [str(c) for c in g["files"]]


def reference_file(p1, p2) -> bytes:
    """the reference's `<chrom>.allValidPairs`: p1 TAB p2 TAB |p2 - p1| CR LF (csv.writer's line end)"""
    return b"".join(b"%d\t%d\t%d\r\n" % (a, b, abs(b - a)) for a, b in zip(p1.tolist(), p2.tolist()))


def test_restatement_reproduces_every_reference_file_byte_for_byte(golden):
    g, data, chroms, files = golden
    assert len(data) < 200000 and 2000 < data.count(b"\n") < 5000 and not data.endswith(b"\n")
    cols = collections.Counter(ln.count(b"\t") + 1 for ln in data.split(b"\n"))
    assert set(cols) == {8, 9, 12, 13} and min(cols.values()) > 100
    for vectorised in (True, False):
        hp = bin_read_pairs_host(data, chroms=files, vectorised=vectorised)     # a file for every name, as the reference
        for c in files:
            assert reference_file(*hp.binned(c)) == g["out_" + c].tobytes(), c
        assert hp.info["other_chrom"] == 0 and hp.info["inter_chrom"] > 200 and hp.info["too_close"] > 200
        assert hp.info["slow"] == 3 and hp.info["lines"] == data.count(b"\n") + 1
    hp = bin_read_pairs_host(data, chroms=chroms)
    for c in chroms:
        assert reference_file(*hp.binned(c)) == g["out_" + c].tobytes(), c
        p1, p2 = hp.binned(c)
        assert (p1 > p2).sum() > 50 and (p1 < p2).sum() > 50 and min(p1.min(), p2.min()) == 0
    assert hp.info["other_chrom"] > 100 and sum(hp.info["kept_per_chrom"].values()) == hp.info["kept"]


def test_nearest_is_pythons_round_and_floor_is_the_remainder():
    assert [bin_position(x, 1000) for x in (500, 1499, 1500, 2500, 2501)] == [0, 1000, 2000, 2000, 3000]
    rng = np.random.default_rng(1)
    xs = np.concatenate([np.arange(10000), rng.integers(0, 2 ** 31 - 500, 20000)])
    assert bin_position(xs, 1000).tolist() == [round(int(x), -3) for x in xs]
    assert all(bin_position(int(x), 1000) == round(int(x), -3) for x in xs[::37])
    for res in (1000, 5000, 2500, 8, 7777):
        assert np.array_equal(bin_position(xs, res, "floor"), xs - xs % res)
        want = []
        for x in xs.tolist():
            q, r = divmod(x, res)
            want.append((q if 2 * r < res else q + 1 if 2 * r > res else q + q % 2) * res)
        assert bin_position(xs, res).tolist() == want, res
    assert [bin_position(x, 2500) for x in (1249, 1250, 1251, 3749, 3750, 3751)] == [0, 0, 2500, 2500, 5000, 5000]


def test_mixed_file_is_parsed_as_python_parses_it():
    lines = PC.mixed_lines(30000, 3) + PC.tie_lines()
    for kw in ({}, {"res": 5000, "binning": "floor"}, {"res": 2500, "min_diff": 0}, {"min_diff": 5000}):
        use = [ln for ln in lines if not ln.startswith((b"t2147", b"u2147"))] if kw.get("res", 1000) != 1000 else lines
        want, tot, slow = PC.python_rule(use, PC.CHROMS, **kw)
        for data in (PC.join_lines(use), PC.join_lines(use, 2, 0.4, final_terminator=False)):
            for vectorised, block in ((True, 64 << 20), (True, 50000), (False, 64 << 20)):
                hp = bin_read_pairs_host(data, chroms=PC.CHROMS, resolution_bp=kw.get("res", 1000),
                                         binning=kw.get("binning", "nearest"), min_diff=kw.get("min_diff", 10),
                                         vectorised=vectorised, block_bytes=block)
                for c in PC.CHROMS:
                    a, b = PC.arrays(want[c])
                    assert np.array_equal(hp.binned(c)[0], a) and np.array_equal(hp.binned(c)[1], b), (kw, c)
                assert all(hp.info[k] == v for k, v in tot.items()) and hp.info["slow_lines"].tolist() == slow
    assert 0 < len(slow) <= 0.01 * len(lines)


def test_every_slow_spelling_is_parsed_as_python_parses_it():
    lines = [("r\tchr1\t%s\t+\tchr1\t%d" % (s, 5000000 + k)).encode() for k, s in enumerate(PC.SLOW_POS)]
    lines += [("r\tchr1\t%d\t+\tchr1\t%s" % (7000000 + k, s)).encode() for k, s in enumerate(PC.SLOW_POS)]
    lines += [b"r\tchr_sixteen_bytes\t5\t+\tchr_sixteen_bytes\t9000", b"r\t\t5\t+\t\t9000", b"r\tchr1\tx\t+\tchr2\t",
              b"n" * 300 + b"\tchr2\t1500\t+\tchr2\t99500", b"n" * 234 + b"\tchr2\t1500\t+\tchr2\t99500"]
    assert len(lines[-1]) == 257 and not any(PC.is_fast(ln) for ln in lines)
    want, tot, slow = PC.python_rule(lines, PC.CHROMS)
    hp = bin_read_pairs_host(PC.join_lines(lines), chroms=PC.CHROMS)
    assert slow == list(range(len(lines))) == hp.info["slow_lines"].tolist() and all(hp.info[k] == v for k, v in tot.items())
    assert hp.info["kept"] == 2 * len(PC.SLOW_POS) + 2 and hp.info["other_chrom"] == 2 and hp.info["inter_chrom"] == 1
    a, b = PC.arrays(want["chr1"])
    assert np.array_equal(hp.binned("chr1")[0], a) and np.array_equal(hp.binned("chr1")[1], b)
    assert a[:len(PC.SLOW_POS)].tolist() == [round(int(s), -3) for s in PC.SLOW_POS]
    fast = [("r\tchr1\t%s\t+\tchr1\t%d" % (s, 5000000 + k)).encode() for k, s in enumerate(PC.FAST_POS)]
    hp = bin_read_pairs_host(PC.join_lines(fast), chroms=PC.CHROMS)
    assert hp.info["slow"] == 0 and hp.binned("chr1")[0].tolist() == [round(int(s), -3) for s in PC.FAST_POS]


def test_every_malformed_kind_raises_with_the_first_lines_number():
    good = PC.mixed_lines(300, 9)
    for k, (what, ln) in enumerate(PC.MALFORMED + [PC.MALFORMED_NEAREST_1000]):
        body = good[:7 * k] + [ln.format(c="chr1").encode()] + good[7 * k:] + [b"later\tand\tbad"]
        for vectorised in (True, False):
            with pytest.raises(ValueError, match=r"^read pairs: line %d is not " % (7 * k + 1)):
                bin_read_pairs_host(PC.join_lines(body, k, 0.5), chroms=PC.CHROMS, vectorised=vectorised)
    ok = PC.MALFORMED_NEAREST_1000[1].format(c="chr1").encode()               # fine under the floor
    assert bin_read_pairs_host(ok, chroms=PC.CHROMS, binning="floor").binned("chr1")[0].tolist() == [2147483000]
    for kw in ({"chroms": []}, {"chroms": ["a"] * 2}, {"chroms": ["x" * 16]}, {"chroms": ["chr1"] * 65}, {"resolution_bp": 7},
               {"binning": "round"}, {"chroms": ["a\tb"]}):
        with pytest.raises(ValueError):
            bin_read_pairs_host(b"", **kw)
    empty = bin_read_pairs_host(b"")
    assert empty.info["lines"] == 0 and empty.chroms == pairs.DEFAULT_CHROMS and len(pairs.DEFAULT_CHROMS) == 23


def test_dense_files_hold_more_line_starts_per_tile_than_one_round():
    """what tests/test_gpu_pairs.py relies on, from the bytes alone: tiles of 410 kept lines, of 4096 and 2048 empty ones,
    slow lines and a malformed one behind the 256th line start of their tile; and the host's parse of each file"""
    lines = PC.dense_kept()
    data = PC.join_lines(lines)
    tile, rank = PC.tile_ranks(data)
    per_tile = np.bincount(tile)
    assert len(data) == 600000 and all(len(ln) == 9 and PC.is_fast(ln) for ln in lines)
    assert per_tile.max() == 410 <= PC.TILE_KEYS and (per_tile == 410).sum() >= 29 and (data[4096 * 5 - 1:4096 * 5] == b"\n")
    want, tot, slow = PC.python_rule(lines, res=8, binning="nearest", min_diff=-1, chroms=["c"])
    hp = bin_read_pairs_host(data, **PC.DENSE_RULE)
    assert tot["kept"] == len(lines) == hp.info["kept"] and slow == [] and hp.info["slow"] == 0     # every line start is a kept line:
    assert per_tile.max() >= 257 and rank.max() == 409                                           # 410 kept lines in one tile
    a, b = PC.arrays(want["c"])
    assert np.array_equal(hp.binned("c")[0], a) and np.array_equal(hp.binned("c")[1], b) and set(a.tolist()) == {0, 8}
    for data, starts in ((b"\n" * 20000, 4096), (b"\r\n" * 10000, 2048)):
        tile, rank = PC.tile_ranks(data)
        hp = bin_read_pairs_host(data, chroms=["c"])
        assert np.bincount(tile).max() == starts and hp.info["lines"] == hp.info["empty"] == data.count(b"\n")
        assert hp.info["kept"] == hp.info["slow"] == 0 and hp.pos1.size == 0
    lines = PC.dense_mixed()
    data = PC.join_lines(lines)
    tile, rank = PC.tile_ranks(data)
    want, tot, slow = PC.python_rule(lines, chroms=["c"])
    hp = bin_read_pairs_host(data, chroms=["c"])
    assert all(hp.info[k] == v for k, v in tot.items()) and hp.info["slow_lines"].tolist() == slow
    assert min(tot[k] for k in ("empty", "kept", "inter_chrom", "other_chrom", "too_close")) > 3000
    a, b = PC.arrays(want["c"])
    assert np.array_equal(hp.binned("c")[0], a) and np.array_equal(hp.binned("c")[1], b)
    late = [k for k in slow if rank[k] >= PC.ROUND]
    kept_slow = [k for k in late if int(lines[k].split(b"\t")[5]) > 1000]
    assert np.bincount(tile).min() > PC.ROUND and len(late) >= 10 and len(kept_slow) >= 5 and len(late) - len(kept_slow) >= 5
    good = PC.dense_kept(6000)
    for k in (300, 2048 + 350):                                   # tile 0, and tile 5, which starts on line 2048
        body = good[:k] + [PC.BAD_SHORT] + good[k:]
        data = PC.join_lines(body)
        tile, rank = PC.tile_ranks(data)
        assert rank[k] >= 300 and tile[k] == (0 if k == 300 else 5) and body[k] == PC.BAD_SHORT
        with pytest.raises(ValueError, match=r"^read pairs: line %d is not " % (k + 1)):
            bin_read_pairs_host(data, **PC.DENSE_RULE)


def test_stage_b_is_a_counter_over_canonical_bin_pairs(golden, tmp_path):
    _, data, chroms, _ = golden
    hp = bin_read_pairs_host(data, chroms=chroms)
    for c in chroms:
        a, b = hp.binned(c)
        cnt = collections.Counter((min(x, y), max(x, y)) for x, y in zip(a.tolist(), b.tolist()))
        p1, p2, n = pairs_to_contacts_host(a, b, 1000)
        assert p1.dtype == np.int32 and p2.dtype == np.int32 and n.dtype == np.float64
        assert list(zip(p1.tolist(), p2.tolist())) == sorted(cnt) and n.tolist() == [float(cnt[k]) for k in sorted(cnt)]
        assert n.max() >= 20 and n.sum() == a.size
        # through the cache and back
        path = hic.contact_cache_path(str(tmp_path), c)
        hic.save_contacts_cache(path, hic.HostContacts(p1, p2, n, {}, 1000, None))
        back = hic.load_contacts_cache(path)
        assert np.array_equal(back.pos1, p1) and np.array_equal(back.pos2, p2) and back.resolution_bp == 1000
        assert np.array_equal(back.count.view(np.int64), n.view(np.int64))
    e = pairs_to_contacts_host(np.zeros(0, np.int32), np.zeros(0, np.int32), 1000)
    assert all(x.size == 0 for x in e)
    with pytest.raises(ValueError):
        pairs_to_contacts_host(np.array([1500]), np.array([3000]), 1000)


def test_synthetic_pairs_have_the_shape_of_a_hicpro_file():
    sizes = {"chr21": synth.HG19_LEN["chr21"], "chr22": synth.HG19_LEN["chr22"]}
    data = synth.read_pairs(sizes, 20000, 3)
    assert data == synth.read_pairs(sizes, 20000, 3) and data != synth.read_pairs(sizes, 20000, 4)
    lines = data.split(b"\n")
    assert lines[-1] == b"" and len(lines) == 20001 and all(ln.count(b"\t") == 11 for ln in lines[:-1])
    assert len({len(ln.split(b"\t")[0]) for ln in lines[:-1]}) > 5 and max(map(len, lines)) < 160
    hp = bin_read_pairs_host(data)
    assert hp.info["slow"] == 0 and 1000 < hp.info["inter_chrom"] < 6000 and hp.info["too_close"] > 1000
    p1, p2, n = hp.contacts("chr21")
    assert n.max() >= 2 and (hp.binned("chr21")[0] > hp.binned("chr21")[1]).sum() > 1000
    sep = np.abs(hp.binned("chr21")[1].astype(np.int64) - hp.binned("chr21")[0])
    assert np.median(sep) < 0.02 * sizes["chr21"]                              # separations decay with distance


def test_entry_points_reject_bad_arguments_before_any_launch():
    """the checks of cgcn_pairs_parse / cgcn_pairs_reduce that need no device: made on the host, nothing is launched"""
    from chromegcn_amd import _build, _lib
    _build.build_library()
    _lib.load()
    p = 0x100000                                                     # a pointer that is only compared, never followed
    ok = dict(stream=None, text=p, n_bytes=4096, byte_base=0, names=p, n_chroms=3, resolution_bp=1000, binning=0, min_diff=10,
              keys=p, key_capacity=500, flags=p, flag_capacity=8, totals=p, chunk_totals=p, workspace=p,
              workspace_bytes=_lib.query("cgcn_pairs_parse_workspace_bytes", n_bytes=4096))
    assert ok["workspace_bytes"] > 416 * 8 and _lib.query("cgcn_pairs_parse_workspace_bytes", n_bytes=-1) == 0
    for change, code in (({"n_chroms": 65}, -2), ({"n_chroms": 0}, -2), ({"resolution_bp": 7}, -2), ({"binning": 2}, -1),
                         ({"text": p + 8}, -1), ({"names": p + 4}, -1), ({"totals": None}, -1), ({"keys": None}, -1),
                         ({"n_bytes": -1}, -1), ({"workspace_bytes": ok["workspace_bytes"] - 1}, -4), ({"flags": None}, -1)):
        assert _lib.query("cgcn_pairs_parse", **{**ok, **change}) == code, change
    red = dict(stream=None, n_keys=1000, keys=p, n_chroms=3, resolution_bp=1000, pos1_out=p, pos2_out=p, count_out=p,
               chrom_offsets=p, n_records=p, workspace=p, workspace_bytes=_lib.query("cgcn_pairs_reduce_workspace_bytes", n_keys=1000))
    assert red["workspace_bytes"] > 12000 and _lib.query("cgcn_pairs_reduce_workspace_bytes", n_keys=2 ** 31) == 0
    for change, code in (({"n_chroms": 65}, -2), ({"resolution_bp": 4}, -2), ({"n_keys": 2 ** 31}, -2), ({"n_keys": -1}, -1),
                         ({"keys": None}, -1), ({"chrom_offsets": None}, -1), ({"workspace_bytes": 64}, -4)):
        assert _lib.query("cgcn_pairs_reduce", **{**red, **change}) == code, change
    with pytest.raises(RuntimeError, match="needs a GPU"):
        pairs.ReadPairs.from_text(b"", device="cpu")
