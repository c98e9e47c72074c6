"""Hi-C contact text, CPU tier: parse_contacts_text_host (the restatement of the rule in include/chromegcn.h and the
docstring of chromegcn_amd/hic.py) against Python's own int() / float() field by field, its fast / slow / malformed
classification against the rule written out once more with `re` (tests/hic_text_cases.py), the text fixture of the reference's step 7
(tests/golden/g10_hic_text.npz, recorded by tests/golden/make_golden_hic_text.py) through to the matrix, and the argument
checks of the new C entry points.  The lines and generators are in tests/hic_text_cases.py."""
import io

import numpy as np
import pytest

from chromegcn_amd import _build, _lib, hic

from hic_text_cases import (FAST_F3, FAST_POS, LINE_MAX, MALFORMED, SLOW_F3, SLOW_POS, assert_parses_like_python, juicer_text,
                            mixed_lines, rule_is_fast)

BAD_ARG, UNSUPPORTED, WORKSPACE = -1, -2, -4


# ----------------------------------------------------------------------------------------------
def test_every_fast_and_slow_shape_parses_like_python_and_is_classified_by_the_rule():
    lines = [("%s\t%s\t%s" % (a, b, f3)).encode() for f3 in FAST_F3 + SLOW_F3 for a, b in (("1000", "25000"), ("0", "2147483647"))]
    lines += [("%s\t5000\t2.0" % a).encode() for a in SLOW_POS + FAST_POS] + [("5000\t%s\t2.0" % a).encode() for a in SLOW_POS]
    lines += [b"1000\t2000\t" + b"0" * (LINE_MAX - 11) + b"7", b"1000\t2000\t" + b"0" * (LINE_MAX - 10) + b"7"]   # at and beyond the bound
    slow = assert_parses_like_python(lines, b"\n".join(lines) + b"\n")
    for f3 in FAST_F3:
        assert rule_is_fast(b"1\t2\t" + f3.encode()), f3
    for f3 in SLOW_F3:
        assert not rule_is_fast(b"1\t2\t" + f3.encode()), f3
    assert len(lines[-2]) == LINE_MAX and slow.size == 2 * len(SLOW_F3) + 2 * len(SLOW_POS) + 1


def test_generated_lines_of_every_length_parse_like_python():
    lines = mixed_lines(60000, 3, slow_share=0.05)
    slow = assert_parses_like_python(lines, b"\n".join(lines) + b"\n")
    lengths = {len(ln) for ln in lines}
    assert min(lengths) == 5 and {LINE_MAX - 1, LINE_MAX, LINE_MAX + 1} <= lengths and 0.02 < slow.size / len(lines) < 0.08
    # the same records whatever the terminators are
    want = hic.parse_contacts_text_host(b"\n".join(lines))
    for data in (b"\r\n".join(lines) + b"\r\n", b"\r\n".join(lines), b"\n".join(lines) + b"\n"):
        got = hic.parse_contacts_text_host(data)
        assert all(np.array_equal(g.view(np.int64) if g.dtype == np.float64 else g, w.view(np.int64) if w.dtype == np.float64 else w)
                   for g, w in zip(got, want))


def test_no_juicer_line_is_slow():
    rng = np.random.RandomState(5)
    p1, p2 = rng.randint(0, 249251, 100000) * 1000, rng.randint(0, 249251, 100000) * 1000
    cnt = np.concatenate([1.0 + rng.poisson(30.0, 50000), rng.random_sample(50000) * 10 ** rng.randint(0, 8, 50000)])
    data = juicer_text(p1, p2, cnt)
    lines = data.split(b"\n")[:-1]
    assert assert_parses_like_python(lines, data).size == 0


def test_terminators_empty_file_and_single_line():
    for data in (b"", bytearray(), memoryview(b""), np.zeros(0, np.uint8)):
        p1, p2, c, slow = hic.parse_contacts_text_host(data)
        assert p1.size == p2.size == c.size == slow.size == 0 and p1.dtype == np.int32 and c.dtype == np.float64
    for data in (b"1000\t2000\t3.5", b"1000\t2000\t3.5\n", b"1000\t2000\t3.5\r\n"):
        p1, p2, c, slow = hic.parse_contacts_text_host(data)
        assert (p1.tolist(), p2.tolist(), c.tolist(), slow.tolist()) == ([1000], [2000], [3.5], [])
    p1, p2, c, slow = hic.parse_contacts_text_host(b"1\t2\t3\r\n4\t5\t6\n7\t8\t9\r")   # a CR without its LF is part of F3: float() strips it
    assert (p1.tolist(), c.tolist(), slow.tolist()) == ([1, 4, 7], [3.0, 6.0, 9.0], [2])
    with pytest.raises(ValueError, match="line 2 is not"):
        hic.parse_contacts_text_host(b"1\t2\t3\n\n")                                  # only ONE empty piece behind the final LF is no line
    with pytest.raises(ValueError, match="line 1 is not"):
        hic.parse_contacts_text_host(b"\n")


def test_each_malformed_line_raises_with_its_line_number():
    good = [b"1000\t2000\t3.5", b"5\t6\tnan", b"7\t8\t1e3"]
    for bad in MALFORMED:
        for k in range(len(good) + 1):
            if bad == b"" and k == len(good):
                continue   # an empty last piece is no line
            lines = good[:k] + [bad] + good[k:]
            with pytest.raises(ValueError) as e:
                hic.parse_contacts_text_host(b"\n".join(lines) + b"\n")
            assert str(e.value) == "contact text: line %d is not `pos1<TAB>pos2<TAB>count`" % (k + 1), (bad, k)
    with pytest.raises(ValueError, match="line 2 is not"):                            # the FIRST of several
        hic.parse_contacts_text_host(b"1\t2\t3\n#x\n4\t5\t6\n\n#y\n")


def test_text_fixture_of_the_reference_gives_its_matrices(golden, tmp_path):
    z = golden("g10_hic_text.npz")
    bed = tmp_path / "windows.bed"
    bed.write_bytes(z["bed"].tobytes())
    ws = hic.windows_from_bed(str(bed), ["chrT", "chrU", "chrV"])
    assert ws["chrT"].dtype == np.int32 and ws["chrT"].size == int(z["n_windows"]) and ws["chrV"].size == 0
    assert all(np.all(w[1:] > w[:-1]) for w in ws.values()) and 0 < ws["chrU"].size < ws["chrT"].size
    raw = z["raw"].tobytes()
    p1, p2, c, slow = hic.parse_contacts_text_host(raw)
    assert p1.size == raw.count(b"\n") > 300 and 0 < slow.size < p1.size / 4      # the 17-digit counts
    norm = np.loadtxt(io.BytesIO(z["norm"].tobytes()), dtype=np.float64, ndmin=1)
    assert np.isnan(norm).any() and (norm == 0).any()
    ties = 0
    for k in range(int(z["n_cases"])):
        a = hic.build_hic_graph_host(p1, p2, c, norm, int(z["res"]), ws["chrT"], int(z["c%d_edges" % k]))
        assert np.array_equal(a.indptr, z["c%d_indptr" % k]) and np.array_equal(a.indices, z["c%d_indices" % k]), k
        ties += int(z["c%d_tie" % k])
    assert ties >= 2
    # the parent's parser reads the same records from the same file
    path = tmp_path / "chrT_1kb.RAWobserved"
    path.write_bytes(raw)
    old = hic.load_contacts_text(str(path))
    assert np.array_equal(old.pos1, p1) and np.array_equal(old.pos2, p2) and np.array_equal(old.count.view(np.int64), c.view(np.int64))


def test_c_entry_points_reject_null_and_negative_arguments_without_a_gpu():
    _build.build_library()
    _lib.load()
    assert _lib.query("cgcn_text_workspace_bytes", n_bytes=-1) == 0
    assert 0 < _lib.query("cgcn_text_workspace_bytes", n_bytes=0) < _lib.query("cgcn_text_workspace_bytes", n_bytes=3 * 10 ** 9)
    fake = 0x100000   # never dereferenced: every check comes before the first launch
    count = dict(stream=None, text=fake, n_bytes=4096, workspace=fake, workspace_bytes=1 << 20, n_records=fake)
    for over in (dict(text=None), dict(workspace=None), dict(n_records=None), dict(n_bytes=-1), dict(text=fake + 8)):
        assert _lib.query("cgcn_text_count", **dict(count, **over)) == BAD_ARG, over
    assert _lib.query("cgcn_text_count", **dict(count, workspace_bytes=16)) == WORKSPACE
    parse = dict(stream=None, text=fake, n_bytes=4096, M=10, pos1_out=fake, pos2_out=fake, count_out=fake, flags=fake,
                 flag_capacity=4, flag_totals=fake, workspace=fake, workspace_bytes=1 << 20)
    for over in (dict(text=None), dict(workspace=None), dict(pos1_out=None), dict(pos2_out=None), dict(count_out=None),
                 dict(flags=None), dict(flag_totals=None), dict(n_bytes=-1), dict(M=-1), dict(flag_capacity=-1),
                 dict(text=fake + 4)):
        assert _lib.query("cgcn_text_parse", **dict(parse, **over)) == BAD_ARG, over
    assert _lib.query("cgcn_text_parse", **dict(parse, M=2 ** 31)) == UNSUPPORTED
    assert _lib.query("cgcn_text_parse", **dict(parse, workspace_bytes=16)) == WORKSPACE
    with pytest.raises(RuntimeError, match=r"chromegcn_amd: cgcn_text_parse failed: bad argument.*\(code -1\)"):
        _lib.call("cgcn_text_parse", **dict(parse, count_out=None))

