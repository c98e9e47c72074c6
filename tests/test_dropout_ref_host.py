"""tests/dropout_ref.py -- the numpy statement of the kernels' dropout mask -- pinned against accidental edits, and the
statistics of the mask it states.  No GPU: tests/test_gpu_dropout_masks.py holds the kernels to the same functions bit for bit.

The pinned integers were computed once with the restatement and checked against chromegcn_amd/csrc/cgcn_common.hpp by
compiling its mix32 / dropout_key / dropout_threshold text as plain host C++: the same 32 keys, thresholds and scales."""
import functools
import itertools

import numpy as np
import pytest

import dropout_ref as R

HEAD = R.HEAD_STREAM_ID
SEED_LO, SEED_HI = 77, 2 ** 40 + 5
COUNTERS = (0, 1, 2 ** 32, 2 ** 32 + 1)
STREAMS = (0, 1, 2, HEAD)

# dropout_key(seed, counter, stream id), streams in the order of STREAMS
KEYS = {
    (SEED_LO, 0): (4250489033, 3697181324, 704073609, 4275771028),
    (SEED_LO, 1): (800494057, 2661254902, 2770371476, 464102842),
    (SEED_LO, 2 ** 32): (1702355246, 909798601, 3814325733, 3630048709),
    (SEED_LO, 2 ** 32 + 1): (507013470, 329250031, 332620346, 20669197),
    (SEED_HI, 0): (627689560, 24386946, 219193142, 2027178528),
    (SEED_HI, 1): (3846491988, 3449010802, 360223598, 499626186),
    (SEED_HI, 2 ** 32): (4129135400, 4158053777, 1738725902, 3947560340),
    (SEED_HI, 2 ** 32 + 1): (1449568111, 3389131831, 1164881793, 2727472029),
}


def test_head_stream_id_is_the_librarys():
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "chromegcn_amd", "csrc", "cgcn_common.hpp")).read()
    m = re.search(r"#define\s+HEAD_STREAM_ID\s+(0x[0-9A-Fa-f]+)u", src)
    assert m and int(m.group(1), 16) == HEAD == 0x4845


def test_mix32_pinned():
    assert [int(R.mix32(x)) for x in (0, 1, 0xFFFFFFFF)] == [0, 1753845952, 1734902346]
    got = R.mix32(np.array([0, 1, 0xFFFFFFFF], dtype=np.uint32))   # arrays of any integer type, same values
    assert got.dtype == np.uint64 and got.tolist() == [0, 1753845952, 1734902346]
    assert int(R.mix32(2 ** 32 + 1)) == 1753845952                  # only the low 32 bits count


def test_dropout_key_pinned_for_both_seed_halves_both_counter_halves_and_every_stream():
    for (seed, ctr), want in KEYS.items():
        assert tuple(R.dropout_key(seed, ctr, s) for s in STREAMS) == want, (seed, ctr)


def test_first_mask_bits_pinned():
    got = "".join(str(int(b)) for b in R.mask(77, 3, 1, (16,), 0.2))
    assert got == "1110111011011111"


def test_keys_of_neighbouring_steps_seeds_and_streams_differ():
    seed, ctr = SEED_LO, 3
    for s in STREAMS:
        keys = [R.dropout_key(seed, ctr, s), R.dropout_key(seed, ctr + 1, s), R.dropout_key(seed, ctr + 2 ** 32, s),
                R.dropout_key(seed + 2 ** 32, ctr, s)]
        assert len(set(keys)) == 4, (s, keys)
    for sd, c in itertools.product((SEED_LO, SEED_HI), COUNTERS):
        assert len({R.dropout_key(sd, c, s) for s in STREAMS}) == 4, (sd, c)
    assert len({k for v in KEYS.values() for k in v}) == 32


def test_thresholds_take_p_as_a_c_float():
    assert R.dropout_threshold(0.0) == 0 and R.dropout_threshold(-0.5) == 0       # 0 = no dropout
    assert R.dropout_threshold(0.2) == 858993472 != int(0.2 * 2 ** 32) == 858993459
    assert R.dropout_threshold(np.float32(0.2)) == 858993472
    assert R.dropout_threshold(0.5) == 2 ** 31
    assert R.dropout_threshold(0.1) == 429496736 and R.dropout_threshold(0.9) == 3865470464 and R.dropout_threshold(0.3) == 1288490240
    assert R.dropout_threshold(np.nextafter(np.float32(1), np.float32(0))) == 2 ** 32 - 256   # the largest float32 below 1
    assert R.dropout_threshold(1.0) == 2 ** 32 - 1 and R.dropout_threshold(7.0) == 2 ** 32 - 1   # product >= 2^32 - 1: clamped


def test_keep_scale_is_the_float32_quotient():
    s = R.keep_scale(0.2)
    assert s.dtype == np.float32 and s == np.float32(1) / (np.float32(1) - np.float32(0.2))
    assert s == np.float32(1.25) and float(s) != 1.0 / (1.0 - float(np.float32(0.2)))   # rounded once more than the double
    assert R.keep_scale(0.5) == np.float32(2) and R.keep_scale(0.0) == np.float32(1)
    assert R.keep_scale(0.9).tobytes() == np.float32(9.99999809).tobytes()


def test_mask_indexes_elements_in_c_order():
    S, n, d = 2, 5, 8
    m = R.mask(SEED_HI, 2 ** 32 + 7, 2, (S, n, d), 0.5)
    assert m.shape == (S, n, d) and m.dtype == np.bool_
    key, thr = R.dropout_key(SEED_HI, 2 ** 32 + 7, 2), R.dropout_threshold(0.5)
    for s, i, c in ((0, 0, 0), (0, 4, 7), (1, 0, 0), (1, 3, 5)):
        e = (s * n + i) * d + c
        assert bool(m[s, i, c]) == (int(R.mix32((e * R.ELEM_MUL + key) & 0xFFFFFFFF)) >= thr)
    assert np.array_equal(m.reshape(-1), R.mask(SEED_HI, 2 ** 32 + 7, 2, (S * n * d,), 0.5))
    assert R.mask(1, 2, 3, (4, 4), 0.0).all()           # threshold 0: everything kept


# ---- statistics of the stated mask ----------------------------------------------------------------------------------------
# p = 0.2 on [2, 333, 256] for 4 seeds x 6 counters x 5 streams = 120 masks.  Every bound is in binomial standard deviations
# and is a condition on this fixed input set: a pass is reproducible.  Measured with HEAD_STREAM_ID = 0x4845 (the extremes
# of 120, 30 720, 79 920, 7 140 and 8 standard normal draws would be about 2.7, 4.2, 4.4, 3.9 and 1.5):
#   keep rate of a mask <= 4 (2.54), of a column <= 6 (5.31), of a row <= 6 (4.50), correlation of two masks <= 5 (3.85),
#   pooled lag autocorrelation <= 4 (1.39, at lag 3)
P = 0.2
SHAPE = (2, 333, 256)
SEEDS = (0, 77, 0x5DEECE66D, 2 ** 62 + 12345)
STAT_COUNTERS = (0, 1, 2, 3, 2 ** 32, 2 ** 32 + 1)
STAT_STREAMS = (0, 1, 2, 3, HEAD)
LAGS = (1, 2, 3, 4, 64, 128, 256, 256 * 333)


@functools.lru_cache(maxsize=None)
def _masks():
    keys = list(itertools.product(SEEDS, STAT_COUNTERS, STAT_STREAMS))
    m = np.stack([R.mask(sd, c, s, SHAPE, P) for sd, c, s in keys])
    m.setflags(write=False)
    return keys, m


def _q():
    return 1.0 - R.dropout_threshold(P) / 2.0 ** 32   # the keep probability of a uniform 32-bit hash


def _z(kept, count):
    q = _q()
    return (kept - count * q) / np.sqrt(count * q * (1 - q))


def test_stat_keys_are_120_distinct_keys():
    keys, m = _masks()
    assert m.shape == (120,) + SHAPE
    assert len({R.dropout_key(*k) for k in keys}) == 120


def test_keep_rate_of_every_mask():
    _, m = _masks()
    z = _z(m.reshape(120, -1).sum(1), m[0].size)
    print("keep rate, max |z| over 120 masks: %.2f" % np.abs(z).max())
    assert np.abs(z).max() <= 4


def test_keep_rate_of_every_column_and_row():
    _, m = _masks()
    S, n, d = SHAPE
    zc = _z(m.sum((1, 2)), S * n)          # [120, d]
    zr = _z(m.sum(3), d)                   # [120, S, n]
    print("columns, max |z|: %.2f; rows, max |z|: %.2f" % (np.abs(zc).max(), np.abs(zr).max()))
    assert np.abs(zc).max() <= 6
    assert np.abs(zr).max() <= 6


def test_masks_of_different_keys_are_uncorrelated():
    _, m = _masks()
    x = m.reshape(120, -1).astype(np.float64)
    x -= x.mean(1, keepdims=True)
    x /= np.sqrt((x * x).sum(1, keepdims=True))
    corr = x @ x.T                          # sample correlation of every pair
    z = corr[np.triu_indices(120, 1)] * np.sqrt(x.shape[1])
    print("pair correlation, max |z| over %d pairs: %.2f" % (z.size, np.abs(z).max()))
    assert z.size == 7140 and np.abs(z).max() <= 5


@pytest.mark.parametrize("lag", LAGS)
def test_lag_autocorrelation(lag):
    """sum over the 120 masks of sum_e (m[e] - q)(m[e + lag] - q), in standard deviations of that sum for independent bits"""
    _, m = _masks()
    q = _q()
    x = m.reshape(120, -1).astype(np.float64) - q
    terms = x[:, :-lag] * x[:, lag:]
    z = terms.sum() / (np.sqrt(terms.size) * q * (1 - q))
    print("lag %d: z = %.2f" % (lag, z))
    assert abs(z) <= 4
