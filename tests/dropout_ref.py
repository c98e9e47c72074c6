"""The dropout mask of the fused kernels, restated in numpy.  THIS FILE IS THE SPECIFICATION OF THE MASK: the library has no
other independent statement of it (chromegcn_amd/csrc/cgcn_common.hpp: mix32, dropout_key, dropout_keep, dropout_threshold;
cgcn_kernels.hip: dropout_args), every test that needs "the mask the kernels draw" takes it from here
(tests/test_dropout_ref_host.py pins it, tests/test_gpu_dropout_masks.py holds every kernel to it), and a change of the hash,
of the key schedule or of the threshold rule in cgcn_common.hpp means changing it here too, on purpose.

The masks stand for the two F.dropout calls of the reference's model: models/ChromeModels.py:42 (between the gated layers:
layer k drops its own output under stream id k, layer k + 1 un-drops the gradient of its input under the same id) and
models/ChromeModels.py:50 (in the classifier head, after the BatchNorm: stream id HEAD_STREAM_ID).  Same Bernoulli law as
torch's generator, another sequence ("Deviations on purpose").

    keep(element e)  <=>  mix32(e * 0x9E3779B1 + key) >= threshold,       key = dropout_key(seed, step counter, stream id)
    e = (s * n + i) * d + c: the C-order index of element (strand s, node i, column c) of a [S, n, d] tensor
    kept elements are multiplied by keep_scale = 1 / (1 - p)

All of it is uint32 arithmetic, written as uint64 masked to 32 bits (numpy's uint32 multiply wraps too, but warns).  p reaches
the library as a C float, so both the threshold and the scale are functions of float32(p), not of the Python double: for p = 0.2
the threshold is 858993472, the double's would be 858993459.  Builders only: nothing here touches the GPU."""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)
HEAD_STREAM_ID = 0x4845            # cgcn_common.hpp: the classifier head's stream ("HE"); gated layer k uses stream id k
ELEM_MUL = 0x9E3779B1              # dropout_keep


def _u64(x):
    return np.asarray(x, dtype=np.uint64)


def mix32(x):
    """x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16 on uint32 (scalar or array -> uint64 array
    of values below 2^32)"""
    x = _u64(x) & M32
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & M32
    x = x ^ (x >> np.uint64(16))
    return x


def dropout_key(seed, counter, stream_id):
    """the 32-bit key of one (64-bit seed, 64-bit step counter, 32-bit stream id), as a Python int"""
    seed, counter, stream_id = int(seed) & (2 ** 64 - 1), int(counter) & (2 ** 64 - 1), int(stream_id) & 0xFFFFFFFF
    k = int(mix32((seed & 0xFFFFFFFF) ^ 0x9E3779B9))
    k = int(mix32(k ^ (seed >> 32)))
    k = int(mix32((k + (counter & 0xFFFFFFFF) * 0x85EBCA6B) & 0xFFFFFFFF))
    k = int(mix32(k ^ (counter >> 32) ^ ((stream_id * 0xC2B2AE35) & 0xFFFFFFFF)))
    return k


def dropout_threshold(p):
    """trunc(float32(p) * 2^32) clamped to [0, 2^32 - 1] (the product is formed in double, where it is exact); 0 = no dropout"""
    t = float(np.float32(p)) * 4294967296.0
    if t <= 0.0:
        return 0
    if t >= 4294967295.0:
        return 4294967295
    return int(t)


def keep_scale(p):
    """float32(1) / (float32(1) - float32(p)), as a numpy float32"""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def mask(seed, counter, stream_id, shape, p):
    """bool array of `shape`, True = kept, over the C-order element index (for [S, n, d]: (s * n + i) * d + c)"""
    count = int(np.prod(shape))
    assert count <= 2 ** 32, "the kernels index elements with 32 bits"
    e = np.arange(count, dtype=np.uint64)
    h = mix32((e * np.uint64(ELEM_MUL) + np.uint64(dropout_key(seed, counter, stream_id))) & M32)
    return (h >= np.uint64(dropout_threshold(p))).reshape(shape)
