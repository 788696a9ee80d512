"""rt.h's "packed canva transport" restated in NumPy, and the bit-for-bit
comparison the packed-canva tests share: a pixel is one 32-bit word
f0 | f1 << 9 | f2 << 18, field = the channel's value for the integers 0..255
and 256 for everything else, which unpacks as -2147483648.0."""
import numpy as np

MARKER = -2147483648.0


def np_field(v):
    """Field of each channel value: the value for +0.0, 1.0, ..., 255.0 (compared as bit patterns, so -0.0 is
    not among them), else 256."""
    v = np.ascontiguousarray(v, dtype=np.float64)
    table = np.arange(256, dtype=np.float64).view(np.uint64)
    bits = v.view(np.uint64)
    f = np.full(v.shape, 256, dtype=np.uint32)
    for k in range(256):
        f[bits == table[k]] = k
    return f


def np_pack(canva):
    f = np_field(canva)
    return f[..., 0] | f[..., 1] << np.uint32(9) | f[..., 2] << np.uint32(18)


def np_unpack(words):
    w = np.asarray(words, dtype=np.uint32)
    f = np.stack([(w >> np.uint32(9 * k)) & np.uint32(0x1ff) for k in range(3)], axis=-1)
    return np.where(f < 256, f.astype(np.float64), MARKER)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    bad = np.argwhere(a.view(np.uint64) != b.view(np.uint64))
    assert len(bad) == 0, "%d values differ, first at %r: %r vs %r" % (len(bad), tuple(bad[0]), a[tuple(bad[0])],
                                                                     b[tuple(bad[0])])


def every_value_plane():
    """771 pixels: each of the 257 canva values in each channel position, the
    other two channels running through other values."""
    vals = np.concatenate([np.arange(256, dtype=np.float64), [MARKER]])
    px = np.zeros((771, 3))
    for c in range(3):
        for k in range(257):
            px[c * 257 + k, c] = vals[k]
            px[c * 257 + k, (c + 1) % 3] = vals[(k * 7 + 3) % 257]
            px[c * 257 + k, (c + 2) % 3] = vals[(256 - k + 11 * c) % 257]
    return px
