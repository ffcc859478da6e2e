"""numpy reference of the colour pass's ray order (live_order_kernel, csrc/colour_order.hip) and the checks of a packed result -- shared by
tests/test_colour_order.py (GPU) and tests/test_colour_order_host.py (CPU, which checks this reference against a brute-force sort).

Rays are ordered inside blocks of ORDER_RAYS consecutive rays by the bin of their live count, fullest bin first, stably; entry j of a block
is (count << ORDER_SHIFT) | index of the ray in its block.  bin = ceil(count * bins / S): 0 for an empty ray, `bins` bins of equal width
over 1..S; bins = 0 is a single bin (the identity)."""
import numpy as np

ORDER_SHIFT = 12
ORDER_RAYS = 1 << ORDER_SHIFT


def bin_of(count, S, bins):
    return np.minimum((np.asarray(count, np.int64) * bins + S - 1) // S, bins)


def order_reference(count, S, bins):
    count = np.asarray(count, np.int64)
    out = np.empty(count.shape, np.int64)
    for b0 in range(0, count.size, ORDER_RAYS):
        c = count[b0:b0 + ORDER_RAYS]
        idx = np.argsort(-bin_of(c, S, bins), kind="stable")
        out[b0:b0 + c.size] = (c[idx] << ORDER_SHIFT) | idx
    return out.astype(np.int32)


def check_packed(packed, count, S, bins):
    """the four properties of a packed result, block by block: the low bits are a permutation of 0..M-1, the high bits are that ray's
    original count, the bins do not increase, and the original order holds inside a bin"""
    packed = np.asarray(packed, np.int64)
    count = np.asarray(count, np.int64)
    assert packed.shape == count.shape
    for b0 in range(0, count.size, ORDER_RAYS):
        c = count[b0:b0 + ORDER_RAYS]
        e = packed[b0:b0 + c.size]
        idx, n = e & (ORDER_RAYS - 1), e >> ORDER_SHIFT
        assert np.array_equal(np.sort(idx), np.arange(c.size)), "block at %d: not a permutation" % b0
        assert np.array_equal(n, c[idx]), "block at %d: a count is not its ray's" % b0
        b = bin_of(n, S, bins)
        assert np.all(b[1:] <= b[:-1]), "block at %d: bins increase" % b0
        same = b[1:] == b[:-1]
        assert np.all(idx[1:][same] > idx[:-1][same]), "block at %d: order inside a bin" % b0
