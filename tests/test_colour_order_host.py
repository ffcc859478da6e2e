"""CPU test of the yardstick of tests/test_colour_order.py: the numpy reference of the colour pass's ray order (colour_order_ref.py) against
a brute-force sort written without numpy's argsort, on tiny cases, and check_packed against results that are wrong in one property each."""
import numpy as np
import pytest

from colour_order_ref import ORDER_RAYS, ORDER_SHIFT, bin_of, check_packed, order_reference


def _brute(count, S, bins):
    """insertion into a list, one ray at a time: a ray goes behind every ray whose bin is at least its own"""
    out = []
    for b0 in range(0, len(count), ORDER_RAYS):
        block = []
        for i, c in enumerate(count[b0:b0 + ORDER_RAYS]):
            b = min(-((-int(c) * bins) // S), bins)          # ceil(c bins / S)
            at = len(block)
            while at > 0 and block[at - 1][0] < b:
                at -= 1
            block.insert(at, (b, int(c), i))
        out += [(c << ORDER_SHIFT) | i for _, c, i in block]
    return np.array(out, np.int32)


CASES = [
    ([0], 1, 16), ([1], 1, 16), ([3, 3, 3, 3], 5, 16), ([0, 1, 2, 3, 4, 5], 5, 16), ([5, 4, 3, 2, 1, 0], 5, 4),
    ([0, 0, 7, 0, 0], 7, 16), ([1, 12, 13, 24, 0, 192, 191, 12, 1, 96], 192, 16), ([1, 12, 13, 24, 0, 192, 191, 12, 1, 96], 192, 8),
    ([2, 0, 1, 2, 0, 1], 2, 0),
]


@pytest.mark.parametrize("count,S,bins", CASES)
def test_reference_equals_brute_force(count, S, bins):
    ref = order_reference(np.array(count), S, bins)
    assert np.array_equal(ref, _brute(count, S, bins))
    check_packed(ref, count, S, bins)


def test_reference_two_blocks_and_identity():
    rng = np.random.default_rng(0)
    count = rng.integers(0, 41, ORDER_RAYS + 5)
    ref = order_reference(count, 40, 16)
    assert np.array_equal(ref, _brute(list(count), 40, 16))
    assert np.array_equal(np.sort(ref[ORDER_RAYS:] & (ORDER_RAYS - 1)), np.arange(5))        # the ragged block is ordered on its own
    ident = order_reference(count, 40, 0)
    assert np.array_equal(ident, (count << ORDER_SHIFT) | (np.arange(count.size) % ORDER_RAYS))
    assert np.array_equal(order_reference(np.full(300, 7), 40, 16) & (ORDER_RAYS - 1), np.arange(300))      # equal counts: stability


def test_bins_are_equal_width_with_one_for_empty_rays():
    b = bin_of(np.arange(0, 193), 192, 16)
    assert b[0] == 0 and b[1] == 1 and b[12] == 1 and b[13] == 2 and b[192] == 16
    assert np.array_equal(np.bincount(b), [1] + [12] * 16)
    assert np.array_equal(bin_of(np.array([0, 1]), 1, 16), [0, 16])


def test_check_packed_rejects_wrong_results():
    count = np.array([1, 40, 0, 40, 20])
    good = order_reference(count, 40, 16)
    check_packed(good, count, 40, 16)
    swapped = good.copy()
    swapped[[0, 1]] = swapped[[1, 0]]                       # the two full rays out of their original order
    wrong_count = good.copy()
    wrong_count[0] += 1 << ORDER_SHIFT
    repeated = good.copy()
    repeated[1] = repeated[0]
    for bad in (swapped, wrong_count, repeated, good[::-1].copy()):
        with pytest.raises(AssertionError):
            check_packed(bad, count, 40, 16)
