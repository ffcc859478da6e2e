"""CPU tests of the numpy reference of the point-major colour pass's order of points (tests/colour_points_ref.py) against the properties the
kernels rely on (csrc/render3.hip PHASE 3): every live entry once, a ray's entries in sample order, one run per ray and step, the step counts."""
import numpy as np
import pytest

from colour_order_ref import ORDER_RAYS, ORDER_SHIFT, order_reference
from colour_points_ref import GROUP, POINT_NONE, bands_of_depths, bands_of_indices, check_points, point_order_reference


def _lists(count, S, rng):
    """sorted sample indices of every ray's live entries, [N, S] (rows padded with S - 1)"""
    rank = np.argsort(np.argsort(rng.random((count.size, S)), 1), 1)
    idx = np.sort(np.where(rank < count[:, None], np.arange(S)[None, :], S + 1), 1)
    return np.minimum(idx, S - 1)


@pytest.mark.parametrize("nb", [1, 4, 8, 16, 0])
@pytest.mark.parametrize("S", [1, 8, 24])
def test_reference_has_the_orders_properties(S, nb):
    rng = np.random.default_rng(S * 100 + nb)
    N = ORDER_RAYS + 513
    count = rng.integers(0, S + 1, N)
    count[GROUP:2 * GROUP] = 0
    count[7] = S
    nbands = nb if 1 <= nb <= S else S
    packed = order_reference(count, S, 32)
    pts, steps, offs = point_order_reference(packed, bands_of_indices(_lists(count, S, rng), S, nbands), S, nbands)
    check_points(pts, steps, packed, S)
    assert np.array_equal(offs, np.arange(pts.shape[0]) * S)
    assert int(steps.sum()) * GROUP >= int(count.sum()) > (int(steps.sum()) - pts.shape[0]) * GROUP      # at most one padded step per group


def test_bands_order_the_points_and_runs_are_contiguous():
    """one group, identity entries, hand-made lists: the global order is (band, slot, k); a step is then sorted by (slot, k)"""
    S, nb = 8, 4
    count = np.zeros(GROUP, np.int64)
    count[[0, 1, 2]] = [3, 2, 8]
    idx = np.zeros((GROUP, S), np.int64)
    idx[0, :3] = [0, 1, 7]
    idx[1, :2] = [2, 6]
    idx[2] = np.arange(8)
    packed = (count << ORDER_SHIFT) | np.arange(GROUP)
    pts, steps, _ = point_order_reference(packed, bands_of_indices(idx, S, nb), S, nb)
    assert steps[0] == 1
    got = pts[0, :13].view(np.uint32).astype(np.int64)
    assert np.array_equal(got >> 24, [0] * 3 + [1] * 2 + [2] * 8) and np.array_equal(got & 0xffffff, [0, 1, 2, 0, 1] + list(range(8)))
    assert np.all(pts[0, 13:] == POINT_NONE)
    # band 0 holds 257 points (every ray's sample 0 and ray 2's sample 1): the cut falls inside it, slot 255's point opens the second step;
    # ray 2's samples 2..7 lie in three bands of that step and still form one run, in sample order
    count[:] = 2
    idx[:, 0], idx[:, 1] = 0, 7
    count[2], idx[2] = 8, np.arange(8)
    packed = (count << ORDER_SHIFT) | np.arange(GROUP)
    pts, steps, _ = point_order_reference(packed, bands_of_indices(idx, S, nb), S, nb)
    check_points(pts, steps, packed, S)
    first, second = (pts[0, t * GROUP:(t + 1) * GROUP].view(np.uint32).astype(np.int64) for t in (0, 1))
    assert steps[0] == 3 and np.array_equal(first[(first >> 24) == 2] & 0xffffff, [0, 1])
    at = np.flatnonzero((second >> 24) == 2)
    assert np.array_equal(second[at] & 0xffffff, np.arange(2, 8)) and np.array_equal(at, at[0] + np.arange(6))
    assert second[-1] == (255 << 24) | 0


def test_depth_bands_are_float32_and_clamped():
    z = np.array([[1.0, 2.0, 3.999, 4.0, 6.0, 7.0, np.nan]], np.float32)
    b = bands_of_depths(z, np.array([2.0]), np.array([6.0]), 8)
    assert np.array_equal(b[0], [0, 0, 3, 4, 7, 7, 0])
