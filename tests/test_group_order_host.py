"""CPU test of the yardstick of tests/test_group_order.py: the numpy reference of the colour pass's order of dispatch (group_order_ref.py)
against a brute-force sort written without numpy's argsort, its properties, and the handle-off mapping against the parent's formula."""
import numpy as np
import pytest

from colour_order_ref import ORDER_SHIFT
from group_order_ref import GROUP_RAYS, MAX_G, MAX_S, check_group_order, eighths, group_order_reference, group_trips


def _brute(trips):
    """insertion into a list, one group at a time: a group goes behind every group whose trip is at least its own; then every run of equal
    trips is dealt: its groups, in order, fill piece 0, then piece 1, .. (piece k = every eighth rank of the run from its k-th on)"""
    out = []
    for g, t in enumerate(trips):
        at = len(out)
        while at > 0 and out[at - 1][0] < t:
            at -= 1
        out.insert(at, (int(t), g))
    slot = [None] * len(out)
    a = 0
    while a < len(out):
        b = a
        while b < len(out) and out[b][0] == out[a][0]:
            b += 1
        ranks = [r for k in range(8) for r in range(a + k, b, 8)]
        for (_, g), r in zip(out[a:b], ranks):
            slot[r] = g
        a = b
    return np.array(slot, np.int32)


def _cases():
    rng = np.random.default_rng(3)
    yield [0], 1
    yield [1], 1
    yield [5, 5, 5, 5], 9
    yield [0, 0, 0], 4
    yield [0, 0, 192, 0, 0], 192
    yield [1, 12, 13, 24, 0, 192, 191, 12, 1, 96], 192
    yield list(rng.integers(0, 65, 17)), 64
    yield list(rng.integers(0, 193, 300)), 192
    yield list(rng.integers(0, 2, 300)), 1
    yield list(rng.integers(0, 193, 2500)), 192


@pytest.mark.parametrize("trips,S", list(_cases()))
def test_reference_is_a_descending_sort_with_runs_dealt_in_pieces(trips, S):
    ref = group_order_reference(trips, S)
    assert np.array_equal(ref, _brute(trips))
    check_group_order(ref, trips, S)


def test_equal_trips_everywhere_give_the_parents_mapping():
    for G in (1, 7, 8, 9, 17, 300, 2500):
        assert np.array_equal(group_order_reference(np.full(G, 7), 40), eighths(G))
        assert np.array_equal(group_order_reference(np.zeros(G, np.int64), 40), eighths(G))


def test_runs_shorter_than_eight_keep_group_order():
    """distinct trips, or fewer than 8 groups of a trip: every piece holds one group at most, the order is the stable sort's"""
    rng = np.random.default_rng(4)
    t = rng.permutation(193)
    assert np.array_equal(group_order_reference(t, 192), np.argsort(-t, kind="stable"))
    t = np.repeat(np.arange(40), 7)[rng.permutation(280)]
    assert np.array_equal(group_order_reference(t, 40), np.argsort(-t, kind="stable"))


@pytest.mark.parametrize("G", [1, 7, 8, 9, 2500])
def test_handle_off_is_the_parents_formula(G):
    """workgroup b of the parent runs ray block xcd * per + min(xcd, rem) + (b >> 3), xcd = b & 7, per = G >> 3, rem = G & 7 (render3.hip)"""
    rng = np.random.default_rng(G)
    got = group_order_reference(rng.integers(0, 65, G), 64, sorted_=False)
    want = []
    for b in range(G):
        xcd, per, rem = b & 7, G >> 3, G & 7
        want.append(xcd * per + (xcd if xcd < rem else rem) + (b >> 3))
    assert np.array_equal(got, np.array(want, np.int32))
    assert np.array_equal(np.sort(got), np.arange(G))                  # a permutation: every block is run once
    # XCD x (workgroups x, x + 8, ...) runs a contiguous run of blocks, and the eight runs follow one another
    runs = [got[x::8] for x in range(min(8, G))]
    assert all(np.array_equal(r, np.arange(r[0], r[0] + r.size)) for r in runs)
    assert np.array_equal(np.concatenate(runs), np.arange(G))


def test_beyond_one_workgroup_it_is_the_parents_mapping():
    rng = np.random.default_rng(1)
    assert np.array_equal(group_order_reference(rng.integers(0, 65, MAX_G + 1), 64), eighths(MAX_G + 1))
    assert np.array_equal(group_order_reference(rng.integers(0, MAX_S + 2, 9), MAX_S + 1), eighths(9))
    t = rng.integers(0, MAX_S + 1, MAX_G)
    check_group_order(group_order_reference(t, MAX_S), t, MAX_S)


def test_group_trips_are_the_groups_maxima():
    rng = np.random.default_rng(2)
    n = 3 * GROUP_RAYS + 37
    count = rng.integers(0, 41, n)
    count[GROUP_RAYS:2 * GROUP_RAYS] = 0                                # a group of empty rays
    packed = (count << ORDER_SHIFT) | (np.arange(n) % 4096)
    t = group_trips(packed)
    assert t.shape == (4,) and t[1] == 0
    for g in range(4):
        assert t[g] == max(int(c) for c in count[g * GROUP_RAYS:(g + 1) * GROUP_RAYS])      # (the ragged last group: what it has)


def test_check_group_order_rejects_wrong_results():
    trips = np.array([3, 9, 0, 9, 5])
    good = group_order_reference(trips, 9)
    check_group_order(good, trips, 9)
    swapped = good.copy()
    swapped[[0, 1]] = swapped[[1, 0]]                                   # the two heaviest groups out of their original order
    repeated = good.copy()
    repeated[1] = repeated[0]
    for bad in (swapped, repeated, good[::-1].copy()):
        with pytest.raises(AssertionError):
            check_group_order(bad, trips, 9)
    trips = np.full(20, 3)
    check_group_order(group_order_reference(trips, 9), trips, 9)
    with pytest.raises(AssertionError):
        check_group_order(np.arange(20), trips, 9)                      # equal trips dealt one by one
