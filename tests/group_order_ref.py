"""numpy reference of the colour pass's order of dispatch (group_order_kernel and the group_trip output of live_order_kernel,
csrc/colour_order.hip) -- shared by tests/test_group_order.py (GPU) and tests/test_group_order_host.py (CPU, which checks this reference against a
brute-force sort).

A group is 256 consecutive entries of the ray order's packed array; its trip is the largest count among them.  group_slot[r] is the group
that workgroup r of the colour launch runs (on XCD r % 8): the groups sorted by trip, heaviest first.  A run of m groups of equal trip
occupies m consecutive ranks and is dealt in pieces: taken in group order, the run is cut into 8 contiguous pieces (the first m % 8 of them
one group longer), and piece k goes to the ranks k, k + 8, k + 16, .. of the run -- the ranks that share an XCD run consecutive groups.
With the handle off (or beyond MAX_G groups / MAX_S samples, which one workgroup does not sort) it is the mapping of the density kernel: XCD
r % 8 runs the (r % 8)-th contiguous eighth -- which is also what equal trips everywhere give."""
import numpy as np

from colour_order_ref import ORDER_SHIFT

GROUP_RAYS = 256
MAX_G = 4096
MAX_S = 511


def group_trips(packed):
    """largest count of every group of GROUP_RAYS packed entries (a ragged last group counts what it has)"""
    c = np.asarray(packed, np.int64) >> ORDER_SHIFT
    G = (c.size + GROUP_RAYS - 1) // GROUP_RAYS
    c = np.concatenate([c, np.zeros(G * GROUP_RAYS - c.size, np.int64)])
    return c.reshape(G, GROUP_RAYS).max(1).astype(np.int32)


def eighths(G):
    """the parent's mapping: workgroup r -> ray block (r % 8) * (G // 8) + min(r % 8, G % 8) + r // 8"""
    r = np.arange(G, dtype=np.int64)
    xcd, per, rem = r & 7, G >> 3, G & 7
    return (xcd * per + np.minimum(xcd, rem) + (r >> 3)).astype(np.int32)


def group_order_reference(trips, S, sorted_=True):
    trips = np.asarray(trips, np.int64)
    G = trips.size
    if not sorted_ or G > MAX_G or S > MAX_S:
        return eighths(G)
    key = np.clip(trips, 0, S)
    order = np.argsort(-key, kind="stable")
    out = np.empty(G, np.int64)
    k = key[order]
    starts = np.flatnonzero(np.concatenate([[True], k[1:] != k[:-1]]))
    for a, b in zip(starts, np.concatenate([starts[1:], [G]])):
        out[a:b] = order[a:b][eighths(b - a)]
    return out.astype(np.int32)


def check_group_order(slot, trips, S):
    """a permutation of the groups; trips do not increase along it; inside a run of equal trips, read piece by piece (ranks k, k + 8, .. of the
    run for k = 0..7), the groups are in group order, and the pieces' lengths differ by one at most, the longer ones first"""
    slot = np.asarray(slot, np.int64)
    t = np.clip(np.asarray(trips, np.int64), 0, S)
    assert slot.shape == t.shape
    assert np.array_equal(np.sort(slot), np.arange(t.size)), "not a permutation"
    along = t[slot]
    assert np.all(along[1:] <= along[:-1]), "trips increase"
    starts = np.flatnonzero(np.concatenate([[True], along[1:] != along[:-1]]))
    for a, b in zip(starts, np.concatenate([starts[1:], [t.size]])):
        pieces = np.concatenate([slot[a + k:b:8] for k in range(8)])      # (ranks a + k, a + k + 8, ..: one XCD's)
        assert np.all(pieces[1:] > pieces[:-1]), "run at rank %d: its pieces are not the run in group order" % a
