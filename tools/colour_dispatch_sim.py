#!/usr/bin/env python3
"""Dispatch model of the colour kernels (csrc/render3.hip): how long a launch takes, in steps, under a given order of its
workgroups.  CPU only.

A colour workgroup runs `trip` steps, the largest live count among its 256 rays.  The model: workgroup b goes to XCD b % 8; an XCD has 32
CUs holding one workgroup each; the next workgroup of the XCD, in id order, goes to the first CU that frees; a workgroup's time is its trip.
It knows nothing of the clock (idle CUs let busy ones run faster) nor of the L2 (neighbouring groups share texels): its gain is an upper
bound.  Orders compared, against the balanced bound sum(trip) / 256:
  eighths        workgroup b runs ray block (b % 8) * (G // 8) + min(b % 8, G % 8) + b // 8: XCD x takes the x-th contiguous eighth
                 (the density kernels' mapping; NVSR_COLOUR_GROUP_ORDER=0)
  eighths sorted the same eighths, heaviest group first inside each
  dealt          the groups heaviest first over the whole launch, rank r to workgroup r, hence to XCD r % 8 (group_order_kernel)

Input: an .npz with the packed entries that nvsr_internal_copy_live_counts returns for a pass, (count << 12) | index, one array per pass
(any names), or a .json with lists of group trips named <pass>_trips.  --save-trips writes the latter (2 G ints per frame instead of 2 N).

    python tools/colour_dispatch_sim.py profiles/colour_group_trips.json
"""
import argparse
import heapq
import json

import numpy as np

ORDER_SHIFT, GROUP_RAYS, XCDS, CUS_PER_XCD = 12, 256, 8, 32


def group_trips(packed):
    c = np.asarray(packed, np.int64) >> ORDER_SHIFT
    G = (c.size + GROUP_RAYS - 1) // GROUP_RAYS
    c = np.concatenate([c, np.zeros(G * GROUP_RAYS - c.size, np.int64)])
    return c.reshape(G, GROUP_RAYS).max(1)


def eighths(G):
    r = np.arange(G, dtype=np.int64)
    xcd, per, rem = r & 7, G >> 3, G & 7
    return xcd * per + np.minimum(xcd, rem) + (r >> 3)


def makespan(trips_in_workgroup_order):
    """steps until the last workgroup ends, and each XCD's own end"""
    ends = []
    for x in range(XCDS):
        free = [0] * CUS_PER_XCD
        for t in trips_in_workgroup_order[x::XCDS]:
            heapq.heappush(free, heapq.heappop(free) + int(t))
        ends.append(max(free))
    return max(ends), ends


def orders(trips):
    G = trips.size
    e = eighths(G)
    es = e.copy()
    for x in range(XCDS):                                   # heaviest first inside XCD x's eighth
        blocks = e[x::XCDS]
        es[x::XCDS] = blocks[np.argsort(-trips[blocks], kind="stable")]
    return {"eighths": e, "eighths sorted": es, "dealt": np.argsort(-trips, kind="stable")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("counts")
    ap.add_argument("--save-trips", default=None, metavar="JSON")
    a = ap.parse_args()
    if a.counts.endswith(".json"):
        with open(a.counts) as f:
            data = {k: np.asarray(v, np.int64) for k, v in json.load(f).items()}
    else:
        data = dict(np.load(a.counts))
    passes = {}
    for name in data:
        passes[name[:-6] if name.endswith("_trips") else name] = np.asarray(data[name], np.int64) if name.endswith("_trips") else group_trips(data[name])
    if a.save_trips:
        with open(a.save_trips, "w") as f:
            f.write("{\n" + ",\n".join('"%s_trips": [%s]' % (n, ", ".join(str(int(x)) for x in t)) for n, t in passes.items()) + "\n}\n")
    print("%-8s %6s %10s %9s   %s" % ("pass", "groups", "sum trip", "balanced", "makespan in steps (over balanced)"))
    for name, trips in passes.items():
        bal = trips.sum() / (XCDS * CUS_PER_XCD)
        row = []
        for label, order in orders(trips).items():
            assert np.array_equal(np.sort(order), np.arange(trips.size))
            m, ends = makespan(trips[order])
            row.append("%s %d (%+.1f %%)" % (label, m, 100 * (m / bal - 1)))
        print("%-8s %6d %10d %9.1f   %s" % (name, trips.size, trips.sum(), bal, "   ".join(row)))
        sums = [int(trips[eighths(trips.size)[x::XCDS]].sum()) for x in range(XCDS)]
        print("%-8s XCD sums of trips under eighths: max / mean %.3f" % ("", max(sums) / (sum(sums) / XCDS)))


if __name__ == "__main__":
    main()
