"""numpy reference of the point-major colour pass's order of points (csrc/colour_order.hip: point_order_kernel; include/nvsr.h, "The two-phase
render pass").  A plain helper module (not collected): tests/test_colour_points_host.py checks it against the order's properties on the CPU,
tests/test_colour_points.py holds the kernel against it."""
import numpy as np

from colour_order_ref import ORDER_RAYS, ORDER_SHIFT

GROUP = 256          # slots of a group = points of a step
POINT_NONE = -1      # the padding of a group's last step


def bands_of_indices(idx, S, nb):
    """band of a sample index (lists of the pass with its depths in registers): idx nb / S"""
    return np.clip(idx.astype(np.int64) * nb // S, 0, nb - 1)


def bands_of_depths(z, near, far, nb):
    """band of a stored depth over the ray's near..far, in float32 as the kernel computes it: ((z - near) nb) / (far - near), truncated,
    clamped to 0..nb-1, a NaN to band 0"""
    z, near, far = (np.asarray(a, np.float32) for a in (z, near, far))
    with np.errstate(all="ignore"):
        u = ((z - near[:, None]) * np.float32(nb)) / (far - near)[:, None]
        t = np.where(u < nb, np.trunc(np.where(u < nb, u, 0)), nb - 1)
    return np.where(u >= 0, t, 0).astype(np.int64)


def point_order_reference(packed, bands, S, nb):
    """packed: the N packed entries of the ray order (slot i of block i // ORDER_RAYS holds the ray it names and that ray's count);
    bands [N, S]: band of live entry k of ray r in bands[r, k] (the first count entries of a row count).
    -> (points [G, GROUP * S], padded with POINT_NONE; steps [G]; offsets [G], in steps): group g's live points in the order (band, slot, k),
    the band made monotone along the ray, cut into steps of GROUP and every step sorted by (slot, k)."""
    packed = np.asarray(packed, np.int64)
    N = packed.size
    G = (N + GROUP - 1) // GROUP
    pts = np.full((G, GROUP * S), POINT_NONE, np.int32)
    steps = np.zeros(G, np.int32)
    for g in range(G):
        rows = []
        for j in range(min(GROUP, N - g * GROUP)):
            e = packed[g * GROUP + j]
            n, ray = e >> ORDER_SHIFT, (g * GROUP) // ORDER_RAYS * ORDER_RAYS + (e & (ORDER_RAYS - 1))
            b = np.maximum.accumulate(np.clip(bands[ray, :n], 0, nb - 1)) if n else np.zeros(0, np.int64)
            rows.append(np.stack([b, np.full(n, j, np.int64), np.arange(n, dtype=np.int64)], 1))
        p = np.concatenate(rows) if rows else np.zeros((0, 3), np.int64)
        p = p[np.lexsort((p[:, 2], p[:, 1], p[:, 0]))]
        steps[g] = (len(p) + GROUP - 1) // GROUP
        for t in range(steps[g]):
            q = p[t * GROUP:(t + 1) * GROUP]
            q = q[np.lexsort((q[:, 2], q[:, 1]))]
            pts[g, t * GROUP:t * GROUP + len(q)] = ((q[:, 1] << 24) | q[:, 2]).astype(np.uint32).view(np.int32)
    return pts, steps, (np.arange(G) * S).astype(np.int32)


def check_points(pts, steps, packed, S):
    """the order's properties, whatever the bands: every live entry exactly once; a ray's entries in increasing k over the whole sequence;
    a ray forms one run inside a step; the step counts; padding only behind the last point"""
    packed = np.asarray(packed, np.int64)
    N = packed.size
    for g in range(pts.shape[0]):
        n = np.zeros(GROUP, np.int64)
        m = min(GROUP, N - g * GROUP)
        n[:m] = packed[g * GROUP:g * GROUP + m] >> ORDER_SHIFT
        total = int(n.sum())
        assert steps[g] == (total + GROUP - 1) // GROUP, g
        row = pts[g].view(np.uint32).astype(np.int64)
        assert np.all(pts[g, total:] == POINT_NONE) and np.all(pts[g, :total] != POINT_NONE), g
        slot, k = row[:total] >> 24, row[:total] & 0xffffff
        for j in range(GROUP):
            assert np.array_equal(k[slot == j], np.arange(n[j])), (g, j)          # exactly once, in increasing k
        for t in range(steps[g]):
            s = slot[t * GROUP:(t + 1) * GROUP]
            assert np.all(np.diff(s) >= 0), (g, t)                               # sorted by slot: every ray is one run
