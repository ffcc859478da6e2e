"""numpy float32 transcriptions of the occupancy grid's kernels (csrc/occupancy.hip; include/nvsr.h, "Occupancy grid") for
tests/test_occupancy_host.py and tests/test_occupancy.py: the probe formula, the cell formula, bit packing, dilation and the kept lists.
A plain helper module (not collected).  Every step of the float32 formulas is one correctly rounded float32 operation, as in the kernels."""
import numpy as np

f32 = np.float32


def words(G):
    return (G ** 3 + 31) // 32


def probes(lo, rng, G, K):
    """x [G^3 K^3, 6]: probe (jz K + jy) K + jx of cell i = (iz G + iy) G + ix at row i K^3 + it; along each axis
    u = ((float)(c K + j) + 0.5f) / (float)(G K), world = lo + u range; view direction (1, 0, 0)"""
    lo, rng = np.asarray(lo, f32), np.asarray(rng, f32)
    c = np.arange(G)
    j = np.arange(K)
    iz, iy, ix, jz, jy, jx = np.meshgrid(c, c, c, j, j, j, indexing="ij")
    x = np.empty((G ** 3 * K ** 3, 6), f32)
    for a, (cc, jj) in enumerate(((ix, jx), (iy, jy), (iz, jz))):
        u = ((cc * K + jj).astype(f32) + f32(0.5)) / f32(G * K)
        x[:, a] = (lo[a] + u * rng[a]).reshape(-1)
    x[:, 3:] = (1.0, 0.0, 0.0)
    return x


def cell_axis(n, G):
    """clamp((int)floorf(((n + 1.0f) * 0.5f) * (float)G), 0, G - 1) of float32 n (NaN: undefined here, the callers keep such a sample)"""
    n = np.asarray(n, f32)
    with np.errstate(invalid="ignore", over="ignore"):
        f = np.floor(((n + f32(1.0)) * f32(0.5)) * f32(G))
        return np.clip(np.nan_to_num(f, nan=0.0), 0, G - 1).astype(np.int64)


def cell_axis_f64(n, G):
    n = np.asarray(n, np.float64)
    return np.clip(np.floor((n + 1.0) * 0.5 * G), 0, G - 1).astype(np.int64)


def norm_points(rays, z, lo, rng):
    """the render body's normalised points, [N, S, 3] float32: 2 ((o + d z) - lo) / range - 1, one rounding per operation"""
    rays, z = np.asarray(rays, f32), np.asarray(z, f32)
    lo, rng = np.asarray(lo, f32)[:3], np.asarray(rng, f32)[:3]
    with np.errstate(invalid="ignore", over="ignore"):
        p = rays[:, None, 0:3] + rays[:, None, 3:6] * z[:, :, None]
        return (f32(2.0) * (p - lo)) / rng - f32(1.0)


def cell_index(n, G):
    """[..., 3] normalised points -> linear cell index i = (iz G + iy) G + ix and the NaN mask"""
    nan = np.isnan(n).any(-1)
    c = cell_axis(n, G)
    return (c[..., 2] * G + c[..., 1]) * G + c[..., 0], nan


def pack_bits(cells, G):
    """bool [G^3] in linear cell order -> uint32 words, bit i & 31 of word i >> 5, padding bits 0"""
    b = np.zeros(words(G) * 32, np.uint8)
    b[:G ** 3] = np.asarray(cells, bool).reshape(-1)
    return np.packbits(b.reshape(-1, 32), axis=1, bitorder="little").view("<u4").reshape(-1)


def unpack_bits(grid, G):
    g = np.ascontiguousarray(np.asarray(grid).view(np.uint32)).astype("<u4")
    return np.unpackbits(g.view(np.uint8), bitorder="little")[:G ** 3].astype(bool)


def mark(sigma, K, threshold):
    """sigma_raw [G^3 K^3] of probes() -> bool [G^3]: any probe of the cell above the threshold, or NaN"""
    s = np.asarray(sigma, f32).reshape(-1, K ** 3)
    with np.errstate(invalid="ignore"):
        return ((s > f32(threshold)) | np.isnan(s)).any(1)


def dilate(cells, G, rounds=1):
    """`rounds` rounds of a 3 x 3 x 3 OR, clipped at the faces"""
    v = np.asarray(cells, bool).reshape(G, G, G)
    for _ in range(rounds):
        p = np.zeros((G + 2, G + 2, G + 2), bool)
        p[1:-1, 1:-1, 1:-1] = v
        out = np.zeros_like(v)
        for dz in range(3):
            for dy in range(3):
                for dx in range(3):
                    out |= p[dz:dz + G, dy:dy + G, dx:dx + G]
        v = out
    return v.reshape(-1)


def keep_mask(rays, z, lo, rng, grid, G):
    """bool [N, S]: the sample's cell bit is set, or its normalised point has a NaN coordinate"""
    i, nan = cell_index(norm_points(rays, z, lo, rng), G)
    return unpack_bits(grid, G)[i] | nan


def kept_lists(keep):
    """bool [N, S] -> kept [N, S] int32 (the kept sample indices in sample order, then -1) and kept_n [N]"""
    keep = np.asarray(keep, bool)
    N, S = keep.shape
    order = np.argsort(~keep, axis=1, kind="stable")
    n = keep.sum(1).astype(np.int32)
    kept = np.where(np.arange(S)[None, :] < n[:, None], order, -1).astype(np.int32)
    return kept, n
