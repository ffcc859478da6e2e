"""numpy statements of the occupancy route of the generic decoder geometries (include/nvsr.h, "generic decoder, occupancy grid";
csrc/occupancy.hip: generic_occupancy_keep_kernel, nvsr_generic_occupancy_build_ext; the GF_DENSITY_LIST phase of csrc/generic_fused*.hip) on top
of tests/occupancy_ref.py: the keep mask of a point list with its outside-the-box rule, the raw rows a culled point gets, the raw tensor after
the density phase over a list, and the grid of a build from the sigmas at the probes.  A plain helper module (not collected)."""
import numpy as np

import occupancy_ref as occ
from generic_two_phase_ref import live_list

f32 = np.float32
CULLED_SIGMA = f32(-1e30)          # NVSR_CULLED_SIGMA


def norm_points(x, lo, rng):
    """[P,3] float32: 2 (x - lo) / range - 1 of the points' positions, one rounding per operation (gen_position without jitter)"""
    x, lo, rng = np.asarray(x, f32)[:, :3], np.asarray(lo, f32)[:3], np.asarray(rng, f32)[:3]
    with np.errstate(invalid="ignore", over="ignore"):
        return (f32(2.0) * (x - lo)) / rng - f32(1.0)


def keep_mask(x, lo, rng, grid, G):
    """bool [P]: a normalised coordinate is NaN, or lies outside the box (|n| > 1; n = +-1 exactly is inside), or the cell's bit is set"""
    n = norm_points(x, lo, rng)
    i, nan = occ.cell_index(n, G)
    with np.errstate(invalid="ignore"):
        outside = (np.abs(n) > f32(1.0)).any(-1)
    return nan | outside | occ.unpack_bits(grid, G)[i]


def culled_raw(before, keep):
    """`before` [P,4] after the keep kernel: a culled row is [+0, +0, +0, CULLED_SIGMA], a kept row is untouched"""
    out = np.array(before, f32, copy=True)
    out[~np.asarray(keep, bool)] = (0.0, 0.0, 0.0, CULLED_SIGMA)
    return out


def kept_list(keep):
    """the ascending kept points: the live list of the mask written as 1.0 / 0.0"""
    return live_list(np.asarray(keep, bool).astype(f32))


def density_list_raw(before, one_phase, index):
    """`before` [P,4] after a density phase on the points `index`: their rows are [+0, +0, +0, sigma] of the one-launch tensor"""
    out = np.array(before, f32, copy=True)
    index = np.asarray(index, np.int64)
    out[index, :3] = 0.0
    out[index, 3] = np.asarray(one_phase, f32)[index, 3]
    return out


def kept_raw(one_phase, keep):
    """the raw tensor of density_field_kept in terms of density_field's (or the one-launch tensor's): culled sigmas replaced"""
    out = np.zeros_like(np.asarray(one_phase, f32))
    out[:, 3] = np.where(np.asarray(keep, bool), np.asarray(one_phase, f32)[:, 3], CULLED_SIGMA)
    return out


def built_grid(sigma, G, K, threshold, rounds):
    """the words of a build from sigma_raw at occupancy_ref.probes(lo, range, G, K)"""
    return occ.pack_bits(occ.dilate(occ.mark(sigma, K, threshold), G, rounds), G)


def central_cells(G, half=0.5):
    """bool [G^3]: the cells whose centre lies in the central part |n| < half of the box along every axis"""
    c = (np.arange(G) + 0.5) / G * 2.0 - 1.0
    inside = np.abs(c) < half
    return (inside[:, None, None] & inside[None, :, None] & inside[None, None, :]).reshape(-1)
