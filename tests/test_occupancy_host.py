"""CPU tests of the occupancy grid's reference transcriptions (tests/occupancy_ref.py: what tests/test_occupancy.py holds the kernels of
csrc/occupancy.hip to, bit for bit): the float32 cell formula against float64, dilation, bit packing and the kept lists."""
import numpy as np
import pytest

import occupancy_ref as ref


@pytest.mark.parametrize("G", [1, 5, 16, 33, 128, 512])
def test_cell_formula_agrees_with_float64_away_from_faces(G):
    """c = clamp(floor(((n + 1) * 0.5) * G), 0, G - 1) in float32, one rounding per step, gives the float64 cell for every point at least 1e-4 cell
    widths from a cell face -- no other point is excluded -- and at least 99 % of the drawn points qualify.  (Three roundings of 2^-24
    relative on a value below G = 512 cells: an error below 3 * 512 * 6e-8 = 9.2e-5 cells.)"""
    rng = np.random.default_rng(G)
    n = np.concatenate([rng.uniform(-1.2, 1.2, 200000), rng.uniform(-1.0, -0.99, 20000), rng.uniform(0.99, 1.0, 20000)]).astype(np.float32)
    t = (n.astype(np.float64) + 1.0) * 0.5 * G
    far = np.abs(t - np.round(t)) >= 1e-4
    assert far.mean() >= 0.99
    assert np.array_equal(ref.cell_axis(n, G)[far], ref.cell_axis_f64(n, G)[far])
    c = ref.cell_axis(n, G)
    assert c.min() >= 0 and c.max() <= G - 1


def test_cell_formula_clamps_outside_and_infinite_points():
    n = np.array([-np.inf, -3.0, -1.0, 1.0, 3.0, np.inf], np.float32)
    assert ref.cell_axis(n, 16).tolist() == [0, 0, 0, 15, 15, 15]


@pytest.mark.parametrize("G", [1, 2, 5, 8])
def test_dilation_of_a_single_bit_gives_its_clipped_neighbourhood(G):
    for cell in {(0, 0, 0), (G - 1, G - 1, G - 1), (G // 2, 0, G - 1), (G // 2, G // 2, G // 2)}:
        ix, iy, iz = cell
        v = np.zeros(G ** 3, bool)
        v[(iz * G + iy) * G + ix] = True
        d = ref.dilate(v, G).reshape(G, G, G)
        want = np.zeros((G, G, G), bool)
        want[max(iz - 1, 0):iz + 2, max(iy - 1, 0):iy + 2, max(ix - 1, 0):ix + 2] = True
        assert np.array_equal(d, want)
        n = [min(c + 1, G - 1) - max(c - 1, 0) + 1 for c in cell]
        assert d.sum() == n[0] * n[1] * n[2] <= 27
        d2 = ref.dilate(v, G, rounds=2).reshape(G, G, G)
        want2 = np.zeros((G, G, G), bool)
        want2[max(iz - 2, 0):iz + 3, max(iy - 2, 0):iy + 3, max(ix - 2, 0):ix + 3] = True
        assert np.array_equal(d2, want2)


@pytest.mark.parametrize("G", [1, 5, 16])
def test_full_and_empty_grids_are_fixed_points_of_dilation(G):
    for v in (np.ones(G ** 3, bool), np.zeros(G ** 3, bool)):
        assert np.array_equal(ref.dilate(v, G), v) and np.array_equal(ref.dilate(v, G, rounds=3), v)
    assert np.array_equal(ref.dilate(np.ones(G ** 3, bool), G, rounds=0), np.ones(G ** 3, bool))


def test_padding_bits_of_the_last_word_stay_zero():
    G = 5                                     # 125 bits: 4 words, 3 unused bits
    assert ref.words(G) == 4
    full = ref.pack_bits(np.ones(G ** 3, bool), G)
    assert full.dtype == np.dtype("<u4") and full.tolist() == [0xffffffff] * 3 + [(1 << 29) - 1]
    assert ref.pack_bits(ref.dilate(np.ones(G ** 3, bool), G), G)[-1] == (1 << 29) - 1
    rng = np.random.default_rng(0)
    v = rng.random(G ** 3) < 0.3
    w = ref.pack_bits(v, G)
    assert w[-1] >> 29 == 0
    assert np.array_equal(ref.unpack_bits(w, G), v)
    for i in np.flatnonzero(v)[:10]:          # cell i is bit i & 31 of word i >> 5
        assert (int(w[i >> 5]) >> (i & 31)) & 1
    assert np.array_equal(ref.unpack_bits(w.view(np.int32), G), v)      # (an int32 tensor's view of the words)


def test_mark_sets_a_cell_for_any_probe_above_the_threshold_or_nan():
    K = 2
    s = np.full((4, K ** 3), -1.0, np.float32)
    s[1, 3] = 0.5
    s[2, 7] = np.nan
    s[3, 0] = 0.0                              # not above a threshold of 0
    assert ref.mark(s.reshape(-1), K, 0.0).tolist() == [False, True, True, False]
    assert ref.mark(s.reshape(-1), K, -np.inf).tolist() == [True] * 4


def test_probes_sit_inside_their_cells():
    lo, rng_ = np.array([-1.5, -1.0, 0.25], np.float32), np.array([3.0, 2.0, 0.5], np.float32)
    for G, K in ((1, 1), (5, 2), (4, 3)):
        x = ref.probes(lo, rng_, G, K)
        assert x.shape == (G ** 3 * K ** 3, 6) and x.dtype == np.float32
        assert np.array_equal(x[:, 3:], np.tile(np.array([1, 0, 0], np.float32), (x.shape[0], 1)))
        n = (2.0 * (x[:, :3].astype(np.float64) - lo) / rng_ - 1.0)
        c = ref.cell_axis_f64(n, G)
        cell = np.repeat(np.arange(G ** 3), K ** 3)
        assert np.array_equal((c[:, 2] * G + c[:, 1]) * G + c[:, 0], cell)


@pytest.mark.parametrize("S", [1, 8, 70])
def test_kept_lists_agree_with_a_brute_force_loop(S):
    rng = np.random.default_rng(S)
    N, G = 97, 6
    lo, rg = np.array([-1.0, -1.0, -1.0], np.float32), np.array([2.0, 2.0, 2.0], np.float32)
    rays = np.zeros((N, 11), np.float32)
    rays[:, 0:3] = rng.uniform(-1.5, 1.5, (N, 3))
    rays[:, 3:6] = rng.normal(size=(N, 3))
    rays[5, 0] = np.nan                        # a NaN origin: every sample of the ray is kept
    z = np.sort(rng.uniform(0.0, 2.0, (N, S)).astype(np.float32), 1)
    cells = rng.random(G ** 3) < 0.3
    grid = ref.pack_bits(cells, G)
    keep = ref.keep_mask(rays, z, lo, rg, grid, G)
    kept, kept_n = ref.kept_lists(keep)
    assert kept.shape == (N, S) and kept.dtype == np.int32 and kept_n.dtype == np.int32
    assert kept_n[5] == S and kept[5].tolist() == list(range(S))
    for r in range(N):
        row = []
        for s in range(S):
            p = rays[r, 0:3] + rays[r, 3:6] * z[r, s]
            n = np.float32(2.0) * (p - lo) / rg - np.float32(1.0)
            if np.isnan(n).any():
                row.append(s)
                continue
            c = [min(max(int(np.floor(np.float32(np.float32(np.float32(v + np.float32(1.0)) * np.float32(0.5)) * np.float32(G)))), 0), G - 1) for v in n]
            i = (c[2] * G + c[1]) * G + c[0]
            if (int(grid[i >> 5]) >> (i & 31)) & 1:
                row.append(s)
        assert kept_n[r] == len(row)
        assert kept[r, :len(row)].tolist() == row and (kept[r, len(row):] == -1).all()
    assert 0 < keep.mean() < 1
