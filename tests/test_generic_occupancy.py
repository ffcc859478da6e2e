"""Occupancy grids of the generic decoder geometries (include/nvsr.h, "generic decoder, occupancy grid"): the density phase over an index list
(GF_DENSITY_LIST of csrc/generic_fused*.hip) against the BITS of the one-launch kernel; the keep mask of a point list and the build against
their numpy statements (tests/generic_occupancy_ref.py on tests/occupancy_ref.py); frames through eval_nerf with a grid against frames
assembled from the grid-less operators; routing, staleness, the range flag and the healing; opcheck.
"Equal": test_generic_fused.same -- the same NaN positions and the same bits everywhere else.  No tolerance anywhere."""
import functools
import warnings

import numpy as np
import pytest
import torch

import generic_occupancy_ref as ref
import occupancy_ref as occ
from conftest import load_golden
from test_generic_fused import SHAPES, SID, points, random_model, same
from test_generic_limb import flag_of
from test_generic_two_phase import ARITHS, F16X2, F32, SENTINEL, args_of, bits, fixture_models, one_launch
from test_hip_parity import DEV, N_, T, make_options

pytestmark = pytest.mark.gpu
nv = torch.ops.nvsr
LIST_OP, KEEP_OP, BUILD_OP = "triplane_density_list_generic_fused_arith", "generic_occupancy_keep", "generic_occupancy_build"


def i32(a):
    return torch.as_tensor(np.asarray(a, np.int32), device=DEV)


def density_list(m, x, arith, raw, index, count, noise=None, max_count=-1):
    """the density phase over the list index[:count] on a copy of raw (numpy); index may hold more entries than count"""
    head, tail = args_of(m, x, arith, noise)
    buf = T(raw).contiguous()
    nv.triplane_density_list_generic_fused_arith(buf, *head, i32(index), i32([count]), *tail, max_count)
    return N_(buf)


def check_list(m, x, arith, noise=None, what="", seed=0):
    """sentinel-filled raw, a shuffled list of `count` points followed by further valid, distinct indices the kernel must not read: the listed
    rows are [+0, +0, +0, sigma of the one-launch kernel], every other row keeps its sentinel; then a list with indices outside [0, P), and a
    launch sized below the device count"""
    P = x.shape[0]
    full = one_launch(m, x, arith, noise)
    order = np.random.default_rng(seed).permutation(P).astype(np.int32)
    before = np.full((P, 4), SENTINEL, np.float32)
    for count in sorted({0, 1, 31, 32, 33, P} & set(range(P + 1))):
        got = density_list(m, x, arith, before, order, count, noise)
        assert same(got, ref.density_list_raw(before, full, order[:count])), (what, count)
        assert not bits(got[order[:count], :3]).any(), (what, count)                       # +0.0 bit for bit
        assert (got[order[count:]] == SENTINEL).all(), (what, count)
    if P >= 8:
        wild = np.array([order[0], -1, P, order[1], P + 5, -2 ** 31, 2 ** 31 - 1, order[2]], np.int32)
        got = density_list(m, x, arith, before, wild, wild.size, noise)
        assert same(got, ref.density_list_raw(before, full, order[:3])), what
        got = density_list(m, x, arith, before, order, min(P, 33), noise, max_count=5)
        assert same(got, ref.density_list_raw(before, full, order[:5])), what
    return full


@pytest.mark.parametrize("arith", list(ARITHS))
@pytest.mark.parametrize("case", list(SHAPES))
def test_list_phase_equals_the_one_launch_kernel_on_every_shape(hip, case, arith):
    n_pos, kw = SHAPES[case]
    m, *_ = random_model(hip, 7, n_pos=n_pos, **kw)
    with torch.no_grad():
        full = check_list(m, points(100, seed=11), ARITHS[arith], what=case)
    assert np.isfinite(full).all()


@pytest.mark.parametrize("arith", list(ARITHS))
def test_list_phase_equals_the_one_launch_kernel_on_the_fixture_geometries(hip, arith):
    with torch.no_grad():
        for name, m, x, noise in fixture_models(hip):
            check_list(m, x, ARITHS[arith], noise, name)


# ---- the keep mask --------------------------------------------------------------------------------------------------------------------------
LO, RNG = np.float32([-4.0, -3.0, -2.5, -np.pi, -np.pi / 2]), np.float32([8.0, 6.0, 5.0, 2 * np.pi, np.pi])
CONSTS = [float(v) for v in LO] + [float(v) for v in RNG] + [0.0] * 18


def keep_points(P, seed):
    """points in and around the box (1.3 x its size: about half of them outside); every fifth of the first rows a special one: on the faces
    (n = +-1 exactly), just beyond a face, NaN and infinite coordinates"""
    rng = np.random.default_rng(seed)
    x = np.concatenate([(LO[:3] + RNG[:3] / 2) + rng.uniform(-0.65, 0.65, (P, 3)) * RNG[:3], rng.standard_normal((P, 3))], 1).astype(np.float32)
    hi = LO[:3] + RNG[:3]
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    special = [(hi[0], LO[1], hi[2]), (LO[0], hi[1], LO[2]), (hi[0] * np.float32(1.0001), 0, 0), (0, LO[1] * np.float32(1.0001), 0), (nan, 0, 0),
               (0, 0, nan), (inf, 0, 0), (0, -inf, 0), (nan, inf, -inf), (LO[0], 0, 0), (0, 0, hi[2])]
    for k, s in enumerate(special):
        if 5 * k < P:
            x[5 * k, :3] = s
    return x


@pytest.mark.parametrize("P", [1, 63, 64, 65, 2049])
@pytest.mark.parametrize("G", [1, 5, 8])
def test_keep_mask_is_the_numpy_statement(hip, G, P):
    x = keep_points(P, seed=P + G)
    n = ref.norm_points(x, LO, RNG)
    assert (n[0] == (1, -1, 1)).all() and (P < 6 or (n[5] == (-1, 1, -1)).all())          # the face points are on n = +-1 exactly
    xd = T(x)
    before = np.full((P, 4), SENTINEL, np.float32)
    rng = np.random.default_rng(G)
    grids = [np.uint32([0]), np.uint32([1])] if G == 1 else [rng.integers(0, 2 ** 32, occ.words(G), dtype=np.uint64).astype(np.uint32)
                                                             for _ in range(2)]
    seen = set()
    for words in grids:                      # (random words: the padding bits of the last word are set at random too, and must not matter)
        want = ref.keep_mask(x, LO, RNG, words, G)
        seen |= set(want.tolist())
        keep, raw = nv.generic_occupancy_keep(CONSTS, xd, T(words.view(np.int32)), G, T(before))
        assert keep.dtype == torch.float32 and tuple(keep.shape) == (P,) and tuple(raw.shape) == (P, 4)
        assert np.array_equal(N_(keep), want.astype(np.float32))
        assert same(N_(raw), ref.culled_raw(before, want))                                  # kept rows keep their sentinel
        assert not bits(N_(raw)[~want, :3]).any()
        index, count = nv.generic_live_list(keep)
        kept = ref.kept_list(want)
        assert int(count.item()) == kept.size and np.array_equal(N_(index)[:kept.size], kept)
        assert want[0] == bool(ref.keep_mask(x[:1], LO, RNG, words, G)[0])
    assert P < 63 or seen == {True, False}
    # the face point goes by its cell, not by the outside rule: with no bit set it is culled, a point just beyond the face is kept
    none = np.zeros(occ.words(G), np.uint32)
    want = ref.keep_mask(x, LO, RNG, none, G)
    assert not want[0] and (P < 16 or (n[10, 0] > 1 and n[15, 1] < -1 and want[10] and want[15]))
    keep, _ = nv.generic_occupancy_keep(CONSTS, xd, T(none.view(np.int32)), G)
    assert np.array_equal(N_(keep), want.astype(np.float32))


# ---- the build ------------------------------------------------------------------------------------------------------------------------------
BUILD_MODELS = {
    "hidden32": (3, dict(dec_channels=32, proj_combination="avg", viewdir_proj_combination="concat_pos", skip_connect_every=2)),
    "hidden64-planes5": (5, dict(dec_channels=64, proj_combination="avg", viewdir_proj_combination="concat_pos")),
    "hidden64-bicubic": (3, dict(dec_channels=64, proj_combination="sum", viewdir_proj_combination="concat_pos", plane_interp="bicubic")),
}
BUILD_SHAPES = [("hidden32", 5, 1, 0), ("hidden32", 8, 2, 1), ("hidden32", 40, 4, 0), ("hidden64-planes5", 8, 2, 2), ("hidden64-planes5", 5, 1, 0),
                ("hidden64-bicubic", 8, 2, 1), ("hidden64-bicubic", 8, 2, 2)]


@functools.lru_cache(maxsize=2)
def probes_of(G, K):
    box = np.float32([-4.0] * 3), np.float32([8.0] * 3)
    return occ.probes(box[0], box[1], G, K)


def box_of(m):
    consts = m.scene_args(check_native=False)[1]
    return np.float32(consts[0:3]), np.float32(consts[5:8])


@pytest.mark.parametrize("arith", list(ARITHS))
@pytest.mark.parametrize("model,G,K,rounds", BUILD_SHAPES)
def test_build_is_pack_dilate_mark_of_the_density_field_at_the_probes(hip, monkeypatch, model, G, K, rounds, arith):
    """the grid of build_occupancy == pack_bits(dilate(mark(sigma))) with sigma = density_field at occupancy_ref.probes; the threshold is the
    median over the cells of their largest sigma, so that about half the cells are marked before the dilation.  (5, 1, 0): 125 bits, the
    three padding bits of the last word are 0; (40, 4, 0): 4 096 000 probes, two slabs of the build"""
    monkeypatch.setenv("NVSR_GENERIC_FUSED", "1")
    n_pos, kw = BUILD_MODELS[model]
    m, *_ = random_model(hip, 31, n_pos=n_pos, **kw)
    m.arithmetic = None if arith == "f32" else "f16x2"
    x = probes_of(G, K)
    with torch.no_grad():
        assert m.generic_arithmetic() == arith
        lo, rng = box_of(m)
        assert np.array_equal(lo, np.float32([-4] * 3)) and np.array_equal(rng, np.float32([8] * 3))
        sigma = N_(m.density_field(T(x)))[:, 3]
    assert np.isfinite(sigma).all()
    threshold = float(np.median(sigma.reshape(-1, K ** 3).max(1)))
    marked = occ.mark(sigma, K, threshold)
    assert 0.25 < marked.mean() < 0.75
    want = ref.built_grid(sigma, G, K, threshold, rounds)
    assert rounds == 0 or occ.unpack_bits(want, G).sum() > marked.sum()                     # the dilation has something to do
    grid = m.build_occupancy(SID, resolution=G, probes=K, threshold=threshold, dilate=rounds)
    assert grid.dtype == torch.int32 and grid.numel() == occ.words(G)
    assert np.array_equal(N_(grid).view(np.uint32), want)
    assert m.occupancy(SID) is grid and m.occupancy_entry(SID) == (grid, G)
    if G ** 3 % 32:
        assert int(N_(grid).view(np.uint32)[-1]) >> (G ** 3 % 32) == 0
    if (G, K, rounds) == (8, 2, 1):
        # a NaN texel sets the cells it reaches -- and with the threshold at +inf only those.  'f16x2' carries the NaN to sigma (its ReLU keeps
        # NaN); the f32 kernels' fmaxf(., 0) answers 0 to a NaN activation, like the layered route whose bits they have: there the texel sets
        # nothing, and a NaN in fc_alpha's weights -- behind the last ReLU -- sets every cell
        with torch.no_grad():
            m.planes_[hip.models.get_plane_name(SID, 0)][0, 3, 4, 5] = float("nan")
            assert m.occupancy(SID) is None                                                  # stale: dropped
            sigma = N_(m.density_field(T(x)))[:, 3]
        want = ref.built_grid(sigma, G, K, np.inf, 0)
        if arith == "f16x2":
            assert 0 < occ.unpack_bits(want, G).sum() < G ** 3 and np.isnan(sigma).any()
        grid = m.build_occupancy(SID, resolution=G, probes=K, threshold=float("inf"), dilate=0)
        assert np.array_equal(N_(grid).view(np.uint32), want)
        if arith == "f32":
            with torch.no_grad():
                m.fc_alpha["0"].weight[0, 0] = float("nan")
                assert np.isnan(N_(m.density_field(T(x)))[:, 3]).all()
            grid = m.build_occupancy(SID, resolution=G, probes=K, threshold=float("inf"), dilate=0)
            assert np.array_equal(N_(grid).view(np.uint32), occ.pack_bits(np.ones(G ** 3, bool), G))


# ---- frames ---------------------------------------------------------------------------------------------------------------------------------
FRAME_MODELS = {
    "hidden64-avg-concat_pos": dict(dec_channels=64, proj_combination="avg", viewdir_proj_combination="concat_pos", skip_connect_every=3),
    "hidden128-sum": dict(dec_channels=128, proj_combination="sum", viewdir_proj_combination="concat_pos"),
}
HW, NC, NF = 32, 16, 16
FOV = 1.4             # wide enough that the frame's rays do not all cross the centre of the box (kept shares: see numpy_coarse_share)


def camera():
    pose = load_golden("g18_decoder_variants.npz")["pose"]
    return pose, 0.5 * HW / np.tan(0.5 * FOV)


def numpy_coarse_points():
    """the coarse pass's sample points of the frame, in numpy alone: get_ray_bundle's pinhole rays, 16 depths from 2 to 6"""
    pose, focal = camera()
    j, i = np.meshgrid(np.arange(HW), np.arange(HW), indexing="ij")
    dirs = np.stack([(i - HW * 0.5) / focal, -(j - HW * 0.5) / focal, -np.ones_like(i, float)], -1)
    rd = (dirs[..., None, :] * pose[:3, :3]).sum(-1).reshape(-1, 3)
    z = np.linspace(2.0, 6.0, NC)
    return (pose[:3, 3] + rd[:, None, :] * z[None, :, None]).reshape(-1, 3).astype(np.float32)


def counted(monkeypatch):
    calls = {}
    for name in (LIST_OP, KEEP_OP, "triplane_density_generic_fused_arith", "triplane_colour_generic_fused_arith", "generic_live_list",
                 "triplane_decode_generic_fused_arith", "triplane_decode_generic_fused", "triplane_decode_generic"):
        def hook(*a, _op=getattr(nv, name), _name=name, **k):
            calls[_name] = calls.get(_name, 0) + 1
            return _op(*a, **k)
        monkeypatch.setattr(nv, name, hook)
    return calls


class Scene:
    """a seeded coarse / fine pair on shared planes, the frame's rays, and the frame through eval_nerf"""

    def __init__(self, hip, monkeypatch, model, arith, seed=51):
        monkeypatch.setenv("NVSR_GENERIC_FUSED", "1")
        monkeypatch.setenv("NVSR_GENERIC_TWO_PHASE", "1")
        self.hip, kw = hip, FRAME_MODELS[model]
        self.mc, *_ = random_model(hip, seed, **kw)
        self.mf, *_ = random_model(hip, seed + 1, **kw)
        self.mf.planes_ = self.mc.planes_
        self.mc.arithmetic = self.mf.arithmetic = None if arith == "f32" else "f16x2"
        pose, self.focal = camera()
        self.pose = T(pose)
        self.opts, self.scfg = make_options(NC, NF)
        with torch.no_grad():
            self.ro, self.rd = hip.nerf_helpers.get_ray_bundle(HW, HW, self.focal, self.pose)
            self.rays = hip.train_utils.pack_rays(self.ro.reshape(-1, 3), self.rd.reshape(-1, 3), 2.0, 6.0, HW, HW, self.focal, no_ndc=True)
        self.N = self.rays.shape[0]
        self.lo, self.rng = box_of(self.mc)

    models = property(lambda self: (self.mc, self.mf))

    def shift_bias(self, live_share):
        """fc_alpha's bias of either model moved so that `live_share` of its sigmas at the coarse pass's points are positive"""
        with torch.no_grad():
            pts = nv.ray_points(self.rays, nv.coarse_z(self.rays, NC, False, None))
            for m in self.models:
                sigma = N_(m.density_field(pts))[:, 3].astype(np.float64)
                dict(m.named_parameters())["fc_alpha.0.bias"].add_(float(-np.quantile(sigma, 1.0 - live_share)))

    def frame(self):
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            with torch.no_grad():
                out = self.hip.train_utils.eval_nerf(HW, HW, self.focal, self.mc, self.mf, self.ro, self.rd, self.opts, scene_id=SID,
                                                     scene_config=self.scfg)
        return [N_(t) for t in out if torch.is_tensor(t)]

    def install(self, cells, G):
        """build a grid for either model, then overwrite its words with the hand-made cells: the stored tensor is the one returned"""
        words = T(occ.pack_bits(cells, G).view(np.int32))
        for m in self.models:
            m.build_occupancy(SID, resolution=G, probes=1, threshold=0.0, dilate=0).copy_(words)
            assert m.occupancy_entry(SID) is not None
        return N_(words).view(np.uint32)

    def clear(self):
        for m in self.models:
            m.clear_occupancy()

    def by_hand(self, grid, G):
        """the frame assembled from the grid-less operators: density_field with the culled samples' sigma replaced by CULLED_SIGMA (the keep
        mask in numpy), the weights, their live list, colour_field_, the compositor -> (rgb_c, rgb_f, kept share per pass); along the way
        density_field_kept is held to the same raw tensor and the numpy kept count"""
        shares, rgb = [], []
        with torch.no_grad():
            z = nv.coarse_z(self.rays, NC, False, None)
            for m, fine in ((self.mc, False), (self.mf, True)):
                if fine:
                    z = nv.importance_resample(z, w, NF, None)
                S = z.shape[1]
                pts = nv.ray_points(self.rays, z)
                keep = ref.keep_mask(N_(pts), self.lo, self.rng, grid, G)
                shares.append(float(keep.mean()))
                raw = T(ref.kept_raw(N_(m.density_field(pts)), keep))
                got, index, count = m.density_field_kept(pts, T(grid.view(np.int32)), G)
                assert int(count.item()) == int(keep.sum()) and np.array_equal(N_(index)[:int(keep.sum())], ref.kept_list(keep))
                assert same(N_(got), N_(raw))
                wd = nv.composite_rays(raw.reshape(self.N, S, 4), z, self.rays, None, False, True)[3]
                index, count = nv.generic_live_list(wd)
                done = m.colour_field_(raw, pts, index, count)
                out = nv.composite_rays(done.reshape(self.N, S, 4), z, self.rays, None, False, True)
                w = out[3]
                rgb.append(N_(out[0]))
        return rgb[0], rgb[1], shares


def numpy_coarse_share(cells, G):
    x = numpy_coarse_points()
    box = np.float32([-4.0] * 3), np.float32([8.0] * 3)
    return float(ref.keep_mask(x, box[0], box[1], occ.pack_bits(cells, G), G).mean())


@pytest.mark.parametrize("arith", list(ARITHS))
@pytest.mark.parametrize("model", list(FRAME_MODELS))
def test_frame_with_a_full_grid_and_with_a_hand_made_grid(hip, monkeypatch, model, arith):
    """32 x 32 rays, 16 + 16 samples through eval_nerf.  (a) a grid with every bit set (threshold -inf) gives the grid-less two-phase frame.
    (b) the cells whose centre lies in the central half of the box (G = 8): the frame equals the one assembled from density_field with the
    culled samples' sigma replaced by CULLED_SIGMA; kept shares of both passes within [0.1, 0.9].  The coarse pass's share is checked in
    numpy alone, from pinhole rays restated here, before the GPU is involved.  The fine pass's sample points depend on the coarse pass's
    weights, so its share can only be checked afterwards: in numpy, from the points the frame's operators produced"""
    G = 8
    cells = ref.central_cells(G)
    share = numpy_coarse_share(cells, G)
    assert 0.1 <= share <= 0.9, share
    s = Scene(hip, monkeypatch, model, arith)
    s.shift_bias(1.0 / 3)
    calls = counted(monkeypatch)
    plain = s.frame()
    assert LIST_OP not in calls and calls["triplane_density_generic_fused_arith"] == 2
    assert len(plain) >= 2 and all(np.isfinite(t).all() for t in plain)
    # (a)
    for m in s.models:
        g = m.build_occupancy(SID, resolution=G, probes=1, threshold=float("-inf"), dilate=0)
        assert np.array_equal(occ.unpack_bits(N_(g), G), np.ones(G ** 3, bool))
    calls.clear()
    full = s.frame()
    assert calls[LIST_OP] == 2 and calls[KEEP_OP] == 2 and "triplane_density_generic_fused_arith" not in calls, calls
    assert len(full) == len(plain) and all(same(a, b) for a, b in zip(full, plain))
    # (b)
    grid = s.install(cells, G)
    calls.clear()
    culled = s.frame()
    assert calls[LIST_OP] == 2 and calls["triplane_colour_generic_fused_arith"] == 2 and calls["generic_live_list"] == 4, calls
    rgb_c, rgb_f, shares = s.by_hand(grid, G)
    print("%s %s: kept shares %.3f (numpy rays %.3f) coarse, %.3f fine" % (model, arith, shares[0], share, shares[1]))
    assert all(0.1 <= v <= 0.9 for v in shares), shares
    assert same(culled[0].reshape(-1, 3), rgb_c) and same(culled[1].reshape(-1, 3), rgb_f)
    assert not same(culled[1], plain[1])                                                    # the grid cuts density the plain frame sees


@pytest.mark.parametrize("arith", list(ARITHS))
@pytest.mark.parametrize("model", list(FRAME_MODELS))
def test_frame_of_a_scene_whose_culled_samples_are_empty_equals_the_plain_frame(hip, monkeypatch, model, arith):
    """(c) position plane 0 is zero outside its texels 4 .. 5 (three times a seeded plane there, so that an 'avg' of three planes sees the
    plane's own size) and the other two position planes are zero -- three planes with a central block each would leave three bars through
    the whole box, which this frame's rays, all aimed at the centre, hardly leave (kept share 0.84 in numpy).  fc_alpha's weights are negated
    where the seeded decoder answers the plane with less density, and its bias puts the empty space's sigma at -q, q = the median of what
    the plane adds to sigma at the coarse samples it reaches; the grid is built with G = 16, K = 4, threshold -0.9 q (just above the empty
    space's sigma: whatever the plane lifts is marked), dilate = 1.  Premise, asserted from the grid-less density_field: every culled sample has sigma_raw <= 0.  Then the frame with the grid
    is the grid-less frame, every returned tensor.  Kept shares: the coarse pass's is checked in numpy alone first, from the cells the plane's
    support overlaps; both passes' are then asserted in numpy from the built grids and the frame's own sample points (the fine pass's only
    exist once the coarse pass has run)"""
    G = 16
    tex = -1 + 2 * np.arange(10) / 9
    c = (np.arange(G) + 0.5) / G * 2 - 1
    reach = (c + 1.0 / G > tex[3]) & (c - 1.0 / G < tex[6])             # cells the bilinear support of texels 4 .. 5 overlaps, per axis
    bar = np.broadcast_to(reach[None, :, None] & reach[:, None, None], (G, G, G)).reshape(-1)       # plane 0: axes y, z
    share = numpy_coarse_share(occ.dilate(bar, G, 1), G)
    assert 0.1 <= share <= 0.9, share
    s = Scene(hip, monkeypatch, model, arith, seed=61)
    with torch.no_grad():
        for d in range(3):
            p = s.mc.planes_[hip.models.get_plane_name(SID, d)]
            mask = torch.zeros_like(p)
            if d == 0:
                mask[:, :, 4:6, 4:6] = 1.0
            p.mul_(mask * 3.0)
        far = T(np.float32([[3.5, 3.5, 3.5, 1, 0, 0]]))
        pts = nv.ray_points(s.rays, nv.coarse_z(s.rays, NC, False, None))
        n = ref.norm_points(N_(pts), s.lo, s.rng)
        reached = (np.abs(n[:, 1]) < tex[6]) & (np.abs(n[:, 2]) < tex[6])
        thresholds = []
        lift_of = lambda m: N_(m.density_field(pts))[reached, 3].astype(np.float64) - float(m.density_field(far)[0, 3])
        for m in s.models:
            if np.median(lift_of(m)) < 0:                                  # a seeded decoder may as well answer the plane with LESS density
                m.fc_alpha["0"].weight.neg_()
            q = float(np.median(lift_of(m)))
            assert q > 0.01, q
            m.fc_alpha["0"].bias.add_(-float(m.density_field(far)[0, 3]) - q)
            assert abs(float(m.density_field(far)[0, 3]) + q) < 1e-3 * max(1.0, q)
            thresholds.append(-0.9 * q)
    calls = counted(monkeypatch)
    plain = s.frame()
    assert LIST_OP not in calls
    grids = [N_(m.build_occupancy(SID, resolution=G, probes=4, threshold=t, dilate=1)).view(np.uint32) for m, t in zip(s.models, thresholds)]
    calls.clear()
    culled = s.frame()
    assert calls[LIST_OP] == 2, calls
    # the premise and the shares, pass by pass from the grid-less operators
    with torch.no_grad():
        monkeypatch.setenv("NVSR_GENERIC_TWO_PHASE", "0")
        z = nv.coarse_z(s.rays, NC, False, None)
        for m, grid, fine in ((s.mc, grids[0], False), (s.mf, grids[1], True)):
            if fine:
                z = nv.importance_resample(z, w, NF, None)
            pts = nv.ray_points(s.rays, z)
            sigma = N_(m.density_field(pts))[:, 3]
            keep = ref.keep_mask(N_(pts), s.lo, s.rng, grid, G)
            print("%s %s %s: kept share %.3f, positive sigma %.3f" % (model, arith, "fine" if fine else "coarse", keep.mean(), (sigma > 0).mean()))
            assert 0.1 <= keep.mean() <= 0.9, keep.mean()
            assert (sigma[~keep] <= 0).all()                                                # the premise
            assert (sigma > 0).mean() > 0.02                                                # and something to render
            w = nv.composite_rays(m(pts).reshape(s.N, z.shape[1], 4), z, s.rays, None, False, True)[3]
    assert len(culled) == len(plain) >= 2 and all(same(a, b) for a, b in zip(culled, plain))
    assert np.isfinite(plain[1]).all() and plain[1].std() > 0


# ---- routing, staleness, the range flag -----------------------------------------------------------------------------------------------------
def test_routing_and_staleness(hip, monkeypatch):
    """a grid is used while it is current: an in-place change of a plane or of a decoder weight drops it, and the next frame is the grid-less
    one.  NVSR_GENERIC_TWO_PHASE=0, gradients, a noise tensor and a jitter each decline the route; a model without a grid launches what it
    launched before"""
    G = 8
    cells = ref.central_cells(G)
    s = Scene(hip, monkeypatch, "hidden64-avg-concat_pos", "f32")
    s.shift_bias(1.0 / 3)
    calls = counted(monkeypatch)
    plain = s.frame()
    assert set(calls) == {"triplane_density_generic_fused_arith", "generic_live_list", "triplane_colour_generic_fused_arith"}

    def with_grid():
        s.install(cells, G)
        calls.clear()
        out = s.frame()
        assert calls[LIST_OP] == 2, calls
        assert not same(out[1], plain[1])
        return out

    culled = with_grid()
    # staleness: the values stay, the versions move
    for touch in (lambda: s.mc.planes_[hip.models.get_plane_name(SID, 1)].add_(0.0),                   # (the planes are shared)
                  lambda: [m.density_dec["0"][1].weight.mul_(1.0) for m in s.models], lambda: [m.fc_alpha["0"].bias.add_(0.0) for m in s.models]):
        with_grid()
        with torch.no_grad():
            touch()
        calls.clear()
        out = s.frame()
        assert all(same(a, b) for a, b in zip(out, plain))
        assert LIST_OP not in calls and s.mc.occupancy(SID) is None and s.mf.occupancy(SID) is None
    s.clear()
    # each model its own grid: the fine model alone
    s.mf.build_occupancy(SID, resolution=G, probes=1, threshold=0.0, dilate=0).copy_(T(occ.pack_bits(cells, G).view(np.int32)))
    calls.clear()
    out = s.frame()
    assert calls[LIST_OP] == 1 and calls["triplane_density_generic_fused_arith"] == 1 and same(out[0], plain[0]) and not same(out[1], plain[1])
    # the switch
    with_grid()
    monkeypatch.setenv("NVSR_GENERIC_TWO_PHASE", "0")
    calls.clear()
    assert all(same(a, b) for a, b in zip(s.frame(), plain)) and set(calls) == {"triplane_decode_generic_fused"}
    monkeypatch.delenv("NVSR_GENERIC_TWO_PHASE")           # unset: a built grid selects the route whatever the measured default says
    for m in s.models:
        monkeypatch.setattr(m, "GENERIC_TWO_PHASE_DEFAULT_HIDDEN", {"f32": None, "f16x2": None}, raising=False)
        assert m.generic_frame_route() == "one_phase"
    calls.clear()
    assert all(same(a, b) for a, b in zip(s.frame(), culled)) and calls[LIST_OP] == 2
    monkeypatch.setenv("NVSR_GENERIC_TWO_PHASE", "1")
    # gradients on (the parameters take them): the layered route, no grid
    calls.clear()
    out = hip.train_utils.eval_nerf(HW, HW, s.focal, s.mc, s.mf, s.ro, s.rd, s.opts, scene_id=SID, scene_config=s.scfg)
    assert set(calls) == {"triplane_decode_generic"} and all(same(N_(a.detach()), b) for a, b in zip([t for t in out if torch.is_tensor(t)], plain))
    # a noise tensor, a jitter (zeros: the values of the plain frame)
    render = hip.train_utils.predict_and_render_radiance
    with torch.no_grad():
        calls.clear()
        base = render(s.rays, s.mc, s.mf, s.opts, SID, mode="validation", randoms={})
        assert calls[LIST_OP] == 2
        for randoms in (dict(noise_coarse=torch.zeros(s.N, NC), noise_fine=torch.zeros(s.N, NC + NF)),
                        dict(jitter_coarse=torch.zeros(s.N * NC, 3), jitter_fine=torch.zeros(s.N * (NC + NF), 3))):
            calls.clear()
            out = render(s.rays, s.mc, s.mf, s.opts, SID, mode="validation", randoms=randoms)
            assert LIST_OP not in calls and KEEP_OP not in calls, (list(randoms), calls)
            assert same(N_(out[3]), plain[1].reshape(-1, 3)) and not same(N_(out[3]), N_(base[3]))
        # one of the two alone declines its own pass only
        calls.clear()
        out = render(s.rays, s.mc, s.mf, s.opts, SID, mode="validation", randoms=dict(noise_fine=torch.zeros(s.N, NC + NF)))
        assert calls[LIST_OP] == 1 and same(N_(out[0]), N_(base[0]))
    assert s.mc.occupancy(SID) is not None and s.mf.occupancy(SID) is not None


def test_range_flag_follows_the_list_and_the_frame_heals_with_its_grid(hip, monkeypatch):
    """'f16x2': a position-plane texel beyond the range raises bit 1 in the list phase exactly when a point on the texel is listed.  A frame whose
    density decoder overflows in a hidden activation inside kept cells heals through the f32 route as before, warned once -- and the healing
    frame keeps using the grid: the bits of arithmetic=None with the same grid"""
    from test_generic_limb import range_model
    m, sd, planes, kw, x = range_model(hip)
    P = x.shape[0]
    before = np.full((P, 4), SENTINEL, np.float32)
    with torch.no_grad():
        everyone = np.arange(P, dtype=np.int32)
        _, raised = flag_of(hip, lambda: density_list(m, x, F16X2, before, everyone, P))
        assert raised == 0
        m.planes_[hip.models.get_plane_name(SID, 0)][0, 3, 4, 5] = 20000.0
        full = one_launch(m, x, F16X2)
        got, raised = flag_of(hip, lambda: density_list(m, x, F16X2, before, everyone, P))
        assert raised & 1 and np.isnan(got[:6, 3]).all() and same(got, ref.density_list_raw(before, full, everyone))
        clean = np.flatnonzero(np.isfinite(full[:, 3])).astype(np.int32)
        assert 100 < clean.size < P
        _, raised = flag_of(hip, lambda: density_list(m, x, F16X2, before, clean, clean.size))
        assert raised == 0
        _, raised = flag_of(hip, lambda: density_list(m, x, F16X2, before, np.concatenate([clean[:40], [2]]).astype(np.int32), 41))
        assert raised & 1
        _, raised = flag_of(hip, lambda: density_list(m, x, F16X2, before, np.concatenate([clean[:40], [2]]).astype(np.int32), 40))
        assert raised == 0                      # the entry beyond the count is not read
    # the frame
    G = 8
    cells = ref.central_cells(G)
    s = Scene(hip, monkeypatch, "hidden64-avg-concat_pos", "f16x2")
    s.shift_bias(1.0 / 3)
    calls = counted(monkeypatch)

    def frame(arithmetic, healing=False):
        s.mc.arithmetic = s.mf.arithmetic = arithmetic
        calls.clear()
        with torch.no_grad():
            if healing:
                with pytest.warns(UserWarning, match="range"):
                    out = hip.train_utils.eval_nerf(HW, HW, s.focal, s.mc, s.mf, s.ro, s.rd, s.opts, scene_id=SID, scene_config=s.scfg)
                return [N_(t) for t in out if torch.is_tensor(t)]
        return s.frame()

    s.install(cells, G)
    fine = frame("f16x2")
    assert calls[LIST_OP] == 2
    with torch.no_grad():
        s.mf.density_dec["0"][0].bias[11] = 5000.0
    assert s.mf.occupancy(SID) is None
    s.mf.arithmetic = None
    s.install(cells, G)
    plain = frame(None)
    assert calls[LIST_OP] == 2
    healed = frame("f16x2", healing=True)
    assert calls[LIST_OP] == 4, calls                                                      # the limb frame, then the f32 frame: both with the grid
    assert all(same(a, b) for a, b in zip(healed, plain)) and np.isfinite(healed[1]).all() and not same(healed[1], fine[1])
    again = frame("f16x2")
    assert calls[LIST_OP] == 2 and all(same(a, b) for a, b in zip(again, plain))


def test_opcheck(hip):
    m, *_ = random_model(hip, 3, dec_channels=64, proj_combination="avg", viewdir_proj_combination="concat_pos", skip_connect_every=3)
    tests = ("test_schema", "test_faketensor", "test_autograd_registration")
    x = points(50)
    with torch.no_grad():
        for arith in (F32, F16X2):
            head, tail = args_of(m, x, arith)
            build = head[:5] + (5, 1, 0.0, 1, tail[0], tail[2], arith)
            torch.library.opcheck(nv.generic_occupancy_build, build, test_utils=tests)
            grid = nv.generic_occupancy_build(*build)
            before = torch.full((50, 4), SENTINEL, device=DEV)
            torch.library.opcheck(nv.generic_occupancy_keep, (head[1], head[5], grid, 5, before), test_utils=tests)
            keep, raw = nv.generic_occupancy_keep(head[1], head[5], grid, 5, before)
            assert (before == SENTINEL).all()                                               # the operator works on a copy
            index, count = nv.generic_live_list(keep)
            torch.library.opcheck(nv.triplane_density_list_generic_fused_arith, (raw,) + head + (index, count) + tail, test_utils=tests)
    for name in (BUILD_OP, KEEP_OP, LIST_OP):
        assert name in hip.ops.FORWARD_OPS
