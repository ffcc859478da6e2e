"""GPU tests of the occupancy grid (csrc/occupancy.hip; the density pass over the kept lists in csrc/render3.hip; include/nvsr.h, "Occupancy
grid"), every comparison bit for bit:
  1. the probe kernel against tests/occupancy_ref.py;
  2. the built grid against mark + dilate, in numpy, of torch.ops.nvsr.triplane_decode on those same probes;
  3. the cull kernel's kept lists against the float32 reference;
  4. the occupancy pass against the ORACLE ROUTE: the two-phase pass (nvsr_render_pass3_launch / nvsr_render_pass3_coarse_z_launch) with
     noise = 0 on kept samples and -1e30 on culled ones -- all five outputs and the packed live entries;
  5. with a conservative grid (exactly the cells that hold a sample of sigma_raw > 0 or NaN) the occupancy pass is the plain pass;
  6. the frame entry point against its passes, and against render_rays with all-one and without grids;
  7. the Python layer: build_occupancy, the route taken in validation and ignored in training, stale grids, opcheck, shape errors.
Outputs start as NaN, so an element a route does not write fails the comparison."""
import ctypes as C

import numpy as np
import pytest
import torch

import occupancy_ref as ref
from two_phase_checks import ARITHS, DEV, OUTPUTS, _env, _same, _scene

pytestmark = pytest.mark.gpu

N_RAYS = 4096 + 256 + 37      # one block of the ray order, one full group and a ragged one
NAN_RAY = 7                   # a NaN origin: every sample kept
GROUP = slice(256, 512)       # a group of 256 rays whose every sample lies in one corner cell (cleared in the grids below)
NEAR, FAR = 2.0, 6.0
CULLED = -1e30                # the oracle route's noise on a culled sample: sigma + noise <= 0


@pytest.fixture(scope="module")
def scene(hip):
    """(coarse model, fine model, rays [N_RAYS, 11], lo[3], range[3]) of bench.py's synthetic scene at plane_res = 64"""
    mc, mf, rays = _scene(hip, 11, 72, 72, plane_res=64, n_rays=N_RAYS)
    rays = rays.clone()
    rays[GROUP, 0:3] = 100.0
    rays[GROUP, 3:6] = 1.0
    rays[NAN_RAY, 0] = float("nan")
    _, consts = mf.scene_args()
    return mc, mf, rays.contiguous(), np.array(consts[0:3], np.float32), np.array(consts[5:8], np.float32)


def _random_grid(G, density, seed):
    """a random grid with the far corner cell (where GROUP's samples clamp to) cleared"""
    cells = np.random.default_rng(seed).random(G ** 3) < density
    cells[-1] = False
    return cells


def _to_dev(words):
    return torch.from_numpy(np.ascontiguousarray(words).view(np.int32)).to(DEV)


def _depths(hip, rays, S, mode, seed=0):
    """mode 'read': sorted random depths, some beyond far (points leave the box and clamp) -> (z tensor for the kernels, z for the reference,
    lindisp); 'lin' / 'disp': depths in registers, the reference's from torch.ops.nvsr.coarse_z"""
    N = rays.shape[0]
    if mode == "read":
        g = torch.Generator(device="cpu").manual_seed(seed + S)
        z = torch.sort(NEAR + (1.5 * FAR - NEAR) * torch.rand(N, S, generator=g), dim=1).values.to(DEV).contiguous()
        return z, z, 0
    lindisp = int(mode == "disp")
    return None, torch.ops.nvsr.coarse_z(rays, S, bool(lindisp), None), lindisp


def _cull(hip, model, rays, S, z, lindisp, grid, G):
    capi = hip.capi
    sc, keep = model.native_scene()
    N = rays.shape[0]
    kept = torch.full((N, S), -7, dtype=torch.int32, device=DEV)
    kept_n = torch.full((N,), -7, dtype=torch.int32, device=DEV)
    capi.call("nvsr_internal_occupancy_cull", C.byref(sc), N, S, capi.ptr(rays), capi.ptr(z), lindisp, capi.ptr(grid), G, capi.ptr(kept), capi.ptr(kept_n),
              capi.stream())
    torch.cuda.synchronize()
    return kept.cpu().numpy(), kept_n.cpu().numpy()


def _outputs(N, S):
    nan = float("nan")
    return dict(rgb=torch.full((N, 3), nan, device=DEV), disp=torch.full((N,), nan, device=DEV), acc=torch.full((N,), nan, device=DEV),
                weights=torch.full((N, S), nan, device=DEV), depth=torch.full((N,), nan, device=DEV))


def _live_entries(hip, N):
    t = torch.full((N,), -1, dtype=torch.int32, device=DEV)
    assert hip.capi.lib().nvsr_internal_copy_live_counts(t.data_ptr(), N, hip.capi.stream()) == 0, "the two-phase route did not run"
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _plain_pass(hip, model, rays, S, arith, z, lindisp, noise, white, raw=False, **env):
    """the two-phase pass by the launch symbols (no minimum ray count): -> (outputs, packed live entries [, raw [N, S, 4] of the fused kernel])"""
    capi = hip.capi
    sc, keep = model.native_scene()
    packed = model.packed_decoder()
    N = rays.shape[0]
    out = _outputs(N, S)
    raw_out = torch.full((N, S, 4), float("nan"), device=DEV) if raw else None
    tail = (int(white), capi.ptr(out["rgb"]), capi.ptr(out["disp"]), capi.ptr(out["acc"]), capi.ptr(out["weights"]), capi.ptr(out["depth"]), capi.ptr(raw_out),
            capi.stream())
    with _env(**env):
        if z is not None:
            capi.call("nvsr_render_pass3_launch", capi.ARITHMETIC[arith], C.byref(sc), capi.ptr(packed), N, S, capi.ptr(rays), capi.ptr(z), capi.ptr(noise), *tail)
        else:
            capi.call("nvsr_render_pass3_coarse_z_launch", capi.ARITHMETIC[arith], C.byref(sc), capi.ptr(packed), N, S, capi.ptr(rays), lindisp, capi.ptr(noise), *tail)
        torch.cuda.synchronize()
    if raw:
        return out, raw_out
    return out, _live_entries(hip, N)


def _occ_pass(hip, model, rays, S, arith, z, lindisp, grid, G, white, **env):
    """nvsr_render_pass_occupancy_arith -> (outputs, packed live entries, packed kept entries)"""
    capi = hip.capi
    sc, keep = model.native_scene()
    packed = model.packed_decoder()
    N = rays.shape[0]
    out = _outputs(N, S)
    with _env(**env):
        capi.call("nvsr_render_pass_occupancy_arith", C.byref(sc), capi.ptr(packed), N, S, capi.ptr(rays), capi.ptr(z), lindisp, int(white), capi.ptr(out["rgb"]),
                  capi.ptr(out["disp"]), capi.ptr(out["acc"]), capi.ptr(out["weights"]), capi.ptr(out["depth"]), capi.ptr(grid), G, capi.ARITHMETIC[arith],
                  capi.stream())
        torch.cuda.synchronize()
    t = torch.full((N,), -1, dtype=torch.int32, device=DEV)
    assert capi.lib().nvsr_internal_copy_kept_counts(t.data_ptr(), N, capi.stream()) == 0, "the occupancy route did not run"
    torch.cuda.synchronize()
    return out, _live_entries(hip, N), t.cpu().numpy()


def _assert_same(got, want, what=""):
    for k in OUTPUTS:
        assert _same(got[k], want[k]), "%s differs %s" % (k, what)


def _masked_noise(kept, kept_n, S):
    """noise [N, S]: 0 on the samples of the kernel's own kept lists, CULLED on the others"""
    N = kept.shape[0]
    noise = np.full((N, S), CULLED, np.float32)
    r, k = np.nonzero(np.arange(S)[None, :] < kept_n[:, None])
    noise[r, kept[r, k]] = 0.0
    return torch.from_numpy(noise).to(DEV).contiguous()


# ---- 1. probes ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [1, 5, 16])
@pytest.mark.parametrize("K", [1, 2, 3])
def test_probes_equal_the_reference(hip, scene, G, K):
    mc, mf, rays, lo, rng = scene
    sc, keep = mf.native_scene()
    x = torch.full((G ** 3 * K ** 3, 6), float("nan"), device=DEV)
    hip.capi.call("nvsr_internal_occupancy_probes", C.byref(sc), G, K, hip.capi.ptr(x), hip.capi.stream())
    torch.cuda.synchronize()
    assert np.array_equal(x.cpu().numpy(), ref.probes(lo, rng, G, K))


# ---- 2. build -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("G,K", [(5, 1), (5, 2), (16, 1), (16, 2), (33, 1), (33, 2)])
def test_built_grid_equals_mark_and_dilate_of_the_decoded_probes(hip, scene, G, K, arith):
    mc, mf, rays, lo, rng = scene
    planes, consts = mf.scene_args()
    packed = mf.packed_decoder()
    code = hip.capi.ARITHMETIC[arith]
    x = torch.from_numpy(ref.probes(lo, rng, G, K)).to(DEV)
    sigma = torch.ops.nvsr.triplane_decode(planes, consts, packed, x, code)[:, 3].cpu().numpy()
    assert (sigma > 0).any() and (sigma <= 0).any()
    for threshold in (0.0, float(np.median(sigma))):
        cells = ref.mark(sigma, K, threshold)
        assert 0 < cells.sum() < G ** 3
        for dilate in (0, 1, 2):
            grid = torch.ops.nvsr.occupancy_build(planes, consts, packed, G, K, threshold, dilate, code)
            assert grid.dtype == torch.int32 and grid.shape == (ref.words(G),)
            want = ref.pack_bits(ref.dilate(cells, G, dilate), G)
            assert np.array_equal(grid.cpu().numpy().view(np.uint32), want), (threshold, dilate)
    ones = torch.ops.nvsr.occupancy_build(planes, consts, packed, G, K, float("-inf"), 0, code)
    assert np.array_equal(ones.cpu().numpy().view(np.uint32), ref.pack_bits(np.ones(G ** 3, bool), G))


@pytest.mark.parametrize("arith", ARITHS)
def test_a_nan_texel_marks_its_cells(hip, scene, arith):
    mc, mf, rays, lo, rng = scene
    planes, consts = mf.scene_args()
    planes = [p.clone() for p in planes]
    planes[0][20, 30, :] = float("nan")
    G, K = 16, 2
    code = hip.capi.ARITHMETIC[arith]
    x = torch.from_numpy(ref.probes(lo, rng, G, K)).to(DEV)
    sigma = torch.ops.nvsr.triplane_decode(planes, consts, mf.packed_decoder(), x, code)[:, 3].cpu().numpy()
    # f16x2: the NaN texel reaches sigma_raw and must mark its cells.  bf16x3: the 3-limb decoder's ReLU (a maximum) turns a NaN activation into
    # 0, its sigma_raw stays a number and the NaN case is vacuous in that arithmetic: what is left is grid == reference on the poisoned planes.
    if arith == "f16x2":
        assert np.isnan(sigma).any() and ref.mark(sigma, K, float("inf")).any()
    big = float(np.nanmax(sigma)) + 1.0                   # above every number: only the NaN probes mark
    for threshold in (big, 0.0):
        cells = ref.mark(sigma, K, threshold)
        if threshold == big:
            assert np.array_equal(cells, np.isnan(sigma.reshape(-1, K ** 3)).any(1))
        grid = torch.ops.nvsr.occupancy_build(planes, consts, mf.packed_decoder(), G, K, threshold, 0, code)
        assert np.array_equal(grid.cpu().numpy().view(np.uint32), ref.pack_bits(cells, G))


# ---- 3. cull ------------------------------------------------------------------------------------------------------------------------------
def _grids():
    return [("random", 16, ref.pack_bits(_random_grid(16, 0.3, 5), 16)), ("zero", 16, ref.pack_bits(np.zeros(16 ** 3, bool), 16)),
            ("one", 16, ref.pack_bits(np.ones(16 ** 3, bool), 16)), ("G1 set", 1, np.array([1], np.uint32)), ("G1 clear", 1, np.array([0], np.uint32))]


@pytest.mark.parametrize("S", [1, 8, 24, 70])
@pytest.mark.parametrize("mode", ["read", "lin", "disp"])
def test_kept_lists_equal_the_reference(hip, scene, S, mode):
    mc, mf, rays, lo, rng = scene
    z, z_ref, lindisp = _depths(hip, rays, S, mode)
    rays_np, z_np = rays.cpu().numpy(), z_ref.cpu().numpy()
    for name, G, words in _grids():
        kept, kept_n = _cull(hip, mf, rays, S, z, lindisp, _to_dev(words), G)
        want, want_n = ref.kept_lists(ref.keep_mask(rays_np, z_np, lo, rng, words, G))
        assert np.array_equal(kept_n, want_n), name
        assert np.array_equal(kept, want), name
        assert kept_n[NAN_RAY] == S
        if name in ("zero", "G1 clear"):
            assert kept_n.sum() == S                      # the NaN ray alone
        if name in ("one", "G1 set"):
            assert (kept_n == S).all()
        if name == "random":
            assert (kept_n[GROUP] == 0).all() and 0 < kept_n.sum() < S * N_RAYS


# ---- 4. the pass against the oracle route ---------------------------------------------------------------------------------------------------
def _check_against_oracle(hip, model, rays, S, arith, mode, words, G, white=1, **env):
    z, z_ref, lindisp = _depths(hip, rays, S, mode)
    grid = _to_dev(words)
    kept, kept_n = _cull(hip, model, rays, S, z, lindisp, grid, G)
    noise = _masked_noise(kept, kept_n, S)
    want, want_live = _plain_pass(hip, model, rays, S, arith, z, lindisp, noise, white, **env)
    got, got_live, got_kept = _occ_pass(hip, model, rays, S, arith, z, lindisp, grid, G, white, **env)
    _assert_same(got, want, "(S %d %s %s %r)" % (S, arith, mode, env))
    assert np.array_equal(got_live, want_live)
    assert np.array_equal(np.sort(got_kept >> 12), np.sort(kept_n))      # the kept counts the launch left, as packed entries of the ray order
    return got, kept_n


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("mode", ["read", "lin", "disp"])
@pytest.mark.parametrize("S", [1, 8, 24])
def test_pass_equals_the_oracle_route(hip, scene, S, mode, arith):
    mc, mf, rays, lo, rng = scene
    got, kept_n = _check_against_oracle(hip, mf, rays, S, arith, mode, ref.pack_bits(_random_grid(16, 0.3, 5), 16), 16)
    assert (kept_n[GROUP] == 0).all() and kept_n[NAN_RAY] == S
    assert (got["acc"][GROUP] == 0).all() and (got["rgb"][GROUP] == 1).all() and (got["weights"][GROUP] == 0).all()


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("mode", ["read", "lin"])
@pytest.mark.parametrize("handle", ["NVSR_COLOUR_POINTS", "NVSR_COLOUR_ORDER", "NVSR_COLOUR_GROUP_ORDER"])
def test_pass_equals_the_oracle_route_under_the_handles(hip, scene, handle, mode, arith):
    mc, mf, rays, lo, rng = scene
    _check_against_oracle(hip, mf, rays, 24, arith, mode, ref.pack_bits(_random_grid(16, 0.3, 5), 16), 16, **{handle: "0"})


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("mode", ["read", "lin"])
def test_all_zero_grid_renders_the_background_without_a_colour_step(hip, scene, mode, arith):
    mc, mf, rays, lo, rng = scene
    S = 24
    got, kept_n = _check_against_oracle(hip, mf, rays, S, arith, mode, ref.pack_bits(np.zeros(16 ** 3, bool), 16), 16)
    rest = torch.ones(N_RAYS, dtype=torch.bool, device=DEV)
    rest[NAN_RAY] = False
    assert (got["acc"][rest] == 0).all() and (got["rgb"][rest] == 1).all() and (got["weights"][rest] == 0).all()
    live = _live_entries(hip, N_RAYS) >> 12
    assert np.sort(live)[-2] == 0                         # no ray but the NaN one can have a live sample: no colour step for them
    G = (N_RAYS + 255) // 256
    steps = torch.full((G,), -1, dtype=torch.int32, device=DEV)
    assert hip.capi.lib().nvsr_internal_copy_point_steps(steps.data_ptr(), G, hip.capi.stream()) == 0
    torch.cuda.synchronize()
    assert steps.cpu().numpy().sum() <= 1                 # at most the NaN ray's points: one step of one group


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("mode", ["read", "lin"])
def test_all_one_grid_equals_the_plain_route(hip, scene, mode, arith):
    mc, mf, rays, lo, rng = scene
    S = 24
    z, z_ref, lindisp = _depths(hip, rays, S, mode)
    want, want_live = _plain_pass(hip, mf, rays, S, arith, z, lindisp, None, 1)
    got, got_live, got_kept = _occ_pass(hip, mf, rays, S, arith, z, lindisp, _to_dev(ref.pack_bits(np.ones(16 ** 3, bool), 16)), 16, 1)
    _assert_same(got, want)
    assert np.array_equal(got_live, want_live) and ((got_kept >> 12) == S).all()


def test_two_launches_of_growing_size_without_a_release(hip, scene):
    mc, mf, rays, lo, rng = scene
    words = ref.pack_bits(_random_grid(16, 0.3, 5), 16)
    assert hip.capi.lib().nvsr_release_render_scratch() == 0
    _check_against_oracle(hip, mf, rays[:300].contiguous(), 8, "f16x2", "read", words, 16)
    _check_against_oracle(hip, mf, rays, 24, "f16x2", "read", words, 16)
    _check_against_oracle(hip, mf, rays[:300].contiguous(), 8, "f16x2", "lin", words, 16)


# ---- 5. exactness with a conservative grid --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("mode", ["read", "lin"])
def test_conservative_grid_changes_nothing(hip, scene, mode, arith):
    """the grid that holds exactly the cells with a sample of sigma_raw > 0 (or NaN): every culled sample had w = +0.0 in the plain pass"""
    mc, mf, rays, lo, rng = scene
    S, G = 24, 16
    z, z_ref, lindisp = _depths(hip, rays, S, mode)
    _, raw = _plain_pass(hip, mf, rays, S, arith, z, lindisp, None, 1, raw=True)
    sigma = raw[:, :, 3].cpu().numpy()
    i, nan = ref.cell_index(ref.norm_points(rays.cpu().numpy(), z_ref.cpu().numpy(), lo, rng), G)
    cells = np.zeros(G ** 3, bool)
    with np.errstate(invalid="ignore"):
        dense = ((sigma > 0) | np.isnan(sigma)) & ~nan
    cells[i[dense]] = True
    assert 0 < cells.sum() < G ** 3
    want, want_live = _plain_pass(hip, mf, rays, S, arith, z, lindisp, None, 1)
    got, got_live, got_kept = _occ_pass(hip, mf, rays, S, arith, z, lindisp, _to_dev(ref.pack_bits(cells, G)), G, 1)
    _assert_same(got, want)
    assert np.array_equal(got_live, want_live)
    assert (got_kept >> 12).sum() < S * N_RAYS            # something was culled


# ---- 6. the frame ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def frame(hip):
    N = 65536 + 4096 + 37
    mc, mf, rays = _scene(hip, 12, 270, 270, plane_res=64, n_rays=N)
    return mc, mf, rays


@pytest.mark.parametrize("arith", ARITHS)
def test_frame_equals_its_passes(hip, frame, arith):
    mc, mf, rays = frame
    capi = hip.capi
    N, Nc, Nf, Gc, Gf = rays.shape[0], 8, 16, 16, 12
    code = capi.ARITHMETIC[arith]
    planes, consts = mc.scene_args()
    grid_c = _to_dev(ref.pack_bits(np.random.default_rng(1).random(Gc ** 3) < 0.4, Gc))
    grid_f = _to_dev(ref.pack_bits(np.random.default_rng(2).random(Gf ** 3) < 0.4, Gf))
    got = torch.ops.nvsr.render_rays_occupancy(planes, consts, mc.packed_decoder(), mf.packed_decoder(), rays, Nc, Nf, False, True, None, None, grid_c, Gc,
                                               grid_f, Gf, code)
    rgb_c, disp_c, acc_c, w_c = torch.ops.nvsr.render_pass_occupancy(planes, consts, mc.packed_decoder(), rays, None, Nc, False, True, True, grid_c, Gc, code)
    z_f = torch.full((N, Nc + Nf), float("nan"), device=DEV)
    capi.call("nvsr_importance_resample_rays", N, Nc, Nf, capi.ptr(rays), 0, capi.ptr(w_c), None, capi.ptr(z_f), capi.stream())
    rgb_f, disp_f, acc_f, _ = torch.ops.nvsr.render_pass_occupancy(planes, consts, mf.packed_decoder(), rays, z_f, Nc + Nf, False, True, False, grid_f, Gf, code)
    for g, w in zip(got, (rgb_c, disp_c, acc_c, rgb_f, disp_f, acc_f)):
        assert _same(g, w)
    assert not _same(got[3], torch.ops.nvsr.render_rays(planes, consts, mc.packed_decoder(), mf.packed_decoder(), rays, Nc, Nf, False, True, None, None, None,
                                                        None, code)[3])      # (the random grids do cull)


@pytest.mark.parametrize("arith", ARITHS)
def test_jittered_frame_equals_its_passes(hip, frame, arith):
    """stratified jitter (t_rand given) with both grids: the coarse depths are stored, so the frame is nvsr_coarse_z, the occupancy pass on
    those depths, nvsr_importance_resample on them, the occupancy pass -- the frame driver's branch that test_frame_equals_its_passes
    (depths in registers) does not take"""
    mc, mf, rays = frame
    capi = hip.capi
    N, Nc, Nf, Gc, Gf = rays.shape[0], 8, 16, 16, 12
    code = capi.ARITHMETIC[arith]
    planes, consts = mc.scene_args()
    grid_c = _to_dev(ref.pack_bits(np.random.default_rng(1).random(Gc ** 3) < 0.4, Gc))
    grid_f = _to_dev(ref.pack_bits(np.random.default_rng(2).random(Gf ** 3) < 0.4, Gf))
    t_rand = torch.rand(N, Nc, generator=torch.Generator(device="cpu").manual_seed(9)).to(DEV)
    frame_of = lambda t: torch.ops.nvsr.render_rays_occupancy(planes, consts, mc.packed_decoder(), mf.packed_decoder(), rays, Nc, Nf, False, True, t, None,
                                                              grid_c, Gc, grid_f, Gf, code)
    got = frame_of(t_rand)
    z_c = torch.full((N, Nc), float("nan"), device=DEV)
    capi.call("nvsr_coarse_z", N, Nc, capi.ptr(rays), 0, capi.ptr(t_rand), capi.ptr(z_c), capi.stream())
    rgb_c, disp_c, acc_c, w_c = torch.ops.nvsr.render_pass_occupancy(planes, consts, mc.packed_decoder(), rays, z_c, Nc, False, True, True, grid_c, Gc, code)
    z_f = torch.full((N, Nc + Nf), float("nan"), device=DEV)
    capi.call("nvsr_importance_resample", N, Nc, Nf, capi.ptr(z_c), capi.ptr(w_c), None, capi.ptr(z_f), capi.stream())
    rgb_f, disp_f, acc_f, _ = torch.ops.nvsr.render_pass_occupancy(planes, consts, mf.packed_decoder(), rays, z_f, Nc + Nf, False, True, False, grid_f, Gf, code)
    for g, w in zip(got, (rgb_c, disp_c, acc_c, rgb_f, disp_f, acc_f)):
        assert _same(g, w)
    assert not _same(got[0], frame_of(None)[0])            # (the jitter does move the samples)


@pytest.mark.parametrize("arith", ARITHS)
def test_frame_with_full_or_no_grids_equals_render_rays(hip, frame, arith):
    mc, mf, rays = frame
    Nc, Nf, G = 8, 16, 8
    code = hip.capi.ARITHMETIC[arith]
    planes, consts = mc.scene_args()
    ones = _to_dev(ref.pack_bits(np.ones(G ** 3, bool), G))
    want = torch.ops.nvsr.render_rays(planes, consts, mc.packed_decoder(), mf.packed_decoder(), rays, Nc, Nf, False, True, None, None, None, None, code)
    for gc, gf in ((ones, ones), (None, None), (ones, None), (None, ones)):
        got = torch.ops.nvsr.render_rays_occupancy(planes, consts, mc.packed_decoder(), mf.packed_decoder(), rays, Nc, Nf, False, True, None, None, gc, G, gf, G,
                                                   code)
        for g, w in zip(got, want):
            assert _same(g, w)


# ---- 7. the Python layer ----------------------------------------------------------------------------------------------------------------------
def _kept_hook(hip, N):
    t = torch.full((N,), -1, dtype=torch.int32, device=DEV)
    return hip.capi.lib().nvsr_internal_copy_kept_counts(t.data_ptr(), N, hip.capi.stream())


def test_models_build_use_and_drop_their_grids(hip):
    from bench import make_synthetic_scene, render_options
    nv = hip
    mc, mf, sid, pose = make_synthetic_scene(DEV, plane_res=64, view_res=16, seed=5)
    H = W = 264                                            # 69 696 rays: above capi.fused_min_rays()
    assert H * W >= nv.capi.fused_min_rays()
    focal = 0.5 * W / np.tan(0.5 * 0.6911112)
    ro, rd = nv.nerf_helpers.get_ray_bundle(H, W, focal, pose)
    opts, scfg = render_options(8, 16)
    render = lambda mode: nv.train_utils.run_one_iter_of_nerf(H, W, focal, mc, mf, torch.stack([ro.reshape(-1, 3), rd.reshape(-1, 3)], 0), opts, scene_id=sid,
                                                              mode=mode, scene_config=scfg)
    with torch.no_grad():
        assert mc.occupancy(sid) is None and mf.occupancy(sid) is None
        plain = render("validation")
        torch.cuda.synchronize()
        assert nv.capi.lib().nvsr_release_render_scratch() == 0
        g_c = mc.build_occupancy(sid, resolution=16, probes=2)
        g_f = mf.build_occupancy(sid, resolution=12, probes=1, threshold=0.0, dilate=0)
        assert mc.occupancy(sid) is g_c and mf.occupancy(sid) is g_f and g_c.shape == (ref.words(16),) and g_f.shape == (ref.words(12),)
        assert _kept_hook(nv, H * W) != 0                  # no occupancy launch yet
        got = render("validation")
        torch.cuda.synchronize()
        assert _kept_hook(nv, H * W) == 0, "the validation render did not take the occupancy route"
        # the operator by hand
        rays = nv.train_utils.pack_rays(ro, rd, 2.0, 6.0)
        planes, consts = mc.scene_args()
        code = nv.capi.resolve_decoder_arithmetic(mc.arithmetic)
        hand = torch.ops.nvsr.render_rays_occupancy(planes, consts, mc.packed_decoder(), mf.packed_decoder(), rays, 8, 16, False,
                                                    bool(opts.nerf.validation.white_background), None, None, g_c, 16, g_f, 12, code)
        assert _same(got[0].reshape(-1, 3), hand[0]) and _same(got[3].reshape(-1, 3), hand[3])
        assert not _same(got[3], plain[3])                 # (these grids do cull)
        # training mode ignores the grids
        assert nv.capi.lib().nvsr_release_render_scratch() == 0
        render("train")
        torch.cuda.synchronize()
        assert _kept_hook(nv, H * W) != 0
        # an in-place update of a plane, or of a decoder weight, retires the grid: the frame is the plain one again
        mc.planes_[nv.models.get_plane_name(sid, 0)].mul_(1.0)
        assert mc.occupancy(sid) is None and mf.occupancy(sid) is None      # (the two models of the synthetic scene share their planes)
        mc.build_occupancy(sid, resolution=16)
        mf.build_occupancy(sid, resolution=12, probes=1)
        mf.fc_alpha["0"].bias.add_(0.0)
        assert mf.occupancy(sid) is None and mc.occupancy(sid) is not None  # (a decoder weight: that model's grid alone)
        mc.clear_occupancy(sid)
        again = render("validation")
        torch.cuda.synchronize()
        assert _same(again[0], plain[0]) and _same(again[3], plain[3])
        mc.build_occupancy(sid, resolution=8)
        mc.clear_occupancy(sid)
        assert mc.occupancy(sid) is None
        mc.build_occupancy(sid, resolution=8)
        mc.clear_occupancy()
        assert mc.occupancy(sid) is None


def test_super_resolving_model_keeps_its_grid_when_the_sr_planes_are_remade(hip):
    """the key of a super-resolving model's grid is what the SR planes are made from (SR parameters, LR planes), not the SR output: remaking
    the planes (what the f16 range re-render in 'bf16x3' does) keeps the grid, an in-place update of an SR parameter retires it"""
    from bench import make_synthetic_scene
    mc, mf, sid, pose = make_synthetic_scene(DEV, plane_res=16, view_res=16, seed=6)
    torch.manual_seed(3)
    sr = hip.models.PlanesSR(hip.models.EDSR, 4, 48, 48, {"model": {"hidden_size": 16, "n_blocks": 2}}, "bilinear").to(DEV)
    with torch.no_grad():
        mf.assign_SR_model(sr, SR_viewdir=False)
        mf.assign_LR_planes()
        for m in (mf, sr):
            m.eval()
        planes, _ = mf.scene_args()
        assert planes[0].shape[0] == 64                     # (super-resolved x 4)
        grid = mf.build_occupancy(sid, resolution=8, probes=1)
        assert mf.occupancy(sid) is grid
        sr.clear_SR_planes()                               # the planes are remade at the next use: another tensor, the same scene
        assert mf.occupancy(sid) is grid
        want = torch.ops.nvsr.occupancy_build(*mf.scene_args(), mf.packed_decoder(), 8, 1, 0.0, 1, mf.arith())
        assert torch.equal(grid, want)
        next(iter(sr.inner_model.parameters())).mul_(1.0)
        assert mf.occupancy(sid) is None


# ---- 7. operators and errors ------------------------------------------------------------------------------------------------------------------
def test_opcheck_on_the_three_operators(hip, scene):
    mc, mf, rays, lo, rng = scene
    planes, consts = mf.scene_args()
    packed = mf.packed_decoder()
    G = 8
    grid = _to_dev(ref.pack_bits(_random_grid(G, 0.5, 3), G))
    chk = lambda op, args: torch.library.opcheck(op, args, test_utils=("test_schema", "test_faketensor"))
    chk(torch.ops.nvsr.occupancy_build, (planes, consts, packed, 5, 2, 0.0, 1, 2))
    r = rays[:600].contiguous()
    z = torch.ops.nvsr.coarse_z(r, 8, False, None)
    chk(torch.ops.nvsr.render_pass_occupancy, (planes, consts, packed, r, z, 8, False, True, True, grid, G, 2))
    chk(torch.ops.nvsr.render_pass_occupancy, (planes, consts, packed, r, None, 8, True, True, False, grid, G, 3))
    chk(torch.ops.nvsr.render_rays_occupancy, (planes, consts, mc.packed_decoder(), packed, r, 8, 16, False, True, None, None, grid, G, None, G, 2))


def test_shape_errors_launch_nothing(hip, scene):
    mc, mf, rays, lo, rng = scene
    capi = hip.capi
    lib = capi.lib()
    sc, keep = mf.native_scene()
    packed = mf.packed_decoder()
    SHAPE = 1
    grid = torch.full((ref.words(8),), 0x55555555, dtype=torch.int32, device=DEV)
    ws = torch.empty(max(int(lib.nvsr_occupancy_workspace_floats(8, 2)), 4), device=DEV)
    build = lambda G, K, dilate, arith=2: lib.nvsr_occupancy_build(C.byref(sc), capi.ptr(packed), G, K, 0.0, dilate, arith, capi.ptr(grid), capi.ptr(ws), capi.stream())
    for G, K, dilate in ((0, 2, 1), (513, 2, 1), (8, 0, 1), (8, 5, 1), (8, 2, -1)):
        assert build(G, K, dilate) == SHAPE
    assert build(8, 2, 1, 7) == SHAPE
    assert lib.nvsr_occupancy_words(0) == 0 and lib.nvsr_occupancy_words(513) == 0 and lib.nvsr_occupancy_words(512) == 512 ** 3 // 32
    assert lib.nvsr_occupancy_workspace_floats(8, 0) == 0 and lib.nvsr_occupancy_workspace_floats(8, 5) == 0
    torch.cuda.synchronize()
    assert (grid == 0x55555555).all()                     # nothing was launched
    S = 8
    r = rays[:600].contiguous()
    out = _outputs(600, S)
    occ = lambda G, arith: lib.nvsr_render_pass_occupancy_arith(C.byref(sc), capi.ptr(packed), 600, S, capi.ptr(r), None, 0, 1, capi.ptr(out["rgb"]),
                                                                capi.ptr(out["disp"]), capi.ptr(out["acc"]), capi.ptr(out["weights"]), None, capi.ptr(grid), G,
                                                                arith, capi.stream())
    assert occ(0, 2) == SHAPE and occ(513, 2) == SHAPE and occ(8, 0) == SHAPE and occ(8, 7) == SHAPE
    torch.cuda.synchronize()
    assert all(torch.isnan(v).all() for v in out.values())
    assert occ(8, 2) == 0
    torch.cuda.synchronize()
    assert not torch.isnan(out["acc"][:NAN_RAY]).any()
