"""GPU tests (-m gpu) of the density kernels' resident weights (csrc/render3.hip, PHASE 1 and PHASE 4 with two f16 limbs; csrc/pair_core.h,
Lds3: the density plan).  The density pass keeps the first nine K-blocks of the density decoder in LDS for the whole launch and streams the
other eighteen through the ring, five chunks per step; the fused kernel (NVSR_RENDER_ONE_PHASE=1) has its own plan, which that change does
not touch, so it is the reference.  Every comparison is bit for bit on rgb, disp, acc, depth and the coarse weights (NaNs in the same
places), and the live counts the two-phase route left in its scratch must be the counts of the nonzero weights.

What can go wrong and where it would show:
  S = 1, 2, 3            one step with no next sample, both parities of the ring (five chunks per step: the slots swap roles every step), and
                         the copy issued behind the last sample -- with the depths read and with the depths in registers;
  S = 24, 40, ragged N   a last workgroup with clamped rays, per-point noise, a white background;
  coarse, fine, coarse   two decoders of independent weights on one stream: a resident region left over from the other decoder, or read
                         before it has landed, changes the third result or one of the three;
  the kept lists         PHASE 4 shares the body: all-one grid = the plain pass; a grid that culls = the two-phase pass under noise 0 / -1e30;
  'f16' and bf16x3       one and three limbs keep the streamed plan: they must be what they were;
  a weight of 1e6        packed as inf, in a resident K-block or in a streamed one: NaN everywhere and the range flag."""
import ctypes as C

import numpy as np
import pytest
import torch

import occupancy_ref as occ_ref
import test_occupancy as occ
from colour_order_ref import ORDER_RAYS, ORDER_SHIFT      # packed entries of the ray order: (count << ORDER_SHIFT) | index of the ray in its block
from two_phase_checks import DEV, OUTPUTS, _env, _same, _scene

pytestmark = pytest.mark.gpu


def _launch(hip, model, rays, S, arith, z=None, noise=None, white=0, lindisp=0):
    """enqueue one render pass by the C ABI (no synchronisation): with `z` nvsr_render_pass_arith, without it the coarse launch with its
    depths in registers.  Outputs start as NaN: an element the route does not write fails."""
    capi = hip.capi
    N = rays.shape[0]
    sc, keep = model.native_scene()
    packed = model.packed_decoder()
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)
    out = dict(rgb=nan(N, 3), disp=nan(N), acc=nan(N), weights=nan(N, S), depth=nan(N))
    code = capi.RENDER_ARITHMETIC[arith]
    tail = (int(white), capi.ptr(out["rgb"]), capi.ptr(out["disp"]), capi.ptr(out["acc"]), capi.ptr(out["weights"]), capi.ptr(out["depth"]), None)
    if z is not None:
        assert N >= capi.fused_min_rays()
        capi.call("nvsr_render_pass_arith", C.byref(sc), capi.ptr(packed), N, S, capi.ptr(rays), capi.ptr(z), capi.ptr(noise), *tail, code, capi.stream())
    else:
        capi.call("nvsr_render_pass3_coarse_z_launch", code, C.byref(sc), capi.ptr(packed), N, S, capi.ptr(rays), int(lindisp), capi.ptr(noise), *tail,
                  capi.stream())
    return out, (sc, keep, packed)


def _live_counts(hip, N):
    """per-ray live counts of the latest two-phase launch, unpacked from the entries of the ray order"""
    t = torch.full((N,), -1, dtype=torch.int32, device=DEV)
    assert hip.capi.lib().nvsr_internal_copy_live_counts(t.data_ptr(), N, hip.capi.stream()) == 0, "the two-phase route did not run"
    torch.cuda.synchronize()
    e = t.cpu().numpy()
    counts = np.full(N, -1, np.int64)
    ray = (np.arange(N) // ORDER_RAYS) * ORDER_RAYS + (e & (ORDER_RAYS - 1))
    counts[ray] = e >> ORDER_SHIFT
    return counts


def _routes_agree(hip, model, rays, S, arith, what="", **kw):
    lib = hip.capi.lib()
    assert lib.nvsr_release_render_scratch() == 0
    with _env(NVSR_RENDER_ONE_PHASE="1"):
        one, k1 = _launch(hip, model, rays, S, arith, **kw)
        torch.cuda.synchronize()
    assert lib.nvsr_render_scratch_bytes() == 0
    with _env(NVSR_RENDER_ONE_PHASE="0"):
        two, k2 = _launch(hip, model, rays, S, arith, **kw)
        torch.cuda.synchronize()
    N = rays.shape[0]
    assert lib.nvsr_render_scratch_bytes() == 2 * 4 * N * S + 4 * N, "the two-phase route did not run"
    for name in OUTPUTS:
        print("%s two-phase vs fused, %s: %d elements differ" % (what, name, int((torch.nan_to_num(one[name]) != torch.nan_to_num(two[name])).sum())))
    for name in OUTPUTS:
        assert _same(one[name], two[name]), (what, name)
    want = (one["weights"] != 0).sum(1).cpu().numpy()          # (a NaN weight is live)
    assert np.array_equal(_live_counts(hip, N), want), what
    return one, two


def _depths(N, S, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.sort(torch.rand(N, S, device=DEV, generator=g) * 4 + 2, -1).values.contiguous()


@pytest.fixture(scope="module")
def square(hip):
    """256 x 256 rays: the smallest count that reaches these kernels through nvsr_render_pass_arith"""
    mc, mf, rays = _scene(hip, 21, 256, 256)
    assert rays.shape[0] == hip.capi.fused_min_rays()
    return mc, mf, rays


@pytest.fixture(scope="module")
def ragged(hip):
    mc, mf, rays = _scene(hip, 22, 257, 257)
    assert rays.shape[0] % 256 != 0
    return mc, mf, rays


@pytest.fixture(scope="module", autouse=True)
def _clean(hip):
    yield
    hip.capi.lib().nvsr_release_render_scratch()
    if hip.capi._range_flag is not None:
        hip.capi._range_flag.reset()


@pytest.mark.parametrize("S", [1, 2, 3])
@pytest.mark.parametrize("depths", ["read", "lin", "disp"])
def test_one_two_and_three_steps(hip, square, S, depths):
    mc, mf, rays = square
    N = rays.shape[0]
    z = _depths(N, S, 10 + S) if depths == "read" else None
    one, two = _routes_agree(hip, mf, rays, S, "f16x2", "S %d %s" % (S, depths), z=z, lindisp=int(depths == "disp"))
    assert torch.isfinite(two["rgb"]).all() and bool((two["weights"] != 0).any())


@pytest.mark.parametrize("S,depths", [(24, "disp"), (40, "read")])
def test_ragged_ray_count_noise_and_white_background(hip, ragged, S, depths):
    mc, mf, rays = ragged
    N = rays.shape[0]
    z = _depths(N, S, 3) if depths == "read" else None
    g = torch.Generator(device=DEV).manual_seed(9)
    noise = 0.7 * torch.randn(N, S, device=DEV, generator=g)
    kw = dict(z=z, lindisp=int(depths == "disp"))
    _routes_agree(hip, mf, rays, S, "f16x2", "plain", **kw)
    one, two = _routes_agree(hip, mf, rays, S, "f16x2", "noise, white", noise=noise, white=1, **kw)
    assert torch.isfinite(two["rgb"]).all()
    w = two["weights"]
    assert 0.02 < float((w == 0).float().mean()) < 0.98         # dead and live samples


@pytest.mark.parametrize("depths", ["read", "lin"])
def test_two_decoders_alternate_on_one_stream(hip, square, depths):
    """coarse, fine, coarse without a synchronisation in between: the third equals the first, and each equals its fused reference"""
    mc, mf, rays = square
    N, S = rays.shape[0], 5
    z = _depths(N, S, 4) if depths == "read" else None
    pc, pf = mc.packed_decoder(), mf.packed_decoder()
    assert float((pc != pf).float().mean()) > 0.9               # independent weights: every K-block differs
    kw = dict(z=z, lindisp=0)
    with _env(NVSR_RENDER_ONE_PHASE="1"):
        ref_c, k1 = _launch(hip, mc, rays, S, "f16x2", **kw)
        ref_f, k2 = _launch(hip, mf, rays, S, "f16x2", **kw)
        torch.cuda.synchronize()
    with _env(NVSR_RENDER_ONE_PHASE="0"):
        a, k3 = _launch(hip, mc, rays, S, "f16x2", **kw)
        b, k4 = _launch(hip, mf, rays, S, "f16x2", **kw)
        c, k5 = _launch(hip, mc, rays, S, "f16x2", **kw)
        torch.cuda.synchronize()
    assert hip.capi.lib().nvsr_render_scratch_bytes() > 0, "the two-phase route did not run"
    for name in OUTPUTS:
        assert _same(a[name], c[name]), ("third vs first", name)
        assert _same(a[name], ref_c[name]), ("coarse", name)
        assert _same(b[name], ref_f[name]), ("fine", name)
    assert not _same(a["weights"], b["weights"])                # the two decoders really answer differently


@pytest.mark.parametrize("depths", ["read", "lin"])
def test_kept_lists_all_one_grid_equals_the_plain_pass(hip, square, depths):
    mc, mf, rays = square
    S, G = 24, 16
    z = _depths(rays.shape[0], S, 6) if depths == "read" else None
    want, want_live = occ._plain_pass(hip, mf, rays, S, "f16x2", z, 0, None, 1)
    got, got_live, got_kept = occ._occ_pass(hip, mf, rays, S, "f16x2", z, 0, occ._to_dev(occ_ref.pack_bits(np.ones(G ** 3, bool), G)), G, 1)
    occ._assert_same(got, want)
    assert np.array_equal(got_live, want_live) and ((got_kept >> ORDER_SHIFT) == S).all()


@pytest.mark.parametrize("depths", ["read", "lin"])
def test_kept_lists_culling_grid_equals_the_pass_under_noise(hip, square, depths):
    """a grid that culls about half the cells: the occupancy pass = the two-phase pass with noise 0 on kept and -1e30 on culled samples"""
    mc, mf, rays = square
    S, G = 24, 16
    N = rays.shape[0]
    z = _depths(N, S, 7) if depths == "read" else None
    cells = np.random.default_rng(5).random(G ** 3) < 0.5
    grid = occ._to_dev(occ_ref.pack_bits(cells, G))
    kept, kept_n = occ._cull(hip, mf, rays, S, z, 0, grid, G)
    assert 0.2 * N * S < kept_n.sum() < 0.8 * N * S and kept_n.min() < kept_n.max()
    noise = occ._masked_noise(kept, kept_n, S)
    want, want_live = occ._plain_pass(hip, mf, rays, S, "f16x2", z, 0, noise, 1)
    got, got_live, got_kept = occ._occ_pass(hip, mf, rays, S, "f16x2", z, 0, grid, G, 1)
    occ._assert_same(got, want)
    assert np.array_equal(got_live, want_live)
    assert np.array_equal(np.sort(got_kept >> ORDER_SHIFT), np.sort(kept_n))
    # ... and that pass is the fused kernel's under the same noise
    _routes_agree(hip, mf, rays, S, "f16x2", "masked noise", z=z, lindisp=0, noise=noise, white=1)


@pytest.mark.parametrize("S", [3, 24])
@pytest.mark.parametrize("arith", ["f16", "bf16x3"])
def test_one_and_three_limbs(hip, square, arith, S):
    mc, mf, rays = square
    _routes_agree(hip, mf, rays, S, arith, arith + " read", z=_depths(rays.shape[0], S, 8), lindisp=0)
    _routes_agree(hip, mf, rays, S, arith, arith + " lin", z=None, lindisp=0)


@pytest.mark.parametrize("where", ["resident", "streamed"])
def test_a_weight_beyond_the_f16_range_is_still_nan_and_raises_the_flag(hip, where):
    """a density layer-1 weight of 1e6 is packed as inf.  Input channel 7 lies in the layer's first K-block (resident), channel 120 in its last
    (streamed): every output is NaN in both routes, and both raise the range flag."""
    mc, mf, rays = _scene(hip, 23, 256, 256)
    N, S = rays.shape[0], 3
    with torch.no_grad():
        mf.density_dec["0"][1].weight[5, 7 if where == "resident" else 120] = 1.0e6
    flag = hip.capi.range_flag()
    try:
        for z in (_depths(N, S, 2), None):
            words, outs = [], []
            for one_phase in ("1", "0"):
                flag.reset()
                with _env(NVSR_RENDER_ONE_PHASE=one_phase):
                    o, keep = _launch(hip, mf, rays, S, "f16x2", z=z, white=1)
                    torch.cuda.synchronize()
                outs.append(o)
                words.append(int(flag.word))
            assert words == [1, 1], words
            for name in OUTPUTS:
                assert _same(outs[0][name], outs[1][name]), name
            assert torch.isnan(outs[1]["rgb"]).all() and torch.isnan(outs[1]["acc"]).all() and torch.isnan(outs[1]["weights"]).all()
    finally:
        flag.reset()
