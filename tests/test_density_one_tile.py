"""GPU tests (-m gpu) of the one-tile density kernels (csrc/density_tile.hip: density_tile_kernel, density_tile_z_kernel) -- the density pass of
the two-phase route on two f16 limbs with one 32-ray tile per wave, eight waves per workgroup, the two waves of a SIMD staggered (waves 4..7,
rays 128..255 of every block, gather a sample's features a step ahead); selected by NVSR_DENSITY_ONE_TILE=1.
The reference is the fused kernel (NVSR_RENDER_ONE_PHASE=1), which has its own code.  Every comparison is bit for bit on rgb, disp, acc,
depth and the weights (NaNs in the same places), the live counts the route left in its scratch must be the counts of the nonzero weights,
and every case asserts by nvsr_internal_density_kernel that the one-tile kernel ran -- and, with the handle at 0, that the tile-pair kernel
ran and wrote the same bits.

What can go wrong and where it would show:
  S = 1, 2, 3            one step with no successor: the gather a step ahead has no sample to gather for, the first sample's features are
                         gathered in the loop by every wave; the copy issued behind the last sample (4 chunks per step: the ring's slots
                         keep their roles) -- depths read, linear in registers, linear in disparity;
  S = 24, 40, ragged N   a last workgroup with clamped rays (257 x 257 = 258 workgroups and one ray), per-point noise, a white
                         background, dead and live samples;
  coarse, fine, coarse   two decoders of independent weights on one stream without a synchronisation: resident layers left over from
                         the other decoder, or read before they have landed, change the third result or one of the three;
  a weight of 1e6        packed as inf, in density layer 0 (resident here) or in layer 2 (streamed): NaN everywhere and the range flag;
  a frame                nvsr_render_rays_arith, 8 + 16 samples: every output and both workspace tensors with the handle on and off."""
import ctypes as C

import numpy as np
import pytest
import torch

from colour_order_ref import ORDER_RAYS, ORDER_SHIFT      # packed entries of the ray order: (count << ORDER_SHIFT) | index of the ray in its block
from two_phase_checks import DEV, OUTPUTS, _env, _same, _scene

pytestmark = pytest.mark.gpu

ONE_TILE, TILE_PAIR = 1, 0      # what nvsr_internal_density_kernel answers


def _launch(hip, model, rays, S, z=None, noise=None, white=0, lindisp=0):
    """enqueue one 'f16x2' render pass by the C ABI (no synchronisation): with `z` nvsr_render_pass_arith, without it the coarse launch with its
    depths in registers.  Outputs start as NaN: an element the route does not write fails."""
    capi = hip.capi
    N = rays.shape[0]
    sc, keep = model.native_scene()
    packed = model.packed_decoder()
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)
    out = dict(rgb=nan(N, 3), disp=nan(N), acc=nan(N), weights=nan(N, S), depth=nan(N))
    code = capi.RENDER_ARITHMETIC["f16x2"]
    tail = (int(white), capi.ptr(out["rgb"]), capi.ptr(out["disp"]), capi.ptr(out["acc"]), capi.ptr(out["weights"]), capi.ptr(out["depth"]), None)
    if z is not None:
        assert N >= capi.fused_min_rays()
        capi.call("nvsr_render_pass_arith", C.byref(sc), capi.ptr(packed), N, S, capi.ptr(rays), capi.ptr(z), capi.ptr(noise), *tail, code, capi.stream())
    else:
        capi.call("nvsr_render_pass3_coarse_z_launch", code, C.byref(sc), capi.ptr(packed), N, S, capi.ptr(rays), int(lindisp), capi.ptr(noise), *tail,
                  capi.stream())
    return out, (sc, keep, packed)


def _density_kernel(hip):
    return hip.capi.lib().nvsr_internal_density_kernel(hip.capi.stream())


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


def _routes_agree(hip, model, rays, S, what="", **kw):
    """fused kernel (the reference), one-tile density kernels, tile-pair density kernels: the same bits, the routes proven by the hook"""
    lib = hip.capi.lib()
    N = rays.shape[0]
    assert lib.nvsr_release_render_scratch() == 0
    with _env(NVSR_RENDER_ONE_PHASE="1"):
        ref, k0 = _launch(hip, model, rays, S, **kw)
        torch.cuda.synchronize()
    assert lib.nvsr_render_scratch_bytes() == 0 and _density_kernel(hip) == -1
    want = (ref["weights"] != 0).sum(1).cpu().numpy()          # (a NaN weight is live)
    got = {}
    for handle, kernel in (("1", ONE_TILE), ("0", TILE_PAIR)):
        with _env(NVSR_RENDER_ONE_PHASE="0", NVSR_DENSITY_ONE_TILE=handle):
            two, k1 = _launch(hip, model, rays, S, **kw)
            torch.cuda.synchronize()
        assert lib.nvsr_render_scratch_bytes() == 2 * 4 * N * S + 4 * N, "the two-phase route did not run"
        assert _density_kernel(hip) == kernel, (what, handle)
        for name in OUTPUTS:
            print("%s handle %s vs fused, %s: %d elements differ" % (what, handle, name, int((torch.nan_to_num(ref[name]) != torch.nan_to_num(two[name])).sum())))
        for name in OUTPUTS:
            assert _same(ref[name], two[name]), (what, handle, name)
        assert np.array_equal(_live_counts(hip, N), want), (what, handle)
        got[handle] = two
    return ref, got["1"]


def _depths(N, S, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.sort(torch.rand(N, S, device=DEV, generator=g) * 4 + 2, -1).values.contiguous()


@pytest.fixture(scope="module")
def square(hip):
    """256 x 256 rays: the smallest count that reaches these kernels through nvsr_render_pass_arith"""
    mc, mf, rays = _scene(hip, 31, 256, 256)
    assert rays.shape[0] == hip.capi.fused_min_rays()
    return mc, mf, rays


@pytest.fixture(scope="module")
def ragged(hip):
    mc, mf, rays = _scene(hip, 32, 257, 257)
    assert rays.shape[0] % 256 == 1
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
    ref, two = _routes_agree(hip, mf, rays, S, "S %d %s" % (S, depths), z=z, lindisp=int(depths == "disp"))
    assert torch.isfinite(two["rgb"]).all() and bool((two["weights"] != 0).any())


@pytest.mark.parametrize("S,depths", [(24, "disp"), (40, "read")])
def test_ragged_ray_count_noise_and_white_background(hip, ragged, S, depths):
    mc, mf, rays = ragged
    N = rays.shape[0]
    z = _depths(N, S, 3) if depths == "read" else None
    g = torch.Generator(device=DEV).manual_seed(9)
    noise = 0.7 * torch.randn(N, S, device=DEV, generator=g)
    ref, two = _routes_agree(hip, mf, rays, S, "noise, white", z=z, lindisp=int(depths == "disp"), noise=noise, white=1)
    assert torch.isfinite(two["rgb"]).all()
    share = float((two["weights"] == 0).float().mean())
    print("share of zero weights: %.4f" % share)
    assert 0.02 < share < 0.98                                 # dead and live samples


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
        ref_c, k1 = _launch(hip, mc, rays, S, **kw)
        ref_f, k2 = _launch(hip, mf, rays, S, **kw)
        torch.cuda.synchronize()
    with _env(NVSR_RENDER_ONE_PHASE="0", NVSR_DENSITY_ONE_TILE="1"):
        a, k3 = _launch(hip, mc, rays, S, **kw)
        b, k4 = _launch(hip, mf, rays, S, **kw)
        c, k5 = _launch(hip, mc, rays, S, **kw)
        torch.cuda.synchronize()
    assert _density_kernel(hip) == ONE_TILE
    for name in OUTPUTS:
        assert _same(a[name], c[name]), ("third vs first", name)
        assert _same(a[name], ref_c[name]), ("coarse", name)
        assert _same(b[name], ref_f[name]), ("fine", name)
    assert not _same(a["weights"], b["weights"])                # the two decoders really answer differently


@pytest.mark.parametrize("where", ["resident", "streamed"])
def test_a_weight_beyond_the_f16_range_is_nan_and_raises_the_flag(hip, where):
    """a density weight of 1e6 is packed as inf.  Layer 0 lies in the resident K-blocks of the one-tile kernels, layer 2 (input channel 120: its
    last K-block) goes through the ring: every output is NaN in the fused, the one-tile and the tile-pair route, and each raises the flag."""
    mc, mf, rays = _scene(hip, 33, 256, 256)
    N, S = rays.shape[0], 3
    with torch.no_grad():
        if where == "resident":
            mf.density_dec["0"][0].weight[5, 7] = 1.0e6
        else:
            mf.density_dec["0"][2].weight[5, 120] = 1.0e6
    flag = hip.capi.range_flag()
    routes = (dict(NVSR_RENDER_ONE_PHASE="1"), dict(NVSR_RENDER_ONE_PHASE="0", NVSR_DENSITY_ONE_TILE="1"), dict(NVSR_RENDER_ONE_PHASE="0", NVSR_DENSITY_ONE_TILE="0"))
    try:
        for z in (_depths(N, S, 2), None):
            words, outs, kernels = [], [], []
            for env in routes:
                flag.reset()
                with _env(**env):
                    o, keep = _launch(hip, mf, rays, S, z=z, white=1)
                    torch.cuda.synchronize()
                outs.append(o)
                words.append(int(flag.word))
                kernels.append(_density_kernel(hip))
            assert words == [1, 1, 1], words
            assert kernels[1:] == [ONE_TILE, TILE_PAIR], kernels
            for o in outs[1:]:
                for name in OUTPUTS:
                    assert _same(outs[0][name], o[name]), name
            assert torch.isnan(outs[1]["rgb"]).all() and torch.isnan(outs[1]["acc"]).all() and torch.isnan(outs[1]["weights"]).all()
    finally:
        flag.reset()


def test_frame_with_the_handle_on_equals_the_frame_with_it_off(hip):
    """nvsr_render_rays_arith on 256 x 256 rays, 8 + 16 samples: the six outputs, the coarse weights and the fine depths in the workspace and the
    fine pass's live counts -- what the colour passes consume -- are the same bytes with the one-tile and with the tile-pair density kernels"""
    capi = hip.capi
    lib = capi.lib()
    mc, mf, rays = _scene(hip, 34, 256, 256)
    N, Nc, Nf = rays.shape[0], 8, 16
    assert N >= capi.fused_min_rays()
    nws = int(lib.nvsr_render_workspace_floats(N, Nc, Nf))
    sc_c, keep_c = mc.native_scene()
    r4 = lambda n: (n + 3) // 4 * 4
    frames, counts = [], []
    for handle, kernel in (("1", ONE_TILE), ("0", TILE_PAIR)):
        ws = torch.full((nws,), float("nan"), device=DEV)
        o = [torch.full(s, float("nan"), device=DEV) for s in ((N, 3), (N,), (N,), (N, 3), (N,), (N,))]
        with _env(NVSR_RENDER_ONE_PHASE="0", NVSR_DENSITY_ONE_TILE=handle):
            capi.call("nvsr_render_rays_arith", C.byref(sc_c), capi.ptr(mc.packed_decoder()), capi.ptr(mf.packed_decoder()), N, Nc, Nf, capi.ptr(rays),
                      0, 0, None, None, None, None, *[capi.ptr(t) for t in o], capi.ptr(ws), capi.ARITHMETIC["f16x2"], capi.stream())
            torch.cuda.synchronize()
        assert _density_kernel(hip) == kernel, handle
        counts.append(_live_counts(hip, N))
        frames.append(o + [ws[r4(N * Nc):r4(N * Nc) + N * Nc].clone(), ws[2 * r4(N * Nc):2 * r4(N * Nc) + N * (Nc + Nf)].clone()])
    names = ("rgb_coarse", "disp_coarse", "acc_coarse", "rgb_fine", "disp_fine", "acc_fine", "weights_coarse", "z_fine")
    for name, a, b in zip(names, *frames):
        assert _same(a, b), name
    assert np.array_equal(counts[0], counts[1])
    assert torch.isfinite(frames[0][0]).all() and torch.isfinite(frames[0][3]).all()
