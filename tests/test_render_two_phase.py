"""GPU tests (-m gpu) of the two-phase render pass (csrc/render3.hip; include/nvsr.h "The two-phase render pass"): the density pass + the
colour pass on the live samples against the fused kernel (NVSR_RENDER_ONE_PHASE=1), output for output, bit for bit.

A sample whose weight is +0.0 added +0.0 to every sum of the fused kernel, so leaving it out changes no bit: every case asserts torch.equal
on rgb, disp, acc, depth and the coarse weights (disp is NaN by definition on a ray with acc == 0: NaNs must sit in the same places and the
numbers must be equal)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from test_hip_parity import DEV

pytestmark = pytest.mark.gpu

ARITHS = ["f16x2", "bf16x3"]


class _route:
    """NVSR_RENDER_ONE_PHASE for the launches inside the block (the library reads it at every launch)"""

    def __init__(self, one_phase):
        self.value = "1" if one_phase else "0"

    def __enter__(self):
        self.old = os.environ.get("NVSR_RENDER_ONE_PHASE")
        os.environ["NVSR_RENDER_ONE_PHASE"] = self.value

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("NVSR_RENDER_ONE_PHASE", None)
        else:
            os.environ["NVSR_RENDER_ONE_PHASE"] = self.old


def _same(a, b):
    """torch.equal with NaNs: in the same places, and every number equal"""
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0))


def _scene(hip, seed, H, W, plane_res=64):
    from bench import make_synthetic_scene
    mc, mf, sid, pose = make_synthetic_scene(DEV, plane_res=plane_res, view_res=16, seed=seed)
    focal = 0.5 * W / np.tan(0.5 * 0.6911112)
    ro, rd = hip.nerf_helpers.get_ray_bundle(H, W, focal, pose)
    rays = hip.train_utils.pack_rays(ro, rd, 2.0, 6.0)
    return mc, mf, rays


def _pass(hip, model, rays, S, arith, one_phase, z=None, noise=None, white=0, lindisp=0):
    """one render pass by the C ABI: with `z` nvsr_render_pass_arith (depths read; weights requested: the coarse kernel), without it the
    coarse pass with its depths in registers (nvsr_render_pass3_coarse_z_launch).  Outputs start as NaN: an element a route does not write fails."""
    capi = hip.capi
    N = rays.shape[0]
    assert N >= capi.fused_min_rays()
    sc, keep = model.native_scene()
    packed = model.packed_decoder()
    out = dict(rgb=torch.full((N, 3), float("nan"), device=DEV), disp=torch.full((N,), float("nan"), device=DEV),
               acc=torch.full((N,), float("nan"), device=DEV), weights=torch.full((N, S), float("nan"), device=DEV),
               depth=torch.full((N,), float("nan"), device=DEV))
    with _route(one_phase):
        if z is not None:
            capi.call("nvsr_render_pass_arith", C.byref(sc), capi.ptr(packed), N, S, capi.ptr(rays), capi.ptr(z), capi.ptr(noise), int(white),
                      capi.ptr(out["rgb"]), capi.ptr(out["disp"]), capi.ptr(out["acc"]), capi.ptr(out["weights"]), capi.ptr(out["depth"]), None,
                      capi.ARITHMETIC[arith], capi.stream())
        else:
            f = capi.lib().nvsr_render_pass3_coarse_z_launch
            f.restype = C.c_int
            f.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 7
            st = f(capi.ARITHMETIC[arith], C.cast(C.byref(sc), C.c_void_p), capi.ptr(packed), N, S, capi.ptr(rays), int(lindisp), capi.ptr(noise), int(white),
                   capi.ptr(out["rgb"]), capi.ptr(out["disp"]), capi.ptr(out["acc"]), capi.ptr(out["weights"]), capi.ptr(out["depth"]), None,
                   capi.stream())
            assert st == 0
        torch.cuda.synchronize()
    return out


def _assert_routes_agree(hip, model, rays, S, arith, **kw):
    lib = hip.capi.lib()
    assert lib.nvsr_release_render_scratch() == 0
    one = _pass(hip, model, rays, S, arith, True, **kw)
    assert lib.nvsr_render_scratch_bytes() == 0                  # the fused kernel needs no lists
    two = _pass(hip, model, rays, S, arith, False, **kw)
    N = rays.shape[0]
    assert lib.nvsr_render_scratch_bytes() == 2 * 4 * N * S + 4 * N, "the two-phase route did not run"
    for name in ("rgb", "disp", "acc", "depth", "weights"):
        print("two-phase vs fused, %s: %d elements differ" % (name, int((torch.nan_to_num(one[name]) != torch.nan_to_num(two[name])).sum())))
    for name in ("rgb", "disp", "acc", "depth", "weights"):
        assert _same(one[name], two[name]), name
    return one, two


def _depths(N, S, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.sort(torch.rand(N, S, device=DEV, generator=g) * 4 + 2, -1).values.contiguous()


@pytest.mark.parametrize("arith", ARITHS)
def test_frame_256x256_two_phase_equals_fused(hip, arith):
    """The product path of a frame (nvsr_render_rays_arith, 64 + 128 samples, 65 536 rays): coarse pass with depths in registers, resampling, fine
    pass -- both images, disp, acc and the coarse weights (the resampler's input: the fine depths follow from them)."""
    capi = hip.capi
    H = W = 256
    mc, mf, rays = _scene(hip, 3, H, W)
    N, Nc, Nf = H * W, 64, 128
    assert N >= capi.fused_min_rays()
    lib = capi.lib()
    nws = int(lib.nvsr_render_workspace_floats(N, Nc, Nf))
    sc_c, keep_c = mc.native_scene()
    frames = []
    # which route ran is observable: the live lists live in a scratch of the library's own, allocated by the first two-phase launch
    # (sized for the frame's larger pass) and by nothing else -- a silent fall-back to the fused kernel would leave it empty
    assert lib.nvsr_release_render_scratch() == 0 and lib.nvsr_render_scratch_bytes() == 0
    for one_phase in (True, False):
        ws = torch.full((nws,), float("nan"), device=DEV)
        o = [torch.full(s, float("nan"), device=DEV) for s in ((N, 3), (N,), (N,), (N, 3), (N,), (N,))]
        with _route(one_phase):
            capi.call("nvsr_render_rays_arith", C.byref(sc_c), capi.ptr(mc.packed_decoder()), capi.ptr(mf.packed_decoder()), N, Nc, Nf, capi.ptr(rays),
                      0, 0, None, None, None, None, *[capi.ptr(t) for t in o], capi.ptr(ws), capi.ARITHMETIC[arith], capi.stream())
            torch.cuda.synchronize()
        assert lib.nvsr_render_scratch_bytes() == (0 if one_phase else 2 * 4 * N * (Nc + Nf) + 4 * N)
        r4 = lambda n: (n + 3) // 4 * 4
        frames.append(o + [ws[r4(N * Nc):r4(N * Nc) + N * Nc].clone(), ws[2 * r4(N * Nc):2 * r4(N * Nc) + N * (Nc + Nf)].clone()])
    names = ("rgb_coarse", "disp_coarse", "acc_coarse", "rgb_fine", "disp_fine", "acc_fine", "weights_coarse", "z_fine")
    for name, a, b in zip(names, *frames):
        assert _same(a, b), name
    assert torch.isfinite(frames[1][0]).all() and torch.isfinite(frames[1][3]).all()
    w = frames[1][6]
    assert 0.05 < float((w == 0).float().mean()) < 0.98         # the scene has both dead and live samples: the colour pass really skips work
    assert lib.nvsr_release_render_scratch() == 0 and lib.nvsr_render_scratch_bytes() == 0     # given back; the next launch allocates anew


@pytest.mark.parametrize("arith", ARITHS)
def test_ragged_ray_count_noise_and_white_background(hip, arith):
    """N = 257 x 257 = 66 049 rays (258 workgroups and one ray), per-point density noise, white background -- the pass that reads its depths
    (S = 40) and the pass with its depths in registers (S = 24, lindisp)."""
    H = W = 257
    mc, mf, rays = _scene(hip, 5, H, W)
    N = rays.shape[0]
    assert N % 256 != 0
    g = torch.Generator(device=DEV).manual_seed(9)
    for S, z, lindisp in ((40, _depths(N, 40, 1), 0), (24, None, 1)):
        noise = 0.7 * torch.randn(N, S, device=DEV, generator=g)
        _assert_routes_agree(hip, mf, rays, S, arith, z=z, lindisp=lindisp)                           # plain
        _assert_routes_agree(hip, mf, rays, S, arith, z=z, lindisp=lindisp, noise=noise)              # density noise
        one, two = _assert_routes_agree(hip, mf, rays, S, arith, z=z, lindisp=lindisp, noise=noise, white=1)
        assert torch.isfinite(two["rgb"]).all()


@pytest.mark.parametrize("arith", ARITHS)
def test_every_weight_zero_and_every_weight_positive(hip, arith):
    """The two ends of the live lists.  A density head that answers -1000 everywhere: every weight is +0.0, every list is empty, the colour pass
    runs no step and writes rgb = 0 (white background: 1).  A density head that answers +0.05 everywhere: every weight is positive, every list
    holds all S samples (trip = S: nothing is saved, nothing may change)."""
    H = W = 257
    mc, mf, rays = _scene(hip, 6, H, W)
    N, S = rays.shape[0], 32
    # evenly spaced depths with a per-ray offset: two random depths may coincide, and a sample of zero length has weight 0 whatever its density
    g = torch.Generator(device=DEV).manual_seed(2)
    z = (2.0 + (torch.arange(S, device=DEV)[None, :] + 0.5 * torch.rand(N, 1, device=DEV, generator=g)) * (4.0 / S)).contiguous()
    head = mf.fc_alpha["0"]
    for bias, all_zero in ((-1000.0, True), (0.05, False)):
        with torch.no_grad():
            head.weight.zero_()
            head.bias.fill_(bias)
        for zz in (z, None):
            for white in (0, 1):
                one, two = _assert_routes_agree(hip, mf, rays, S, arith, z=zz, white=white)
                if all_zero:
                    assert bool((two["weights"] == 0).all()) and bool((two["acc"] == 0).all())
                    assert torch.equal(two["rgb"], torch.full_like(two["rgb"], float(white)))
                else:
                    assert bool((two["weights"] > 0).all()) and torch.isfinite(two["rgb"]).all()


def test_density_side_overflow_is_still_nan_and_raises_the_flag(hip):
    """f16x2 with a density hidden bias of 5000 (activations beyond the f16 range, tests/test_hip_round4.py): the weights are NaN, NaN weights are
    live, the pixels are NaN in both routes and both raise the range flag."""
    H = W = 257
    mc, mf, rays = _scene(hip, 4, H, W)
    N, S = rays.shape[0], 24
    z = _depths(N, S, 3)
    with torch.no_grad():
        mf.density_dec["0"][1].bias[3] = 5000.0
    flag = hip.capi.range_flag()
    try:
        for zz in (z, None):
            words = []
            outs = []
            for one_phase in (True, False):
                flag.reset()
                assert hip.capi.lib().nvsr_release_render_scratch() == 0
                outs.append(_pass(hip, mf, rays, S, "f16x2", one_phase, z=zz, white=1))
                assert (hip.capi.lib().nvsr_render_scratch_bytes() > 0) == (not one_phase)
                words.append(int(flag.word))
            assert words == [1, 1], words
            for name in ("rgb", "disp", "acc", "depth", "weights"):
                assert _same(outs[0][name], outs[1][name]), name
            assert torch.isnan(outs[1]["rgb"]).any() and torch.isnan(outs[1]["acc"]).any()
    finally:
        flag.reset()
