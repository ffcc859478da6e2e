"""GPU tests (-m gpu) of the two-phase render pass (csrc/render3.hip: the kernels; csrc/colour_order.hip: the lists' scratch; include/nvsr.h "The two-phase render pass"): the density pass + the
colour pass on the live samples against the fused kernel (NVSR_RENDER_ONE_PHASE=1), output for output, bit for bit.

A sample whose weight is +0.0 added +0.0 to every sum of the fused kernel, so leaving it out changes no bit: every case asserts torch.equal
on rgb, disp, acc, depth and the coarse weights (disp is NaN by definition on a ray with acc == 0: NaNs must sit in the same places and the
numbers must be equal)."""
import ctypes as C

import numpy as np
import pytest
import torch

from colour_order_ref import order_reference
from two_phase_checks import ARITHS, DEV, OUTPUTS, _env, _pass, _same, _scene

pytestmark = pytest.mark.gpu

def _assert_routes_agree(hip, model, rays, S, arith, **kw):
    lib = hip.capi.lib()
    assert lib.nvsr_release_render_scratch() == 0
    one, _ = _pass(hip, model, rays, S, arith, NVSR_RENDER_ONE_PHASE="1", **kw)
    assert lib.nvsr_render_scratch_bytes() == 0                  # the fused kernel needs no lists
    two, _ = _pass(hip, model, rays, S, arith, NVSR_RENDER_ONE_PHASE="0", **kw)
    N = rays.shape[0]
    assert lib.nvsr_render_scratch_bytes() == 2 * 4 * N * S + 4 * N, "the two-phase route did not run"
    for name in OUTPUTS:
        print("two-phase vs fused, %s: %d elements differ" % (name, int((torch.nan_to_num(one[name]) != torch.nan_to_num(two[name])).sum())))
    for name in OUTPUTS:
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
        with _env(NVSR_RENDER_ONE_PHASE="1" if one_phase else "0"):
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
                outs.append(_pass(hip, mf, rays, S, "f16x2", z=zz, white=1, NVSR_RENDER_ONE_PHASE="1" if one_phase else "0")[0])
                assert (hip.capi.lib().nvsr_render_scratch_bytes() > 0) == (not one_phase)
                words.append(int(flag.word))
            assert words == [1, 1], words
            for name in OUTPUTS:
                assert _same(outs[0][name], outs[1][name]), name
            assert torch.isnan(outs[1]["rgb"]).any() and torch.isnan(outs[1]["acc"]).any()
    finally:
        flag.reset()


def test_scratch_grows_across_launches_without_a_release(hip):
    """The growth path of the lists' scratch (csrc/colour_order.hip), which every other test releases in front of each launch: four coarse
    passes with their depths in registers (nvsr_render_pass3_coarse_z_launch: no minimum ray count), f16x2, one stream, no release in between
      (a) N = 4096 + 513, S = 8       two blocks of the ray order, 19 groups, a ragged last group
      (b) the same N, S = 24          the lists grow, the group buffer does not
      (c) N = 2 * 4096 + 513, S = 24  both buffers grow
      (d) (a) again                   nothing grows
    each against the fused route bit for bit, and the scratch holds 2 * 4 N S + 4 N bytes of the LARGEST launch so far.  (e) what (d) left
    behind is (d)'s: asking with (c)'s N is refused, (d)'s N gives the reference order of its live counts.  (f) released: nothing is held."""
    capi = hip.capi
    lib = capi.lib()
    Na, Nc = 4096 + 513, 2 * 4096 + 513
    mc, mf, rays = _scene(hip, 7, 96, 96, n_rays=Nc)
    assert (Na + 255) // 256 == 19 and Na % 256 != 0
    assert lib.nvsr_release_render_scratch() == 0 and lib.nvsr_render_scratch_bytes() == 0
    largest = 0
    for step, N, S in (("a", Na, 8), ("b", Na, 24), ("c", Nc, 24), ("d", Na, 8)):
        r = rays[:N].contiguous()
        one, _ = _pass(hip, mf, r, S, "f16x2", NVSR_RENDER_ONE_PHASE="1")
        two, entries = _pass(hip, mf, r, S, "f16x2", NVSR_RENDER_ONE_PHASE="0")
        for name in OUTPUTS:
            assert _same(one[name], two[name]), "(%s) %s" % (step, name)
        largest = max(largest, 2 * 4 * N * S + 4 * N)
        assert lib.nvsr_render_scratch_bytes() == largest, step
    # (e)
    t = torch.full((Nc,), -1, dtype=torch.int32, device=DEV)
    assert lib.nvsr_internal_copy_live_counts(t.data_ptr(), Nc, capi.stream()) == 1      # NVSR_ERR_SHAPE: the latest launch had Na rays
    assert lib.nvsr_internal_copy_live_counts(t.data_ptr(), Na, capi.stream()) == 0
    torch.cuda.synchronize()
    c = (one["weights"] != 0).sum(1).cpu().numpy()
    assert c.max() <= 8 and np.unique(c).size > 1                                         # the order has something to sort
    want = order_reference(c, 8, lib.nvsr_internal_colour_order_bins())
    assert np.array_equal(t[:Na].cpu().numpy(), want) and np.array_equal(entries, want)
    assert bool((t[Na:] == -1).all())
    # (f)
    assert lib.nvsr_release_render_scratch() == 0 and lib.nvsr_render_scratch_bytes() == 0
