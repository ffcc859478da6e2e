"""GPU tests (-m gpu) of the render pass in plain f16, NVSR_ARITH_F16 = 1 / 'f16' (csrc/render3.hip at LIMBS = 1: one v_mfma_f32_32x32x16_f16 per
product block on operands rounded once to f16; include/nvsr.h "NVSR_ARITH_F16 in the render pass").

  1. the decoder's raw outputs against the numpy reference of the arithmetic (tests/render_f16_ref.py) and against float64, by rms
  2. one arithmetic on every route -- fused, lockstep two-phase, point-major -- bit for bit
  3. the bits of 'f16x2' where nothing is rounded
  4. the range contract: an operand beyond the f16 range never yields a finite number
  5. the public surface: model.arithmetic = 'f16' renders evaluation frames, heals like 'f16x2', refuses training; the entries that refuse

Measured on an MI355X (profiles/render_f16_ab.txt), test 1: sigma rms(gpu - float64) / E_ref = 1.0001, rms(gpu - reference) / E_ref = 0.044; rgb logits
1.0004 and 0.167 (bounds 1.25 and 0.25); the 14 tests take 6 s.
"""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

import render_f16_ref as R
import triplane_checks as tc
from two_phase_checks import DEV, N_RAYS, OUTPUTS, _counts_and_noise, _env, _same, _scene

pytestmark = pytest.mark.gpu

F16 = 1                     # NVSR_ARITH_F16
SIZES = [(64, 64)] * 4
ERR_SHAPE = 1


def T(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


class Device:
    """a scene of numpy planes and a packed numpy decoder on the device"""

    def __init__(self, hip, planes, nat):
        self.capi = capi = hip.capi
        self.scene = scene = tc.make_scene(SIZES)
        self.planes = [T(p) for p in planes]
        self.nat = T(nat)
        self.packed = torch.zeros(capi.DECODER_PACKED_FLOATS, device=DEV)
        capi.call("nvsr_pack_decoder", capi.ptr(self.nat), capi.ptr(self.packed), capi.stream())
        sc = capi.Scene()
        for d in range(4):
            sc.planes[d] = self.planes[d].data_ptr()
            sc.ph[d], sc.pw[d] = scene.ph[d], scene.pw[d]
        for i in range(5):
            sc.lo[i], sc.range[i] = float(scene.lo[i]), float(scene.range[i])
        for d in range(3):
            for j in range(6):
                sc.proj[d][j] = float(scene.proj[d][j])
        self.sc = sc

    def render(self, arith, rays, z, noise=None, white=0, raw=False, **env):
        """nvsr_render_pass_arith on buffers that start as NaN -> dict of tensors (raw: [N, S, 4], asks for the fused kernel)"""
        capi, p = self.capi, self.capi.ptr
        N, S = z.shape
        assert N >= capi.fused_min_rays()
        nan = lambda *s: torch.full(s, float("nan"), device=DEV)
        o = dict(rgb=nan(N, 3), disp=nan(N), acc=nan(N), weights=nan(N, S), depth=nan(N))
        if raw:
            o["raw"] = nan(N, S, 4)
        with _env(**env):
            capi.call("nvsr_render_pass_arith", C.byref(self.sc), p(self.packed), N, S, p(rays), p(z), p(noise), int(white), p(o["rgb"]), p(o["disp"]),
                      p(o["acc"]), p(o["weights"]), p(o["depth"]), p(o.get("raw")), arith, capi.stream())
            torch.cuda.synchronize()
        return o


def _pass(hip, model, rays, S, arith, z=None, noise=None, white=0, lindisp=0, **env):
    """two_phase_checks._pass for any code of capi.RENDER_ARITHMETIC (that one indexes capi.ARITHMETIC): one pass by the C ABI under `env`; with
    `z` nvsr_render_pass_arith, without it the coarse launch with its depths in registers (no minimum ray count)"""
    capi = hip.capi
    N = rays.shape[0]
    sc, keep = model.native_scene()
    packed = model.packed_decoder()
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)
    out = dict(rgb=nan(N, 3), disp=nan(N), acc=nan(N), weights=nan(N, S), depth=nan(N))
    code = capi.RENDER_ARITHMETIC[arith]
    with _env(**env):
        if z is not None:
            assert N >= capi.fused_min_rays()
            capi.call("nvsr_render_pass_arith", C.byref(sc), capi.ptr(packed), N, S, capi.ptr(rays), capi.ptr(z), capi.ptr(noise), int(white),
                      capi.ptr(out["rgb"]), capi.ptr(out["disp"]), capi.ptr(out["acc"]), capi.ptr(out["weights"]), capi.ptr(out["depth"]), None, code, capi.stream())
        else:
            capi.call("nvsr_render_pass3_coarse_z_launch", code, C.byref(sc), capi.ptr(packed), N, S, capi.ptr(rays), int(lindisp), capi.ptr(noise), int(white),
                      capi.ptr(out["rgb"]), capi.ptr(out["disp"]), capi.ptr(out["acc"]), capi.ptr(out["weights"]), capi.ptr(out["depth"]), None, capi.stream())
        torch.cuda.synchronize()
    return out


FUSED = dict(NVSR_RENDER_ONE_PHASE="1")
TWO_PHASE = [dict(NVSR_RENDER_ONE_PHASE="0", NVSR_COLOUR_POINTS=pts, NVSR_COLOUR_ORDER=order, NVSR_COLOUR_GROUP_ORDER=order)
             for pts in ("0", "1") for order in ("1", "0")]


def _depths(N, S, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (2.0 + (torch.arange(S, device=DEV)[None, :] + 0.5 * torch.rand(N, 1, device=DEV, generator=g)) * (4.0 / S)).contiguous()


def _assert_routes_agree(hip, model, rays, S, release=True, **kw):
    """'f16': the fused pass, then the lockstep and the point-major two-phase passes with the two orders on and off, bit for bit"""
    lib = hip.capi.lib()
    N = rays.shape[0]
    if release:
        assert lib.nvsr_release_render_scratch() == 0
    one = _pass(hip, model, rays, S, "f16", **FUSED, **kw)
    if release:
        assert lib.nvsr_render_scratch_bytes() == 0
    for env in TWO_PHASE:
        two = _pass(hip, model, rays, S, "f16", **env, **kw)
        assert lib.nvsr_render_scratch_bytes() >= 2 * 4 * N * S + 4 * N, "the two-phase route did not run"
        for name in OUTPUTS:
            assert _same(one[name], two[name]), (name, env)
    return one


@pytest.fixture(scope="module", autouse=True)
def _clean(hip):
    yield
    hip.capi.lib().nvsr_release_render_scratch()
    if hip.capi._range_flag is not None:
        hip.capi._range_flag.reset()


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------------------

def test_decoder_outputs_against_the_reference_of_the_arithmetic(hip):
    """raw_out of the fused kernel in NVSR_ARITH_F16 on every 16th ray and the last 300 (the ragged last group): per output -- sigma, the rgb
    logits -- with E_ref = rms(reference - float64):  rms(gpu - float64) <= 1.25 E_ref  and  rms(gpu - reference) <= 0.25 E_ref.
    (rms: a 1-ulp f32 difference in an accumulator can flip an f16 rounding of the next layer's input -- the worst element is then as large as
    the arithmetic's own error, the mean is not.  0.25: a CPU stand-in with f32 accumulation in K-blocks of 16 sits at 0.065-0.075 E_ref from the
    float64-accumulating reference; the margin of about 3.5 is for the matrix pipe's internal order.)"""
    N, S = N_RAYS, 8
    scene = tc.make_scene(SIZES)
    planes, nat = tc.make_planes(scene, 21), tc.make_decoder(20)
    rays, z = tc.make_rays(N, S, 22)
    tc.assert_exact_taps(rays[:4096], z[:4096], scene)
    dev = Device(hip, planes, nat)
    out = dev.render(F16, T(rays), T(z), raw=True)
    raw = out["raw"].cpu().numpy().astype(np.float64)
    assert np.isfinite(raw).all()
    sel = np.unique(np.concatenate([np.arange(0, N, 16), np.arange(N - 300, N)]))
    dec = tc.unpack(nat)
    ref = R.forward(dec, planes, rays[sel], z[sel], scene)
    f64 = tc.forward64(dec, [torch.as_tensor(p).double() for p in planes], rays[sel], z[sel], scene)[0].numpy()
    got = raw[sel].reshape(-1, 4)
    for name, cols in (("sigma", slice(3, 4)), ("rgb", slice(0, 3))):
        e_ref = R.rms(ref[:, cols] - f64[:, cols])
        to64, toref = R.rms(got[:, cols] - f64[:, cols]) / e_ref, R.rms(got[:, cols] - ref[:, cols]) / e_ref
        print("render_f16 ratio | %s | E_ref=%.3e (%.2e of rms(float64))  rms(gpu - float64)/E_ref=%.4f  rms(gpu - reference)/E_ref=%.4f"
              % (name, e_ref, e_ref / R.rms(f64[:, cols]), to64, toref))
        assert e_ref > 0
        assert to64 <= 1.25, (name, to64)
        assert toref <= 0.25, (name, toref)


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def bench_scene(hip):
    mc, mf, rays = _scene(hip, 11, 264, 264, n_rays=N_RAYS)
    return mf, rays


@pytest.mark.parametrize("S", [1, 8, 24])
def test_routes_agree_depths_read(hip, bench_scene, S):
    """depths read, N = 65536 + 4096 + 37: plain; white background; dictated live counts with one emptied group; one NaN ray"""
    mf, rays = bench_scene
    N = rays.shape[0]
    z = _depths(N, S, S)
    one = _assert_routes_agree(hip, mf, rays, S, z=z)
    assert torch.isfinite(one["rgb"]).all()
    _assert_routes_agree(hip, mf, rays, S, z=z, white=1)
    c, noise = _counts_and_noise(S, 40 + S, empty_group=3)
    # (sigma = 0.05 everywhere makes the dictated counts the live counts)
    head = mf.fc_alpha["0"]
    keep = (head.weight.detach().clone(), head.bias.detach().clone())
    try:
        with torch.no_grad():
            head.weight.zero_()
            head.bias.fill_(0.05)
        one = _assert_routes_agree(hip, mf, rays, S, z=z, noise=noise, white=1)
        assert np.array_equal((one["weights"] != 0).sum(1).cpu().numpy(), c)
        positive = _assert_routes_agree(hip, mf, rays, S, z=z)                      # every weight positive: every list holds all S samples
        assert bool((positive["weights"] > 0).all())
        noise = noise.clone()
        noise[4099, S // 2] = float("nan")                                           # one NaN ray: its weights from that sample on
        one = _assert_routes_agree(hip, mf, rays, S, z=z, noise=noise)
        assert torch.isnan(one["rgb"][4099]).all() and int(torch.isnan(one["acc"]).sum()) == 1
    finally:
        with torch.no_grad():
            head.weight.copy_(keep[0])
            head.bias.copy_(keep[1])


@pytest.mark.parametrize("S", [1, 8, 24])
def test_routes_agree_depths_in_registers_and_the_scratch_grows(hip, bench_scene, S):
    """the coarse launch with its depths in registers, 256 + 37 rays (no minimum), linear in depth and in disparity, white background; then without
    a release in between: more rays and more samples than the scratch holds"""
    mf, rays = bench_scene
    small = rays[:256 + 37].contiguous()
    for lindisp, white in ((0, 0), (1, 1)):
        one = _assert_routes_agree(hip, mf, small, S, lindisp=lindisp, white=white)
        assert torch.isfinite(one["rgb"]).all()
    lib = hip.capi.lib()
    held = lib.nvsr_render_scratch_bytes()
    more = rays[:4096 + 513].contiguous()
    _assert_routes_agree(hip, mf, more, S + 3, release=False)
    assert lib.nvsr_render_scratch_bytes() > held
    _assert_routes_agree(hip, mf, small, S, release=False)


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------------------

def test_same_bits_as_f16x2_where_nothing_is_rounded(hip):
    """zero planes (every blend is exactly 0), +-2^-k weights, short biases: the low limbs of 'f16x2' are all zero and the block order is shared --
    raw outputs and pixels of 'f16' and 'f16x2' are identical, and the raw outputs equal the float64 forward"""
    N, S = N_RAYS, 8
    scene = tc.make_scene(SIZES)
    planes, nat = R.zero_planes(scene), R.exact_decoder(11)
    rays, z = tc.make_rays(N, S, 23)
    dev = Device(hip, planes, nat)
    a = dev.render(F16, T(rays), T(z), raw=True)
    b = dev.render(hip.capi.ARITHMETIC["f16x2"], T(rays), T(z), raw=True)
    for name in a:
        assert _same(a[name], b[name]), name
    sel = np.arange(0, N, 64)
    f64 = tc.forward64(tc.unpack(nat), [torch.as_tensor(p).double() for p in planes], rays[sel], z[sel], scene)[0].numpy()
    assert np.array_equal(a["raw"].cpu().numpy()[sel].reshape(-1, 4).astype(np.float64), f64)
    two = dev.render(F16, T(rays), T(z), NVSR_RENDER_ONE_PHASE="0")
    for name in two:
        assert _same(a[name], two[name]), name


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------------------

ROUTES = [("fused", FUSED), ("lockstep", TWO_PHASE[0]), ("points", TWO_PHASE[2])]


@pytest.mark.parametrize("route", ROUTES, ids=[r[0] for r in ROUTES])
def test_operands_beyond_the_range_never_render_a_number(hip, route):
    N, S = N_RAYS, 8
    scene = tc.make_scene(SIZES)
    rays, z = tc.make_rays(N, S, 24)
    rays_d, z_d = T(rays), T(z)
    flag = hip.capi.range_flag()
    env = route[1]
    # a density-layer weight of 300: 300 x 2^8 is beyond f16 -- NaN pixels, and the flag
    nat = tc.make_decoder(30)
    nat[tc.N_DEN_W1 + tc.N_HID_STRIDE + 5 * tc.HID + 7] = 300.0
    flag.reset()
    out = Device(hip, tc.make_planes(scene, 31), nat).render(F16, rays_d, z_d, **env)
    assert torch.isnan(out["rgb"]).all() and torch.isnan(out["acc"]).all() and int(flag.word) == 1
    # a plane feature of 5000 (x 2^4: inf) under negative first-layer weights: every density accumulator is -inf, which an integer-max ReLU
    # alone would turn into 0 and a pixel of sigma(0) -- NaN, and the flag
    nat = tc.make_decoder(30)
    W0 = nat[tc.N_DEN_W0:tc.N_DEN_W0 + tc.HID * tc.C].reshape(tc.HID, tc.C)
    W0[:, 0] = -np.abs(W0[:, 0]) - 0.01
    planes = tc.make_planes(scene, 31)
    for d in range(3):
        planes[d][..., 0] = 5000.0
    flag.reset()
    out = Device(hip, planes, nat).render(F16, rays_d, z_d, **env)
    assert torch.isnan(out["acc"]).all() and torch.isnan(out["weights"]).all() and torch.isnan(out["rgb"]).all() and int(flag.word) == 1
    flag.reset()


@pytest.mark.parametrize("route", ROUTES[1:], ids=[r[0] for r in ROUTES[1:]])
def test_a_weightless_samples_colour_nan_stays_out_of_the_pixel(hip, route):
    """view-plane features of 5000: every colour chain is NaN, the density chain is not.  On the two-phase route a ray whose samples are all
    weightless (noise -1000) never runs the colour decoder: its pixel is the background, a number; a ray with a live sample is NaN"""
    N, S = N_RAYS, 8
    scene = tc.make_scene(SIZES)
    rays, z = tc.make_rays(N, S, 25)
    nat = tc.make_decoder(32)
    nat[tc.N_ALPHA_W:tc.N_ALPHA_W + tc.HID] = 0.0
    nat[tc.N_ALPHA_B] = 0.05
    planes = tc.make_planes(scene, 33)
    planes[3][...] = 5000.0
    c, noise = _counts_and_noise(S, 7)
    # (equal depths of the dyadic grid make samples of zero length: spread them)
    z = np.ascontiguousarray(2.0 + (np.arange(S)[None, :] + 0.5) * (4.0 / S) + 0 * z, dtype=np.float32)
    out = Device(hip, planes, nat).render(F16, T(rays), T(z), noise=noise, white=1, **route[1])
    dead = torch.as_tensor(c == 0).to(DEV)
    assert bool(dead.any()) and bool((~dead).any())
    assert torch.equal(out["rgb"][dead], torch.ones_like(out["rgb"][dead])) and torch.isfinite(out["acc"]).all()
    assert torch.isnan(out["rgb"][~dead]).all()
    hip.capi.range_flag().reset()


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------------------

def test_public_surface(hip):
    from bench import make_synthetic_scene, render_options
    capi = hip.capi
    mc, mf, sid, pose = make_synthetic_scene(DEV, plane_res=64, view_res=16, seed=4)
    H = W = 264
    assert H * W >= capi.fused_min_rays()
    focal = 0.5 * W / np.tan(0.5 * 0.6911112)
    ro, rd = hip.nerf_helpers.get_ray_bundle(H, W, focal, pose)
    opts, scfg = render_options(8, 16)
    batch = torch.stack([ro.reshape(-1, 3), rd.reshape(-1, 3)], 0)
    render = lambda mode="validation": hip.train_utils.run_one_iter_of_nerf(H, W, focal, mc, mf, batch, opts, scene_id=sid, mode=mode, scene_config=scfg)
    flag = capi.range_flag()
    with torch.no_grad():
        x2 = render()
        mc.arithmetic = mf.arithmetic = "f16"
        got = render()
        assert torch.isfinite(got[0]).all() and torch.isfinite(got[3]).all() and int(flag.word) == 0 and "_f16_unfit" not in mf.__dict__
        assert not torch.equal(got[3], x2[3]), "'f16' rendered the 'f16x2' frame: a silent fall-back"
        ev = hip.train_utils.eval_nerf(H, W, focal, mc, mf, ro, rd, opts, scene_id=sid, scene_config=scfg)
        assert torch.equal(ev[3].reshape(-1, 3), got[3].reshape(-1, 3))
        # a frame below fused_min_rays(): its un-fused passes run in 'f16x2' (the decode kernels have no one-limb mode)
        Hs = Ws = 24
        ros, rds = hip.nerf_helpers.get_ray_bundle(Hs, Ws, 0.5 * Ws / np.tan(0.5 * 0.6911112), pose)
        small = lambda: hip.train_utils.eval_nerf(Hs, Ws, 0.5 * Ws / np.tan(0.5 * 0.6911112), mc, mf, ros, rds, opts, scene_id=sid, scene_config=scfg)[3].clone()
        s16 = small()
        mc.arithmetic = mf.arithmetic = "f16x2"
        assert torch.equal(s16, small()) and torch.isfinite(s16).all()
        mc.arithmetic = mf.arithmetic = "f16"
        # a weight of 300: the frame is the 'bf16x3' frame, one warning, later frames go there directly
        w = mf.density_dec["0"][1].weight
        w[5, 7] = 300.0
        with warnings.catch_warnings(record=True) as wl:
            warnings.simplefilter("always")
            healed = render()
            again = render()
        assert len([m for m in wl if "bf16x3" in str(m.message)]) == 1
        assert int(flag.word) == 0
        mc.arithmetic = mf.arithmetic = "bf16x3"
        want = render()
        assert torch.equal(healed[0], want[0]) and torch.equal(healed[3], want[3]) and torch.equal(again[3], want[3])
    # a training iteration raises before any launch
    mc.arithmetic, mf.arithmetic = None, "f16"
    with pytest.raises(capi.NvsrError, match="'f16'"):
        render("train")
    mc.arithmetic = mf.arithmetic = None
    # the entries that refuse the value
    lib = capi.lib()
    rays = hip.train_utils.pack_rays(ro, rd, 2.0, 6.0)
    N, Nc, Nf = rays.shape[0], 8, 16
    sc, keep = mc.native_scene()
    packed = mc.packed_decoder()
    o = [torch.zeros(s, device=DEV) for s in ((N, 3), (N,), (N,), (N, 3), (N,), (N,))]
    ws = torch.zeros(int(lib.nvsr_render_shared_workspace_floats(N, Nc, Nf)), device=DEV)
    p = capi.ptr
    assert lib.nvsr_render_rays_shared_arith(C.byref(sc), p(packed), N, Nc, Nf, p(rays), 0, 0, None, None, None, None, *[p(t) for t in o], p(ws), F16,
                                             capi.stream()) == ERR_SHAPE
    z = _depths(N, Nc, 1)
    grid = torch.full((int(lib.nvsr_occupancy_words(8)),), -1, dtype=torch.int32, device=DEV)
    wts = torch.zeros(N, Nc, device=DEV)
    assert lib.nvsr_render_pass_occupancy_arith(C.byref(sc), p(packed), N, Nc, p(rays), p(z), 0, 0, p(o[0]), p(o[1]), p(o[2]), p(wts), None, p(grid), 8, F16,
                                                capi.stream()) == ERR_SHAPE
    x = torch.zeros(64, 6, device=DEV)
    out = torch.zeros(64, 4, device=DEV)
    assert lib.nvsr_triplane_decode_arith(C.byref(sc), p(packed), 64, p(x), p(out), F16, capi.stream()) == ERR_SHAPE
    assert lib.nvsr_decode_rays_arith(C.byref(sc), p(packed), N, Nc, p(rays), p(z), p(ws), None, None, F16, capi.stream()) == ERR_SHAPE
    torch.cuda.synchronize()
