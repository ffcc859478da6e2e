"""GPU tests of every forward compositor, per stage, against float64 (tests/render_checks.py holds the reference, the derivation of the bounds
and the cases): render_pass_kernel (csrc/render.hip), render_pass2_kernel (render2.hip), render_pass3_coarse_kernel / render_pass3_kernel and
the kernels with their depths in registers (render3.hip: _coarse_z_, _density_, _density_z_, _colour_, _colour_z_), composite_kernel (aux.hip:
nvsr_composite, nvsr_composite_rays, nvsr_composite_mip) -- through the C ABI on buffers the test owns, every output buffer NaN before the launch.

  stage A, decoder ....... raw_out of the fused given-depth kernels against triplane_checks.forward64 at exact taps, within 2e-5 of the float64
                           range of the outputs; nvsr_coarse_z against coarse_depth64 under its rounding bound; a kernel with its depths in
                           registers against the given-depth kernel run on nvsr_coarse_z's depths, raw_out and the five outputs bit for bit
  stage B, compositor .... composite64 on the kernel's OWN raw_out: weights, acc, depth, disp and rgb of the same launch under the derived
                           bounds; then the routes that cannot write raw_out -- the two-phase route for given and in-register depths,
                           render_pass3_kernel (no weights) -- against the same float64 result and bit for bit against the fused route's
                           (nvsr_render_scratch_bytes says that the two-phase route ran); nvsr_composite* on random raw
  launches ............... noise off / on, white background off / on; the knife-edge launch (noise = -raw3 of the launch's own raw_out, moved by
                           0, +-1, +-3 ulps: sn exactly 0, barely positive, barely negative, the 1e10 last sample included); the NaN / inf launch
  the NaN rule ........... a NaN density (and inf x 0) makes the weights from that sample on NaN and the ray's acc, depth, disp and rgb NaN;
                           earlier weights are those of the launch without it; +inf on an interval of positive length is an opaque sample and
                           -inf a dead one, both finite.  No compositor may turn a NaN into a finite wrong number.
Shapes (render_checks.FUSED_SHAPES, COMPOSITE_SHAPES): N = 1, 33, 293, 2305 and 4096 + 513 (two blocks of the ray order) by S = 1, 2, 3, 33, 65;
composite_kernel at S = 1, 63, 64, 65, 129, 192.

What these tests found: render_pass_kernel and composite_kernel applied relu(sigma + noise) with fmaxf, which returns its non-NaN operand -- a
NaN density became an empty sample and the pixel came out finite.  Both now use the compare + select of composite_sample (side_work.h).
Measured on an MI355X, worst err / bound over all cases, launches and routes: weights 0.50 (one rounding against its allowance), acc 0.22, depth
0.35, disp 0.22, rgb 0.33; raw_out within 0.04 of the decoder tolerance; nvsr_coarse_z 0.50; 375 tests in 5 s (profiles/render_forward_edges.txt,
with the mutation checks).
"""
import ctypes as C
import functools
import time
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import render_checks as rc
import triplane_checks as tc
from nerf_baseline_checks import DEV, T
from two_phase_checks import _env

pytestmark = pytest.mark.gpu

KERNELS = [("v1", "f32"), ("pass2", "f32"), ("pass3", "bf16x3"), ("pass3", "f16x2")]
FUSED = rc.fused_cases()
RUNS = [(c, k, a) for c in FUSED for k, a in KERNELS if k == "pass3" or (c.N, c.S) != rc.TWO_PHASE_SHAPE]
RUNS3 = [r for r in RUNS if r[1] == "pass3"]
_id = lambda p: "%s-%s-%s" % (p[1], p[2], rc.case_id(p[0]))
T0 = time.time()


def N_(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def _inputs(i):
    """case i -> scene, rays, z (numpy) and forward64's raw [N, S, 4] (float64), shared by the four kernels"""
    c = FUSED[i]
    scene, rays, z = rc.make_inputs(c)
    dec = tc.unpack(rc.make_decoder())
    planes = [torch.as_tensor(p).double() for p in rc.make_planes(scene)]
    raw = tc.forward64(dec, planes, rays, z, scene)[0].numpy().reshape(c.N, c.S, 4)
    return scene, rays, z, raw


@functools.lru_cache(maxsize=None)
def _decoder_range():
    """the float64 range of the decoder's outputs on the tests' scene: max |rgb logit| and max |sigma| over the 293 x 33 case"""
    raw = _inputs([rc.case_id(c) for c in FUSED].index("293x33"))[3]
    return float(np.abs(raw[..., :3]).max()), float(np.abs(raw[..., 3]).max())


class Device:
    """the scene, the planes and the packed decoder on the device (one per module)"""

    def __init__(self, hip):
        self.capi = capi = hip.capi
        scene = tc.make_scene(rc.SIZES)
        self.planes = [T(p) for p in rc.make_planes(scene)]
        self.nat = T(rc.make_decoder())
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

    def render(self, kernel, arith, rays, z, noise, white, weights=True, raw=True, lindisp=0, two_phase=False):
        """one render pass -> NS of numpy outputs (weights / raw None where not requested).  z None: the depths in registers.  two_phase: the
        density + colour kernels (no raw_out), asserted by the scratch they alone allocate."""
        capi, p = self.capi, self.capi.ptr
        lib = capi.lib()
        N, S = rays.shape[0], (z.shape[1] if z is not None else noise.shape[1])
        nan = lambda *s: torch.full(s, float("nan"), device=DEV)
        o = NS(rgb=nan(N, 3), disp=nan(N), acc=nan(N), depth=nan(N), weights=nan(N, S) if weights else None, raw=nan(N, S, 4) if raw else None)
        r_, z_, n_ = T(rays), (T(z) if z is not None else None), (T(noise) if noise is not None else None)
        tail = (int(white), p(o.rgb), p(o.disp), p(o.acc), p(o.weights), p(o.depth), p(o.raw))
        assert not (two_phase and raw)
        assert lib.nvsr_release_render_scratch() == 0
        with _env(NVSR_RENDER_ONE_PHASE="0" if two_phase else "1"):
            if kernel == "v1":
                assert N < 16384
                capi.call("nvsr_render_pass_arith", C.byref(self.sc), p(self.packed), N, S, p(r_), p(z_), p(n_), *tail, capi.ARITHMETIC[arith], capi.stream())
            elif kernel == "pass2":
                capi.call("nvsr_render_pass2_launch", C.byref(self.sc), p(self.packed), N, S, p(r_), p(z_), p(n_), *tail, capi.stream())
            elif z is not None:
                capi.call("nvsr_render_pass3_launch", capi.ARITHMETIC[arith], C.byref(self.sc), p(self.packed), N, S, p(r_), p(z_), p(n_), *tail, capi.stream())
            else:
                capi.call("nvsr_render_pass3_coarse_z_launch", capi.ARITHMETIC[arith], C.byref(self.sc), p(self.packed), N, S, p(r_), int(lindisp), p(n_), *tail,
                          capi.stream())
            torch.cuda.synchronize()
        assert lib.nvsr_render_scratch_bytes() == (2 * 4 * N * S + 4 * N if two_phase else 0), "the %s route did not run" % ("two-phase" if two_phase else "fused")
        return NS(**{k: (None if v is None else N_(v)) for k, v in vars(o).items()})

    def coarse_z(self, rays, S, lindisp):
        z, r_ = torch.full((rays.shape[0], S), float("nan"), device=DEV), T(rays)
        self.capi.call("nvsr_coarse_z", rays.shape[0], S, self.capi.ptr(r_), int(lindisp), None, self.capi.ptr(z), self.capi.stream())
        torch.cuda.synchronize()
        return N_(z)


@pytest.fixture(scope="module")
def dev(hip):
    d = Device(hip)
    yield d
    hip.capi.lib().nvsr_release_render_scratch()
    if hip.capi._range_flag is not None:             # the NaN launches raise the f16x2 range flag of a process that registered one
        hip.capi._range_flag.reset()


def _same(a, b):
    """bit for bit, a NaN equal to a NaN"""
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.nan_to_num(a, nan=0.0).view(np.uint32), np.nan_to_num(b, nan=0.0).view(np.uint32))


def _launch_list(c, z, raw3):
    """(name, noise, white) of the launches of a case, from the first launch's own raw3; the knife mask; the special positions"""
    on = rc.make_noise(c, raw3)
    knife, mask = rc.knife_noise(c, raw3, on)
    special, where = rc.special_noise(c, z, on)
    return [("plain", None, 0), ("white", None, 1), ("noise", on, 0), ("noise+white", on, 1), ("knife", knife, 0), ("special", special, 1)], mask, where


def _check(tag, got, ref, outputs=rc.OUTPUTS):
    """every output of a launch against composite64's under the bounds -> {output: worst err / bound}"""
    rep = {}
    for name in outputs:
        g = getattr(got, name)
        assert g is not None
        rep[name] = rc.compare(tag, name, g, getattr(ref, name), getattr(ref.bound, name))
    print("render_forward_edges ratio | %s | %s" % (tag, " ".join("%s=%.3f" % kv for kv in rep.items())))
    return rep


_RUNS = {}


def _run(dev, c, kernel, arith):
    """the fused launches of one (case, kernel, arithmetic), each with its float64 reference from its own raw_out"""
    key = (rc.case_id(c), kernel, arith)
    if key in _RUNS:
        return _RUNS[key]
    scene, rays, z, raw64 = _inputs(FUSED.index(c))
    first = dev.render(kernel, arith, rays, z, None, 0)
    launches, mask, where = _launch_list(c, z, first.raw[..., 3])
    r = NS(c=c, kernel=kernel, arith=arith, rays=rays, z=z, raw64=raw64, mask=mask, where=where, tag="%s %s %s" % (kernel, arith, rc.case_id(c)), L={})
    for name, noise, white in launches:
        got = first if name == "plain" else dev.render(kernel, arith, rays, z, noise, white)
        r.L[name] = NS(noise=noise, white=white, got=got, ref=rc.composite64(got.raw, z, rays, noise, white))
    _RUNS[key] = r
    return r


@pytest.fixture(scope="module", params=RUNS, ids=_id)
def run(request, dev):
    return _run(dev, *request.param)


@pytest.fixture(scope="module", params=RUNS3, ids=_id)
def run3(request, dev):
    return _run(dev, *request.param)


# ---- stage A ------------------------------------------------------------------------------------------------------------------------------------

def test_decoder_raw_out_equals_float64(run):
    """raw_out of the fused given-depth kernel against forward64 at exact taps: 2e-5 of the float64 range (rgb logits and sigma apart: the
    density head is scaled); the decoder does not see the noise or the background: every launch writes the same bits"""
    r = run
    raw = r.L["plain"].got.raw
    assert np.isfinite(raw).all(), r.tag
    for name, l in r.L.items():
        assert _same(l.got.raw, raw), "%s %s: raw_out differs from the plain launch's" % (r.tag, name)
    rng_c, rng_s = _decoder_range()
    err_c = float(np.abs(raw[..., :3] - r.raw64[..., :3]).max()) / rng_c
    err_s = float(np.abs(raw[..., 3] - r.raw64[..., 3]).max()) / rng_s
    print("render_forward_edges decoder | %s | rgb=%.3f sigma=%.3f (of 2e-5 of the range)" % (r.tag, err_c / rc.DECODER_TOLERANCE, err_s / rc.DECODER_TOLERANCE))
    assert err_c <= rc.DECODER_TOLERANCE, "%s rgb logits: %.3g of the range %.3g" % (r.tag, err_c, rng_c)
    assert err_s <= rc.DECODER_TOLERANCE, "%s sigma: %.3g of the range %.3g" % (r.tag, err_s, rng_s)


@pytest.mark.parametrize("lindisp", [0, 1])
@pytest.mark.parametrize("S", [1, 2, 3, 33, 65])
def test_coarse_z_equals_coarse_depth64(dev, S, lindisp):
    rays = rc.z_rays(np.zeros((293, 11), np.float32), 5)
    got = dev.coarse_z(rays, S, lindisp).astype(np.float64)
    z, bound = rc.coarse_depth64(rays[:, 6], rays[:, 7], np.arange(S), S, lindisp)
    ratio = float((np.abs(got - z) / bound).max())
    print("render_forward_edges ratio | coarse_z S=%d lindisp=%d | z=%.3f" % (S, lindisp, ratio))
    assert ratio <= 1.0, (S, lindisp, ratio)


# ---- stage B ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("launch", ["plain", "white", "noise", "noise+white", "knife"])
def test_compositor_within_the_bounds(run, launch):
    r, l = run, run.L[launch]
    _check("%s %s" % (r.tag, launch), l.got, l.ref)
    if launch == "noise":
        rc.assert_live_mix(r.tag, l.ref.live, r.c.S, r.c.N)
    if launch == "knife" and r.c.N >= 8:
        sn = l.ref.sn[r.mask]
        assert (sn == 0).any() and (sn > 0).any() and (sn < 0).any(), r.tag


def _assert_rule(tag, got, base, where):
    """the NaN rule on a kernel's outputs (`base`: the same launch without the special values)"""
    for kind in (5, 6, 7, 2):
        for i, s in where.get(kind, []):
            what = "%s ray %d (%s at sample %d)" % (tag, i, "inf x 0" if kind == 2 else "NaN", s)
            if got.weights is not None:
                assert np.isnan(got.weights[i, s:]).all(), what + ": a weight from that sample on is not NaN"
                assert _same(got.weights[i, :s], base.weights[i, :s]), what + ": an earlier weight changed"
            for name in ("acc", "depth", "disp", "rgb"):
                assert np.isnan(getattr(got, name)[i]).all(), what + ": %s is finite" % name
    for kind in (1, 3):
        for i, s in where.get(kind, []):
            for name in ("acc", "depth", "rgb"):
                assert np.isfinite(getattr(got, name)[i]).all(), "%s ray %d (%sinf at sample %d): %s is not finite" % (tag, i, "+-"[kind == 3], s, name)


def test_nan_and_inf_densities(run):
    """the rule for the fused kernels: NaNs exactly where composite64 puts them, every finite element within its bound"""
    r, l = run, run.L["special"]
    _assert_rule(r.tag, l.got, r.L["noise+white"].got, r.where)
    _check("%s special" % r.tag, l.got, l.ref)


@pytest.mark.parametrize("launch", ["plain", "noise+white", "knife", "special"])
def test_routes_without_raw_out(run3, dev, launch):
    """the two-phase route (density + colour kernels) with and without the weights, and render_pass3_kernel (fused, no weights): against the
    float64 result of the fused launch's raw_out, and bit for bit against the fused coarse kernel"""
    r, l = run3, run3.L[launch]
    for route, kw in (("two-phase", dict(two_phase=True)), ("two-phase no weights", dict(two_phase=True, weights=False)), ("fused no weights", dict(weights=False))):
        got = dev.render(r.kernel, r.arith, r.rays, r.z, l.noise, l.white, raw=False, **kw)
        tag = "%s %s %s" % (r.tag, launch, route)
        names = [n for n in rc.OUTPUTS if getattr(got, n) is not None]
        if launch == "special":
            _assert_rule(tag, got, r.L["noise+white"].got, r.where)
        _check(tag, got, l.ref, names)
        for n in names:
            assert _same(getattr(got, n), getattr(l.got, n)), "%s: %s is not the fused route's bit for bit" % (tag, n)


@pytest.mark.parametrize("lindisp", [0, 1])
def test_depths_in_registers(run3, dev, lindisp):
    """render_pass3_coarse_z_kernel against render_pass3_coarse_kernel on nvsr_coarse_z's depths (near and far per ray, some equal): raw_out and
    the five outputs bit for bit; both against composite64; then the two-phase route with its depths in registers"""
    r = run3
    rays = rc.z_rays(r.rays, r.c.seed)
    z = dev.coarse_z(rays, r.c.S, lindisp)
    plain = dev.render("pass3", r.arith, rays, z, None, 0)
    launches, _, where = _launch_list(r.c, z, plain.raw[..., 3])
    base = None
    for name, noise, white in launches:
        if name not in ("noise", "noise+white", "special"):      # (the launch takes S from the noise where there are no depths)
            continue
        tag = "%s lindisp=%d %s" % (r.tag, lindisp, name)
        given = dev.render("pass3", r.arith, rays, z, noise, white)
        ref = rc.composite64(given.raw, z, rays, noise, white)
        _check(tag + " given", given, ref)
        for route, kw in (("in registers", dict(raw=True)), ("in registers two-phase", dict(raw=False, two_phase=True))):
            got = dev.render("pass3", r.arith, rays, None, noise, white, lindisp=lindisp, **kw)
            if kw["raw"]:
                assert _same(got.raw, given.raw), "%s %s: raw_out is not the given-depth kernel's" % (tag, route)
            for n in rc.OUTPUTS:
                assert _same(getattr(got, n), getattr(given, n)), "%s %s: %s is not the given-depth kernel's bit for bit" % (tag, route, n)
            if name == "special":
                _assert_rule(tag + " " + route, got, base, where)
        if name == "noise+white":
            base = given


# ---- composite_kernel ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("entry", ["nvsr_composite", "nvsr_composite_rays", "nvsr_composite_mip"])
@pytest.mark.parametrize("c", rc.composite_cases(), ids=rc.case_id)
def test_composite_kernel(hip, c, entry):
    capi, p = hip.capi, hip.capi.ptr
    mip = entry.endswith("mip")
    scene, rays, z = rc.make_inputs(c)
    if mip:
        z = np.concatenate([z, z[:, -1:] + np.float32(0.25)], -1)
    raw = rc.make_raw(c)
    on = rc.make_noise(c, raw[..., 3])
    knife, mask = rc.knife_noise(c, raw[..., 3], on, mip)
    special, where = rc.special_noise(c, z[:, :c.S], on)
    d = T(rays) if entry.endswith("rays") else T(np.ascontiguousarray(rays[:, 3:6]))
    raw_, z_ = T(raw), T(z)
    base = None
    for name, noise, white in (("plain", None, 0), ("white", None, 1), ("noise", on, 0), ("noise+white", on, 1), ("knife", knife, 0), ("special", special, 1)):
        nan = lambda *s: torch.full(s, float("nan"), device=DEV)
        o = NS(rgb=nan(c.N, 3), disp=nan(c.N), acc=nan(c.N), weights=nan(c.N, c.S), depth=nan(c.N))
        n_ = T(noise) if noise is not None else None
        capi.call(entry, c.N, c.S, p(raw_), p(z_), p(d), p(n_), white, p(o.rgb), p(o.disp), p(o.acc), p(o.weights), p(o.depth), capi.stream())
        torch.cuda.synchronize()
        got = NS(**{k: N_(v) for k, v in vars(o).items()})
        ref = rc.composite64(raw, z, rays, noise, white, mip=mip)
        tag = "%s %s %s" % (entry, rc.case_id(c), name)
        if name == "special":
            _assert_rule(tag, got, base, where)
        _check(tag, got, ref)
        if name == "noise+white":
            base = got


def test_wall_time_of_this_file():
    print("render_forward_edges wall | %.1f s since the module was imported" % (time.time() - T0))
