"""GPU tests of the backward compositor, per sample, against float64 (tests/render_backward_checks.py holds the reference backward64, the
derivation of its bound and the cases): composite_backward_kernel (csrc/render_bwd.hip) through nvsr_composite_backward_depth and _rays on every
launch, and through nvsr_composite_backward and _mip on the launches they can express -- through the C ABI on buffers the test owns, g_raw NaN
before the launch; the entry points must give the same bits.

  shapes ................. render_checks.COMPOSITE_SHAPES (1x1, 33x63, 33x64, 5x65, 33x129, 37x192: the training S) + 6x2, 33x3, 5x511, 9x512 (the LDS
                           arrays are [4][512]), each with mip off and on
  launches ............... plain, white, noise, noise+white (g_acc / g_dep given or NULL as the table of render_backward_checks.LAUNCHES says), the
                           knife-edge launch (sn exactly 0, barely positive, barely negative: the gate is >, and +0.0 at sn == 0), the NaN / inf launch
  stage A ................ rgb logits of exactly 0 and g_rgb = (4, 4, 4): g_raw[..., c] is then the backward's own weight w, compared bit for bit with
                           the `weights` of nvsr_composite / nvsr_composite_mip (noise, knife and special launches) -- "the transmittances recomputed
                           here are the forward's bit for bit", and the forward's weights are held under bounds by test_render_forward_edges.py
  the NaN rule ........... a NaN density at (ray, s), or inf x 0, makes g_raw[ray, s, 3] NaN, every g_raw[ray, k, 3] NaN for k < s with sn > 0 (a gated-off
                           sample keeps +0.0) and every g_raw[ray, k, 0..2] NaN for k >= s; other rays are untouched; +inf on an interval of positive
                           length, -inf and a zero direction give finite gradients
  refusals, operator ..... S = 513 -> NVSR_ERR_SHAPE with g_raw untouched, N = 0 -> OK, no g_rgb -> NVSR_ERR_NULL, torch.ops.nvsr.composite_backward
                           raises NotImplementedError; autograd of torch.ops.nvsr.composite with a gradient on disp: empty rays (q NaN) and clamped
                           rays (q < 1e-10) get the bits of the launch without it, the others backward64 at the folded g_acc / g_depth

What these tests found: the kernel gated the density gradient with (sn > 0) ? g : 0, which stores 0 at a NaN density where relu's backward passes
the gradient through (NaN).  The select is now (sn <= 0) ? 0 : g.  Depending on the fix: check_rule's "the density gradient of that sample is not
NaN" in test_nan_rule and the NaN pattern of test_within_the_bound[*-special]; nothing else.  Reading the kernel for the bound also showed that the
exclusive suffix is formed as (inclusive - own_s) + carry: a rounding term gamma_m |w_s gw_s| that does not hold fac_s is divided by fac_s.  The
computed 1 - alpha the output multiplies by cancels it (fac >= 1 - alpha), so it stays small; the bound names it ("- own") and the kernel is unchanged.
Measured on an MI355X, worst err / bound over all cases, launches and entry points: 0.49 on the colour columns and 0.48 on g_sigma in front of a
ray's first saturated sample (alpha exactly 1), 1.000 at and behind it, where the bound states the kernel's value; stage A is exact on the device
(expf(-0) == 1, 1 / 2 == 0.5) and the weights were the forward's bits in all 60 launches; without the fix 32 tests fail (test_nan_rule and
test_within_the_bound[*-special] of the 16 pairs that hold a NaN); 206 tests in 6.4 s (profiles/render_backward_edges.txt).
"""
import time

import numpy as np
import pytest
import torch

import render_backward_checks as bc
import render_checks as rc
from nerf_baseline_checks import DEV, T

pytestmark = pytest.mark.gpu

T0 = time.time()
PAIRS = [(i, mip) for i in range(len(bc.CASES)) for mip in (0, 1)]
PAIR_IDS = ["%s-%s" % (bc.IDS[i], "mip" if mip else "plain") for i, mip in PAIRS]
NVSR_OK, NVSR_ERR_SHAPE, NVSR_ERR_NULL = 0, 1, 3
WORST = {}


def N_(t):
    return t.detach().cpu().numpy()


def _same(a, b):
    """bit for bit, a NaN equal to a NaN"""
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.nan_to_num(a, nan=0.0).view(np.uint32), np.nan_to_num(b, nan=0.0).view(np.uint32))


def backward(hip, entry, raw, z, rays, noise, white, mip, g_rgb, g_acc, g_dep):
    """one launch of an entry point on fresh device buffers, g_raw NaN before it -> g_raw [N, S, 4] (numpy)"""
    capi, p = hip.capi, hip.capi.ptr
    N, S = raw.shape[:2]
    d = T(rays) if entry.endswith("rays") else T(rays[:, 3:6])
    opt = lambda a: None if a is None else T(a)
    raw_, z_, n_, g_, ga_, gd_ = T(raw), T(z), opt(noise), T(g_rgb), opt(g_acc), opt(g_dep)
    out = torch.full((N, S, 4), float("nan"), device=DEV)
    head = (N, S, p(raw_), p(z_), p(d), p(n_), int(white), p(g_), p(ga_))
    if entry in ("nvsr_composite_backward_depth", "nvsr_composite_backward_rays"):
        capi.call(entry, *head, p(gd_), int(mip), p(out), capi.stream())
    else:
        assert g_dep is None and bool(mip) == entry.endswith("_mip")
        capi.call(entry, *head, p(out), capi.stream())
    torch.cuda.synchronize()
    return N_(out)


def forward_weights(hip, raw, z, rays, noise, white, mip):
    capi, p = hip.capi, hip.capi.ptr
    N, S = raw.shape[:2]
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)
    rgb, disp, acc, w, depth = nan(N, 3), nan(N), nan(N), nan(N, S), nan(N)
    raw_, z_, d, n_ = T(raw), T(z), T(rays[:, 3:6]), (None if noise is None else T(noise))
    capi.call("nvsr_composite_mip" if mip else "nvsr_composite", N, S, p(raw_), p(z_), p(d), p(n_), int(white), p(rgb), p(disp), p(acc), p(w), p(depth),
              capi.stream())
    torch.cuda.synchronize()
    return N_(w), N_(acc), N_(depth)


_GOT = {}


def _got(hip, i, mip, name):
    """g_raw of a launch through every entry point that can express it, asserted to be the same bits -> the _depth entry point's"""
    key = (i, mip, name)
    if key not in _GOT:
        p = bc.inputs(i, mip)
        l = p.L[name]
        entries = ["nvsr_composite_backward_depth", "nvsr_composite_backward_rays"]
        if l.g_dep is None:
            entries.append("nvsr_composite_backward_mip" if mip else "nvsr_composite_backward")
        got = [backward(hip, e, p.raw, p.z, p.rays, l.noise, l.white, mip, p.g_rgb, l.g_acc, l.g_dep) for e in entries]
        for e, g in zip(entries[1:], got[1:]):
            assert _same(g, got[0]), "%s %s: %s does not give the bits of %s" % (PAIR_IDS[PAIRS.index((i, mip))], name, e, entries[0])
        _GOT[key] = got[0]
    return _GOT[key]


@pytest.mark.parametrize("name", bc.LAUNCH_NAMES)
@pytest.mark.parametrize("i,mip", PAIRS, ids=PAIR_IDS)
def test_within_the_bound(hip, i, mip, name):
    """NaN exactly where backward64 is NaN, every other element within its own bound; the entry points give the same bits"""
    tag = "%s %s" % (PAIR_IDS[PAIRS.index((i, mip))], name)
    rep = bc.compare(tag, _got(hip, i, mip, name), bc.reference(i, mip, name))
    for k, v in rep.items():
        WORST[k] = max(WORST.get(k, 0.0), v)


@pytest.mark.parametrize("i,mip", PAIRS, ids=PAIR_IDS)
def test_nan_rule(hip, i, mip):
    p = bc.inputs(i, mip)
    l = p.L["special"]
    got = _got(hip, i, mip, "special")
    base = backward(hip, "nvsr_composite_backward_depth", p.raw, p.z, p.rays, p.L["noise"].noise, l.white, mip, p.g_rgb, l.g_acc, l.g_dep)
    bc.check_rule(PAIR_IDS[PAIRS.index((i, mip))], got.astype(np.float64), bc.reference(i, mip, "special").sn, p.where, base.astype(np.float64))


def test_knife_edge_gate(hip):
    """sn == 0 stores +0.0 (relu's subgradient) and the smallest positive sn a gradient that is not 0, on samples of positive length"""
    i = bc.IDS.index("33x64")
    p, got, ref = bc.inputs(i, 0), _got(hip, i, 0, "knife"), bc.reference(i, 0, "knife")
    zero = p.mask & (ref.sn == 0)
    pos = p.mask & (ref.sn > 0) & (ref.g_raw[..., 3] != 0) & (np.abs(ref.g_raw[..., 3]) > 4 * ref.bound[..., 3])
    assert zero.any() and pos.any()
    assert (got[..., 3][zero] == 0).all() and not np.signbit(got[..., 3][zero]).any()
    assert (got[..., 3][pos] != 0).all()


# ---- stage A: the backward's weights are the forward's bits -----------------------------------------------------------------------------------------

def test_stage_a_premise(hip):
    """expf(-0) is 1 and 1 / 2 is 0.5 on the device: one sample of weight exactly 1 (alpha = 1, T = 1) must come back as exactly 1.0 from
    ((w 4) c)(1 - c) with c = 1 / (1 + expf(-0))"""
    raw = np.array([[[0, 0, 0, 1e4]]], np.float32)
    rays = np.zeros((1, 11), np.float32)
    rays[0, 5] = 1.0
    g = backward(hip, "nvsr_composite_backward_depth", raw, np.full((1, 1), 2, np.float32), rays, None, 0, 0, np.full((1, 3), 4, np.float32), None, None)
    print("render_backward_edges stage A premise | g_raw[0, 0, :3] = %r (exactly 1.0: expf(-0) == 1 and 1 / 2 exact)" % (g[0, 0, :3].tolist(),))
    assert (g[0, 0, :3] == 1.0).all()


@pytest.mark.parametrize("name", ["noise", "knife", "special"])
@pytest.mark.parametrize("i,mip", PAIRS, ids=PAIR_IDS)
def test_stage_a_weights_are_the_forwards_bits(hip, i, mip, name):
    p = bc.inputs(i, mip)
    l = p.L[name]
    raw = p.raw.copy()
    raw[..., :3] = 0.0
    g = backward(hip, "nvsr_composite_backward_depth", raw, p.z, p.rays, l.noise, 0, mip, np.full((p.c.N, 3), 4, np.float32), None, None)
    w = forward_weights(hip, raw, p.z, p.rays, l.noise, 0, mip)[0]
    ok = (w == 0) | (np.abs(w) >= 2.0 ** -126) | np.isnan(w)                 # (a subnormal weight times 4 may leave the subnormals: not compared)
    assert ok.mean() > 0.99
    for c in range(3):
        col = g[..., c]
        assert np.array_equal(np.isnan(col), np.isnan(w)), "%s %s column %d: NaN pattern" % (PAIR_IDS[PAIRS.index((i, mip))], name, c)
        m = ok & ~np.isnan(w)
        bad = m & (col != w)
        assert not bad.any(), "%s %s column %d: %d weights differ from the forward's, the first at %s: %r against %r" % (
            PAIR_IDS[PAIRS.index((i, mip))], name, c, int(bad.sum()), tuple(np.argwhere(bad)[0]), col[tuple(np.argwhere(bad)[0])], w[tuple(np.argwhere(bad)[0])])


# ---- refusals and the operator -------------------------------------------------------------------------------------------------------------------------

def test_refusals(hip):
    capi, p = hip.capi, hip.capi.ptr
    lib = capi.lib()
    N, S = 3, 513
    raw, z, rd, g = torch.zeros(N, S, 4, device=DEV), torch.zeros(N, S + 1, device=DEV), torch.ones(N, 3, device=DEV), torch.ones(N, 3, device=DEV)
    out = torch.full((N, S, 4), float("nan"), device=DEV)
    for entry, tail in (("nvsr_composite_backward_depth", (None, 0)), ("nvsr_composite_backward_rays", (None, 1)), ("nvsr_composite_backward", ()),
                        ("nvsr_composite_backward_mip", ())):
        d = torch.ones(N, 11, device=DEV) if entry.endswith("rays") else rd
        call = lambda n, s, g_: getattr(lib, entry)(n, s, p(raw), p(z), p(d), None, 0, p(g_), None, *tail, p(out), capi.stream())
        assert call(N, S, g) == NVSR_ERR_SHAPE, entry
        assert call(0, 512, g) == NVSR_OK, entry
        assert call(N, 512, None) == NVSR_ERR_NULL, entry
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all()), entry + ": a refused launch wrote g_raw"
    with pytest.raises(NotImplementedError):
        torch.ops.nvsr.composite_backward(raw, z[:, :S], rd, None, False, False, g, None, None)
    with pytest.raises(NotImplementedError):
        torch.ops.nvsr.composite_backward(raw, z, rd, None, False, True, g, None, None)


@pytest.mark.parametrize("mip", [0, 1], ids=["plain", "mip"])
def test_operator_folds_the_gradient_of_disp(hip, mip):
    """autograd of torch.ops.nvsr.composite on 33 x 65 with a gradient on disp_map = 1 / max(1e-10, depth / acc)"""
    from types import SimpleNamespace as NS
    c = NS(N=33, S=65, seed=430, grid=7)
    _, rays, z = rc.make_inputs(c)
    if mip:
        z = np.concatenate([z, z[:, -1:] + bc.MIP_TAIL], -1)
    raw = rc.make_raw(c)
    noise = rc.make_noise(c, raw[..., 3])
    clamp = np.arange(c.N) % 8 == 2                                           # depths near 5e-11: q = depth / acc is below 1e-10 (scaled by 2^-36: exact)
    z[clamp] *= np.float32(2.0 ** -36)
    raw[clamp, :, 3] = np.where(noise[clamp] == np.float32(rc.DEAD), np.float32(-1), np.float32(2.0 ** 38))
    noise[clamp] = 0
    rng = np.random.default_rng(c.seed + 90)
    g_rgb, g_disp, g_acc, g_dep = (rng.standard_normal(s).astype(np.float32) for s in ((c.N, 3), c.N, c.N, c.N))
    rd = np.ascontiguousarray(rays[:, 3:6])

    def grad(with_disp):
        rt = T(raw).requires_grad_(True)
        rgb, disp, acc, w, depth = torch.ops.nvsr.composite(rt, T(z), T(rd), T(noise), False, bool(mip))
        outs, gs = [rgb, acc, depth], [T(g_rgb), T(g_acc), T(g_dep)]
        if with_disp:
            outs, gs = outs + [disp], gs + [T(g_disp)]
        return N_(torch.autograd.grad(outs, rt, gs)[0]), N_(acc).astype(np.float64), N_(depth).astype(np.float64)

    got, acc, depth = grad(True)
    base = grad(False)[0]
    with np.errstate(all="ignore"):
        q = depth / acc
    empty, clamped, live = acc == 0, (acc != 0) & (q < 1e-10), q > 1e-10
    assert empty.any() and np.isnan(q[empty]).all() and clamped[clamp].all() and clamped.sum() >= 4 and live.sum() >= 16
    assert _same(got[empty], base[empty]), "an empty ray's gradient changed with a gradient on disp"
    assert _same(got[clamped], base[clamped]), "a clamped ray's gradient changed with a gradient on disp"
    assert not _same(got[live], base[live])
    # the fold in float64 from the kernel's own acc and depth; fold_disp_grad rounds q, q q, the quotient, dq / acc (gd: gamma_5 with the doubled
    # rounding of q), and dq depth, acc acc, their quotient on top (ga: gamma_8), then the addition to the incoming gradient
    with np.errstate(all="ignore"):
        dq = np.where(live, -g_disp.astype(np.float64) / (q * q), 0.0)
        gd = np.where(live, dq / acc, 0.0)
        ga = np.where(live, -dq * depth / (acc * acc), 0.0)
    ga64, gd64 = g_acc + ga, g_dep + gd
    e_ga, e_gd = rc._rnd(ga64, rc.gamma(8) * np.abs(ga)), rc._rnd(gd64, rc.gamma(5) * np.abs(gd))
    ref = bc.backward64(raw, z, rays, noise, 0, bool(mip), g_rgb, ga64, gd64, e_acc=e_ga, e_dep=e_gd)
    bc.compare("operator 33x65 %s" % ("mip" if mip else "plain"), got, ref)


def test_wall_time_of_this_file():
    print("render_backward_edges worst | %s" % " ".join("%s=%.3f" % kv for kv in sorted(WORST.items())))
    print("render_backward_edges wall | %.1f s since the module was imported" % (time.time() - T0))
