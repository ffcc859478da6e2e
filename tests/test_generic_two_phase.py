"""The generic decoder geometries' frame in two phases (csrc/generic_fused.hip and csrc/generic_fused_limb.hip compiled per phase,
csrc/generic_live.hip; torch.ops.nvsr.triplane_density_generic_fused_arith, triplane_colour_generic_fused_arith, generic_live_list;
TwoDimPlanesModel.density_field, colour_field_, generic_frame_route): each phase against the BITS of the one-launch kernel at the same points,
in f32 and in 'f16x2'; what the colour phase must leave alone; the live list against its numpy statement (tests/generic_two_phase_ref.py);
frames through eval_nerf, two phases against one, every returned tensor; the range flag and the healing; the routing; opcheck.
"Equal": test_generic_fused.same -- the same NaN positions and the same bits everywhere else."""
import warnings

import numpy as np
import pytest
import torch

import generic_two_phase_ref as ref
from conftest import load_golden
from test_generic_fused import SHAPES, SID, op_args, points, random_model, same
from test_generic_limb import flag_of, pack
from test_hip_parity import DEV, N_, T, make_options
from test_oracle import G18_VARIANTS, G22_BOX

pytestmark = pytest.mark.gpu
F32, F16X2 = 0, 2
ARITHS = {"f32": F32, "f16x2": F16X2}
SENTINEL = -7.25
nv = torch.ops.nvsr


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def args_of(m, x, arith, noise=None):
    """(head, tail) of the phase operators' arguments around (index, count): the model's geometry, planes and weights on the points x"""
    planes, consts, nat, geometry = op_args(m)
    packed = pack(m) if arith == F16X2 else nat.new_empty(0)
    return (planes, consts, nat, packed, geometry, T(x)), (bool(m.align_corners), None if noise is None else T(noise), m.plane_interp == "bicubic", arith)


def one_launch(m, x, arith, noise=None):
    head, tail = args_of(m, x, arith, noise)
    return N_(nv.triplane_decode_generic_fused_arith(*head, *tail))


def density(m, x, arith, noise=None):
    head, tail = args_of(m, x, arith, noise)
    return N_(nv.triplane_density_generic_fused_arith(*head, *tail))


def colour(m, x, arith, raw, index, count, noise=None, max_count=-1):
    """the colour phase on a copy of raw (numpy) with the list index[:count]; index may hold more entries than count"""
    head, tail = args_of(m, x, arith, noise)
    buf = T(raw).contiguous()
    nv.triplane_colour_generic_fused_arith(buf, *head, torch.as_tensor(np.asarray(index, np.int32), device=DEV),
                                           torch.tensor([count], dtype=torch.int32, device=DEV), *tail, max_count)
    return N_(buf)


def fixture_models(hip):
    """(name, model, the fixture's points, its jitter or None) for every g18 geometry and every g22 option"""
    from test_hip_round2 import _variant_model
    from test_hip_round4 import _g22_model
    g = load_golden("g18_decoder_variants.npz")
    for name in G18_VARIANTS:
        yield name, _variant_model(hip, g, name)[0], g[name + ".x"], None
    g = load_golden("g22_model_options.npz")
    for name, n_pos, over in (("align_false", 3, dict(align_corners=False, dec_channels=64)), ("planes5", 5, dict(dec_channels=64)), ("noise", 3, {}),
                              ("bicubic", 3, dict(plane_interp="bicubic", dec_channels=64)),
                              ("bicubic_noalign", 3, dict(plane_interp="bicubic", align_corners=False, dec_channels=64))):
        yield name, _g22_model(hip, g, name, n_planes=n_pos, **over), g[name + ".x"], g["noise.jitter"] if name == "noise" else None


def check_density(m, x, arith, noise=None, what=""):
    full = one_launch(m, x, arith, noise)
    raw = density(m, x, arith, noise)
    assert raw.shape == full.shape and same(raw[:, 3], full[:, 3]), what
    assert not bits(raw[:, :3]).any(), what                    # +0.0 bit for bit
    return full, raw


def check_colour(m, x, arith, full, noise=None, what="", seed=0):
    """sentinel-filled raw, a shuffled list of `count` points followed by further valid, distinct indices the kernel must not read"""
    P = x.shape[0]
    order = np.random.default_rng(seed).permutation(P).astype(np.int32)
    before = np.full((P, 4), SENTINEL, np.float32)
    for count in sorted({0, 1, 31, 32, 33, P} & set(range(P + 1))):
        got = colour(m, x, arith, before, order, count, noise)
        assert same(got, ref.colour_raw(before, full, order[:count])), (what, count)
        assert (got[:, 3] == SENTINEL).all() and (got[order[count:]] == SENTINEL).all(), (what, count)


@pytest.mark.parametrize("arith", list(ARITHS))
@pytest.mark.parametrize("case", list(SHAPES))
def test_phases_equal_the_one_launch_kernel_on_every_shape(hip, case, arith):
    """seeded weights, 10 x 10 planes, 100 points (four waves, the last one ragged): sigma of the density phase and the colours of the colour
    phase carry the one-launch kernel's bits; the density phase writes +0.0 colours; the colour phase writes the listed rows' colours only"""
    n_pos, kw = SHAPES[case]
    m, *_ = random_model(hip, 7, n_pos=n_pos, **kw)
    x = points(100, seed=11)
    with torch.no_grad():
        full, _ = check_density(m, x, ARITHS[arith], what=case)
        assert np.isfinite(full).all()
        check_colour(m, x, ARITHS[arith], full, what=case)


@pytest.mark.parametrize("arith", list(ARITHS))
def test_phases_equal_the_one_launch_kernel_on_the_fixture_geometries(hip, arith):
    """every g18 geometry and every g22 option (align_corners=False, bicubic both ways, the jitter, five position planes) on the fixture's
    points"""
    with torch.no_grad():
        for name, m, x, noise in fixture_models(hip):
            full, _ = check_density(m, x, ARITHS[arith], noise, name)
            check_colour(m, x, ARITHS[arith], full, noise, name)


@pytest.mark.parametrize("arith", list(ARITHS))
def test_ragged_point_counts_and_non_finite_data(hip, arith):
    """P = 1, 31, 33, 100 row for row the P = 100 launch; then test_non_finite_data_equals_the_layered_route's model: a NaN texel in a position
    plane, an infinite weight in the colour decoder's last hidden layer, a point far outside the box"""
    a = ARITHS[arith]
    m, *_ = random_model(hip, 5, dec_channels=64, proj_combination="avg", viewdir_proj_combination="concat_pos", skip_connect_every=2)
    x = points(200, seed=13)
    x[17, :3] = (1e6, -1e6, 40.0)
    with torch.no_grad():
        for poisoned in (False, True):
            if poisoned:
                m.planes_[hip.models.get_plane_name(SID, 0)][0, 3, 4, 5] = float("nan")
                m.rgb_dec["0"][3].weight[5, 7] = float("inf")
            full = one_launch(m, x[:100], a)
            assert np.isfinite(full).all() != poisoned
            for P in (1, 31, 33, 100):
                part, _ = check_density(m, x[:P], a, what=P)
                assert same(part, full[:P]), P
                check_colour(m, x[:P], a, part, what=P, seed=P)
        full, _ = check_density(m, x, a, what="non-finite")
        # (f32: +inf where the last layer's input is positive, finite rows elsewhere; 'f16x2': an infinite weight is beyond the range, NaN everywhere)
        assert (~np.isfinite(full[:, :3])).any() and (np.isfinite(full[:, :3]).any() or arith == "f16x2") and np.isfinite(full[:, 3]).any()
        check_colour(m, x, a, full, what="non-finite")


SPAN = 2048          # points per workgroup of csrc/generic_live.hip (256 threads x 8 rounds) while P <= 4096 spans


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, SPAN - 1, SPAN, SPAN + 1, 70001, 4096 * SPAN + 5])
def test_live_list_is_the_numpy_statement_twice_in_a_row(hip, n):
    """lengths across the wave, the round of 256 and the workgroup's span; 70 001: 35 workgroups, whose counts are summed in front of each;
    4096 spans + 5: the span itself grows (nine rounds).  Values from {+0.0, -0.0, NaN, a subnormal, positive numbers}"""
    rng = np.random.default_rng(n)
    values = np.array([0.0, -0.0, np.nan, 1e-42, 0.25, 3.0], np.float32)
    w = values[rng.choice(values.size, n, p=[0.3, 0.25, 0.05, 0.1, 0.15, 0.15])]
    want = ref.live_list(w)
    wd = T(w)
    for _ in range(2):
        index, count = nv.generic_live_list(wd)
        assert index.dtype == torch.int32 and tuple(index.shape) == (n,) and tuple(count.shape) == (1,)
        c = int(count.item())
        assert c == want.size and np.array_equal(index[:c].cpu().numpy(), want)
    if n == 65:
        for fill in (0.0, -0.0, 2.0):           # nothing live, everything live
            index, count = nv.generic_live_list(torch.full((n,), fill, device=DEV))
            assert int(count.item()) == (n if fill else 0) and (not fill or np.array_equal(index.cpu().numpy(), np.arange(n)))
        assert int(nv.generic_live_list(torch.zeros(0, device=DEV))[1].item()) == 0


def counted(monkeypatch):
    """calls of the operators a frame may launch, by name"""
    calls = {}
    for name in ("triplane_density_generic_fused_arith", "triplane_colour_generic_fused_arith", "generic_live_list",
                 "triplane_decode_generic_fused_arith", "triplane_decode_generic_fused", "triplane_decode_generic"):
        def hook(*a, _op=getattr(nv, name), _name=name, **k):
            calls[_name] = calls.get(_name, 0) + 1
            return _op(*a, **k)
        monkeypatch.setattr(nv, name, hook)
    return calls


def g18_pair(hip):
    from test_hip_round2 import _variant_model
    g = load_golden("g18_decoder_variants.npz")
    mc, sid, *_ = _variant_model(hip, g, "concat24", state_prefix="concat24.render.coarse.")
    mf, *_ = _variant_model(hip, g, "concat24", state_prefix="concat24.render.fine.")
    mf.planes_ = mc.planes_
    H, W, focal = int(g["concat24.render.hwf"][0]), int(g["concat24.render.hwf"][1]), float(g["concat24.render.hwf"][2])
    return mc, mf, sid, H, W, focal, T(g["pose"]), None


def seeded_pair(hip):
    """a seeded coarse / fine pair whose fc_alpha biases are shifted so that about a third of the samples have a positive sigma: the shift comes
    from float64 sigmas (oracle/generic_decoder.py) at the coarse pass's sample points, computed on the CPU"""
    from oracle.generic_decoder import decode
    kw = dict(dec_channels=64, proj_combination="avg", viewdir_proj_combination="concat_pos", skip_connect_every=3)
    mc, sd_c, planes, kwc = random_model(hip, 41, **kw)
    mf, sd_f, _, _ = random_model(hip, 42, **kw)
    mf.planes_ = mc.planes_
    g = load_golden("g18_decoder_variants.npz")
    H = W = 8
    focal = 0.5 * W / np.tan(0.5 * 0.6911112)
    pose = T(g["pose"])
    with torch.no_grad():
        ro, rd = hip.nerf_helpers.get_ray_bundle(H, W, focal, pose)
        rays = hip.train_utils.pack_rays(ro.reshape(-1, 3), rd.reshape(-1, 3), 2.0, 6.0, H, W, focal, no_ndc=True)
        x = N_(nv.ray_points(rays, nv.coarse_z(rays, 16, False, None)))
        shares = []
        for m, sd in ((mc, sd_c), (mf, sd_f)):
            sigma = decode(sd, planes, G22_BOX, x, **kwc)[:, 3].astype(np.float64)
            shift = ref.bias_shift_for_share(sigma, 1.0 / 3)
            shares.append(float((sigma + shift > 0).mean()))
            dict(m.named_parameters())["fc_alpha.0.bias"].add_(float(shift))
    assert all(0.05 < s < 0.8 for s in shares), shares          # the reference alone meets the test's condition
    return mc, mf, SID, H, W, focal, pose, rays


@pytest.mark.parametrize("arith", list(ARITHS))
@pytest.mark.parametrize("pair", ["g18-concat24", "seeded-third-live"])
def test_frame_in_two_phases_equals_the_frame_in_one(hip, monkeypatch, pair, arith):
    """8 x 8 rays, 16 + 16 samples through eval_nerf under NVSR_GENERIC_TWO_PHASE=1 and =0: every returned tensor equal; the operators each
    route launched; the seeded pair's live share (from the one-phase weights) strictly between 0.05 and 0.8, so dead samples are in play"""
    monkeypatch.setenv("NVSR_GENERIC_FUSED", "1")
    mc, mf, sid, H, W, focal, pose, rays = (g18_pair if pair == "g18-concat24" else seeded_pair)(hip)
    mc.arithmetic = mf.arithmetic = None if arith == "f32" else "f16x2"
    ro, rd = hip.nerf_helpers.get_ray_bundle(H, W, focal, pose)
    opts, scfg = make_options(16, 16)
    calls = counted(monkeypatch)

    def frame(two_phase):
        monkeypatch.setenv("NVSR_GENERIC_TWO_PHASE", two_phase)
        calls.clear()
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            with torch.no_grad():
                assert mc.generic_frame_route() == mf.generic_frame_route() == ("two_phase" if two_phase == "1" else "one_phase")
                out = hip.train_utils.eval_nerf(H, W, focal, mc, mf, ro, rd, opts, scene_id=sid, scene_config=scfg)
        return [N_(t) for t in out if torch.is_tensor(t)], dict(calls)

    two, ran2 = frame("1")
    one, ran1 = frame("0")
    whole = "triplane_decode_generic_fused_arith" if arith == "f16x2" else "triplane_decode_generic_fused"
    assert ran2 == {"triplane_density_generic_fused_arith": 2, "generic_live_list": 2, "triplane_colour_generic_fused_arith": 2}, ran2
    assert ran1 == {whole: 2}, ran1
    assert len(two) == len(one) >= 2 and all(np.isfinite(t).all() for t in one)
    for a, b in zip(two, one):
        assert same(a, b)
    if rays is not None:
        with torch.no_grad():
            monkeypatch.setenv("NVSR_GENERIC_TWO_PHASE", "0")
            z_c = nv.coarse_z(rays, 16, False, None)
            N = rays.shape[0]
            raw_c = mc(nv.ray_points(rays, z_c)).reshape(N, 16, 4)
            rgb_c, _, _, w_c = nv.composite_rays(raw_c, z_c, rays, None, False, True)
            z_f = nv.importance_resample(z_c, w_c, 16, None)
            raw_f = mf(nv.ray_points(rays, z_f)).reshape(N, 32, 4)
            rgb_f, _, _, w_f = nv.composite_rays(raw_f, z_f, rays, None, False, True)
            assert same(N_(rgb_c).reshape(-1, 3), one[0].reshape(-1, 3)) and same(N_(rgb_f).reshape(-1, 3), one[1].reshape(-1, 3))
            for what, w, raw_one, mdl, z in (("coarse", w_c, raw_c, mc, z_c), ("fine", w_f, raw_f, mf, z_f)):
                share = ref.live_share(N_(w))
                print("%s %s: live share %.3f" % (arith, what, share))
                assert 0.05 < share < 0.8, (what, share)
                # the pass by hand from the operators: the raw tensor is the numpy statement's
                pts = nv.ray_points(rays, z)
                raw = mdl.density_field(pts)
                wd = nv.composite_rays(raw.reshape(raw_one.shape), z, rays, None, False, True)[3]
                assert same(N_(wd), N_(w))
                index, count = nv.generic_live_list(wd)
                done = N_(mdl.colour_field_(raw, pts, index, count))
                assert same(done, ref.two_phase_raw(N_(raw_one).reshape(-1, 4), N_(w)))


def test_range_flag_in_the_density_phase_and_the_healing_frame(hip, monkeypatch):
    """a position-plane texel beyond f16x2's range (20 000: the mean over three planes leaves |x| < 4094) raises bit 1 in the density phase,
    whose sigma is NaN at the points on the texel; in the colour phase the flag follows the list: raised for a listed point on the texel, not
    for the others.  A frame whose density decoder overflows in a hidden activation only (a bias of 5000: the operand check cannot see it)
    heals through the f32 route, warned once, with the bits of arithmetic=None"""
    from test_generic_limb import range_model
    m, sd, planes, kw, x = range_model(hip)
    with torch.no_grad():
        base, raised = flag_of(hip, lambda: density(m, x, F16X2))
        assert raised == 0 and np.isfinite(base).all()
        m.planes_[hip.models.get_plane_name(SID, 0)][0, 3, 4, 5] = 20000.0
        raw, raised = flag_of(hip, lambda: density(m, x, F16X2))
        assert raised & 1 and np.isnan(raw[:6, 3]).all() and not bits(raw[:, :3]).any()
        assert same(raw[:, 3], one_launch(m, x, F16X2)[:, 3])
        clean = np.flatnonzero(np.isfinite(one_launch(m, x, F16X2)).all(1)).astype(np.int32)
        assert clean.size > 100
        _, raised = flag_of(hip, lambda: colour(m, x, F16X2, raw, clean, clean.size))
        assert raised == 0
        _, raised = flag_of(hip, lambda: colour(m, x, F16X2, raw, np.concatenate([clean[:40], [2]]).astype(np.int32), 41))
        assert raised & 1
        _, raised = flag_of(hip, lambda: colour(m, x, F16X2, raw, np.concatenate([clean[:40], [2]]).astype(np.int32), 40))
        assert raised == 0                      # the entry beyond the count is not read
    # the frame
    monkeypatch.setenv("NVSR_GENERIC_FUSED", "1")
    monkeypatch.setenv("NVSR_GENERIC_TWO_PHASE", "1")
    mc, mf, sid, H, W, focal, pose, _ = seeded_pair(hip)
    ro, rd = hip.nerf_helpers.get_ray_bundle(H, W, focal, pose)
    opts, scfg = make_options(16, 16)
    calls = counted(monkeypatch)

    def frame(arithmetic):
        mc.arithmetic = mf.arithmetic = arithmetic
        calls.clear()
        with torch.no_grad():
            out = hip.train_utils.eval_nerf(H, W, focal, mc, mf, ro, rd, opts, scene_id=sid, scene_config=scfg)
        return [N_(t) for t in out if torch.is_tensor(t)]

    with warnings.catch_warnings():
        warnings.simplefilter("error")
        fine = frame("f16x2")
    assert calls["triplane_density_generic_fused_arith"] == 2
    with torch.no_grad():
        mf.density_dec["0"][0].bias[11] = 5000.0
    plain = frame(None)
    with pytest.warns(UserWarning, match="range"):
        healed = frame("f16x2")
    assert calls["triplane_density_generic_fused_arith"] == 4          # the limb frame, then the f32 frame: both in two phases
    assert all(same(a, b) for a, b in zip(healed, plain)) and np.isfinite(healed[1]).all() and not same(healed[1], fine[1])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        again = frame("f16x2")
    assert calls["triplane_density_generic_fused_arith"] == 2 and all(same(a, b) for a, b in zip(again, plain))


def test_routing(hip, monkeypatch):
    """gradients enabled: one phase, the same results; the layered route: one phase; the switch forces either way; beyond the fused capacity
    the new operators raise like triplane_decode_generic_fused and the frame still renders"""
    monkeypatch.setenv("NVSR_GENERIC_FUSED", "1")
    monkeypatch.setenv("NVSR_GENERIC_TWO_PHASE", "1")
    mc, mf, sid, H, W, focal, pose, _ = seeded_pair(hip)
    ro, rd = hip.nerf_helpers.get_ray_bundle(H, W, focal, pose)
    opts, scfg = make_options(16, 16)
    calls = counted(monkeypatch)

    def frame(models=(mc, mf)):
        calls.clear()
        out = hip.train_utils.eval_nerf(H, W, focal, models[0], models[1], ro, rd, opts, scene_id=sid, scene_config=scfg)
        return [N_(t.detach()) for t in out if torch.is_tensor(t)]

    with torch.no_grad():
        two = frame()
        assert set(calls) == {"triplane_density_generic_fused_arith", "generic_live_list", "triplane_colour_generic_fused_arith"}
    graph = frame()                                     # gradients on, parameters that take them: the layered route, one phase
    assert set(calls) == {"triplane_decode_generic"}
    monkeypatch.setenv("NVSR_GENERIC_TWO_PHASE", "0")
    assert all(same(a, b) for a, b in zip(graph, frame())) and set(calls) == {"triplane_decode_generic"}       # the switch changes nothing there
    monkeypatch.setenv("NVSR_GENERIC_TWO_PHASE", "1")
    for p in list(mc.parameters()) + list(mf.parameters()):
        p.requires_grad_(False)
    assert mc.generic_route() == "fused" and mc.generic_frame_route() == "two_phase"
    nograph = frame()                                   # gradients on, nothing takes them: fused, and still one phase
    assert set(calls) == {"triplane_decode_generic_fused"} and all(same(a, b) for a, b in zip(nograph, two))
    with torch.no_grad():
        monkeypatch.setenv("NVSR_GENERIC_FUSED", "0")
        assert mc.generic_frame_route() == "one_phase"
        layered = frame()
        assert set(calls) == {"triplane_decode_generic"} and all(same(a, b) for a, b in zip(layered, two))
        monkeypatch.setenv("NVSR_GENERIC_FUSED", "1")
        monkeypatch.setenv("NVSR_GENERIC_TWO_PHASE", "0")
        one = frame()
        assert set(calls) == {"triplane_decode_generic_fused"} and all(same(a, b) for a, b in zip(one, two))
        monkeypatch.delenv("NVSR_GENERIC_TWO_PHASE")
        span = mc.GENERIC_TWO_PHASE_DEFAULT_HIDDEN["f32"]
        default = "two_phase" if span is not None and span[0] <= mc.dec_channels <= span[1] else "one_phase"
        assert mc.generic_frame_route() == default
        frame()
        assert ("triplane_density_generic_fused_arith" in calls) == (default == "two_phase")
        # beyond the capacity
        monkeypatch.setenv("NVSR_GENERIC_TWO_PHASE", "1")
        big_c, *_ = random_model(hip, 9, dec_channels=4096, dec_density_layers=1, dec_rgb_layers=1, proj_combination="sum")
        big_f, *_ = random_model(hip, 10, dec_channels=4096, dec_density_layers=1, dec_rgb_layers=1, proj_combination="sum")
        big_f.planes_ = big_c.planes_
        xb = points(40)
        head, tail = args_of(big_c, xb, F32)
        with pytest.raises(Exception, match="capacity"):
            nv.triplane_density_generic_fused_arith(*head, *tail)
        with pytest.raises(Exception, match="capacity"):
            nv.triplane_colour_generic_fused_arith(torch.zeros(40, 4, device=DEV), *head, torch.zeros(40, dtype=torch.int32, device=DEV),
                                                   torch.zeros(1, dtype=torch.int32, device=DEV), *tail)
        with pytest.raises(Exception, match="capacity"):
            big_c.density_field(T(xb))
        assert big_c.generic_frame_route() == "one_phase"
        out = frame((big_c, big_f))
        assert set(calls) == {"triplane_decode_generic"} and len(out) >= 2 and all(np.isfinite(t).all() for t in out)


def test_opcheck(hip):
    m, *_ = random_model(hip, 3, dec_channels=64, proj_combination="avg", viewdir_proj_combination="concat_pos", skip_connect_every=3)
    tests = ("test_schema", "test_faketensor", "test_autograd_registration")
    x = points(50)
    with torch.no_grad():
        for arith in (F32, F16X2):
            head, tail = args_of(m, x, arith)
            torch.library.opcheck(nv.triplane_density_generic_fused_arith, head + tail, test_utils=tests)
            raw = nv.triplane_density_generic_fused_arith(*head, *tail)
            index, count = nv.generic_live_list(raw[:, 3])
            torch.library.opcheck(nv.triplane_colour_generic_fused_arith, (raw,) + head + (index, count) + tail, test_utils=tests)
        torch.library.opcheck(nv.generic_live_list, (torch.ones(300, device=DEV),), test_utils=tests)
    for name in ("triplane_density_generic_fused_arith", "triplane_colour_generic_fused_arith", "generic_live_list"):
        assert name in hip.ops.FORWARD_OPS
