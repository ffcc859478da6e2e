"""The generic decoder geometries evaluated in 'f16x2' (csrc/generic_fused_limb.hip, torch.ops.nvsr.triplane_decode_generic_fused_arith,
torch.ops.nvsr.pack_generic_decoder, TwoDimPlanesModel.generic_arithmetic): the packed layout against its numpy restatement, the kernel
against float64 and against the numpy reference of the arithmetic (tests/generic_limb_ref.py) under the project's bound for these kernels
(2e-5 max(1, max|ref|)), a derived bound where only the accumulation order differs, bit equality with the f32 route on operands that need no
rounding, ragged point counts, the range contract (NaN and the range flag, never a finite wrong number), the refusals, the model and a frame
through eval_nerf with its self-healing."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

import generic_limb_ref as ref
from conftest import load_golden
from test_generic_fused import SHAPES, SID, op_args, points, random_model, same, within_bound
from test_hip_parity import DEV, N_, T, make_options
from test_oracle import G18_VARIANTS, G22_BOX, G22_KW

pytestmark = pytest.mark.gpu
F32, F16, F16X2, BF16X3 = 0, 1, 2, 3
ERR_SHAPE, ERR_NULL = 1, 3


def pack(m):
    return torch.ops.nvsr.pack_generic_decoder(m.natural_blob(), m.generic_geometry(), int(m.num_density_planes))


def limb(m, x, noise=None, arith=F16X2):
    """the fused route of model m's geometry, planes and weights on the points x with the hidden layers in `arith`"""
    with torch.no_grad():
        planes, consts, nat, geometry = op_args(m)
        return N_(torch.ops.nvsr.triplane_decode_generic_fused_arith(planes, consts, nat, pack(m), geometry, T(x), bool(m.align_corners),
                                                                     None if noise is None else T(noise), m.plane_interp == "bicubic", arith))


def flag_of(hip, fn):
    """(fn(), the range flag's bits after it) with the word zeroed before"""
    flag = hip.capi.range_flag(torch.device(DEV))
    flag.reset()
    out = fn()
    bits = hip.capi.RangeFlag.raised(flag.read_async())
    flag.reset()
    return out, bits


PACK_CASES = {"hidden33-skip1": SHAPES["hidden33-skip1"], "hidden1": SHAPES["hidden1-skip1"], "c24": SHAPES["hidden96-c24"],
              "hidden160": (3, dict(dec_channels=160, proj_combination="avg", viewdir_proj_combination="concat_pos", skip_connect_every=2))}


@pytest.mark.parametrize("case", list(PACK_CASES))
def test_pack_kernel_is_the_numpy_layout(hip, case):
    """bit for bit: a K-block across X1 | X2 and a second tile with one live row (hidden 33, skip 1), hidden 1, K = 24, five tiles (hidden 160)"""
    n_pos, kw = PACK_CASES[case]
    m, sd, _, kw = ref.seeded_state(hip, 7, n_pos=n_pos, **kw)
    want = ref.pack(ref.hidden_layers(sd, m.dec_density_layers, m.dec_rgb_layers), kw["dec_channels"])
    got = N_(torch.ops.nvsr.pack_generic_decoder(T(N_(m.natural_blob())), m.generic_geometry(), n_pos)).view(np.uint32)
    geo = hip.capi.DecoderGeometry(*m.generic_geometry())
    assert got.size == want.size == hip.capi.lib().nvsr_generic_packed_floats_ext(C.byref(geo), n_pos)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]


@pytest.mark.parametrize("case", list(SHAPES))
def test_shapes_meet_the_bound_of_float64_and_of_the_limb_reference(hip, case):
    from oracle.generic_decoder import decode
    n_pos, kw = SHAPES[case]
    m, sd, planes, kw = random_model(hip, 7, n_pos=n_pos, **kw)
    assert hip.capi.lib().nvsr_generic_fused_supported_arith(C.byref(hip.capi.DecoderGeometry(*m.generic_geometry())), n_pos, F16X2) == 1
    x = points(77, seed=11)
    out, bits = flag_of(hip, lambda: limb(m, x))
    assert bits == 0 and np.isfinite(out).all()
    within_bound(out, decode(sd, planes, G22_BOX, x, **kw), case)
    within_bound(out, ref.decode_limb(sd, planes, G22_BOX, x, **kw), case)
    assert same(limb(m, x, arith=F32), N_(torch.ops.nvsr.triplane_decode_generic_fused(*op_args(m), T(x)))), "'f32' forwards to the f32 kernel"


def test_fixture_geometries_meet_the_bound(hip):
    """every g18 geometry and every g22 option on the fixture's own points: within the bound of the reference's outputs, of float64 and of
    the numpy limb reference"""
    from oracle.generic_decoder import decode
    from test_hip_round2 import _variant_model
    from test_hip_round4 import _g22_model
    g = load_golden("g18_decoder_variants.npz")
    for name in G18_VARIANTS:
        m, sid, kw, sd, planes = _variant_model(hip, g, name)
        out = limb(m, g[name + ".x"])
        within_bound(out, g[name + ".out"], name)
        within_bound(out, decode(sd, planes, g["box"], g[name + ".x"], **kw), name)
        within_bound(out, ref.decode_limb(sd, planes, g["box"], g[name + ".x"], **kw), name)
    g = load_golden("g22_model_options.npz")
    for name, n_pos, over, extra in (("align_false", 3, dict(align_corners=False, dec_channels=64), dict(align_corners=False)),
                                     ("planes5", 5, dict(dec_channels=64), {}), ("noise", 3, {}, dict(coord_noise=g["noise.jitter"])),
                                     ("bicubic", 3, dict(plane_interp="bicubic", dec_channels=64), dict(plane_interp="bicubic")),
                                     ("bicubic_noalign", 3, dict(plane_interp="bicubic", align_corners=False, dec_channels=64),
                                      dict(plane_interp="bicubic", align_corners=False))):
        m = _g22_model(hip, g, name, n_planes=n_pos, **over)
        out = limb(m, g[name + ".x"], extra.get("coord_noise"))
        within_bound(out, g[name + ".out"], name)
        sd = {k[len(name) + 4:]: v for k, v in g.items() if k.startswith(name + ".sd.")}
        planes = [g["%s.plane%d" % (name, d)] for d in range(n_pos + 1)]
        within_bound(out, decode(sd, planes, G22_BOX, g[name + ".x"], **G22_KW, **extra), name)
        within_bound(out, ref.decode_limb(sd, planes, G22_BOX, g[name + ".x"], **G22_KW, **extra), name)


@pytest.mark.parametrize("hidden", [33, 64])
def test_one_hidden_layer_within_the_derived_accumulation_bound(hip, hidden):
    """One hidden layer per decoder on inputs that stage 0 computes without a rounding: 9 x 9 position planes of multiples of 1/64 sampled at
    their texel centres (integer coordinates in the box [-4, 4]^3: tap weights (1, 0, 0, 0)), summed ('sum': exact), and a zero view plane.
    The kernel then differs from the numpy limb reference by the order of its f32 accumulation alone, and the bound is derived, not tuned:
      activation a[m]:  e_a = 1.01 n 2^-24 sum_k |w^||x^| / 4096      n = 3 ceil(K / 16) accumulating MFMAs (conv_f16_ref.bound's model: one f32
                        rounding of at most the absolute sum per MFMA; the roundings of the activation itself to f32, 2^-24 |a| in the kernel's
                        fma and in the reference, are left to the model's slack: the measured worst error is 0.02 of the bound)
      output o[j]:      sum_m |W_head[j][m]| e_a[m] + K 2^-24 sum_m |W_head[j][m]| |a[m]|    the head's own f32 sum over K = hidden terms."""
    m, sd, _, kw = random_model(hip, 17, dec_channels=hidden, dec_density_layers=1, dec_rgb_layers=1, proj_combination="sum",
                                viewdir_proj_combination="concat_pos")
    rng = np.random.default_rng(hidden)
    planes = [(rng.integers(-128, 129, (1, 48, 9, 9)) / 64.0).astype(np.float32) for _ in range(3)] + [np.zeros((1, 48, 9, 9), np.float32)]
    m.planes_ = torch.nn.ParameterDict({hip.models.get_plane_name(SID, d): torch.nn.Parameter(T(planes[d])) for d in range(4)})
    x = np.concatenate([rng.integers(-4, 5, (77, 3)), rng.standard_normal((77, 3))], 1).astype(np.float32)
    Xd, Xr = ref.inputs(sd, planes, G22_BOX, x, **kw)
    assert np.array_equal(Xd * 64, np.round(Xd * 64)) and np.abs(Xd).max() > 1 and not Xr[:, 144:].any()       # exact inputs, as designed
    out = limb(m, x)
    want = ref.decode_limb(sd, planes, G22_BOX, x, **kw)
    for X, dec, hd, cols in ((Xd, "density_dec", "fc_alpha", slice(3, 4)), (Xr, "rgb_dec", "fc_rgb", slice(0, 3))):
        W, b, Wh = sd[dec + ".0.0.weight"], sd[dec + ".0.0.bias"], np.abs(np.asarray(sd[hd + ".0.weight"], np.float64))
        a = ref.layer(W, b, X).astype(np.float64)
        n = 3 * -(-X.shape[1] // 16)
        e_a = 1.01 * n * ref.U24 * ref.layer_absum(W, X)
        e_o = e_a @ Wh.T + hidden * ref.U24 * (np.abs(a) @ Wh.T)
        err = np.abs(out[:, cols] - want[:, cols])
        print("hidden %d %s: worst error / bound %.3f (bound %.3g .. %.3g)" % (hidden, dec, float((err / e_o).max()), e_o.min(), e_o.max()))
        assert (err <= e_o).all(), (dec, float((err / e_o).max()))


@pytest.mark.parametrize("case", ["hidden33-skip1", "hidden1-skip1", "concat4-256"])
def test_exact_operands_equal_the_f32_route_bit_for_bit(hip, case):
    """one weight +-1 or +-1/2 per row, biases multiples of 1/8, heads two +-1/2 per row, zero planes: every operand is an f16 number after
    its scale and every sum is exact in f32, so the limb route must give the f32 fused route's bits"""
    n_pos, kw = SHAPES[case]
    m, sd, planes, kw = random_model(hip, 7, n_pos=n_pos, **kw)
    ex = ref.exact_state(sd, 3, m.dec_density_layers, m.dec_rgb_layers)
    with torch.no_grad():
        for k, p in m.named_parameters():
            p.zero_() if k.startswith("planes_.") else p.copy_(T(ex[k]))
    x = points(77, seed=11)
    a, b = limb(m, x), limb(m, x, arith=F32)
    assert same(a, b) and np.isfinite(a).all()
    if kw["dec_channels"] > 1:
        assert np.abs(a).max() > 0


def test_ragged_point_counts_and_rows_past_the_end(hip):
    """row for row the P = 257 result; rows past P of an over-allocated output keep their sentinel; P == 0 is NVSR_OK without a launch"""
    n_pos, kw = SHAPES["hidden33-skip1"]
    m, *_ = random_model(hip, 7, n_pos=n_pos, **kw)
    x = points(257)
    with torch.no_grad():
        planes, consts, nat, geometry = op_args(m)
        packed = pack(m)
        full = N_(torch.ops.nvsr.triplane_decode_generic_fused_arith(planes, consts, nat, packed, geometry, T(x)))
        for P in (0, 1, 31, 32, 33, 63, 65, 127, 129, 257):
            xp = T(x[:P])
            out = N_(torch.ops.nvsr.triplane_decode_generic_fused_arith(planes, consts, nat, packed, geometry, xp))
            assert out.shape == (P, 4) and same(out, full[:P]), P
            geo, n_pos, _, sc = hip.ops._generic_setup(planes, consts, nat, geometry, True, None, P)
            buf = torch.full((P + 70, 4), -7.25, device=DEV)
            hip.capi.call("nvsr_generic_decode_fused_arith_ext", C.byref(sc), C.byref(geo), hip.capi.ptr(nat), hip.capi.ptr(packed), P,
                          hip.capi.ptr(xp) if P else hip.capi.ptr(nat), None, hip.capi.ptr(buf), F16X2, hip.capi.stream())
            buf = N_(buf)
            assert same(buf[:P], full[:P]) and np.all(buf[P:] == -7.25), P


def range_model(hip):
    m, sd, planes, kw = random_model(hip, 5, dec_channels=64, proj_combination="avg", viewdir_proj_combination="concat_pos", skip_connect_every=2)
    x = points(200, seed=13)
    x[:6, 1] = 4.0 / 9 + np.linspace(-0.02, 0.02, 6)        # texel (row 4, column 5) of plane 0 (axes y, z) with a weight close to 1
    x[:6, 2] = -4.0 / 9
    return m, sd, planes, kw, x


def test_out_of_range_texel_is_nan_where_it_reaches_and_raises_the_flag(hip):
    """one texel at 5000: NaN outputs exactly where the numpy limb reference has them -- the decoders whose input 5000 x (tap weight) leaves
    the range |x| < 4094 (the colour decoder reads the raw feature, the density decoder the mean over three planes, which stays inside); six
    points sit on the texel -- all NaN rows among the points whose taps touch the texel with a weight that is not zero; the flag's bit 1; the
    rows of the points that do not touch it keep their bits"""
    from oracle.generic_decoder import decode
    m, sd, planes, kw, x = range_model(hip)
    base, bits = flag_of(hip, lambda: limb(m, x))
    assert bits == 0 and np.isfinite(base).all()
    planes = [p.copy() for p in planes]
    before = decode(sd, planes, G22_BOX, x, **kw)
    planes[0][0, 3, 4, 5] = 5000.0
    with torch.no_grad():
        m.planes_[hip.models.get_plane_name(SID, 0)][0, 3, 4, 5] = 5000.0
    touched = (decode(sd, planes, G22_BOX, x, **kw) != before).any(1)
    out, bits = flag_of(hip, lambda: limb(m, x))
    nan = np.isnan(out).any(1)
    assert bits & 1
    assert np.array_equal(np.isnan(out), np.isnan(ref.decode_limb(sd, planes, G22_BOX, x, **kw))) and np.isfinite(out[~np.isnan(out)]).all()
    assert nan[:6].all() and not (nan & ~touched).any()
    assert same(out[~touched], base[~touched]) and (~touched).sum() > 100
    within_bound(out[~nan], decode(sd, planes, G22_BOX, x, **kw)[~nan], "finite rows")


def test_out_of_range_weight_is_nan_everywhere_and_raises_the_flag(hip):
    m, sd, planes, kw, x = range_model(hip)
    base = limb(m, x)
    with torch.no_grad():
        m.density_dec["0"][1].weight[5, 7] = 300.0
    out, bits = flag_of(hip, lambda: limb(m, x))
    assert bits & 1 and np.isnan(out[:, 3]).all() and same(out[:, :3], base[:, :3])


def test_nan_and_inf_texels_come_out_as_nan(hip):
    """a NaN texel and an infinite texel: NaN rows (all four outputs) at the points the numpy reference names, the bits of the untouched launch
    elsewhere -- no finite garbage.  An input NaN RAISES the flag: the kernel reports every non-finite row it writes, wherever the NaN came
    from (a re-render in f32 then returns what the f32 route makes of the same input)."""
    m, sd, planes, kw, x = range_model(hip)
    base = limb(m, x)
    planes = [p.copy() for p in planes]
    for value, at in ((float("nan"), (0, 3, 4, 5)), (float("inf"), (0, 9, 2, 2))):
        planes[0][at] = value
        with torch.no_grad():
            m.planes_[hip.models.get_plane_name(SID, 0)][at] = value
        out, bits = flag_of(hip, lambda: limb(m, x))
        want = np.isnan(ref.decode_limb(sd, planes, G22_BOX, x, **kw))
        assert bits & 1 and want.any() and not want.all()
        assert np.array_equal(np.isnan(out), want) and np.array_equal(want.any(1), want.all(1)) and np.isfinite(out[~want]).all()
        assert same(out[~want.any(1)], base[~want.any(1)])


def test_refusals(hip):
    m, *_ = random_model(hip, 3, dec_channels=64, proj_combination="avg", viewdir_proj_combination="concat_pos")
    big, *_ = random_model(hip, 9, dec_channels=4096, dec_density_layers=1, dec_rgb_layers=1, proj_combination="sum")
    x = T(points(40))
    fn, ptr = hip.capi.lib().nvsr_generic_decode_fused_arith_ext, hip.capi.ptr
    with torch.no_grad():
        for mdl, arith, null_packed, status in ((m, F16, False, ERR_SHAPE), (m, BF16X3, False, ERR_SHAPE), (m, -1, False, ERR_SHAPE),
                                                (m, 7, False, ERR_SHAPE), (big, F16X2, False, ERR_SHAPE), (m, F16X2, True, ERR_NULL),
                                                (m, F32, True, 0), (m, F16X2, False, 0)):
            planes, consts, nat, geometry = op_args(mdl)
            geo, n_pos, _, sc = hip.ops._generic_setup(planes, consts, nat, geometry, True, None, 40)
            packed = pack(mdl)
            out = torch.full((40, 4), -7.25, device=DEV)
            got = fn(C.byref(sc), C.byref(geo), ptr(nat), None if null_packed else ptr(packed), 40, ptr(x), None, ptr(out), arith, hip.capi.stream())
            assert got == status, (arith, null_packed, got)
            assert bool((out == -7.25).all()) == (status != 0)
        with pytest.raises(Exception, match="arithmetic"):
            torch.ops.nvsr.triplane_decode_generic_fused_arith(*op_args(m)[:3], pack(m), m.generic_geometry(), x, True, None, False, BF16X3)


def test_model_routes_by_name_and_follows_its_weights(hip, monkeypatch):
    monkeypatch.setenv("NVSR_GENERIC_FUSED", "1")
    m, *_ = random_model(hip, 3, dec_channels=64, proj_combination="avg", viewdir_proj_combination="concat_pos", skip_connect_every=3)
    x = points(150)
    with torch.no_grad():
        assert m.arithmetic is None and m.generic_arithmetic() == "f32"
        assert same(N_(m(T(x))), N_(torch.ops.nvsr.triplane_decode_generic_fused(*op_args(m), T(x))))
        m.arithmetic = "f16x2"
        assert m.generic_arithmetic() == "f16x2" and m.generic_route() == "fused"
        a = N_(m(T(x)))
        assert same(a, limb(m, x)) and not same(a, limb(m, x, arith=F32))
        first = m.packed_generic_decoder()
        assert m.packed_generic_decoder() is first
        m.rgb_dec["0"][2].weight.mul_(0.5)                     # in place: the version moves, the cache is rebuilt
        assert m.packed_generic_decoder() is not first
        b = N_(m(T(x)))
        assert same(b, limb(m, x)) and not same(a[:, :3], b[:, :3]) and same(a[:, 3], b[:, 3])
    assert m.generic_arithmetic() == "f32" and m.generic_route() == "layered"        # gradients on, parameters that take them
    c = m(T(x))
    assert c.requires_grad and same(N_(c), N_(torch.ops.nvsr.triplane_decode_generic(*op_args(m), T(x))))
    assert m.arithmetic == "f16x2"


def test_frame_through_eval_nerf_and_its_self_healing(hip, monkeypatch):
    """16 x 16 rays, 8 + 8 samples, hidden-64 coarse and fine models in 'f16x2': the frame is the passes composed by hand from the operators;
    an operand beyond the range -- a plane value, which the operand check finds, or a bias that only a hidden activation shows, which the
    range flag finds -- is warned about once and rendered through the f32 route, the bits of arithmetic=None; the next frame of the same
    parameters launches no limb kernel; model.arithmetic stays"""
    monkeypatch.setenv("NVSR_GENERIC_FUSED", "1")
    kw = dict(dec_channels=64, proj_combination="avg", viewdir_proj_combination="concat_pos", skip_connect_every=3)
    mc, *_ = random_model(hip, 31, **kw)
    mf, *_ = random_model(hip, 32, **kw)
    mf.planes_ = mc.planes_
    g = load_golden("g18_decoder_variants.npz")
    H = W = 16
    focal = 0.5 * W / np.tan(0.5 * 0.6911112)
    ro, rd = hip.nerf_helpers.get_ray_bundle(H, W, focal, T(g["pose"]))
    opts, scfg = make_options(8, 8)
    nv = torch.ops.nvsr
    calls = []
    op = nv.triplane_decode_generic_fused_arith
    monkeypatch.setattr(nv, "triplane_decode_generic_fused_arith", lambda *a: calls.append(1) or op(*a))

    def frame(arithmetic="f16x2"):
        mc.arithmetic = mf.arithmetic = arithmetic
        try:
            with torch.no_grad():
                out = hip.train_utils.eval_nerf(H, W, focal, mc, mf, ro, rd, opts, scene_id=SID, scene_config=scfg)
            return [N_(t).reshape(-1, 3) for t in out if torch.is_tensor(t)]
        finally:
            mc.arithmetic = mf.arithmetic = "f16x2"

    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got = frame()
    assert len(calls) == 2 and len(got) == 2
    with torch.no_grad():
        rays = hip.train_utils.pack_rays(ro.reshape(-1, 3), rd.reshape(-1, 3), 2.0, 6.0, H, W, focal, no_ndc=True)
        N = rays.shape[0]

        def raw(mdl, z):
            planes, consts, nat, geometry = op_args(mdl)
            return op(planes, consts, nat, pack(mdl), geometry, nv.ray_points(rays, z), True, None, False, F16X2).reshape(N, z.shape[1], 4)

        z_c = nv.coarse_z(rays, 8, False, None)
        rgb_c, _, _, w_c = nv.composite_rays(raw(mc, z_c), z_c, rays, None, False, True)
        z_f = nv.importance_resample(z_c, w_c, 8, None)
        rgb_f = nv.composite_rays(raw(mf, z_f), z_f, rays, None, False, False)[0]
    assert same(got[0], N_(rgb_c)) and same(got[1], N_(rgb_f)) and np.isfinite(got[1]).all()
    plain = frame(None)
    assert not same(plain[1], got[1])
    # a plane value at 5000
    name = hip.models.get_plane_name(SID, 1)
    with torch.no_grad():
        keep = float(mc.planes_[name][0, 3, 4, 5])
        mc.planes_[name][0, 3, 4, 5] = 5000.0
    plain = frame(None)
    del calls[:]
    with pytest.warns(UserWarning, match="range"):
        healed = frame()
    assert all(same(a, b) for a, b in zip(healed, plain)) and np.isfinite(healed[1]).all()
    del calls[:]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        again = frame()
    assert not calls and all(same(a, b) for a, b in zip(again, plain))
    # a bias that pushes a hidden activation beyond the range: only the flag can see it
    with torch.no_grad():
        mc.planes_[name][0, 3, 4, 5] = keep
        mf.rgb_dec["0"][0].bias[11] = 5000.0
    plain = frame(None)
    del calls[:]
    with warnings.catch_warnings():
        warnings.simplefilter("error")              # (warned once per model pair)
        healed = frame()
    assert len(calls) == 2 and all(same(a, b) for a, b in zip(healed, plain)) and np.isfinite(healed[1]).all()
    del calls[:]
    assert all(same(a, b) for a, b in zip(frame(), plain)) and not calls
    assert mc.arithmetic == "f16x2" and mf.arithmetic == "f16x2"


def test_opcheck(hip):
    m, *_ = random_model(hip, 3, dec_channels=64, proj_combination="avg", viewdir_proj_combination="concat_pos", skip_connect_every=3)
    tests = ("test_schema", "test_faketensor", "test_autograd_registration")
    with torch.no_grad():
        planes, consts, nat, geometry = op_args(m)
        packed = pack(m)
    torch.library.opcheck(torch.ops.nvsr.pack_generic_decoder, (nat, geometry, 3), test_utils=tests)
    torch.library.opcheck(torch.ops.nvsr.triplane_decode_generic_fused_arith, (planes, consts, nat, packed, geometry, T(points(50)), True, None, False, F16X2),
                          test_utils=tests)
    assert "pack_generic_decoder" in hip.ops.FORWARD_OPS and "triplane_decode_generic_fused_arith" in hip.ops.FORWARD_OPS
