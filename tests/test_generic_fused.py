"""The fused evaluation route of the generic decoder geometries (csrc/generic_fused.hip, torch.ops.nvsr.triplane_decode_generic_fused): one
launch whose result has the BITS of the layer-by-layer route (csrc/generic.hip, torch.ops.nvsr.triplane_decode_generic), which stays the
reference implementation.  "Equal" below: the same NaN positions and the same bits everywhere else.  Where a float64 restatement or the
reference's own output exists, the result is also held to the project's bound for these kernels, 2e-5 * max(1, max|ref|)
(test_generic_decoder_geometries_vs_reference_and_oracle)."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import load_golden
from test_hip_parity import DEV, N_, T, make_options
from test_oracle import G18_VARIANTS, G22_BOX, G22_KW

pytestmark = pytest.mark.gpu
SID = "lego_DS8_PlRes10_6"


def same(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.int32)[~na], b.view(np.int32)[~nb])


def within_bound(out, ref, what):
    np.testing.assert_allclose(out, ref, rtol=0, atol=2e-5 * max(1.0, float(np.abs(ref).max())), err_msg=str(what))


def op_args(m):
    planes = [m.channel_last_plane(d) for d in range(m.num_density_planes + 1)]
    planes, consts = m.scene_args(planes=planes, check_native=False)
    return planes, consts, m.natural_blob(), m.generic_geometry()


def both(m, x, noise=None):
    """(fused, layered) of model m's geometry, planes and weights on the points x"""
    with torch.no_grad():
        a = op_args(m) + (T(x), bool(m.align_corners), None if noise is None else T(noise), m.plane_interp == "bicubic")
        return N_(torch.ops.nvsr.triplane_decode_generic_fused(*a)), N_(torch.ops.nvsr.triplane_decode_generic(*a))


def points(P, seed=3):
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.uniform(-4.3, 4.3, (P, 3)), rng.standard_normal((P, 3))], 1).astype(np.float32)


def random_model(hip, seed, n_pos=3, **kw):
    """a seeded model on 10 x 10 planes: (model, state dict and planes as numpy for the float64 restatement, the restatement's keywords)"""
    torch.manual_seed(seed)
    np.random.seed(seed)                      # (more than three position planes: CoordProjector draws its frames from NumPy's generator)
    m = hip.models.TwoDimPlanesModel(use_viewdirs=True, align_corners=True, num_planes_or_rot_mats=n_pos, **kw)
    with torch.no_grad():                     # (He weights and mostly positive biases: no layer whose ReLUs are all shut, at any width)
        for p in m.decoder_parameters():
            p.normal_(0.0, float(np.sqrt(2.0 / p.shape[1]))) if p.dim() == 2 else p.uniform_(-0.1, 0.4)
    sd ={k: v.detach().numpy().copy() for k, v in m.state_dict().items()}
    rng = np.random.default_rng(seed)
    planes = [rng.standard_normal((1, kw.get("num_plane_channels", 48), 10, 10)).astype(np.float32) for _ in range(n_pos + 1)]
    m = m.to(DEV).eval()
    m.planes_ = torch.nn.ParameterDict({hip.models.get_plane_name(SID, d): torch.nn.Parameter(T(planes[d])) for d in range(n_pos + 1)})
    m.box_coords = {SID: torch.as_tensor(G22_BOX, dtype=torch.float64)}
    m.set_cur_scene_id(SID)
    return m, sd, planes, kw


def test_fixture_geometries_equal_the_layered_route_and_meet_the_bound(hip):
    """every g18 geometry and every g22 option (align_corners=False, bicubic both ways, the jitter, five position planes) on the fixture's
    points: equal to the layered route; within the bound of the reference's outputs and of the float64 restatement.  The fixtures hold no
    four-plane model: that one is seeded here (CoordProjector's random frames) and held to the restatement."""
    from oracle.generic_decoder import decode
    from test_hip_round2 import _variant_model
    from test_hip_round4 import _g22_model
    g = load_golden("g18_decoder_variants.npz")
    for name in G18_VARIANTS:
        m, sid, kw, sd, planes = _variant_model(hip, g, name)
        assert m.generic_route() == "layered"                  # (gradients are on here and the parameters take them)
        fused, layered = both(m, g[name + ".x"])
        assert same(fused, layered), name
        within_bound(fused, g[name + ".out"], name)
        within_bound(fused, decode(sd, planes, g["box"], g[name + ".x"], **kw), name)
    g = load_golden("g22_model_options.npz")
    for name, n_pos, over, extra in (("align_false", 3, dict(align_corners=False, dec_channels=64), dict(align_corners=False)),
                                     ("planes5", 5, dict(dec_channels=64), {}), ("noise", 3, {}, dict(coord_noise=g["noise.jitter"])),
                                     ("bicubic", 3, dict(plane_interp="bicubic", dec_channels=64), dict(plane_interp="bicubic")),
                                     ("bicubic_noalign", 3, dict(plane_interp="bicubic", align_corners=False, dec_channels=64),
                                      dict(plane_interp="bicubic", align_corners=False))):
        m = _g22_model(hip, g, name, n_planes=n_pos, **over)
        fused, layered = both(m, g[name + ".x"], extra.get("coord_noise"))
        assert same(fused, layered), name
        within_bound(fused, g[name + ".out"], name)
        sd = {k[len(name) + 4:]: v for k, v in g.items() if k.startswith(name + ".sd.")}
        planes = [g["%s.plane%d" % (name, d)] for d in range(n_pos + 1)]
        within_bound(fused, decode(sd, planes, G22_BOX, g[name + ".x"], **G22_KW, **extra), name)
    m, sd, planes, kw = random_model(hip, 22, n_pos=4, dec_channels=64, **G22_KW)
    x = points(300)
    fused, layered = both(m, x)
    assert same(fused, layered)
    within_bound(fused, decode(sd, planes, G22_BOX, x, **kw), "planes4")


def test_ragged_point_counts_and_rows_past_the_end(hip):
    """P from 0 across the 32-point wave and the workgroup's point block: row for row the layered route; rows past P of an over-allocated
    output keep their sentinel; P == 0 is NVSR_OK without a launch"""
    g = load_golden("g18_decoder_variants.npz")
    from test_hip_round2 import _variant_model
    m, *_ = _variant_model(hip, g, "skip2")
    x = points(1000)
    with torch.no_grad():
        planes, consts, nat, geometry = op_args(m)
        ref = N_(torch.ops.nvsr.triplane_decode_generic(planes, consts, nat, geometry, T(x)))
        for P in (0, 1, 31, 32, 33, 63, 65, 127, 129, 257, 1000):
            xp = T(x[:P])
            out = N_(torch.ops.nvsr.triplane_decode_generic_fused(planes, consts, nat, geometry, xp))
            assert out.shape == (P, 4) and same(out, ref[:P]), P
            geo, n_pos, _, sc = hip.ops._generic_setup(planes, consts, nat, geometry, True, None, P)
            buf = torch.full((P + 70, 4), -7.25, device=DEV)
            hip.capi.call("nvsr_generic_decode_fused_ext", C.byref(sc), C.byref(geo), hip.capi.ptr(nat), P, hip.capi.ptr(xp) if P else hip.capi.ptr(nat),
                          None, hip.capi.ptr(buf), hip.capi.stream())
            buf = N_(buf)
            assert same(buf[:P], ref[:P]) and np.all(buf[P:] == -7.25), P


SHAPES = {      # † : fails a kernel that pairs k within each operand instead of within [X1 | X2], or that drops the last odd column
    "hidden33-skip1": (3, dict(dec_channels=33, skip_connect_every=1, proj_combination="avg", viewdir_proj_combination="concat_pos")),       # †
    "hidden31-skip1": (3, dict(dec_channels=31, skip_connect_every=1, proj_combination="avg", viewdir_proj_combination="concat_pos")),       # †
    "hidden1-skip1": (3, dict(dec_channels=1, skip_connect_every=1, proj_combination="sum")),                                                # †
    "hidden64-1+5": (3, dict(dec_channels=64, dec_density_layers=1, dec_rgb_layers=5, proj_combination="avg", viewdir_proj_combination="concat_pos")),
    "hidden96-c24": (3, dict(dec_channels=96, num_plane_channels=24, proj_combination="sum", viewdir_proj_combination="concat_pos", skip_connect_every=2)),
    "concat4-256": (4, dict(dec_channels=256, proj_combination="concat", viewdir_proj_combination="concat_pos", skip_connect_every=3)),     # Kd 192, Kr 240
    "sum-sum": (3, dict(dec_channels=40, proj_combination="sum", viewdir_proj_combination="sum", skip_connect_every=2)),
    "avg-avg": (3, dict(dec_channels=40, proj_combination="avg", viewdir_proj_combination="avg")),
    "avg-mult": (3, dict(dec_channels=40, proj_combination="avg", viewdir_proj_combination="mult", skip_connect_every=3)),
    "one-plane": (1, dict(dec_channels=64, proj_combination="avg", viewdir_proj_combination="concat_pos", skip_connect_every=2)),
    "one-plane-concat": (1, dict(dec_channels=48, proj_combination="concat", viewdir_proj_combination="concat")),
}


@pytest.mark.parametrize("case", list(SHAPES))
def test_smallest_shapes_of_the_k_pairing_the_padding_and_the_tiling(hip, case):
    """seeded weights, 10 x 10 planes, 77 points (three waves, the last one ragged): equal to the layered route, within the bound of the
    float64 restatement"""
    from oracle.generic_decoder import decode
    n_pos, kw = SHAPES[case]
    m, sd, planes, kw = random_model(hip, 7, n_pos=n_pos, **kw)
    assert hip.capi.lib().nvsr_generic_fused_supported(C.byref(hip.capi.DecoderGeometry(*m.generic_geometry())), n_pos) == 1
    x = points(77, seed=11)
    fused, layered = both(m, x)
    if kw["dec_channels"] > 1:                # (a live network: the points answer differently; a single unit may well be shut)
        assert np.unique(layered[:, 0]).size > 60 and np.unique(layered[:, 3]).size > 60
    assert same(fused, layered)
    within_bound(fused, decode(sd, planes, G22_BOX, x, **kw), case)


def test_non_finite_data_equals_the_layered_route(hip):
    """a NaN texel in a position plane (a ReLU layer answers 0 to it: fmaxf), an infinite weight in the colour decoder's last hidden layer
    (+inf where its input is positive, 0 x inf = NaN -> 0 where it is not; the head turns the infinity into +-inf or NaN) and a point far
    outside the box (border clamp)"""
    m, sd, planes, kw = random_model(hip, 5, dec_channels=64, proj_combination="avg", viewdir_proj_combination="concat_pos", skip_connect_every=2)
    with torch.no_grad():
        m.planes_[hip.models.get_plane_name(SID, 0)][0, 3, 4, 5] = float("nan")
        m.rgb_dec["0"][3].weight[5, 7] = float("inf")
    x = points(200, seed=13)
    x[17, :3] = (1e6, -1e6, 40.0)
    fused, layered = both(m, x)
    assert (~np.isfinite(layered[:, :3])).any() and np.isfinite(layered[:, :3]).any() and np.isfinite(layered[:, 3]).all()
    assert same(fused, layered)


def test_routing_follows_the_gradient_mode_the_handle_and_the_capacity(hip, monkeypatch):
    from test_hip_round2 import _variant_model
    monkeypatch.delenv("NVSR_GENERIC_FUSED", raising=False)
    g = load_golden("g18_decoder_variants.npz")
    m, *_ = _variant_model(hip, g, "deep5_c24")
    x = T(g["deep5_c24.x"])
    with torch.no_grad():
        assert m.generic_route() == "fused"
        a = N_(m(x))
    assert m.generic_route() == "layered"
    b = N_(m(x))
    monkeypatch.setenv("NVSR_GENERIC_FUSED", "0")
    with torch.no_grad():
        assert m.generic_route() == "layered"
        c = N_(m(x))
    monkeypatch.delenv("NVSR_GENERIC_FUSED")
    assert same(a, b) and same(a, c)
    # 256 wide: within the capacity, but measured slower than the layered route there -- taken only with NVSR_GENERIC_FUSED=1
    wide, *_ = _variant_model(hip, g, "wide256")
    xw = T(g["wide256.x"])
    with torch.no_grad():
        assert wide.generic_route() == "layered"
        lw = N_(wide(xw))
        monkeypatch.setenv("NVSR_GENERIC_FUSED", "1")
        assert wide.generic_route() == "fused"
        fw = N_(wide(xw))
    monkeypatch.delenv("NVSR_GENERIC_FUSED")
    assert same(fw, lw)
    # beyond the capacity: the operator raises, the model stays on the layered route and answers
    big, *_ = random_model(hip, 9, dec_channels=4096, dec_density_layers=1, dec_rgb_layers=1, proj_combination="sum")
    xb = points(40)
    with torch.no_grad():
        with pytest.raises(Exception, match="capacity"):
            torch.ops.nvsr.triplane_decode_generic_fused(*op_args(big), T(xb))
        assert big.generic_route() == "layered"
        out = N_(big(T(xb)))
    assert out.shape == (40, 4) and np.isfinite(out).all()


def test_frame_through_eval_nerf_equals_the_layered_route(hip, monkeypatch):
    """the 'concat24' coarse / fine pair of g18 on its 8 x 8 rays, 16 + 16 samples: every tensor eval_nerf returns"""
    from test_hip_round2 import _variant_model
    monkeypatch.delenv("NVSR_GENERIC_FUSED", raising=False)
    g = load_golden("g18_decoder_variants.npz")
    mc, sid, *_ = _variant_model(hip, g, "concat24", state_prefix="concat24.render.coarse.")
    mf, *_ = _variant_model(hip, g, "concat24", state_prefix="concat24.render.fine.")
    mf.planes_ = mc.planes_
    H, W, focal = int(g["concat24.render.hwf"][0]), int(g["concat24.render.hwf"][1]), float(g["concat24.render.hwf"][2])
    ro, rd = hip.nerf_helpers.get_ray_bundle(H, W, focal, T(g["pose"]))
    opts, scfg = make_options(16, 16)

    def frame():
        with torch.no_grad():
            return [N_(t) for t in hip.train_utils.eval_nerf(H, W, focal, mc, mf, ro, rd, opts, scene_id=sid, scene_config=scfg) if torch.is_tensor(t)]

    with torch.no_grad():
        assert mc.generic_route() == "fused" and mf.generic_route() == "fused"
    fused = frame()
    monkeypatch.setenv("NVSR_GENERIC_FUSED", "0")
    layered = frame()
    assert len(fused) == len(layered) >= 2          # (the coarse and the fine colours at the least)
    for a, b in zip(fused, layered):
        assert same(a, b)
    np.testing.assert_allclose(fused[0], g["concat24.render.rgb_coarse"], rtol=0, atol=3e-5)


def test_opcheck(hip):
    m, *_ = random_model(hip, 3, dec_channels=64, proj_combination="avg", viewdir_proj_combination="concat_pos", skip_connect_every=3)
    with torch.no_grad():
        args = op_args(m) + (T(points(50)), True, None, False)
    torch.library.opcheck(torch.ops.nvsr.triplane_decode_generic_fused, args, test_utils=("test_schema", "test_faketensor", "test_autograd_registration"))
    assert "triplane_decode_generic_fused" in hip.ops.FORWARD_OPS
