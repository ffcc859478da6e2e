"""GPU tests of the geometry outputs of a view (csrc/normals.hip): nvsr_live_ray_points and nvsr_normals_composite against
their numpy float32 transcriptions bit for bit (seeded rows, never a backward's), slabs cut mid-ray, accumulation, NaN; ops.normals_of_pass
and train_utils.eval_geometry against the golden the upstream code wrote in float64 (g28_normals.npz); opcheck; the routing of
evaluate_view(geometry=False).  Shapes: the golden's 6 x 5 frame with 8 + 8 samples on 7 x 7 / 4 x 3 planes, 5 x 3 and 70 x 4 seeded passes."""
import numpy as np
import pytest
import torch

import normals_ref as NR
import points_grad_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SID = "lego_DS8_PlRes7_4"


def T(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def N_(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def case():
    g, sd_c, sd_f, planes, rot = NR.load_case()
    consts = R.scene_consts(g["box"], rot)
    flat = [float(v) for v in consts[0]] + [float(v) for v in consts[1]] + [float(v) for p in consts[2] for v in p]
    return dict(g=g, sd_c=sd_c, sd_f=sd_f, planes=planes, rot=rot, consts=consts, flat=flat, planes_cl=[R.channel_last(p) for p in planes])


def build(hip, case, which, arithmetic):
    m = hip.models.TwoDimPlanesModel(use_viewdirs=True, skip_connect_every=3, proj_combination="avg", viewdir_proj_combination="concat_pos",
                                     align_corners=True)
    m.load_state_dict({k: torch.as_tensor(v) for k, v in case["sd_" + which].items()}, strict=True)
    m = m.to(DEV)
    m.planes_ = torch.nn.ParameterDict({hip.models.get_plane_name(SID, d): torch.nn.Parameter(T(case["planes"][d])) for d in range(4)})
    m.box_coords = {SID: torch.as_tensor(case["g"]["box"], dtype=torch.float64)}
    m.set_cur_scene_id(SID)
    m.arithmetic = arithmetic
    return m.eval()


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the kernels alone
# ---------------------------------------------------------------------------------------------------------------------------------
def test_live_ray_points_equal_the_transcription_bit_for_bit(hip):
    """N = 5, S = 3 (samples in and outside the box); a list with indices outside [0, N S), whose rows stay as they were (the operator hands
    out zeros); M = 0"""
    rays, z, w = NR.seeded_pass(5, 3, 7, dead_rays=(1,), full_rays=(3,))
    op = torch.ops.nvsr.live_ray_points
    for index in (NR.live_list(w), np.array([-3, 0, 4, 14, 15, 99], np.int32), np.zeros(0, np.int32)):
        got = N_(op(T(index), T(rays), T(z)))
        want = NR.live_ray_points_f32(index, rays, z)
        assert got.shape == (len(index), 11) and np.array_equal(bits(got), bits(want))
    assert len(NR.live_list(w)) >= 5
    got = N_(op(T(np.array([-3, 0, 4, 14, 15, 99], np.int32)), T(rays), T(z)))
    assert not got[[0, 4, 5]].any() and got[[1, 2, 3], :3].any(1).all()
    # the C entry leaves the row of a skipped index untouched
    capi = hip.capi
    idx, r_, z_, out = T(np.array([15, 2], np.int32)), T(rays), T(z), torch.full((2, 11), 7.0, device=DEV)
    capi.call("nvsr_live_ray_points", 5, 3, 2, capi.ptr(idx), capi.ptr(r_), capi.ptr(z_), capi.ptr(out), capi.stream())
    torch.cuda.synchronize()
    assert bool((out[0] == 7).all()) and np.array_equal(bits(N_(out[1])), bits(NR.live_ray_points_f32([2], rays, z)[0]))


def _composite(case, index, live, rows, w, start):
    normal = T(start).clone()
    torch.ops.nvsr.normals_composite([T(p) for p in case["planes_cl"]], case["flat"], T(index), T(live), [T(r) for r in rows], T(w), normal)
    return N_(normal)


def _kernel_case(case, name):
    g = case["g"]
    if name == "rays":                 # one ray with no live sample, one with all S live, one all-zero row
        rays, z, w = NR.seeded_pass(5, 3, 7, dead_rays=(1,), full_rays=(3,))
    elif name == "wide":               # 70 rays: five workgroups of 16 ray groups, the last one ragged
        rays, z, w = NR.seeded_pass(70, 4, 9, dead_rays=(0, 69), full_rays=(16, 68))
    else:                              # the golden's live points as S = 1
        r32, z32, w32 = (g[k].astype(np.float32) for k in ("rays", "z_fine", "weights_fine"))
        rays = NR.live_ray_points_f32(NR.live_list(w32), r32, z32)
        z = np.zeros((len(rays), 1), np.float32)
        w = np.random.default_rng(5).uniform(0.1, 1.0, (len(rays), 1)).astype(np.float32)
    index = NR.live_list(w)
    live = NR.live_ray_points_f32(index, rays, z)
    rows = NR.seeded_rows(len(index), 11)
    if name == "rays":
        for r in rows:
            r[2] = 0
    start = np.random.default_rng(3).standard_normal((w.shape[0], 3)).astype(np.float32)
    return index, live, rows, w, start


@pytest.mark.parametrize("name", ["rays", "golden_points", "wide"])
def test_composite_equals_the_transcription_bit_for_bit(hip, case, name):
    """normal (accumulated INTO a seeded start) equals normals_ref.normals_composite_f32 bit for bit and sits within K(T) 2^-24 A of float64;
    a ray without a live sample keeps its bits; an all-zero row gives n = 0: its term adds +0"""
    index, live, rows, w, start = _kernel_case(case, name)
    got = _composite(case, index, live, rows, w, start)
    want = NR.normals_composite_f32(case["planes_cl"], case["consts"], index, live, rows, w, start)
    assert np.array_equal(bits(got), bits(want))
    worst = NR.assert_within_bound(got, case["planes_cl"], case["consts"], index, live, rows, w, start)
    print("%s: M = %d, error / bound %.3f" % (name, len(index), worst))
    dead = ~(w != 0).any(1)
    assert np.array_equal(bits(got[dead]), bits(start[dead])) and (got[~dead] != start[~dead]).any(1).all()
    if name == "rays":
        assert dead[1] and (w[3] != 0).all()
        ray = int(index[2]) // 3
        w0 = w.copy()                                                          # (entry 2's rows are zero: the same pass without that sample)
        w0.reshape(-1)[index[2]] = 0
        keep = np.arange(len(index)) != 2
        skipped = _composite(case, index[keep], live[keep], [r[keep] for r in rows], w0, start)
        assert np.array_equal(bits(skipped[ray]), bits(got[ray])), "n of an all-zero row must be +0"
    # accumulated into, not overwritten: from zeros the result differs from the seeded start's by that start
    zero = _composite(case, index, live, rows, w, np.zeros_like(start))
    assert not zero[dead].any() and not np.array_equal(bits(zero[~dead]), bits(got[~dead]))
    np.testing.assert_allclose(got[~dead] - start[~dead], zero[~dead], rtol=0, atol=2e-6)


def test_composite_in_slabs_cut_mid_ray_equals_one_launch(hip, case):
    """the list cut at every position of a ray with all S = 4 samples live (and elsewhere), the slabs launched in ascending order"""
    index, live, rows, w, start = _kernel_case(case, "wide")
    one = _composite(case, index, live, rows, w, start)
    first = int(np.searchsorted(index, 16 * 4))
    assert np.array_equal(index[first:first + 4], 16 * 4 + np.arange(4))
    planes = [T(p) for p in case["planes_cl"]]
    for cuts in ([first + 1], [first + 2, first + 3], [1, first + 2, len(index) - 1]):
        normal = T(start).clone()
        for a, b in zip([0] + cuts, cuts + [len(index)]):
            torch.ops.nvsr.normals_composite(planes, case["flat"], T(index[a:b]), T(live[a:b]), [T(r[a:b]) for r in rows], T(w), normal)
        assert np.array_equal(bits(N_(normal)), bits(one)), cuts


def test_a_nan_weight_or_point_reaches_exactly_its_ray(hip, case):
    index, live, rows, w, start = _kernel_case(case, "wide")
    one = _composite(case, index, live, rows, w, start)
    bad = w.copy()
    hit = int(index[7])
    bad.reshape(-1)[hit] = np.nan
    got = _composite(case, index, live, rows, bad, start)
    want = NR.normals_composite_f32(case["planes_cl"], case["consts"], index, live, rows, bad, start)
    other = np.arange(70) != hit // 4
    assert np.isnan(got[hit // 4]).all() and np.array_equal(bits(got[other]), bits(one[other])) and np.array_equal(np.isnan(got), np.isnan(want))
    pts = live.copy()
    pts[7, 1] = np.nan
    got = _composite(case, index, pts, rows, w, start)
    assert np.isnan(got[hit // 4]).all() and np.array_equal(bits(got[other]), bits(one[other]))


def test_operators_pass_opcheck_and_refuse_bad_tensors(hip, case):
    index, live, rows, w, start = _kernel_case(case, "rays")
    planes = [T(p) for p in case["planes_cl"]]
    rays, z, _ = NR.seeded_pass(5, 3, 7)
    utils = ("test_schema", "test_faketensor")
    torch.library.opcheck(torch.ops.nvsr.live_ray_points, (T(index), T(rays), T(z)), test_utils=utils)
    torch.library.opcheck(torch.ops.nvsr.normals_composite, (planes, case["flat"], T(index), T(live), [T(r) for r in rows], T(w), T(start)),
                          test_utils=utils)
    mf = build(hip, case, "f", "bf16x3")
    pl, consts = mf.scene_args()
    g = case["g"]
    args = (pl, consts, mf.packed_decoder(), T(g["rays"].astype(np.float32)), T(g["z_fine"].astype(np.float32)), None, False, 3)
    torch.library.opcheck(torch.ops.nvsr.render_pass_geometry, args, test_utils=utils)
    with pytest.raises(ValueError):
        torch.ops.nvsr.live_ray_points(T(index).long(), T(rays), T(z))
    with pytest.raises(ValueError):
        torch.ops.nvsr.normals_composite(planes, case["flat"], T(index), T(live), [T(r)[:, :40] for r in rows], T(w), T(start))
    with pytest.raises(ValueError):
        torch.ops.nvsr.normals_composite(planes, case["flat"], T(index), T(live)[:-1], [T(r) for r in rows], T(w), T(start))


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. against the upstream golden
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arithmetic", ["f16x2", "bf16x3"])
def test_normals_of_pass_against_the_upstream_golden(hip, case, arithmetic):
    """ops.normals_of_pass on the golden's rays, z_fine and weights_fine cast to float32: the relative L2 error of the normal map against the
    golden (upstream's float64 autograd gradient, composited in float64) is at most 2e-4 -- the bound the project applies to x.grad and to the
    ray gradients: the normal is a smooth function of the same feature-gradient rows wherever |g| is not small, which the golden's
    generator guarantees.  slab_points = 7 (slabs cut mid-ray) gives the bits of the default.
    Measured: 6.1e-7 in f16x2, 2.8e-7 in bf16x3."""
    g = case["g"]
    mf = build(hip, case, "f", arithmetic)
    planes, consts = mf.scene_args()
    code = hip.capi.ARITHMETIC[arithmetic]
    rays, z, w = (T(g[k].astype(np.float32)) for k in ("rays", "z_fine", "weights_fine"))
    args = (planes, consts, mf.packed_decoder(), mf.packed_decoder_bwd(), rays, z, w, code)
    normal = N_(hip.ops.normals_of_pass(*args))
    err = R.rel_l2(normal, g["normal"])
    print("%s: normals_of_pass against the golden: relative L2 %.3g" % (arithmetic, err))
    assert normal.shape == (30, 3) and np.isfinite(normal).all()
    assert err <= 2e-4
    assert not normal[g["acc"] == 0].any() and np.linalg.norm(normal, axis=1).max() > 0.5
    assert np.array_equal(bits(N_(hip.ops.normals_of_pass(*args, slab_points=7))), bits(normal))
    assert np.array_equal(bits(N_(hip.ops.normals_of_pass(*args, slab_points=1))), bits(normal))
    with pytest.raises(NotImplementedError):
        hip.ops.normals_of_pass(*args[:-1], hip.capi.ARITHMETIC["f32"])


@pytest.mark.parametrize("arithmetic", ["f16x2", "bf16x3"])
def test_eval_geometry_end_to_end_against_the_upstream_golden(hip, case, arithmetic):
    """the 6 x 5 frame, 8 + 8 samples, depths regenerated on the device: normal within 2e-4 relative L2 of the golden; acc within 2e-5 over the
    rays test_hip_parity.py keeps for a render pass against its golden (the last sample's |sigma_raw| >= 1e-4: below it 1e10 sigma makes
    alpha a step of the sign), depth within rtol 3e-6 + atol 1e-5, the tolerance it applies to the compositor's depth.
    Measured: normal 3.3e-6 (f16x2) / 3.2e-6 (bf16x3); acc 1.6e-6 in both; depth at most 0.40 of its tolerance."""
    from bench import render_options

    g = case["g"]
    mc, mf = build(hip, case, "c", arithmetic), build(hip, case, "f", arithmetic)
    mf.planes_ = mc.planes_
    opts, scfg = render_options(8, 8)
    H, W, focal = int(g["hwf"][0]), int(g["hwf"][1]), float(g["hwf"][2])
    rays = g["rays"].astype(np.float32)
    out = hip.train_utils.eval_geometry(H, W, focal, mc, mf, T(rays[:, 0:3]).reshape(H, W, 3), T(rays[:, 3:6]).reshape(H, W, 3), opts, SID,
                                        scene_config=scfg)
    assert sorted(out) == ["acc", "depth", "normal"]
    assert tuple(out["depth"].shape) == (H, W) and tuple(out["acc"].shape) == (H, W) and tuple(out["normal"].shape) == (H, W, 3)
    normal, acc, depth = N_(out["normal"]).reshape(-1, 3), N_(out["acc"]).reshape(-1), N_(out["depth"]).reshape(-1)
    x_last = np.concatenate([g["rays"][:, 0:3] + g["rays"][:, 3:6] * g["z_fine"][:, -1:], g["rays"][:, 8:11]], 1)
    ok = np.abs(R.model64(case["sd_f"], case["planes"], g["box"], case["rot"], x_last)["out"][:, 3]) >= 1e-4
    err = R.rel_l2(normal, g["normal"])
    e_acc = np.abs(acc - g["acc"])[ok].max()
    e_depth = (np.abs(depth - g["depth"]) / (1e-5 + 3e-6 * np.abs(g["depth"])))[ok].max()
    print("%s: eval_geometry against the golden: normal relative L2 %.3g, acc max error %.3g, depth error / tolerance %.3g (%d of 30 rays kept)"
          % (arithmetic, err, e_acc, e_depth, ok.sum()))
    assert ok.mean() > 0.9
    assert err <= 2e-4
    np.testing.assert_allclose(acc[ok], g["acc"][ok], rtol=0, atol=2e-5)
    np.testing.assert_allclose(depth[ok], g["depth"][ok], rtol=3e-6, atol=1e-5)
    # num_fine == 0: the coarse pass's maps
    opts0, _ = render_options(8, 0)
    out0 = hip.train_utils.eval_geometry(H, W, focal, mc, mf, T(rays[:, 0:3]), T(rays[:, 3:6]), opts0, SID, scene_config=scfg)
    assert tuple(out0["normal"].shape) == (H, W, 3) and bool(torch.isfinite(out0["normal"]).all())
    assert not np.array_equal(N_(out0["acc"]), N_(out["acc"]))


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. routing
# ---------------------------------------------------------------------------------------------------------------------------------
def test_evaluate_view_without_geometry_keeps_todays_launch_sequence(hip, monkeypatch):
    """geometry=False (the default): the same entries in the same order as a call that does not name the argument, none of the new ones;
    geometry=True: that sequence first, then the geometry frame's, and the maps under res['geometry']"""
    from bench import make_synthetic_scene, render_options

    mc, mf, sid, pose = make_synthetic_scene(DEV, plane_res=32, view_res=8, seed=4)
    opts, scfg = render_options(16, 16)
    H = W = 12
    focal = 0.5 * W / np.tan(0.5 * 0.6911112)
    target = torch.rand(H, W, 3, device=DEV)
    real = hip.capi.call

    def spied(**kw):
        calls = []

        def spy(name, *a):
            calls.append(name)
            return real(name, *a)

        monkeypatch.setattr(hip.capi, "call", spy)
        res = hip.training.evaluate_view(mc, mf, opts, sid, scfg, target, pose, H, W, focal, **kw)
        torch.cuda.synchronize()
        monkeypatch.setattr(hip.capi, "call", real)
        return calls, res

    spied()                                                                        # (the first frame packs the decoders; they stay cached)
    base, res0 = spied()
    off, res1 = spied(geometry=False)
    new = ("nvsr_live_ray_points", "nvsr_normals_composite", "nvsr_generic_live_list", "nvsr_render_pass_backward_rows_arith")
    assert base and off == base and not any(n in base for n in new) and "geometry" not in res0 and "geometry" not in res1
    assert torch.equal(res0["rgb_fine"], res1["rgb_fine"])
    on, res2 = spied(geometry=True)
    assert on[:len(base)] == base and all(n in on[len(base):] for n in new)
    assert on[len(base):].count("nvsr_render_pass_arith") == 2 and on[len(base):].count("nvsr_generic_live_list") == 1
    geo = res2["geometry"]
    assert tuple(geo["normal"].shape) == (H, W, 3) and tuple(geo["depth"].shape) == (H, W) and torch.equal(res2["rgb_fine"], res0["rgb_fine"])
    assert bool(torch.isfinite(geo["normal"]).all()) and float(geo["acc"].max()) > 0.1
    length = geo["normal"].norm(dim=-1)
    assert bool((length <= geo["acc"] * (1 + 1e-5) + 1e-6).all())                   # |sum w n| <= sum w: not renormalised
