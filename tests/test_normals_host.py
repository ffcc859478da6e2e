"""CPU tests of the geometry outputs of a view (csrc/normals.hip): the numpy float32 transcription of the two kernels sits
within its derived bound of float64; the all-float64 restatement of the route reproduces the golden the upstream code wrote
(g28_normals.npz: g, normal); the entries' status codes for calls that launch nothing; eval_geometry refuses what it does not cover before
anything is launched.  Nothing here touches a GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import normals_ref as NR
import points_grad_ref as R

OK, ERR_SHAPE, ERR_NULL = 0, 1, 3


@pytest.fixture(scope="module")
def pkg():
    import nvsr_amd

    nvsr_amd.build_extension()
    return nvsr_amd


@pytest.fixture(scope="module")
def case():
    return NR.load_case()


def test_golden_is_the_frame_the_issue_describes(case):
    g = case[0]
    assert [g["plane%d" % d].shape[-2:] for d in range(4)] == [(7, 7), (7, 7), (7, 7), (4, 3)]
    assert g["rays"].shape == (30, 11) and g["z_fine"].shape == (30, 16) and g["weights_fine"].shape == (30, 16)        # 6 x 5, no ray dropped
    assert all(g[k].dtype == np.float64 for k in ("rays", "z_fine", "weights_fine", "depth", "acc", "g", "normal"))
    w = g["weights_fine"].reshape(-1)
    assert np.array_equal(g["index"], NR.live_list(w)) and g["g"].shape == (len(g["index"]), 3) and len(g["index"]) >= 60
    mag = np.linalg.norm(g["g"][w[g["index"]] > 1e-6], axis=1)
    assert mag.min() >= 1e-3 * np.median(mag)
    assert (g["acc"] < 1e-3).any() and (g["acc"] > 0.5).any()                       # background and surface pixels
    np.testing.assert_allclose(g["acc"], g["weights_fine"].sum(1), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(g["depth"], (g["weights_fine"] * g["z_fine"]).sum(1), rtol=1e-12, atol=1e-15)


def test_float64_restatement_reproduces_the_upstream_golden(case):
    """the route in float64 from the golden's rays, z_fine, weights_fine and planes: the live list, the rows of g_raw = (0, 0, 0, 1), the slope
    in the order of include/nvsr.h, the normalisation and the fold -- against upstream's autograd gradient and the normal composited from it,
    1e-10 relative per row of g (both sides are float64: only the order of the sums differs) and 1e-10 of the largest normal"""
    g, _, sd_f, planes, rot = case
    index, gg, normal = NR.normals_exact64(sd_f, planes, g["box"], rot, g["rays"], g["z_fine"], g["weights_fine"])
    assert np.array_equal(index, g["index"])
    err = np.linalg.norm(gg - g["g"], axis=1) / np.linalg.norm(g["g"], axis=1)
    print("g: largest relative error of a row %.3g; normal: largest absolute error %.3g" % (err.max(), np.abs(normal - g["normal"]).max()))
    assert err.max() <= 1e-10
    assert np.abs(normal - g["normal"]).max() <= 1e-10 * np.abs(g["normal"]).max()
    assert not normal[g["acc"] == 0].any()


@pytest.mark.parametrize("name", ["golden_points", "rays"])
def test_float32_transcription_sits_within_the_bound_of_float64(case, name):
    """seeded rows; |f32 - f64| <= K(T) 2^-24 A per ray and component, K(T) = 18 + 4 + 2 T (normals_ref's docstring)"""
    g, _, _, planes, rot = case
    consts, planes_cl = R.scene_consts(g["box"], rot), [R.channel_last(p) for p in planes]
    if name == "golden_points":
        S = g["z_fine"].shape[1]
        rays, z, w = g["rays"].astype(np.float32), g["z_fine"].astype(np.float32), g["weights_fine"].astype(np.float32)
        live = NR.live_ray_points_f32(NR.live_list(w), rays, z)
        rays, z = live, np.zeros((len(live), 1), np.float32)                      # the golden's points as S = 1
        w = np.random.default_rng(5).uniform(0.1, 1.0, (len(live), 1)).astype(np.float32)
    else:
        rays, z, w = NR.seeded_pass(5, 3, 7, dead_rays=(1,), full_rays=(3,))
    index = NR.live_list(w)
    live = NR.live_ray_points_f32(index, rays, z)
    rows = NR.seeded_rows(len(index), 11)
    start = np.random.default_rng(3).standard_normal((w.shape[0], 3)).astype(np.float32)
    got = NR.normals_composite_f32(planes_cl, consts, index, live, rows, w, start)
    worst = NR.assert_within_bound(got, planes_cl, consts, index, live, rows, w, start)
    print("%s: error / bound %.3f" % (name, worst))
    dead = ~(w != 0).any(1)
    assert np.array_equal(got[dead], start[dead]) and (got[~dead] != start[~dead]).any(1).all()
    # the transcription of the live points is nvsr_ray_points' position on the listed samples
    p = np.stack([rays[:, k][:, None] + rays[:, 3 + k][:, None] * z for k in range(3)], -1).reshape(-1, 3)
    assert np.array_equal(live[:, :3], p[index]) and not live[:, 3:8].any() and np.array_equal(live[:, 8:], np.repeat(rays[:, 8:], z.shape[1], 0)[index])


def test_entries_answer_empty_and_bad_calls_without_a_launch(pkg):
    lib = pkg.capi.lib()
    one = C.c_void_p(16)
    pts = lambda N, S, M: lib.nvsr_live_ray_points(N, S, M, one, one, one, one, None)
    assert pts(-1, 3, 4) == ERR_SHAPE and pts(5, 0, 4) == ERR_SHAPE and pts(5, 4097, 4) == ERR_SHAPE and pts(5, 3, -1) == ERR_SHAPE
    assert pts(1 << 20, 4096, 4) == ERR_SHAPE                                       # N * S >= 2^31
    assert pts(5, 3, 0) == OK and pts(0, 3, 4) == OK
    assert lib.nvsr_live_ray_points(5, 3, 4, None, one, one, one, None) == ERR_NULL
    planes = [torch.zeros(2, 2, 48) for _ in range(4)]
    sc = pkg.capi.Scene()                                                          # (ops._scene wants device planes: built by hand)
    for d, p in enumerate(planes):
        sc.planes[d], sc.ph[d], sc.pw[d] = p.data_ptr(), 2, 2
    rows = (C.c_void_p * 3)(16, 16, 16)
    comp = lambda scene, N, S, M, r=rows: lib.nvsr_normals_composite(scene, N, S, M, one, one, r, one, one, None)
    assert comp(None, 5, 3, 4) == ERR_NULL
    assert comp(C.byref(sc), -1, 3, 4) == ERR_SHAPE and comp(C.byref(sc), 5, 0, 4) == ERR_SHAPE and comp(C.byref(sc), 5, 3, 1 << 29) == ERR_SHAPE
    assert comp(C.byref(sc), 5, 3, 0) == OK and comp(C.byref(sc), 0, 3, 4) == OK
    assert comp(C.byref(sc), 5, 3, 4, (C.c_void_p * 3)(16, None, 16)) == ERR_NULL
    assert comp(C.byref(sc), 5, 3, 4, (C.c_void_p * 3)(16, 20, 16)) == 4           # NVSR_ERR_ALIGN


def test_operators_are_registered_with_fake_implementations(pkg):
    from torch._subclasses.fake_tensor import FakeTensorMode

    for name in ("render_pass_geometry", "live_ray_points", "normals_composite"):
        assert hasattr(torch.ops.nvsr, name), name
    with FakeTensorMode():
        index, rays, z = torch.empty(7, dtype=torch.int32), torch.empty(5, 11), torch.empty(5, 3)
        assert torch.ops.nvsr.live_ray_points(index, rays, z).shape == (7, 11)
        planes, consts = [torch.empty(4, 4, 48) for _ in range(4)], [0.0] * 28
        out = torch.ops.nvsr.render_pass_geometry(planes, consts, torch.empty(8), rays, z, None, False, 2)
        assert [tuple(t.shape) for t in out] == [(5, 3), (5,), (5,), (5, 3), (5,)]
        assert torch.ops.nvsr.normals_composite(planes, consts, index, torch.empty(7, 11), [torch.empty(7, 48)] * 3, z, torch.empty(5, 3)) is None


def test_eval_geometry_refuses_what_it_does_not_cover_before_any_launch(pkg, monkeypatch):
    """a generic geometry, 'f32', the one-limb 'f16' and the NeRF baselines raise NotImplementedError; CPU models reach the checks, and no
    entry of the library is called on the way"""
    from bench import render_options

    calls = []
    monkeypatch.setattr(pkg.capi, "call", lambda name, *a: calls.append(name))
    opts, scfg = render_options(8, 8)
    kw = dict(use_viewdirs=True, skip_connect_every=3, viewdir_proj_combination="concat_pos", align_corners=True)
    native = lambda arithmetic: _with(pkg.models.TwoDimPlanesModel(proj_combination="avg", **kw), arithmetic)
    generic = _with(pkg.models.TwoDimPlanesModel(proj_combination="sum", **kw), "bf16x3")
    assert native("bf16x3").is_native_geometry() and not generic.is_native_geometry()
    ro = rd = torch.zeros(2, 2, 3)
    run = lambda mc, mf, o=opts: pkg.train_utils.eval_geometry(2, 2, 1.0, mc, mf, ro, rd, o, "lego_DS8_PlRes7_4", scene_config=scfg)
    with pytest.raises(NotImplementedError, match="shipped decoder geometry only"):
        run(native("bf16x3"), generic)
    with pytest.raises(NotImplementedError, match="shipped decoder geometry only"):
        run(generic, native("f16x2"))
    for bad in ("f32", "f16"):
        with pytest.raises(NotImplementedError, match="'f16x2' / 'bf16x3' only .*'%s'" % bad):
            run(native("f16x2"), native(bad))
        with pytest.raises(NotImplementedError, match="'f16x2' / 'bf16x3' only .*'%s'" % bad):
            run(native(bad), native("bf16x3"))
    baseline = pkg.models.FlexibleNeRFModel()
    with pytest.raises(NotImplementedError, match="tri-plane model only"):
        run(baseline, baseline)
    # num_fine == 0: the fine model is not part of the frame and is not judged
    opts0, _ = render_options(8, 0)
    with pytest.raises(NotImplementedError, match="'f32'"):
        run(native("f32"), generic, opts0)
    assert calls == []


def _with(model, arithmetic):
    model.arithmetic = arithmetic
    return model.eval()
