"""CPU tests of the tri-plane model's input gradient: the float64 restatement of the model call reproduces the golden the
upstream code wrote (g23_points_grad.npz: out, x_grad_full, and -- position columns times 0 -- x_grad_reference); the numpy float32 transcription
of nvsr_triplane_points_grad sits within its derived bound of float64; the C entry, its ctypes signature, the operator's fake
implementation and the warning.  Nothing here touches a GPU."""
import ctypes as C
import os
import re
import warnings

import numpy as np
import pytest
import torch

import points_grad_ref as R
from conftest import ROOT

OK, ERR_SHAPE, ERR_LAUNCH, ERR_NULL, ERR_ALIGN = 0, 1, 2, 3, 4


@pytest.fixture(scope="module")
def pkg():
    import nvsr_amd

    nvsr_amd.build_extension()
    return nvsr_amd


@pytest.fixture(scope="module")
def case():
    g, sd, planes, rot = R.load_case()
    return g, sd, planes, rot, R.model64(sd, planes, g["box"], rot, g["x"], g["g_out"])


def test_golden_holds_the_rows_the_rules_are_about():
    g = R.load_case()[0]
    kinds, x = list(g["kinds"]), g["x"]
    assert x.shape == (67, 6) and x.dtype == np.float32
    assert [g["plane%d" % d].shape[-2:] for d in range(4)] == [(5, 7), (6, 4), (7, 5), (4, 3)]
    for k in range(3):
        assert abs(x[kinds.index("beyond%d" % k), k]) > 4 and x[kinds.index("low%d" % k), k] == -4 and x[kinds.index("high%d" % k), k] == 4
        assert x[kinds.index("line%d" % k), k] == 0
    views = x[np.array(kinds) == "axis_view", 3:]
    assert len(views) == 4 and ((views == 0).sum(1) >= 1).all() and (np.abs(views[:, :2]).max(1) > 0).all()       # on an axis plane, never a pole
    assert kinds.count("interior") >= 40
    assert (g["out"][:, 3] > 0).any() and (g["out"][:, 3] < 0).any()                                               # mixed gates at the head


def test_float64_restatement_reproduces_the_upstream_golden(case):
    """upstream ran in float32: its own rounding through nine layers is ~1e-6 of the result; 1e-5 relative L2 (2e-5 absolute on out) leaves
    room for that and for nothing else -- a wrong cell, a swapped axis or a missing chain factor is an error of order 1"""
    g, _, _, _, m = case
    np.testing.assert_allclose(m["out"], g["out"], rtol=0, atol=2e-5)
    full = g["x_grad_full"]
    assert R.rel_l2(m["x_grad"][:, :3], full[:, :3]) < 1e-5 and R.rel_l2(m["x_grad"][:, 3:], full[:, 3:]) < 1e-5
    # upstream as it runs: the position columns are exactly 0 (CoordProjector projects under no_grad), the view columns are the full run's
    as_it_runs = np.concatenate([m["x_grad"][:, :3] * 0, m["x_grad"][:, 3:]], 1)
    assert not g["x_grad_reference"][:, :3].any()
    assert np.array_equal(g["x_grad_reference"][:, 3:], full[:, 3:])
    assert R.rel_l2(as_it_runs[:, 3:], g["x_grad_reference"][:, 3:]) < 1e-5 and not as_it_runs[:, :3].any()
    # the rule at the borders, in both: exactly 0 along the axis that left the box or sits on its border
    kinds = g["kinds"]
    for k in range(3):
        for kind in ("beyond%d" % k, "low%d" % k, "high%d" % k):
            assert m["x_grad"][kinds == kind, k] == 0 and full[kinds == kind, k] == 0, kind


def _kernel_inputs(case):
    g, _, planes, rot, m = case
    consts = R.scene_consts(g["box"], rot)
    planes_cl = [R.channel_last(p) for p in planes]
    rays, z = R.as_rays(g["x"])
    rows = [r.astype(np.float32) for r in m["rows"]]
    return g, m, consts, planes_cl, rays, z, rows


def test_float32_transcription_sits_within_the_bound_of_float64(case):
    """rows: the float64 model's feature gradients rounded to float32.  The transcription against the float64 value of the same expressions,
    K 2^-24 A per component (points_grad_ref: K = 18 / 24); and that float64 value against autograd's x.grad of the float64 model -- they differ
    by the float32 rounding of the pixel coordinates alone (a slope is piecewise linear in the fractions: 1e-5 relative L2)"""
    g, m, consts, planes_cl, rays, z, rows = _kernel_inputs(case)
    got = R.points_grad_f32(planes_cl, consts, rays, z, rows[:3], rows[3])
    worst = R.assert_within_bound(got, planes_cl, consts, rays, z, rows[:3], rows[3])
    print("error / bound: d_points %.3f, d_viewdir %.3f" % tuple(worst))
    want = R.points_grad_f64(planes_cl, consts, rays, z, rows[:3], rows[3])
    assert R.rel_l2(want[0], m["x_grad"][:, :3]) < 1e-5 and R.rel_l2(want[1], m["x_grad"][:, 3:]) < 1e-5
    kinds = g["kinds"]
    for k in range(3):
        for kind in ("beyond%d" % k, "low%d" % k, "high%d" % k):
            assert got[0][kinds == kind, k] == 0, kind
    # a NaN coordinate: that row all NaN, every other row the same bits; rows[d] = None adds nothing
    x2 = g["x"].copy()
    x2[5, 1], x2[9, 4] = np.nan, np.nan
    got2 = R.points_grad_f32(planes_cl, consts, *R.as_rays(x2), rows[:3], rows[3])
    assert np.isnan(got2[0][5]).all() and np.isnan(got2[1][9]).all()
    keep = np.arange(67) != 5
    assert np.array_equal(got2[0][keep].view(np.uint32), got[0][keep].view(np.uint32))
    keep = np.arange(67) != 9
    assert np.array_equal(got2[1][keep].view(np.uint32), got[1][keep].view(np.uint32))
    parts = [R.points_grad_f64(planes_cl, consts, rays, z, [rows[d] if d == k else None for d in range(3)], None)[0] for k in range(3)]
    np.testing.assert_allclose(sum(parts), want[0], rtol=1e-12, atol=1e-15)


def test_entry_signature_and_status_codes(pkg):
    """no GPU here: a call that reached a launch would come back as NVSR_ERR_LAUNCH; every answer below is another code"""
    lib = pkg.capi.lib()
    name = "nvsr_triplane_points_grad"
    args, res = pkg.capi._PROTOS_OPTIONAL[name]
    assert hasattr(lib, name) and len(args) == 10 and res is C.c_int and name in pkg.capi.exported_symbols()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nvsr.h")).read(), flags=re.S)
    m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, header)
    assert m and len(m.group(1).split(",")) == 10
    p, odd = C.c_void_p(0x10000), C.c_void_p(0x10004)          # never dereferenced: the checks return first
    sc = pkg.capi.Scene()
    for d in range(4):
        sc.planes[d], sc.ph[d], sc.pw[d] = 0x10000, 5, 7
    rows = (C.c_void_p * 3)(0x10000, None, 0x10000)
    call = lib.nvsr_triplane_points_grad
    assert call(None, 4, 2, p, p, rows, p, p, p, None) == ERR_NULL
    assert call(C.byref(sc), 4, 2, None, p, rows, p, p, p, None) == ERR_NULL
    assert call(C.byref(sc), 4, 2, p, None, rows, p, p, p, None) == ERR_NULL             # z with d_points
    assert call(C.byref(sc), -1, 2, p, p, rows, p, p, p, None) == ERR_SHAPE
    assert call(C.byref(sc), 4, 0, p, p, rows, p, p, p, None) == ERR_SHAPE
    assert call(C.byref(sc), 4, 4097, p, p, rows, p, p, p, None) == ERR_SHAPE
    assert call(C.byref(sc), 1 << 28, 2, p, p, rows, p, p, p, None) == ERR_SHAPE          # N * S >= 2^29
    assert call(C.byref(sc), 4, 2, p, p, rows, odd, p, p, None) == ERR_ALIGN
    assert call(C.byref(sc), 4, 2, p, p, (C.c_void_p * 3)(0x10000, 0x10004, None), p, p, p, None) == ERR_ALIGN
    assert call(C.byref(sc), 0, 2, p, p, rows, p, p, p, None) == OK                       # nothing to do, nothing launched
    assert call(C.byref(sc), 4, 2, p, p, rows, p, None, None, None) == OK                 # no output asked for
    assert call(C.byref(sc), 0, 2, p, None, None, None, None, p, None) == OK
    sc.planes[2] = None
    assert call(C.byref(sc), 4, 2, p, p, rows, p, p, p, None) == ERR_NULL


def test_operator_is_registered_with_a_fake_implementation(pkg):
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert hasattr(torch.ops.nvsr, "triplane_points_grad")
    import inspect
    assert list(inspect.signature(pkg.ops.triplane_points_grad._init_fn).parameters) == ["planes", "consts", "rays", "z", "rows", "view_rows"]
    assert hasattr(pkg.models.TwoDimPlanesModel, "density_gradient")
    with FakeTensorMode():
        planes = [torch.empty(5, 7, 48) for _ in range(4)]
        rays, z = torch.empty(5, 11), torch.empty(5, 3)
        rows = [torch.empty(15, 48), torch.empty(0), torch.empty(15, 48)]
        d_points, d_viewdir = torch.ops.nvsr.triplane_points_grad(planes, [0.0] * 28, rays, z, rows, torch.empty(5, 48))
        assert d_points.shape == (15, 3) and d_viewdir.shape == (5, 3) and d_points.dtype == torch.float32
    with pytest.raises(Exception):                                                         # real CPU tensors: there is no CPU fallback
        torch.ops.nvsr.triplane_points_grad([torch.zeros(5, 7, 48)] * 4, [0.0] * 28, torch.zeros(5, 11), torch.zeros(5, 3),
                                            [torch.zeros(15, 48)] * 3, torch.zeros(5, 48))


def test_a_route_without_the_input_gradient_warns_once_per_model(pkg):
    a, b = (pkg.models.TwoDimPlanesModel(use_viewdirs=True, skip_connect_every=3, proj_combination="avg",
                                         viewdir_proj_combination="concat_pos", align_corners=True) for _ in range(2))
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        a._warn_no_points_grad("a generic decoder geometry")
        a._warn_no_points_grad("the 'f32' arithmetic")
        assert len(seen) == 1 and "x.grad stays None" in str(seen[0].message)
        b._warn_no_points_grad("the 'f32' arithmetic")
        assert len(seen) == 2
    # density_gradient refuses what it does not cover before it touches a tensor
    a.arithmetic = "f32"
    with pytest.raises(NotImplementedError):
        a.density_gradient(torch.zeros(3, 6))
    generic = pkg.models.TwoDimPlanesModel(use_viewdirs=True, dec_density_layers=3, proj_combination="avg",
                                           viewdir_proj_combination="concat_pos", align_corners=True)
    assert not generic.is_native_geometry()
    with pytest.raises(NotImplementedError):
        generic.density_gradient(torch.zeros(3, 6))
