"""GPU tests of the tri-plane model's input gradient: nvsr_triplane_points_grad alone against its numpy float32 transcription
bit for bit and against float64 within the derived bound; x.grad of a model call in both limb arithmetics against the golden the upstream
code wrote (g23_points_grad.npz: x_grad_full) with plane and decoder gradients from the same rows; density_gradient; the routing of a call whose
points need no gradient; opcheck.  Shapes: the golden's 67 points on 5x7 / 6x4 / 7x5 / 4x3 planes."""
import warnings

import numpy as np
import pytest
import torch

import points_grad_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SID = "lego_DS8_PlRes7_4"
ARITH = {"bf16x3": 3, "f16x2": 2}


def T(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def N_(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def case():
    g, sd, planes, rot = R.load_case()
    return g, sd, planes, rot, R.model64(sd, planes, g["box"], rot, g["x"], g["g_out"])


def build(hip, case, arithmetic, train=("planes", "decoder")):
    g, sd, planes, _, _ = case
    m = hip.models.TwoDimPlanesModel(use_viewdirs=True, skip_connect_every=3, proj_combination="avg", viewdir_proj_combination="concat_pos",
                                     align_corners=True)
    m.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()}, strict=True)
    m = m.to(DEV)
    m.planes_ = torch.nn.ParameterDict({hip.models.get_plane_name(SID, d): torch.nn.Parameter(T(planes[d])) for d in range(4)})
    m.box_coords = {SID: torch.as_tensor(g["box"], dtype=torch.float64)}
    m.set_cur_scene_id(SID)
    m.arithmetic = arithmetic
    for n, p in m.named_parameters():
        p.requires_grad_(("planes" in train) if "planes_" in n else ("decoder" in train and "rot_mats" not in n))
    return m.train()


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the kernel alone
# ---------------------------------------------------------------------------------------------------------------------------------
def _kernel_case(case, name):
    """rays, z and SEEDED rows (never a backward's): 'points' = the golden's points as one-sample rays; 'rays' = N = 5, S = 3 with real depths"""
    g = case[0]
    rng = np.random.default_rng(41)
    if name == "points":
        rays, z = R.as_rays(g["x"])
    else:
        x = np.concatenate([rng.uniform(-2.5, 2.5, (5, 3)), rng.standard_normal((5, 3))], 1).astype(np.float32)
        x[:, 3:] /= np.linalg.norm(x[:, 3:], axis=1, keepdims=True)
        direction = rng.standard_normal((5, 3)).astype(np.float32)
        rays, z = R.as_rays(x, direction, np.sort(rng.uniform(0.1, 2.5, (5, 3)), 1))      # (some samples leave the box: |o + z d| up to ~7)
    M, N = z.size, z.shape[0]
    rows = [rng.standard_normal((M, 48)).astype(np.float32) for _ in range(3)]
    return rays, z, rows, rng.standard_normal((N, 48)).astype(np.float32)


def _device_az_el(rays):
    """(az, el) of view_taps as the DEVICE's atan2f rounds them (torch.atan2 on the GPU is the same device-library function; numpy's
    arctan2 need not agree in the last bit); sqrt and the sum of squares are single correctly rounded operations on both sides"""
    vx, vy, vz = rays[:, 8], rays[:, 9], rays[:, 10]
    r = np.sqrt(vx * vx + vy * vy)
    return N_(torch.atan2(T(vy), T(vx))), N_(torch.atan2(T(vz), T(r)))


def _launch(hip, planes_cl, consts, rays, z, rows, view_rows):
    flat = [float(v) for v in consts[0]] + [float(v) for v in consts[1]] + [float(v) for p in consts[2] for v in p]
    empty = torch.empty(0, device=DEV)
    out = torch.ops.nvsr.triplane_points_grad([T(p) for p in planes_cl], flat, T(rays), T(z), [empty if r is None else T(r) for r in rows],
                                              empty if view_rows is None else T(view_rows))
    return N_(out[0]), N_(out[1])


@pytest.mark.parametrize("name", ["points", "rays"])
def test_kernel_equals_the_float32_transcription_bit_for_bit(hip, case, name):
    """d_points / d_viewdir equal points_grad_ref.points_grad_f32 bit for bit and sit within K 2^-24 A of float64 per component, K = 18
    (d_points) / 24 (d_viewdir) roundings on the longest path (derived in points_grad_ref's docstring); rows[d] = NULL, view_rows = NULL; exact
    zeros where the rule says 0; NaN rows"""
    g, _, planes, rot, _ = case
    consts, planes_cl = R.scene_consts(g["box"], rot), [R.channel_last(p) for p in planes]
    rays, z, rows, view_rows = _kernel_case(case, name)
    az_el = _device_az_el(rays)
    got = _launch(hip, planes_cl, consts, rays, z, rows, view_rows)
    want = R.points_grad_f32(planes_cl, consts, rays, z, rows, view_rows, az_el)
    assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1]))
    worst = R.assert_within_bound(got, planes_cl, consts, rays, z, rows, view_rows, az_el)
    print("%s: error / bound: d_points %.3f, d_viewdir %.3f" % ((name,) + tuple(worst)))
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all() and np.abs(got[0]).max() > 0.1 and np.abs(got[1]).max() > 1e-3
    # one plane absent; the view rows absent
    rows1 = [rows[0], None, rows[2]]
    got1 = _launch(hip, planes_cl, consts, rays, z, rows1, None)
    want1 = R.points_grad_f32(planes_cl, consts, rays, z, rows1, None, az_el)
    assert np.array_equal(bits(got1[0]), bits(want1[0])) and np.array_equal(bits(got1[1]), bits(want1[1])) and not got1[1].any()
    assert not np.array_equal(bits(got1[0]), bits(got[0]))
    if name == "points":
        kinds = g["kinds"]
        for k in range(3):
            for kind in ("beyond%d" % k, "low%d" % k, "high%d" % k):
                assert got[0][kinds == kind, k] == 0 and np.abs(got[0][kinds == kind]).max() > 0, kind
            assert got[0][kinds == "line%d" % k, k] != 0                       # an interior texel line takes the cell floor selects
    # NaN: a position coordinate (ray 2: every sample of it), a view component (ray 3); every other row keeps its bits
    bad = rays.copy()
    bad[2, 1], bad[3, 9] = np.nan, np.nan
    got2 = _launch(hip, planes_cl, consts, bad, z, rows, view_rows)
    S = z.shape[1]
    hit = np.arange(z.size) // S == 2
    assert np.isnan(got2[0][hit]).all() and np.array_equal(bits(got2[0][~hit]), bits(got[0][~hit]))
    hit = np.arange(z.shape[0]) == 3
    assert np.isnan(got2[1][hit]).all() and np.array_equal(bits(got2[1][~hit]), bits(got[1][~hit]))


def test_kernel_entry_answers_empty_and_bad_calls(hip, case):
    g, _, planes, rot, _ = case
    consts, planes_cl = R.scene_consts(g["box"], rot), [R.channel_last(p) for p in planes]
    rays, z, rows, view_rows = _kernel_case(case, "rays")
    got = _launch(hip, planes_cl, consts, rays[:0], z[:0], [r[:0] for r in rows], view_rows[:0])
    assert got[0].shape == (0, 3) and got[1].shape == (0, 3)
    capi, C = hip.capi, hip.capi.C
    flat = [float(v) for v in consts[0]] + [float(v) for v in consts[1]] + [float(v) for p in consts[2] for v in p]
    keep = [T(p) for p in planes_cl]
    sc = hip.ops._scene(keep, flat)
    r_, z_, rows_, v_ = T(rays), T(z), [T(r) for r in rows], T(view_rows)
    rp = (C.c_void_p * 3)(*[r.data_ptr() for r in rows_])
    dp, dv = torch.full((15, 3), 7.0, device=DEV), torch.full((5, 3), 7.0, device=DEV)
    call = capi.lib().nvsr_triplane_points_grad
    args = lambda N, S, dp_, dv_: (C.byref(sc), N, S, capi.ptr(r_), capi.ptr(z_), rp, capi.ptr(v_), capi.ptr(dp_), capi.ptr(dv_), capi.stream())
    assert call(*args(5, 0, dp, dv)) == 1 and call(*args(-1, 3, dp, dv)) == 1                      # NVSR_ERR_SHAPE
    assert call(None, 5, 3, capi.ptr(r_), capi.ptr(z_), rp, capi.ptr(v_), capi.ptr(dp), capi.ptr(dv), capi.stream()) == 3   # NVSR_ERR_NULL
    assert call(*args(5, 3, None, None)) == 0 and call(*args(0, 3, dp, dv)) == 0                    # nothing to do
    torch.cuda.synchronize()
    assert bool((dp == 7).all()) and bool((dv == 7).all())                                          # ... and nothing written
    assert call(*args(5, 3, None, dv)) == 0                                                         # one output alone
    torch.cuda.synchronize()
    az_el = _device_az_el(rays)
    assert bool((dp == 7).all()) and np.array_equal(bits(N_(dv)), bits(R.points_grad_f32(planes_cl, consts, rays, z, None, view_rows, az_el)[1]))


def test_operator_traces_and_refuses_bad_tensors(hip, case):
    g, _, planes, rot, _ = case
    consts, planes_cl = R.scene_consts(g["box"], rot), [R.channel_last(p) for p in planes]
    rays, z, rows, view_rows = _kernel_case(case, "rays")
    flat = [float(v) for v in consts[0]] + [float(v) for v in consts[1]] + [float(v) for p in consts[2] for v in p]
    args = ([T(p) for p in planes_cl], flat, T(rays), T(z), [T(rows[0]), torch.empty(0, device=DEV), T(rows[2])], T(view_rows))
    torch.library.opcheck(torch.ops.nvsr.triplane_points_grad, args, test_utils=("test_schema", "test_faketensor"))
    with pytest.raises(ValueError):
        torch.ops.nvsr.triplane_points_grad(args[0], flat, args[2], args[3], [T(rows[0])[:, :40]] * 3, args[5])
    with pytest.raises(ValueError):
        torch.ops.nvsr.triplane_points_grad(args[0], flat, args[2], args[3], args[4][:2], args[5])
    with pytest.raises(ValueError):
        torch.ops.nvsr.triplane_points_grad(args[0], flat, args[2], args[3].double(), args[4], args[5])
    with pytest.raises(ValueError):
        torch.ops.nvsr.triplane_points_grad(args[0], flat, args[2], args[3], args[4], T(view_rows)[:4])


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. end to end
# ---------------------------------------------------------------------------------------------------------------------------------
def _backward(hip, model, case):
    g = case[0]
    for p in model.parameters():
        p.grad = None
    x = T(g["x"]).requires_grad_(True)
    out = model(x)
    (out * T(g["g_out"])).sum().backward()
    planes = [N_(model.planes_[hip.models.get_plane_name(SID, d)].grad) for d in range(4)]
    dec = np.concatenate([N_(p.grad).reshape(-1) for p in model.decoder_parameters()])
    return N_(out), N_(x.grad), planes, dec


@pytest.mark.parametrize("arithmetic", ["f16x2", "bf16x3"])
def test_model_call_gives_the_input_gradient_of_the_upstream_golden(hip, case, arithmetic):
    """(model(x) * g_out).sum().backward() with x.requires_grad, planes and decoder training in the same call: x.grad against x_grad_full (what
    the upstream code computes once its no_grad is shimmed away), relative L2 over all rows below 2e-4 -- the bound
    test_model_call_is_differentiable_vs_torch_reference applies to the plane gradients of the same call; it transfers because x.grad is, like a
    plane gradient, a fixed linear map of the same feature-gradient rows.  Plane and decoder gradients against the float64 restatement at the
    same bound: the shared rows route gives all three.  Two runs give the same bits of x.grad and of the plane gradients (no atomics there).
    Measured (profiles/points_grad.txt): x.grad against x_grad_full 7.7e-7 in f16x2, 5.1e-7 in bf16x3; planes and decoder 4.5e-7 ... 9.4e-7."""
    g, _, _, _, m64 = case
    model = build(hip, case, arithmetic)
    flat = model.scene_args()[1]
    consts = R.scene_consts(g["box"], case[3])
    assert np.array_equal(np.array(flat, np.float32), np.concatenate([consts[0], consts[1]] + consts[2]))
    out, gx, gplanes, gdec = _backward(hip, model, case)
    np.testing.assert_allclose(out, g["out"], rtol=0, atol=3e-5)
    full = g["x_grad_full"]
    errs = dict(x=R.rel_l2(gx, full), x_pos=R.rel_l2(gx[:, :3], full[:, :3]), x_view=R.rel_l2(gx[:, 3:], full[:, 3:]),
                x_vs_f64=R.rel_l2(gx, m64["x_grad"]), decoder=R.rel_l2(gdec[None], m64["decoder"][None]))
    errs.update({"plane%d" % d: R.rel_l2(gplanes[d].reshape(1, -1), m64["planes"][d].reshape(1, -1)) for d in range(4)})
    print("%s: relative L2 errors: %s" % (arithmetic, ", ".join("%s %.3g" % kv for kv in errs.items())))
    assert np.isfinite(gx).all()
    assert errs["x"] < 2e-4, errs
    assert errs["x_pos"] < 2e-4 and errs["x_view"] < 2e-4, errs           # (each half is such a linear map on its own)
    assert all(errs["plane%d" % d] < 2e-4 for d in range(4)) and errs["decoder"] < 2e-4, errs
    kinds = g["kinds"]
    for k in range(3):
        for kind in ("beyond%d" % k, "low%d" % k, "high%d" % k):
            assert gx[kinds == kind, k] == 0, kind
    _, gx2, gplanes2, _ = _backward(hip, model, case)
    assert np.array_equal(bits(gx), bits(gx2)) and all(np.array_equal(bits(a), bits(b)) for a, b in zip(gplanes, gplanes2))
    # frozen planes and decoder: the points alone still get their gradient, the same bits
    frozen = build(hip, case, arithmetic, train=())
    x = T(g["x"]).requires_grad_(True)
    (frozen(x) * T(g["g_out"])).sum().backward()
    assert np.array_equal(bits(N_(x.grad)), bits(gx))
    # a NaN coordinate: that row's position gradient is NaN, the other rows keep their bits
    xn = g["x"].copy()
    xn[4, 2] = np.nan
    x = T(xn).requires_grad_(True)
    (frozen(x) * T(g["g_out"])).sum().backward()
    got = N_(x.grad)
    keep = np.arange(67) != 4
    assert np.isnan(got[4, :3]).all() and np.array_equal(bits(got[keep]), bits(gx[keep]))


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. density_gradient
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arithmetic", ["f16x2", "bf16x3"])
def test_density_gradient_against_float64(hip, case, arithmetic):
    """d sigma_raw / d xyz on the golden's points against autograd of the float64 restatement with g_out = (0, 0, 0, 1): relative L2 below 2e-4
    (the end-to-end bound: the same linear map of the density decoder's rows)"""
    g, sd, planes, rot, _ = case
    g_sigma = np.zeros((67, 4))
    g_sigma[:, 3] = 1
    want = R.model64(sd, planes, g["box"], rot, g["x"], g_sigma)["x_grad"][:, :3]
    model = build(hip, case, arithmetic).eval()
    got = model.density_gradient(T(g["x"]))
    assert got.shape == (67, 3) and not got.requires_grad
    err = R.rel_l2(N_(got), want)
    print("%s: density_gradient relative L2 error %.3g" % (arithmetic, err))
    assert err < 2e-4
    assert model.density_gradient(T(g["x"][:0])).shape == (0, 3)
    model.arithmetic = "f32"
    with pytest.raises(NotImplementedError):
        model.density_gradient(T(g["x"]))


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. routing
# ---------------------------------------------------------------------------------------------------------------------------------
WATCHED = ("decode_rays", "backward", "rows", "taps", "points_grad", "weight_grad")


def _spied_backward(hip, monkeypatch, model, case, x_grad):
    calls, real = [], hip.capi.call

    def spy(name, *a):
        if any(w in name for w in WATCHED):
            calls.append(name)
        return real(name, *a)

    monkeypatch.setattr(hip.capi, "call", spy)
    g = case[0]
    x = T(g["x"]).requires_grad_(x_grad)
    (model(x) * T(g["g_out"])).sum().backward()
    torch.cuda.synchronize()
    monkeypatch.setattr(hip.capi, "call", real)
    return calls, x.grad


def test_points_without_grad_keep_todays_launch_sequence(hip, case, monkeypatch):
    """x does not require a gradient: the same entries in the same order as before this operator existed, on the atomic and on the ordered
    route, and nvsr_triplane_points_grad is never called; with x.requires_grad: the rows route once, whatever the mode says"""
    monkeypatch.delenv("NVSR_DETERMINISTIC", raising=False)
    model = build(hip, case, "bf16x3")
    calls, gx = _spied_backward(hip, monkeypatch, model, case, False)
    assert gx is None
    assert calls == ["nvsr_decode_rays_arith", "nvsr_render_pass_backward_gates_arith", "nvsr_decoder_weight_grad_arith"], calls
    ordered = (["nvsr_decode_rays_arith", "nvsr_render_pass_backward_rows_arith"] + ["nvsr_internal_plane_taps", "nvsr_rows_scatter"] * 3 +
               ["nvsr_view_rows_reduce", "nvsr_internal_plane_taps", "nvsr_rows_scatter", "nvsr_decoder_weight_grad_det_arith"])
    with hip.capi.deterministic_scope(True):
        calls, gx = _spied_backward(hip, monkeypatch, model, case, False)
    assert gx is None and calls == ordered, calls
    calls, gx = _spied_backward(hip, monkeypatch, model, case, True)
    assert gx is not None and calls == ordered[:-1] + ["nvsr_triplane_points_grad", "nvsr_decoder_weight_grad_arith"], calls
    # the 'f32' arithmetic: x.grad stays None, warned once per model
    model32 = build(hip, case, "f32")
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        for _ in range(2):
            calls, gx = _spied_backward(hip, monkeypatch, model32, case, True)
            assert gx is None and "nvsr_triplane_points_grad" not in calls
    assert len([w for w in seen if "x.grad stays None" in str(w.message)]) == 1
