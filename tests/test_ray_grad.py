"""GPU tests of the ray and camera-pose gradients (csrc/ray_grad.hip): the four entries against their numpy float32
transcriptions bit for bit and against float64 within the derived bounds (ray_grad_ref's docstring counts the roundings), edge rays, opcheck;
the differentiable forwards; a training render whose rays and pose require a gradient."""
import numpy as np
import pytest
import torch

import ray_grad_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f32, f64 = np.float32, np.float64


def T(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def N_(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


# ---------------------------------------------------------------------------------------------------------------------------------
# nvsr_rays_grad
# ---------------------------------------------------------------------------------------------------------------------------------
def rays_case(N, S, seed=0):
    rng = np.random.default_rng(1000 * N + S + seed)
    rays = rng.standard_normal((N, 11)).astype(f32)
    rays[:, 6:8] = (2.0, 6.0)
    z = np.sort(rng.uniform(2.0, 6.0, (N, S)), 1).astype(f32)
    raw = rng.standard_normal((N, S, 4)).astype(f32)            # (half of the densities are negative: relu shuts them)
    return dict(rays=rays, z=z, d_points=rng.standard_normal((N * S, 3)).astype(f32), d_viewdir=rng.standard_normal((N, 3)).astype(f32), raw=raw,
                noise=(0.3 * rng.standard_normal((N, S))).astype(f32), g_raw=rng.standard_normal((N, S, 4)).astype(f32))


def launch_rays_grad(c, accumulate=False, onto=None):
    N = c["rays"].shape[0]
    out = torch.full((N, 11), float("nan"), device=DEV) if onto is None else T(onto).clone()
    torch.ops.nvsr.rays_grad(T(c["rays"]), T(c["z"]), T(c["d_points"]), T(c["d_viewdir"]), T(c["raw"]), T(c["noise"]), T(c["g_raw"]), out, accumulate)
    return N_(out)


def check_rays_grad(c, accumulate=False, onto=None):
    got = launch_rays_grad(c, accumulate, onto)
    args = (c["rays"], c["z"], c["d_points"], c["d_viewdir"], c["raw"], c["noise"], c["g_raw"], accumulate, onto)
    assert same_bits(got, R.rays_grad(f32, *args))
    exact, terms = R.rays_grad(f64, *args), R.rays_grad(f64, *args, terms=True)
    S = c["z"].shape[1]
    k012, k345 = R.k_rays_grad(S, accumulate)
    K = np.array([k012] * 3 + [k345] * 3 + [0, 0] + [1] * 3, f64)       # (columns 8..10: a copy; one addition with accumulate)
    err = np.abs(got.astype(f64) - exact)
    assert (err <= K * R.U * terms).all(), (err / np.maximum(K * R.U * terms, 1e-300)).max()
    assert not got[:, 6:8].any() and not np.signbit(got[:, 6:8]).any()
    return got, float((err[:, :6] / np.maximum(np.array([k012] * 3 + [k345] * 3) * R.U * terms[:, :6], 1e-300)).max())


@pytest.mark.parametrize("S", [1, 63, 64, 65, 192])
@pytest.mark.parametrize("N", [1, 3, 67])
def test_rays_grad_equals_its_transcription_and_meets_the_float64_bound(hip, N, S):
    c = rays_case(N, S)
    got, worst = check_rays_grad(c)
    print("N %d S %d: worst error / bound %.3f" % (N, S, worst))
    assert np.isfinite(got).all() and np.abs(got[:, :6]).max() > 0.1
    # the fine pass adds onto the coarse pass's row
    onto = rays_case(N, 1, seed=5)["rays"]
    check_rays_grad(c, accumulate=True, onto=onto)
    # without noise; each of d_points / d_viewdir absent
    for drop in (("noise",), ("d_points",), ("d_viewdir",), ("d_points", "d_viewdir", "noise")):
        c2 = {k: (None if k in drop else v) for k, v in c.items()}
        got2, _ = check_rays_grad(c2)
        if "d_viewdir" in drop:
            assert not got2[:, 8:].any()
        if "d_points" in drop:
            assert not got2[:, :3].any()
    # twice: the same bits
    assert same_bits(launch_rays_grad(c), got)


def test_rays_grad_edge_rays(hip):
    """a NaN origin makes that ray's row NaN and changes no other row; a ray whose densities are all shut (sigma = 0 everywhere) has a zero
    compositor term: its direction columns are the points' sum alone"""
    c = rays_case(5, 70)
    good = launch_rays_grad(c)
    bad = dict(c, rays=c["rays"].copy())
    bad["rays"][2, 1] = np.nan
    got = launch_rays_grad(bad)
    assert np.isnan(got[2][[0, 1, 2, 3, 4, 5, 8, 9, 10]]).all() and not got[2, 6:8].any()
    keep = np.arange(5) != 2
    assert same_bits(got[keep], good[keep])
    assert same_bits(got, R.rays_grad(f32, bad["rays"], c["z"], c["d_points"], c["d_viewdir"], c["raw"], c["noise"], c["g_raw"]))
    shut = dict(c, raw=c["raw"].copy(), noise=None)
    shut["raw"][3, :, 3] = -np.abs(shut["raw"][3, :, 3])
    got = launch_rays_grad(shut)
    nopts = launch_rays_grad(dict(shut, g_raw=np.zeros_like(c["g_raw"])))           # (no compositor term anywhere)
    assert same_bits(got[3], nopts[3]) and not same_bits(got[0], nopts[0])


# ---------------------------------------------------------------------------------------------------------------------------------
# packer and NDC backwards
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 65])
def test_pack_rays_backward_equals_its_transcription(hip, N):
    rng = np.random.default_rng(N)
    g, v = rng.standard_normal((N, 11)).astype(f32), rng.standard_normal((N, 3)).astype(f32)
    for view_is_rd in (True, False):
        got = [N_(t) for t in torch.ops.nvsr.pack_rays_backward(T(g), T(v), view_is_rd)]
        want = R.pack_rays_backward(f32, g, v, view_is_rd)
        exact, terms = R.pack_rays_backward(f64, g, v, view_is_rd), R.pack_rays_backward(f64, g, v, view_is_rd, terms=True)
        for i in range(3):
            if want[i] is None:
                assert got[i].size == 0
                continue
            assert same_bits(got[i], want[i])
            K = R.K_PACK_VIEW_IS_RD if (view_is_rd and i == 1) else R.K_PACK
            assert (np.abs(got[i].astype(f64) - exact[i]) <= K * R.U * terms[i]).all()


@pytest.mark.parametrize("N", [1, 65])
def test_ndc_rays_backward_equals_its_transcription(hip, N):
    """bit for bit; against float64 per component within (20 + 8 kappa) 2^-24 A, kappa = (|o_2| + |t d_2|) / |oz| per ray carrying the
    conditioning of the cancelling divisor oz, A the absolute-term version of the expressions (derived in ray_grad_ref's docstring, counted in
    include/nvsr.h)"""
    rng = np.random.default_rng(10 + N)
    H, W, focal, near = 12, 16, 14.0, 1.0
    ro = (rng.standard_normal((N, 3)) * 0.1).astype(f32)
    rd = rng.standard_normal((N, 3)).astype(f32)
    rd[:, 2] = -1.0 - np.abs(rd[:, 2])                       # forward-facing
    go, gd = rng.standard_normal((N, 3)).astype(f32), rng.standard_normal((N, 3)).astype(f32)
    got = [N_(t) for t in torch.ops.nvsr.ndc_rays_backward(H, W, focal, near, T(ro), T(rd), T(go), T(gd))]
    want, exact = R.ndc_rays_backward(f32, H, W, focal, near, ro, rd, go, gd), R.ndc_rays_backward(f64, H, W, focal, near, ro, rd, go, gd)
    A_ro, A_rd, kappa = R.ndc_rays_backward(f64, H, W, focal, near, ro, rd, go, gd, terms=True)
    for g, w, e, A in zip(got, want, exact, (A_ro, A_rd)):
        assert same_bits(g, w)
        ratio = np.abs(g.astype(f64) - e) / ((20 + 8 * kappa)[:, None] * R.U * A)
        assert (ratio <= 1).all(), ratio.max()
    print("N %d: worst error / bound %.3f, kappa up to %.2f" % (N, ratio.max(), kappa.max()))
    # the forward operator is the direct call, bit for bit, and carries this backward
    o1, d1 = hip.nerf_helpers.ndc_rays(H, W, focal, near, T(ro), T(rd))
    ro_t, rd_t = T(ro).requires_grad_(True), T(rd).requires_grad_(True)
    o2, d2 = hip.nerf_helpers.ndc_rays(H, W, focal, near, ro_t, rd_t)
    assert torch.equal(o1, o2) and torch.equal(d1, d2) and o2.requires_grad
    ((o2 * T(go)).sum() + (d2 * T(gd)).sum()).backward()
    assert same_bits(N_(ro_t.grad), want[0]) and same_bits(N_(rd_t.grad), want[1])


# ---------------------------------------------------------------------------------------------------------------------------------
# nvsr_ray_bundle_backward
# ---------------------------------------------------------------------------------------------------------------------------------
def bundle_cases():
    rng = np.random.default_rng(77)
    rc257 = np.stack([rng.integers(-2, 9, 257), rng.integers(-3, 11, 257)], 1).astype(np.int32)        # 6 x 8 image: repeats, out-of-image entries
    rc257[5] = rc257[6] = rc257[200]
    rc3 = np.stack([rng.integers(0, 6, 600), rng.integers(0, 8, 600)], 1).astype(np.int32)              # 600 rays: three slabs of 256
    return {"grid5x7": (5, 7, None, 0), "grid5x7pad2": (5, 7, None, 2), "sel257": (6, 8, rc257, 0), "sel600": (6, 8, rc3, 0)}


@pytest.mark.parametrize("name", list(bundle_cases()))
def test_ray_bundle_backward_equals_its_transcription_and_meets_the_float64_bound(hip, name):
    H, W, rc, pad = bundle_cases()[name]
    fx, fy, off = 9.5, 9.25, 0.4375
    N = (H + 2 * pad) * (W + 2 * pad) if rc is None else rc.shape[0]
    rng = np.random.default_rng(N)
    d_ro, d_rd = rng.standard_normal((N, 3)).astype(f32), rng.standard_normal((N, 3)).astype(f32)
    got = N_(torch.ops.nvsr.ray_bundle_backward(H, W, fx, fy, off, T(rc), pad, T(d_ro), T(d_rd)))
    args = (H, W, fx, fy, off, d_ro, d_rd, rc, pad)
    assert same_bits(got, R.ray_bundle_backward(f32, *args))
    assert not got[3].any() and not np.signbit(got[3]).any()
    exact, terms = R.ray_bundle_backward(f64, *args), R.ray_bundle_backward(f64, *args, terms=True)
    assert (np.abs(got.astype(f64) - exact) <= R.k_bundle(N) * R.U * terms).all()
    assert same_bits(N_(torch.ops.nvsr.ray_bundle_backward(H, W, fx, fy, off, T(rc), pad, T(d_ro), T(d_rd))), got)
    # the forward operators: the direct calls bit for bit, with this backward behind them (a 3 x 4 pose takes the first three rows)
    pose = T(np.concatenate([rng.standard_normal((3, 4)), [[0, 0, 0, 1]]]).astype(f32))
    for rows in (4, 3):
        p = pose[:rows].clone().requires_grad_(True)
        if rc is None:
            ref = hip.nerf_helpers.get_ray_bundle(H, W, [fy, fx], pose, pad, off)
            out = hip.nerf_helpers.get_ray_bundle(H, W, [fy, fx], p, pad, off)
        else:
            ref = hip.training.get_ray_bundle_at(H, W, [fy, fx], pose, T(rc), off)
            out = hip.training.get_ray_bundle_at(H, W, [fy, fx], p, T(rc), off)
        assert torch.equal(ref[0], out[0]) and torch.equal(ref[1], out[1]) and out[1].requires_grad and not ref[1].requires_grad
        ((out[0].reshape(N, 3) * T(d_ro)).sum() + (out[1].reshape(N, 3) * T(d_rd)).sum()).backward()
        assert same_bits(N_(p.grad), got[:rows])


def test_opcheck_of_the_new_operators(hip):
    nv = torch.ops.nvsr
    c = rays_case(3, 5)
    tests = ("test_schema", "test_faketensor", "test_autograd_registration")
    chk = lambda op, args: torch.library.opcheck(op, args, test_utils=tests)
    chk(nv.rays_grad, (T(c["rays"]), T(c["z"]), T(c["d_points"]), T(c["d_viewdir"]), T(c["raw"]), None, T(c["g_raw"]), torch.zeros(3, 11, device=DEV), True))
    chk(nv.pack_rays_backward, (T(c["rays"]), T(c["d_viewdir"]), True))
    chk(nv.pack_rays_backward, (T(c["rays"]), T(c["d_viewdir"]), False))
    v3 = lambda: torch.randn(3, 3, device=DEV) - torch.tensor([0, 0, 3.0], device=DEV)
    chk(nv.ndc_rays_backward, (6, 8, 7.0, 1.0, v3(), v3(), v3(), v3()))
    rc = torch.tensor([[0, 1], [2, 2], [0, 1]], dtype=torch.int32, device=DEV)
    chk(nv.ray_bundle_backward, (6, 8, 7.0, 7.0, 0.0, rc, 0, v3(), v3()))
    chk(nv.ray_bundle_backward, (1, 3, 7.0, 7.0, 0.0, None, 0, v3(), v3()))
    pose = torch.eye(4, device=DEV)
    # the four differentiable forwards: the whole opcheck (its default utilities, test_aot_dispatch_dynamic among them)
    torch.library.opcheck(nv.ray_bundle, (2, 3, 7.0, 7.0, pose.clone().requires_grad_(True), 1, 0.25))
    torch.library.opcheck(nv.ray_bundle_at, (6, 8, 7.0, 7.0, pose.clone().requires_grad_(True), 0.25, rc))
    torch.library.opcheck(nv.ndc_rays, (6, 8, 7.0, 1.0, v3().requires_grad_(True), v3().requires_grad_(True)))
    torch.library.opcheck(nv.pack_rays, (v3().requires_grad_(True), v3().requires_grad_(True), None, 2.0, 6.0))
    torch.library.opcheck(nv.pack_rays, (v3().requires_grad_(True), v3().requires_grad_(True), v3().requires_grad_(True), 2.0, 6.0))


def test_pack_rays_is_differentiable_and_unchanged(hip):
    """train_utils.pack_rays with origins / directions that require a gradient: the direct call's bits; the gradient is pack_rays_backward's,
    with the NDC warp the two direction gradients are added (the view directions come from the directions before the warp)"""
    rng = np.random.default_rng(3)
    N = 65
    ro, rd = (0.1 * rng.standard_normal((N, 3))).astype(f32), rng.standard_normal((N, 3)).astype(f32)
    rd[:, 2] = -1.0 - np.abs(rd[:, 2])
    g = rng.standard_normal((N, 11)).astype(f32)
    for ndc in (False, True):
        kw = dict(H=12, W=16, focal=14.0, no_ndc=not ndc)
        near, far = (0.0, 1.0) if ndc else (2.0, 6.0)
        ref = hip.train_utils.pack_rays(T(ro), T(rd), near, far, **kw)
        o, d = T(ro).requires_grad_(True), T(rd).requires_grad_(True)
        out = hip.train_utils.pack_rays(o, d, near, far, **kw)
        assert torch.equal(ref, out) and out.requires_grad and not ref.requires_grad
        (out * T(g)).sum().backward()
        if not ndc:
            want = R.pack_rays_backward(f32, g, rd, True)
            assert same_bits(N_(o.grad), want[0]) and same_bits(N_(d.grad), want[1])
        else:
            p_ro, p_rd, p_vs = R.pack_rays_backward(f32, g, rd, False)
            n_ro, n_rd = R.ndc_rays_backward(f32, 12, 16, 14.0, 1.0, ro, rd, p_ro, p_rd)
            assert same_bits(N_(o.grad), n_ro)
            assert np.allclose(N_(d.grad), n_rd + p_vs, rtol=0, atol=2 ** -22 * np.abs(n_rd).max())       # (autograd adds the two: either order)


# ---------------------------------------------------------------------------------------------------------------------------------
# a training render whose rays and pose require a gradient (fixture g27: upstream itself, differentiated through its rays)
# ---------------------------------------------------------------------------------------------------------------------------------
class Opt:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def g27_models(hip, ci, arithmetic, what=("planes", "decoder"), proj_combination="avg"):
    """proj_combination other than 'avg': the same layer sizes as a GENERIC decoder geometry (models.is_native_geometry)"""
    g, dec, planes = R.g27_case(ci)
    sid = "lego_DS8_PlRes12_8"
    ms = []
    for tag in ("coarse.", "fine."):
        m = hip.models.TwoDimPlanesModel(use_viewdirs=True, skip_connect_every=3, proj_combination=proj_combination,
                                         viewdir_proj_combination="concat_pos", align_corners=True)
        m.load_state_dict({k[len(tag):]: torch.as_tensor(v) for k, v in dec.items() if k.startswith(tag)}, strict=True)
        m = m.to(DEV)
        m.planes_ = (ms[0].planes_ if ms else
                     torch.nn.ParameterDict({hip.models.get_plane_name(sid, d): torch.nn.Parameter(T(planes[d])) for d in range(4)}))
        m.box_coords = {sid: torch.as_tensor(g["c%d_box" % ci], dtype=torch.float64)}
        m.set_cur_scene_id(sid)
        m.arithmetic = arithmetic
        ms.append(m)
    for m in ms:
        for n, p in m.named_parameters():
            p.requires_grad_(("planes" in what) if "planes_" in n else ("decoder" in what and "rot_mats" not in n))
        m.train()
    focal, near, far, ndc = (float(v) for v in g["c%d_scene" % ci])
    nc, nf, std = g["params"]
    mode = Opt(chunksize=131072, perturb=True, num_coarse=int(nc), num_fine=int(nf), white_background=False, radiance_field_noise_std=float(std),
               lindisp=False)
    opts = Opt(nerf=Opt(use_viewdirs=True, train=mode, validation=mode))
    scfg = Opt(near=near, far=far, no_ndc=not ndc)
    rnd = {k: T(g["c%d_%s" % (ci, k)]) for k in ("t_rand", "u", "noise_coarse", "noise_fine")}
    return g, ms[0], ms[1], sid, focal, opts, scfg, rnd


def g27_render(hip, g, ci, mc, mf, sid, focal, opts, scfg, rnd, pose_grad):
    H, W = (int(v) for v in g["hw"])
    for m in (mc, mf):
        m.zero_grad(set_to_none=True)
    pose = T(g["c%d_pose" % ci]).requires_grad_(pose_grad)
    ro, rd = hip.nerf_helpers.get_ray_bundle(H, W, focal, pose)
    sel = T(g["c%d_sel" % ci].astype(np.int64))
    batch_rays = torch.stack([ro.reshape(-1, 3)[sel], rd.reshape(-1, 3)[sel]], 0)
    if pose_grad:
        batch_rays.retain_grad()
    out = hip.train_utils.run_one_iter_of_nerf(H, W, focal, mc, mf, batch_rays, opts, sid, mode="train", scene_config=scfg, randoms=rnd)
    target = T(g["c%d_target" % ci])
    loss = torch.nn.functional.mse_loss(out[0], target) + torch.nn.functional.mse_loss(out[3], target)
    z_f = N_(out[3].grad_fn.saved["z_f"])
    loss.backward()
    planes = [N_(p.grad) for p in mc.planes_.values()]
    decs = [np.concatenate([N_(p.grad).reshape(-1) for p in m.decoder_parameters()]) for m in (mc, mf)]
    return float(loss.detach()), z_f, pose.grad, batch_rays.grad, planes, decs


def rel_l2(a, b):
    return float(np.linalg.norm(np.asarray(a, f64) - np.asarray(b, f64)) / np.linalg.norm(np.asarray(b, f64)))


@pytest.mark.parametrize("arithmetic", ["f16x2", "bf16x3"])
@pytest.mark.parametrize("ci", [0, 1])
def test_training_render_returns_upstreams_ray_and_pose_gradients(hip, monkeypatch, ci, arithmetic):
    """run_one_iter_of_nerf(mode='train') on g27 (case 0 synthetic, case 1 NDC): batch_rays.grad and pose.grad against upstream's float64 run
    as relative L2 over the whole tensor (per-ray sums cancel: no per-element bound).  The bound is the larger of 2e-4 (the x.grad bound on
    g23) and 8 x the fixture's own float32-versus-float64 relative L2.  Rays whose fine depths differ from upstream's by more than 1e-5
    relative are left out (at most 2 % of them may).  The plane gradients meet g11's tolerance; plane and decoder gradients equal those of the
    same call in deterministic mode without ray gradients bit for bit.  Without the feature both gradients are None."""
    monkeypatch.delenv("NVSR_DETERMINISTIC", raising=False)
    g, mc, mf, sid, focal, opts, scfg, rnd = g27_models(hip, ci, arithmetic)
    loss, z_f, pose_grad, rays_grad, planes, decs = g27_render(hip, g, ci, mc, mf, sid, focal, opts, scfg, rnd, True)
    assert rays_grad is not None and pose_grad is not None
    pre = "c%d_" % ci
    assert abs(loss - float(g[pre + "loss64"])) < 2e-4
    z64 = g[pre + "z_fine64"]
    flipped = (np.abs(z_f - z64) > 1e-5 * np.abs(z64)).any(1)
    assert flipped.mean() <= 0.02, flipped
    keep = ~flipped
    for name, got, k32, k64 in (("rays", N_(rays_grad)[:, keep], g[pre + "rays_grad"][:, keep], g[pre + "rays_grad64"][:, keep]),
                                ("pose", N_(pose_grad), g[pre + "pose_grad"], g[pre + "pose_grad64"])):
        bound = max(2e-4, 8 * rel_l2(k32, k64))
        err = rel_l2(got, k64)
        print("case %d %s %s.grad: relative L2 %.3g (upstream float32 vs float64 %.3g, bound %.3g)" % (ci, arithmetic, name, err, rel_l2(k32, k64), bound))
        assert err <= bound, (name, err, bound)
    assert not N_(pose_grad)[3].any()
    for d in range(4):
        ref = g[pre + "grad64_plane%d" % d]
        assert rel_l2(planes[d], ref) < 1e-2 and np.abs(planes[d] - ref).max() <= 3e-2 * np.abs(ref).max()
    with hip.capi.deterministic_scope(True):
        _, _, pg, rg, planes_det, decs_det = g27_render(hip, g, ci, mc, mf, sid, focal, opts, scfg, rnd, False)
    assert pg is None and rg is None
    for a, b in zip(planes + decs, planes_det + decs_det):
        assert same_bits(a, b)


def test_a_step_whose_pose_needs_no_gradient_keeps_the_parents_entries_and_bits(hip, monkeypatch):
    """the entry sequence of two TrainStep iterations equals the one recorded from the parent commit (tests/ray_grad_entry_table.json), on the
    atomic and on the ordered route, none of the new entries among them; in deterministic mode the parameters afterwards are the parent's bits.
    On the atomic route the OUTPUTS are not compared: its float atomics give no run the same bits twice, the parent's included (the table's
    'atomic' digest is null); what holds there is the entry sequence, and the ordered route's bits stand for the arithmetic both share"""
    import json
    import os
    monkeypatch.delenv("NVSR_DETERMINISTIC", raising=False)
    monkeypatch.setenv("NVSR_OPS_DISPATCH", "0")
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "ray_grad_entry_table.json")) as f:
        table = json.load(f)
    for key, det in (("atomic", False), ("deterministic", True)):
        calls, digest = R.train_step_entries(hip, det)
        assert calls == table[key]["entries"], key
        assert not [c for c in calls if c in ("nvsr_rays_grad", "nvsr_pack_rays_backward", "nvsr_ndc_rays_backward", "nvsr_ray_bundle_backward")]
        if det:
            assert digest == table[key]["sha256"]


def test_every_training_route_keeps_its_recorded_entries(hip):
    """two TrainStep iterations on every host route of a training render (ray_grad_ref.TRAINING_CASES: planes only on two streams and on one,
    planes + decoder atomic and deterministic, decoder only, a fine pass that recomputes, a pose that requires a gradient in 'f16x2' in both
    modes, SR training where only the fine model super-resolves) make the calls tests/training_entry_table.json records (recorded by
    tools/training_entry_table.py at the parent of the change that last touched the route): per entry its name, every scalar argument, which
    pointer arguments are null, and the stream.  Where the route is reproducible the parameters afterwards have the recorded bits; a
    decoder-only step makes no more torch.zeros / zeros_like calls from train_utils and ops in its backward than recorded."""
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "training_entry_table.json")) as f:
        table = json.load(f)
    assert sorted(table) == sorted(R.TRAINING_CASES)
    for name, want in table.items():
        got = R.training_case(hip, name)
        got["entries"] = json.loads(json.dumps(got["entries"]))
        for i, (a, b) in enumerate(zip(got["entries"], want["entries"])):
            assert a == b, (name, i, a, b)
        assert len(got["entries"]) == len(want["entries"]), (name, got["entries"][len(want["entries"]):], want["entries"][len(got["entries"]):])
        assert got["sha256"] == want["sha256"], name
        assert (want["sha256"] is not None) == ("deterministic" in name)
        print("%s: %d entries, %d zero fills in the backward (recorded %d)" % (name, len(got["entries"]), got["zeros"], want["zeros"]))
        if name == "e_decoder_only":
            assert got["zeros"] <= want["zeros"], (got["zeros"], want["zeros"])


def test_five_adam_steps_refine_a_perturbed_pose(hip, monkeypatch):
    """TrainStep with a pose_target that requires a gradient, planes and decoder frozen: g27's camera rotated by 0.02 rad, the target rendered
    from the true one; five Adam steps on the pose: the rendering loss falls and the pose moves towards the true one"""
    monkeypatch.delenv("NVSR_DETERMINISTIC", raising=False)
    g, mc, mf, sid, focal, opts, scfg, _ = g27_models(hip, 0, "bf16x3", what=())
    opts.nerf.train.perturb, opts.nerf.train.radiance_field_noise_std = False, 0.0
    H, W = 12, 16
    focal *= 2
    true = T(g["c0_pose"])
    with torch.no_grad():
        ro, rd = hip.nerf_helpers.get_ray_bundle(H, W, focal, true)
        img = hip.train_utils.run_one_iter_of_nerf(H, W, focal, mc, mf, (ro, rd), opts, sid, mode="validation", scene_config=scfg)[3].reshape(H, W, 3)
    c, s = np.cos(0.02), np.sin(0.02)
    rot = T(np.array([[c, 0, s, 0], [0, 1, 0, 0], [-s, 0, c, 0], [0, 0, 0, 1]], f32))
    pose = (true @ rot).clone().requires_grad_(True)
    start = pose.detach().clone()
    opt = torch.optim.Adam([pose], lr=1e-3)
    # (sr_loss='fine': the loss is the fine pass's alone -- the target is the fine model's image, which the coarse decoder does not render)
    step = hip.training.TrainStep(mc, mf, opts, set(), pixel_sampler=hip.training.DevicePixelSampler(seed=5), sr_loss="fine")
    losses, dists = [], []
    for it in range(5):
        dists.append(float((pose.detach() - true).norm()))
        opt.zero_grad()
        m = step(it, img, pose, H, W, focal, 1, sid, scfg, H * W)
        assert pose.grad is not None and bool(torch.isfinite(pose.grad).all()) and float(pose.grad.abs().max()) > 0
        opt.step()
        losses.append(float(m["loss"]))                    # (rendering_loss_w = 1: the rendering loss)
    d0, d1 = float((start - true).norm()), float((pose.detach() - true).norm())
    print("rendering loss %s; |pose - true| %s -> %.5f" % (["%.3e" % v for v in losses], ["%.5f" % v for v in dists], d1))
    assert losses[-1] < losses[0] and d1 < d0


def _grad_models_on_bench_scene(hip):
    from bench import make_synthetic_scene, render_options
    mc, mf, sid, pose = make_synthetic_scene(DEV, plane_res=16, view_res=8, seed=2)
    for m in (mc, mf):
        for n, p in m.named_parameters():
            p.requires_grad_("rot_mats" not in n)
        m.train()
    opts, scfg = render_options(4, 4)
    H = W = 8
    focal = 0.5 * W / np.tan(0.5 * 0.6911112)
    return mc, mf, sid, pose, opts, scfg, H, W, focal


def test_limits_warn_once_or_raise(hip, monkeypatch):
    """'f32' and evaluation mode warn once per model and leave the gradient None; a pass too large for a forward record raises
    NotImplementedError before any launch of the render and names the ray count that fits; GraphedTrainStep refuses a pose that requires grad"""
    import warnings
    monkeypatch.delenv("NVSR_DETERMINISTIC", raising=False)
    mc, mf, sid, pose, opts, scfg, H, W, focal = _grad_models_on_bench_scene(hip)

    def render(mode="train"):
        p = pose.detach().clone().requires_grad_(True)
        ro, rd = hip.nerf_helpers.get_ray_bundle(H, W, focal, p)
        out = hip.train_utils.run_one_iter_of_nerf(H, W, focal, mc, mf, (ro.reshape(-1, 3), rd.reshape(-1, 3)), opts, sid, mode=mode, scene_config=scfg)
        if out[3].requires_grad:
            out[3].sum().backward()
        return p.grad

    assert render() is not None
    for why, setup in (("'f32' arithmetic", lambda: [setattr(m, "arithmetic", "f32") for m in (mc, mf)]), ("evaluation mode", lambda: None)):
        for m in (mc, mf):
            m.arithmetic = "bf16x3"
            m.__dict__.pop("_rays_grad_warned", None)
        setup()
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            for _ in range(2):
                assert render("validation" if why == "evaluation mode" else "train") is None
        assert len([w for w in seen if "rays require a gradient" in str(w.message) and why in str(w.message)]) == 1, [str(w.message) for w in seen]
    for m in (mc, mf):
        m.arithmetic = "bf16x3"
    monkeypatch.setattr(hip.train_utils, "RECORD_FORWARD_MAX_POINTS", 40 * 8 - 1)
    calls, real = [], hip.capi.call
    monkeypatch.setattr(hip.capi, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    with pytest.raises(NotImplementedError, match="at most 39 rays"):
        render()
    assert not [c for c in calls if "decode" in c or "render" in c or "coarse_z" in c], calls
    monkeypatch.setattr(hip.capi, "call", real)
    step = hip.training.TrainStep(mc, mf, opts, {"LR_planes"}, pixel_sampler=hip.training.DevicePixelSampler(seed=5))
    img = torch.rand(H, W, 3, device=DEV)
    with pytest.raises(ValueError, match="pose that requires a gradient"):
        hip.training.GraphedTrainStep(step, img, pose.detach().clone().requires_grad_(True), H, W, focal, 1, sid, scfg, 16)


def _warned_once(seen, why):
    hits = [str(w.message) for w in seen if "rays require a gradient" in str(w.message)]
    return len(hits) == 1 and why in hits[0]


def test_a_generic_geometry_warns_once_and_returns_no_ray_gradient(hip, monkeypatch):
    """a generic decoder geometry ('sum' instead of 'avg': the layered kernels) in a training render whose pose requires a gradient: the planes
    still get theirs, pose.grad and batch_rays.grad stay None, and the warning -- once per model, over two renders -- names the reason"""
    import warnings
    monkeypatch.delenv("NVSR_DETERMINISTIC", raising=False)
    g, mc, mf, sid, focal, opts, scfg, rnd = g27_models(hip, 0, None, what=("planes",), proj_combination="sum")
    assert not mc.is_native_geometry() and not mf.is_native_geometry()
    H, W = (int(v) for v in g["hw"])
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        for _ in range(2):
            mc.zero_grad(set_to_none=True)
            pose = T(g["c0_pose"]).requires_grad_(True)
            ro, rd = hip.nerf_helpers.get_ray_bundle(H, W, focal, pose)
            batch_rays = torch.stack([ro.reshape(-1, 3), rd.reshape(-1, 3)], 0)
            batch_rays.retain_grad()
            rnd48 = {k: v.repeat(2, 1) for k, v in rnd.items()}                  # (48 rays: the whole 6 x 8 grid)
            out = hip.train_utils.run_one_iter_of_nerf(H, W, focal, mc, mf, batch_rays, opts, sid, mode="train", scene_config=scfg, randoms=rnd48)
            assert out[3].requires_grad
            out[3].sum().backward()
            assert pose.grad is None and batch_rays.grad is None
            assert all(p.grad is not None and float(p.grad.abs().max()) > 0 for p in mc.planes_.values())
    assert _warned_once(seen, "a generic decoder geometry"), [str(w.message) for w in seen]


@pytest.mark.parametrize("encode", ["mip", "positional_encoding"])
def test_the_nerf_baselines_warn_once_and_return_no_ray_gradient(hip, encode):
    """FlexibleNeRFModel as the Mip-NeRF / the positional-encoding baseline in a training render whose pose requires a gradient, synthetic and
    NDC rays (the packer and the warp run as differentiable operators, the baseline detaches what they return): the models still get their
    gradients, pose.grad and batch_rays.grad stay None, and the warning -- once per model, over the renders -- names the baseline"""
    import warnings
    from types import SimpleNamespace as NS
    torch.manual_seed(5)
    kwargs, sid = (dict(include_input_xyz=False), "lego_DS8") if encode == "mip" else ({}, "lego")
    mc, mf = (hip.models.FlexibleNeRFModel(**kwargs).to(DEV).train() for _ in range(2))
    for m in (mc, mf):
        m.arithmetic = "bf16x3"
    mode = NS(chunksize=1024, perturb=False, num_coarse=4, num_fine=4, white_background=False, radiance_field_noise_std=0.0, lindisp=False)
    opts = NS(nerf=NS(use_viewdirs=True, encode_position_fn=encode, train=mode, validation=mode))
    H, W, focal = 4, 6, 5.0
    g = R.g27_case(0)[0]
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        for ci, ndc in ((0, False), (1, True)):
            for m in (mc, mf):
                m.zero_grad(set_to_none=True)
            pose = T(g["c%d_pose" % ci]).requires_grad_(True)
            ro, rd = hip.nerf_helpers.get_ray_bundle(H, W, focal, pose)
            batch_rays = torch.stack([ro.reshape(-1, 3), rd.reshape(-1, 3)], 0)
            batch_rays.retain_grad()
            scfg = {"near": 0.0 if ndc else 2.0, "far": 1.0 if ndc else 6.0, "no_ndc": not ndc}
            out = hip.train_utils.run_one_iter_of_nerf(H, W, focal, mc, mf, batch_rays, opts, sid, mode="train", scene_config=scfg)
            assert out[3].requires_grad and out[3].shape == (H * W, 3)
            (out[0].sum() + out[3].sum()).backward()
            assert pose.grad is None and batch_rays.grad is None
            # (the backward reached both models; an untrained baseline's densities may all be shut, so the values can be zero)
            assert all(any(p.grad is not None for p in m.parameters()) for m in (mc, mf))
    assert _warned_once(seen, "baseline"), [str(w.message) for w in seen]
