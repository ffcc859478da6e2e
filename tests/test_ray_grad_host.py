"""CPU tests of the ray and camera-pose gradients: the float64 formulas of tests/ray_grad_ref.py against torch float64 autograd of
plain-torch restatements, the identity behind the compositor term, fixture g27's two halves, the operators' argument validation, and the direct
host calls staying the direct calls."""
import inspect

import numpy as np
import pytest
import torch

import ray_grad_ref as R

f32, f64 = np.float32, np.float64


def t64(a, grad=False):
    return torch.tensor(np.asarray(a, f64), dtype=torch.float64, requires_grad=grad)


def close(a, b, tol=1e-12):
    a, b = np.asarray(a, f64), np.asarray(b, f64)
    return np.linalg.norm(a - b) <= tol * max(np.linalg.norm(b), 1e-300)


def composite_case(N=5, S=7, seed=0, zero_sigma_ray=True):
    rng = np.random.default_rng(seed)
    o, d = rng.standard_normal((N, 3)), rng.standard_normal((N, 3))
    z = np.sort(rng.uniform(2.0, 6.0, (N, S)), 1)
    raw = rng.standard_normal((N, S, 4))
    raw[1, ::2, 3] = -1.0                                  # sigma = 0 samples: relu shuts them
    if zero_sigma_ray:
        raw[2, :, 3] = -0.5                                # a ray with sigma = 0 everywhere
    noise = 0.2 * rng.standard_normal((N, S))
    noise[1, ::2] = 0.0                                    # (the noise must not reopen what the test shuts)
    if zero_sigma_ray:
        noise[2] = 0.0
    return o, d, z, raw, noise, rng.standard_normal((N, 3)), rng.standard_normal(N)


def test_compositor_term_is_sigma_dot_dsigma_over_norm():
    """d loss / d|rd| = sum_s sigma_s (d loss / d sigma_s) / |rd| through the compositor with dists * |rd|, the 1e10 last interval included, on
    rays with sigma = 0 samples and a ray with sigma = 0 everywhere; and the formula nvsr_rays_grad adds, T rd / (rd . rd), is d loss / d rd"""
    o, d, z, raw, noise, g_rgb, g_acc = composite_case()
    rd, raw_t = t64(d, True), t64(raw, True)
    rgb, acc = R.torch_composite_rgb(raw_t, t64(z), rd, t64(noise))
    ((rgb * t64(g_rgb)).sum() + (acc * t64(g_acc)).sum()).backward()
    sigma = np.maximum(raw[..., 3] + noise, 0.0)
    d_sigma = raw_t.grad[..., 3].numpy()                   # (d loss / d sigma where relu is open; where it is shut sigma = 0 multiplies it)
    T = (sigma * d_sigma).sum(1)
    norm = np.linalg.norm(d, axis=1)
    assert close((rd.grad.numpy() * d).sum(1) / norm, T / norm)                 # the directional derivative along rd / |rd|: d loss / d|rd|
    assert close(rd.grad.numpy(), T[:, None] * d / (d * d).sum(1)[:, None])
    assert T[2] == 0 and not rd.grad[2].any() and np.abs(T[[0, 1, 3, 4]]).min() > 0
    # ... which is what the float64 formula of nvsr_rays_grad returns when no point carries a gradient
    got = R.rays_grad(f64, np.concatenate([o, d, np.zeros((5, 5))], 1), z, None, None, raw, noise, raw_t.grad.numpy())
    assert close(got[:, 3:6], rd.grad.numpy()) and not got[:, :3].any() and not got[:, 6:].any()


def test_rays_grad_formula_is_autograd_of_points_and_compositor():
    """o + z d with z a constant, a per-point gradient and a per-ray view gradient, plus the compositor: the float64 formulas equal autograd"""
    o, d, z, raw, noise, g_rgb, g_acc = composite_case(seed=1, zero_sigma_ray=False)
    N, S = z.shape
    rng = np.random.default_rng(5)
    w_pts, w_view = rng.standard_normal((N, S, 3)), rng.standard_normal((N, 3))
    rays = t64(np.concatenate([o, d, np.zeros((N, 2)), rng.standard_normal((N, 3))], 1), True)
    raw_t = t64(raw, True)
    pts = rays[:, None, 0:3] + rays[:, None, 3:6] * t64(z)[..., None]
    rgb, acc = R.torch_composite_rgb(raw_t, t64(z), rays[:, 3:6], t64(noise))
    loss = (torch.sin(pts) * t64(w_pts)).sum() + (rays[:, 8:11] * t64(w_view)).sum() + (rgb * t64(g_rgb)).sum() + (acc * t64(g_acc)).sum()
    loss.backward()
    d_points = (np.cos(pts.detach().numpy()) * w_pts).reshape(N * S, 3)
    coarse = R.rays_grad(f64, rays.detach().numpy(), z, d_points, w_view, raw, noise, raw_t.grad.numpy())
    assert close(coarse, rays.grad.numpy())
    # a second pass accumulates
    twice = R.rays_grad(f64, rays.detach().numpy(), z, d_points, w_view, raw, noise, raw_t.grad.numpy(), True, coarse)
    assert close(twice[:, [0, 1, 2, 3, 4, 5, 8, 9, 10]], 2 * coarse[:, [0, 1, 2, 3, 4, 5, 8, 9, 10]]) and not twice[:, 6:8].any()


def test_pack_ndc_and_bundle_formulas_are_autograd():
    rng = np.random.default_rng(2)
    N = 9
    # v / |v|
    v, g = rng.standard_normal((N, 3)), rng.standard_normal((N, 11))
    vt = t64(v, True)
    ((vt / vt.norm(dim=-1, keepdim=True)) * t64(g[:, 8:11])).sum().backward()
    d_ro, d_rd, d_vs = R.pack_rays_backward(f64, g, v, False)
    assert close(d_vs, vt.grad.numpy()) and np.array_equal(d_ro, g[:, 0:3]) and np.array_equal(d_rd, g[:, 3:6])
    assert close(R.pack_rays_backward(f64, g, v, True)[1], g[:, 3:6] + vt.grad.numpy())
    # the NDC warp
    H, W, focal, near = 12, 16, 14.0, 1.0
    ro, rd = 0.1 * rng.standard_normal((N, 3)), rng.standard_normal((N, 3))
    rd[:, 2] = -1.0 - np.abs(rd[:, 2])
    go, gd = rng.standard_normal((N, 3)), rng.standard_normal((N, 3))
    ro_t, rd_t = t64(ro, True), t64(rd, True)
    o2, d2 = R.torch_ndc_rays(H, W, focal, near, ro_t, rd_t)
    assert close(o2.detach().numpy(), R.ndc_rays(f64, H, W, focal, near, ro, rd)[0]) and close(d2.detach().numpy(), R.ndc_rays(f64, H, W, focal, near, ro, rd)[1])
    ((o2 * t64(go)).sum() + (d2 * t64(gd)).sum()).backward()
    got = R.ndc_rays_backward(f64, H, W, focal, near, ro, rd, go, gd)
    assert close(got[0], ro_t.grad.numpy()) and close(got[1], rd_t.grad.numpy())
    # the ray generator: full padded grid, selected pixels with repeats
    for rc, pad in ((None, 0), (None, 2), (np.stack([rng.integers(-1, 7, 300), rng.integers(-1, 9, 300)], 1), 0)):
        Hh, Ww = 5, 7
        n = (Hh + 2 * pad) * (Ww + 2 * pad) if rc is None else rc.shape[0]
        c2w = t64(rng.standard_normal((4, 4)), True)
        g_o, g_d = rng.standard_normal((n, 3)), rng.standard_normal((n, 3))
        o3, d3 = R.torch_ray_bundle(Hh, Ww, 9.5, 9.25, c2w, 0.4375, rc, pad)
        ((o3 * t64(g_o)).sum() + (d3 * t64(g_d)).sum()).backward()
        got = R.ray_bundle_backward(f64, Hh, Ww, 9.5, 9.25, 0.4375, g_o, g_d, rc, pad)
        assert close(got, c2w.grad.numpy()) and not got[3].any()


def test_fixture_halves_agree():
    """g27: upstream's float32 and float64 runs agree (their relative L2 is the scale of the end-to-end bound: 8 x it, or 2e-4 if larger)"""
    for ci in (0, 1):
        g, dec, planes = R.g27_case(ci)
        pre = "c%d_" % ci
        for k in ("rays_grad", "pose_grad"):
            a, b = g[pre + k], g[pre + k + "64"]
            rel = np.linalg.norm(a - b) / np.linalg.norm(b)
            print("g27 case %d %s: float32 vs float64 relative L2 %.3g" % (ci, k, rel))
            assert rel < 2.5e-5 and np.abs(b).max() > 1e-3            # (8 x it stays below the 2e-4 floor)
        for d in range(4):
            a, b = g[pre + "grad_plane%d" % d], g[pre + "grad64_plane%d" % d]
            assert np.linalg.norm(a - b) <= 1e-4 * np.linalg.norm(b)
        z, z64 = g[pre + "z_fine"], g[pre + "z_fine64"]
        assert (np.abs(z - z64) <= 1e-5 * np.abs(z64)).all()          # no importance bin flipped between the two runs
        assert not g[pre + "pose_grad64"][3].any() and g[pre + "rays_grad64"].shape == (2, 24, 3)
        assert len(set(g[pre + "sel"].tolist())) < 24                 # pixels drawn more than once
        assert dec["coarse.fc_alpha.0.weight"].shape == (1, 128)


def test_operators_validate_their_arguments():
    import nvsr_amd  # noqa: F401  (registers torch.ops.nvsr)
    nv = torch.ops.nvsr
    for name in ("rays_grad", "pack_rays_backward", "ndc_rays_backward", "ray_bundle_backward", "ray_bundle", "ray_bundle_at", "ndc_rays", "pack_rays"):
        assert hasattr(nv, name), name
        assert "nvsr_" + {"ray_bundle": "get_ray_bundle", "ray_bundle_at": "get_ray_bundle_at"}.get(name, name) in nvsr_amd.capi.exported_symbols()
    ops = nvsr_amd.ops
    z = torch.zeros
    with pytest.raises(nvsr_amd.capi.NvsrError, match="GPU only"):
        ops.direct.rays_grad(z(2, 11), z(2, 3), None, None, z(2, 3, 4), None, z(2, 3, 4), z(2, 11), False)
    with pytest.raises(ValueError, match=r"z is \[N,S >= 1\]"):
        ops.direct.rays_grad(z(2, 11), z(2, 0), None, None, z(2, 0, 4), None, z(2, 0, 4), z(2, 11), False)
    with pytest.raises(ValueError, match="d_ro is"):
        ops.direct.ray_bundle_backward(4, 4, 1.0, 1.0, 0.0, None, 0, z(3), z(3))
    with pytest.raises(ValueError, match="d_rays is"):
        ops.direct.pack_rays_backward(z(11), z(3), True)
    with pytest.raises(ValueError, match="ro is"):
        ops.direct.ndc_rays_backward(4, 4, 1.0, 1.0, z(3), z(3), z(3), z(3))
    # shapes through the fake implementations (no GPU): what a traced graph sees
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        e = lambda *s: torch.empty(s, device="cuda")
        assert [tuple(t.shape) for t in nv.pack_rays_backward(e(5, 11), e(5, 3), True)] == [(5, 3), (5, 3), (0,)]
        assert [tuple(t.shape) for t in nv.pack_rays_backward(e(5, 11), e(5, 3), False)] == [(5, 3), (5, 3), (5, 3)]
        assert [tuple(t.shape) for t in nv.ndc_rays_backward(4, 4, 1.0, 1.0, e(5, 3), e(5, 3), e(5, 3), e(5, 3))] == [(5, 3), (5, 3)]
        assert tuple(nv.ray_bundle_backward(4, 4, 1.0, 1.0, 0.0, None, 0, e(16, 3), e(16, 3)).shape) == (4, 4)
        assert [tuple(t.shape) for t in nv.ray_bundle(4, 6, 1.0, 1.0, e(4, 4), 1, 0.0)] == [(6, 8, 3), (6, 8, 3)]
        assert tuple(nv.pack_rays(e(5, 3), e(5, 3), None, 2.0, 6.0).shape) == (5, 11)
        assert nv.rays_grad(e(2, 11), e(2, 3), None, None, e(2, 3, 4), None, e(2, 3, 4), e(2, 11), False) is None


def test_direct_host_calls_are_still_the_direct_calls():
    """nothing that requires a gradient: get_ray_bundle, ndc_rays, get_ray_bundle_at and pack_rays reach the C entry they reached before, with the
    arguments they passed before, and never the new operators (the source of each function: the differentiable branch sits behind a
    requires_grad test, the rest of the body is the parent's)"""
    import nvsr_amd
    calls = []

    class Stop(Exception):
        pass

    def spy(name, *a):
        calls.append((name, len(a)))
        raise Stop()

    real, real_req, real_stream = nvsr_amd.capi.call, nvsr_amd.capi.require_cuda, nvsr_amd.capi.stream
    nvsr_amd.capi.call, nvsr_amd.capi.require_cuda, nvsr_amd.capi.stream = spy, lambda *t: None, lambda: None
    try:
        pose = torch.eye(4)
        o, d = torch.zeros(6, 3), torch.ones(6, 3)
        rc = torch.zeros(6, 2, dtype=torch.int32)
        for fn, want in ((lambda: nvsr_amd.nerf_helpers.get_ray_bundle(2, 3, 1.5, pose), ("nvsr_get_ray_bundle", 10)),
                         (lambda: nvsr_amd.nerf_helpers.ndc_rays(2, 3, 1.5, 1.0, o, d), ("nvsr_ndc_rays", 10)),
                         (lambda: nvsr_amd.training.get_ray_bundle_at(2, 3, 1.5, pose, rc), ("nvsr_get_ray_bundle_at", 11)),
                         (lambda: nvsr_amd.train_utils.pack_rays(o, d, 2.0, 6.0), ("nvsr_pack_rays", 8))):
            calls.clear()
            with pytest.raises(Stop):
                fn()
            assert calls == [want]
    finally:
        nvsr_amd.capi.call, nvsr_amd.capi.require_cuda, nvsr_amd.capi.stream = real, real_req, real_stream
    for fn in (nvsr_amd.nerf_helpers.get_ray_bundle, nvsr_amd.nerf_helpers.ndc_rays, nvsr_amd.training.get_ray_bundle_at, nvsr_amd.train_utils.pack_rays):
        src = inspect.getsource(fn)
        assert src.count("requires_grad") >= 1 and src.count("torch.ops.nvsr.") == 1
