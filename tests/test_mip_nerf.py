"""GPU tests of the Mip-NeRF baseline (MipNeRF_baseline.yml; csrc/mip.hip) against g23_mip_nerf.npz (the upstream code on the CPU,
tests/golden/gen_golden_mip.py), for both arithmetics of the model kernels.

Tolerances
  encoding .............. degree 0-3 and direction columns |err| <= 2e-6; degrees 4-5: + 4 ulp(|mean|) 2^l (the argument is the mean scaled by
                          2^l: a rounding of the mean that differs by an ulp moves it by 2^l ulp, sin' <= 1)
  model forward ......... f32 |err| <= 1e-5 (as g10); bf16x3: + 2^-20 sum|W||x| through the chain (limb_core.h: <= 2^-21 + 2^-30 per product,
                          measured 9.8e-7 of sum|W||x|), bounded here by 1e-6 x the float64 sum of |W||x| + |b| over the layers
  renders ............... coarse |err| <= 3e-5; fine >= 95 % of rays within 2e-4 and PSNR >= 70 dB (importance bins may flip)
  parameter gradients ... (g23 keeps every element of the small tensors, a fixed 1 024 of the larger ones: tests/golden/mip_params.py; every element
                          of every gradient is checked against float64 in test_at_size_against_float64) as g13: coarse model relative L2 < 1e-4 and max <= 1e-4 max|ref|; fine model 1e-2 and 3e-2 max|ref|
  parameters after Adam . the same relative L2 bounds; per element <= 1e-3 max|ref| (check_grads: Adam's step does not shrink with the gradient)
"""
import sys
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden
from nerf_baseline_checks import DEV, N_, T, chain_abs_sum, check_grads, check_render, cpu_eval, scene
import nerf_baseline_checks as checks

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import mip_params  # noqa: E402

pytestmark = pytest.mark.gpu
ARITHS = ["f32", "bf16x3"]


@pytest.fixture(scope="module")
def g23():
    return load_golden("g23_mip_nerf.npz")


def models_from(hip, g, arith):
    return checks.models_from(hip, g, arith, mip_params, include_input_xyz=False)


def opts(**kw):
    return checks.opts("mip", **kw)


def run(hip, g, mc, mf, o, mode, ndc=False, randoms=None):
    H, W, focal = g["c.hwf"]
    rays = torch.stack((T(g["c.ro"]).reshape(-1, 3), T(g["c.rd"]).reshape(-1, 3)))
    return hip.train_utils.run_one_iter_of_nerf(int(H), int(W), float(focal), mc, mf, rays, o, "lego_DS8", mode=mode, scene_config=scene(ndc),
                                                randoms=randoms)


def test_mip_encode_matches_upstream(hip, g23):
    g = g23
    out = N_(torch.ops.nvsr.mip_encode(T(g["a.rays"]), T(g["a.edges"]), float(g["radius"])))
    ipe, dirs = out[:, :36], out[:, 36:]
    np.testing.assert_allclose(dirs, g["a.dirs"], rtol=0, atol=2e-6)
    mean = np.abs(g["a.means"]).reshape(-1, 1, 3)                                  # [P, 1, axis]
    l = np.arange(6).reshape(1, 6, 1)
    tol = 2e-6 + np.where(l >= 4, 4 * np.spacing(mean.astype(np.float32)) * 2.0 ** l, 0.0)
    tol = np.concatenate([tol.reshape(-1, 18)] * 2, -1)
    err = np.abs(ipe - g["a.ipe"])
    assert (err <= tol).all(), "IPE max|err| %.2e (column %d)" % (err.max(), int(err.max(0).argmax()))
    assert np.abs(g["a.means"]).max() * 32 > 100


@pytest.mark.parametrize("arith", ARITHS)
def test_fused_forward_matches_upstream_model(hip, g23, arith):
    g = g23
    n, S = g["a.edges"].shape[0], g["a.edges"].shape[1] - 1
    for i, m in enumerate(models_from(hip, g, arith)):
        with torch.no_grad():
            raw = N_(m.mip_forward(T(g["a.rays"]), T(g["a.edges"]), float(g["radius"]))).reshape(n * S, 4)
        tol = 1e-5 if arith == "f32" else 1e-5 + 1e-6 * chain_abs_sum(mip_params.state_dict(mip_params.SEEDS[i]), np.concatenate([g["a.ipe"], g["a.dirs"]], -1), 36)
        err = np.abs(raw - g["b.m%d.raw" % i]).max()
        assert err <= tol, "model %d (%s): max|err| %.2e > %.2e" % (i, arith, err, tol)
    # model(x) on already-encoded rows still runs the scalar kernel with its own values
    m = models_from(hip, g, arith)[0]
    x = T(np.concatenate([g["a.ipe"], g["a.dirs"]], -1))
    np.testing.assert_allclose(N_(m(x)), g["b.m0.raw"], rtol=0, atol=1e-5)


@pytest.mark.parametrize("arith", ARITHS)
def test_validation_render_matches_upstream(hip, g23, arith):
    g = g23
    mc, mf = models_from(hip, g, arith)
    for tag, ndc in (("c.", False), ("c.ndc.", True)):
        with torch.no_grad():
            out = run(hip, g, mc, mf, opts(), "validation", ndc=ndc)
        assert len(out) == 9 and out[6] is None
        check_render(out, g, tag)


@pytest.mark.parametrize("arith", ARITHS)
def test_train_step_outputs_and_gradients_match_upstream(hip, g23, arith):
    g = g23
    mc, mf = models_from(hip, g, arith)
    torch.manual_seed(23)
    out = run(hip, g, mc, mf, opts(perturb=True, noise=0.2, chunk=400), "train")
    target = T(g["d.target"])
    loss = torch.nn.functional.mse_loss(out[0], target) + torch.nn.functional.mse_loss(out[3], target)
    loss.backward()
    check_render(out, g, "d.")
    check_grads((mc, mf), g, "d")


@pytest.mark.parametrize("arith", ARITHS)
def test_backward_is_deterministic(hip, g23, arith):
    g = g23
    grads = []
    for _ in range(2):
        mc, mf = models_from(hip, g, arith)
        torch.manual_seed(23)
        out = run(hip, g, mc, mf, opts(perturb=True, noise=0.2, chunk=400), "train")
        (out[0].square().mean() + out[3].square().mean()).backward()
        grads.append([p.grad.clone() for m in (mc, mf) for p in m.parameters()])
    for a, b in zip(*grads):
        assert torch.equal(a, b)


@pytest.mark.parametrize("arith", ARITHS)
def test_three_adam_steps_match_upstream(hip, g23, arith):
    g = g23
    mc, mf = models_from(hip, g, arith)
    target = T(g["d.target"])
    opt = torch.optim.Adam(list(mc.parameters()) + list(mf.parameters()), lr=1e-3)
    torch.manual_seed(29)
    losses = []
    for _ in range(3):
        opt.zero_grad()
        out = run(hip, g, mc, mf, opts(perturb=True, noise=0.2, chunk=400), "train")
        loss = torch.nn.functional.mse_loss(out[0], target) + torch.nn.functional.mse_loss(out[3], target)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    np.testing.assert_allclose(losses, g["e.losses"], rtol=1e-5)
    check_grads((mc, mf), g, "")


@pytest.mark.parametrize("arith", ARITHS)
def test_at_size_against_float64(hip, arith):
    """4096 rays x (64 + 64) intervals: forward and every parameter gradient against a float64 CPU evaluation of the same model on the kernel's
    own encoder output (nvsr_mip_encode on the same edges); the relative error per layer is reported"""
    torch.manual_seed(3)
    m = hip.models.FlexibleNeRFModel(include_input_xyz=False).to(DEV)
    m.arithmetic = arith
    N, S = 4096, 128
    ro = torch.randn(N, 3, device=DEV)
    rd = torch.randn(N, 3, device=DEV)
    rays = hip.train_utils.pack_rays(ro, rd, 2.0, 6.0)
    edges = torch.sort(2.0 + 4.0 * torch.rand(N, S + 1, device=DEV), -1)[0]
    radius = hip.train_utils.mip_radius("lego_DS8")
    raw = m.mip_forward(rays, edges, radius)
    g_raw = torch.randn_like(raw)
    (raw * g_raw).sum().backward()
    x = torch.ops.nvsr.mip_encode(rays, edges, radius).cpu().double()
    gr = g_raw.reshape(-1, 4).cpu().double()
    out64, g64 = cpu_eval(m, x, gr, 36, torch.float64)
    _, g32 = cpu_eval(m, x, gr, 36, torch.float32)     # the reference's own arithmetic: the scale of the summation error over 524 288 points
    e_fwd = float((raw.detach().reshape(-1, 4).cpu().double() - out64).abs().max())
    report = ["forward max|err| %.2e" % e_fwd]
    assert e_fwd <= (1e-5 if arith == "f32" else 1e-4), report
    for k, p in m.named_parameters():
        rel = float((p.grad.cpu().double() - g64[k]).norm() / g64[k].norm().clamp_min(1e-30))
        rel32 = float((g32[k] - g64[k]).norm() / g64[k].norm().clamp_min(1e-30))
        report.append("%s %.2e (torch f32 %.2e)" % (k, rel, rel32))
        # (ReLU gates that flip between f32 and f64 dominate both; the floor is the f32 summation error of a 524 288-point sum, sqrt(P) 2^-24,
        #  and for bf16x3 the limbs' 2^-20 per product through the chain, measured below 1.1e-3)
        assert rel <= 4 * rel32 + (np.sqrt(N * S) * 2.0 ** -24 if arith == "f32" else 2e-3), report
    print("mip at size (%s): " % arith + ", ".join(report))


@pytest.fixture(scope="module")
def fine_pass_at_size(hip):
    """the Mip fine pass of a training step at 4096 rays: Nc + Nf + 1 = 129 intervals per ray, P = 528 384 points = 64.5 slabs of the weight
    gradient.  The model, its inputs, dL/draw and their float64 evaluation, which does not depend on the arithmetic (computed once, on the
    device: rocBLAS DGEMM, not the kernels under test); the torch f32 evaluation on the CPU, as in test_at_size_against_float64"""
    torch.manual_seed(7)
    m = hip.models.FlexibleNeRFModel(include_input_xyz=False).to(DEV)
    N, S = 4096, 129
    rays = hip.train_utils.pack_rays(torch.randn(N, 3, device=DEV), torch.randn(N, 3, device=DEV), 2.0, 6.0)
    edges = torch.sort(2.0 + 4.0 * torch.rand(N, S + 1, device=DEV), -1)[0]
    radius = hip.train_utils.mip_radius("lego_DS8")
    g_raw = torch.randn(N, S, 4, device=DEV)
    x = torch.ops.nvsr.mip_encode(rays, edges, radius).double()
    gr = g_raw.reshape(-1, 4).double()
    out64, g64 = cpu_eval(m, x, gr, 36, torch.float64, device=DEV)
    _, g32 = cpu_eval(m, x.cpu(), gr.cpu(), 36, torch.float32)
    rel32 = {k: float((g32[k] - g64[k].cpu()).norm() / g64[k].norm().clamp_min(1e-30)) for k in g64}
    return NS(state={k: v.detach().clone() for k, v in m.state_dict().items()}, N=N, S=S, rays=rays, edges=edges, radius=radius, g_raw=g_raw,
              out64=out64, g64=g64, rel32=rel32)


@pytest.mark.parametrize("arith", ARITHS + ["f16x2"])
def test_fine_pass_shape_against_float64(hip, fine_pass_at_size, arith):
    """4096 rays x 129 intervals, the shape of the fine pass of every Mip training step (P is not a whole number of weight-gradient slabs):
    forward and every parameter gradient of mip_forward + autograd against float64, with the tolerances of test_at_size_against_float64
    (for f16x2 those of test_f16x2_at_size_against_float64, the same)"""
    f = fine_pass_at_size
    m = hip.models.FlexibleNeRFModel(include_input_xyz=False).to(DEV)
    m.load_state_dict(f.state)
    m.arithmetic = arith
    raw = m.mip_forward(f.rays, f.edges, f.radius)
    (raw * f.g_raw).sum().backward()
    e_fwd = float((raw.detach().reshape(-1, 4).double() - f.out64).abs().max())
    report = ["forward max|err| %.2e" % e_fwd]
    assert e_fwd <= (1e-5 if arith == "f32" else 1e-4), report
    for k, p in m.named_parameters():
        rel = float((p.grad.double() - f.g64[k]).norm() / f.g64[k].norm().clamp_min(1e-30))
        report.append("%s %.2e (torch f32 %.2e)" % (k, rel, f.rel32[k]))
        assert rel <= 4 * f.rel32[k] + (np.sqrt(f.N * f.S) * 2.0 ** -24 if arith == "f32" else 2e-3), report
    print("mip fine pass at size (%s): " % arith + ", ".join(report))


def test_opcheck_mip_operators(hip, g23):
    g = g23
    nv = torch.ops.nvsr
    rays, edges, r = T(g["a.rays"][:4]), T(g["a.edges"][:4]), float(g["radius"])
    m = models_from(hip, g, "f32")[0]
    nat = m.natural_blob()
    chk = lambda op, args: torch.library.opcheck(op, args, test_utils=("test_schema", "test_faketensor"))
    chk(nv.mip_encode, (rays, edges, r))
    for arith in (0, 3):
        chk(nv.mip_nerf, (rays, edges, r, nat, True, arith))
        raw, rec = nv.mip_nerf(rays, edges, r, nat, True, arith)
        grec = nv.mip_nerf_backward(nat, rec, torch.ones_like(raw), arith)
        chk(nv.mip_nerf_backward, (nat, rec, torch.ones_like(raw), arith))
        chk(nv.mip_nerf_weight_grad, (rec, grec))
    torch.library.opcheck(nv.mip_nerf, (rays, edges, r, nat.clone().requires_grad_(True), True, 0),
                          test_utils=("test_schema", "test_autograd_registration", "test_faketensor"))
