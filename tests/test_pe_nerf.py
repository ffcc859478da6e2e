"""GPU tests of the positional-encoding NeRF baseline (MipNeRF_baseline.yml with encode_position_fn: positional_encoding; csrc/pe.hip) against
g24_pe_nerf.npz (the upstream code on the CPU, tests/golden/gen_golden_pe.py), for both arithmetics of the model kernels.

Tolerances (those of tests/test_mip_nerf.py)
  encoding .............. the 3 point columns bit for bit (ro + rd z in two f32 roundings, as the reference); sin / cos and direction columns
                          |err| <= 2e-6 (2^l x is exact, so only the sin / cos of the two libraries differ)
  model forward ......... f32 |err| <= 1e-5; bf16x3: + 1e-6 x the float64 sum of |W||x| + |b| over the layers (limb_core.h)
  renders ............... coarse |err| <= 3e-5; fine >= 95 % of rays within 2e-4 and PSNR >= 70 dB (importance bins may flip)
  parameter gradients ... coarse model relative L2 < 1e-4 and max <= 1e-4 max|ref|; fine model 1e-2 and 3e-2 max|ref| (at pe_params.kept_elements;
                          every element of every gradient is checked against float64 in test_at_size_against_float64)
  parameters after Adam . the same relative L2 bounds; per element <= 1e-3 max|ref|
"""
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden
from nerf_baseline_checks import DEV, N_, T, chain_abs_sum, check_grads, check_render, cpu_eval, scene
import nerf_baseline_checks as checks

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import pe_params  # noqa: E402

pytestmark = pytest.mark.gpu
ARITHS = ["f32", "bf16x3"]


@pytest.fixture(scope="module")
def g24():
    return load_golden("g24_pe_nerf.npz")


def models_from(hip, g, arith):
    return checks.models_from(hip, g, arith, pe_params)


def opts(**kw):
    return checks.opts("positional_encoding", **kw)


def run(hip, g, mc, mf, o, mode, ndc=False, randoms=None):
    H, W, focal = g["c.hwf"]
    rays = torch.stack((T(g["c.ro"]).reshape(-1, 3), T(g["c.rd"]).reshape(-1, 3)))
    return hip.train_utils.run_one_iter_of_nerf(int(H), int(W), float(focal), mc, mf, rays, o, str(g["scene_id"]), mode=mode,
                                                scene_config=scene(ndc), randoms=randoms)


@pytest.mark.parametrize("tag", ["a.", "a.ndc."])
def test_pe_encode_matches_upstream(hip, g24, tag):
    g = g24
    out = N_(torch.ops.nvsr.pe_encode(T(g[tag + "rays"]), T(g[tag + "z"])))
    assert out.shape == (g[tag + "enc"].shape[0], 66)
    np.testing.assert_array_equal(out[:, :3], g[tag + "enc"][:, :3])              # the points, bit for bit
    err = np.abs(out[:, 3:39] - g[tag + "enc"][:, 3:])
    assert err.max() <= 2e-6, "encoding max|err| %.2e (column %d)" % (err.max(), 3 + int(err.max(0).argmax()))
    np.testing.assert_allclose(out[:, 39:], g[tag + "dirs"], rtol=0, atol=2e-6)


@pytest.mark.parametrize("arith", ARITHS)
def test_fused_forward_matches_upstream_model(hip, g24, arith):
    g = g24
    for tag, key in (("a.", "raw"), ("a.ndc.", "ndc.raw")):
        n, S = g[tag + "z"].shape
        x = np.concatenate([g[tag + "enc"], g[tag + "dirs"]], -1)
        for i, m in enumerate(models_from(hip, g, arith)):
            with torch.no_grad():
                raw = N_(m.pe_forward(T(g[tag + "rays"]), T(g[tag + "z"]))).reshape(n * S, 4)
            tol = 1e-5 if arith == "f32" else 1e-5 + 1e-6 * chain_abs_sum(pe_params.state_dict(pe_params.SEEDS[i]), x, 39)
            err = np.abs(raw - g["b.m%d.%s" % (i, key)]).max()
            assert err <= tol, "%s model %d (%s): max|err| %.2e > %.2e" % (tag, i, arith, err, tol)
    # model(x) on already-encoded rows still runs the scalar kernel with its own values
    m = models_from(hip, g, arith)[0]
    x = T(np.concatenate([g["a.enc"], g["a.dirs"]], -1))
    np.testing.assert_allclose(N_(m(x)), g["b.m0.raw"], rtol=0, atol=1e-5)


@pytest.mark.parametrize("arith", ARITHS)
def test_validation_render_matches_upstream(hip, g24, arith):
    g = g24
    mc, mf = models_from(hip, g, arith)
    for tag, ndc in (("c.", False), ("c.ndc.", True)):
        with torch.no_grad():
            out = run(hip, g, mc, mf, opts(), "validation", ndc=ndc)
        assert len(out) == 9 and out[6] is None
        check_render(out, g, tag)
    # eval_nerf takes the same route
    H, W, focal = g["c.hwf"]
    with torch.no_grad():
        ev = hip.train_utils.eval_nerf(int(H), int(W), float(focal), mc, mf, T(g["c.ro"]), T(g["c.rd"]), opts(), str(g["scene_id"]),
                                       scene_config=scene(False))
    assert ev[0].shape == ev[3].shape == (int(H), int(W), 3)
    assert np.abs(N_(ev[0]).reshape(-1, 3) - g["c.rgb_coarse"]).max() <= 3e-5
    assert (np.abs(N_(ev[3]).reshape(-1, 3) - g["c.rgb_fine"]).max(-1) <= 2e-4).mean() >= 0.95


@pytest.mark.parametrize("arith", ARITHS)
def test_train_step_outputs_and_gradients_match_upstream(hip, g24, arith):
    g = g24
    mc, mf = models_from(hip, g, arith)
    torch.manual_seed(24)
    out = run(hip, g, mc, mf, opts(perturb=True, noise=0.2, chunk=100), "train")
    target = T(g["d.target"])
    loss = torch.nn.functional.mse_loss(out[0], target) + torch.nn.functional.mse_loss(out[3], target)
    loss.backward()
    check_render(out, g, "d.")
    check_grads((mc, mf), g, "d")


@pytest.mark.parametrize("arith", ARITHS)
def test_backward_is_deterministic(hip, g24, arith):
    g = g24
    grads = []
    for _ in range(2):
        mc, mf = models_from(hip, g, arith)
        torch.manual_seed(24)
        out = run(hip, g, mc, mf, opts(perturb=True, noise=0.2, chunk=100), "train")
        (out[0].square().mean() + out[3].square().mean()).backward()
        grads.append([p.grad.clone() for m in (mc, mf) for p in m.parameters()])
    for a, b in zip(*grads):
        assert torch.equal(a, b)


@pytest.mark.parametrize("arith", ARITHS)
def test_three_adam_steps_match_upstream(hip, g24, arith):
    g = g24
    mc, mf = models_from(hip, g, arith)
    target = T(g["d.target"])
    opt = torch.optim.Adam(list(mc.parameters()) + list(mf.parameters()), lr=1e-3)
    torch.manual_seed(31)
    losses = []
    for _ in range(3):
        opt.zero_grad()
        out = run(hip, g, mc, mf, opts(perturb=True, noise=0.2, chunk=100), "train")
        loss = torch.nn.functional.mse_loss(out[0], target) + torch.nn.functional.mse_loss(out[3], target)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    np.testing.assert_allclose(losses, g["e.losses"], rtol=1e-5)
    check_grads((mc, mf), g, "")


@pytest.mark.parametrize("arith", ARITHS)
def test_at_size_against_float64(hip, arith):
    """4096 rays x (64 + 64) depths: forward and every parameter gradient against a float64 CPU evaluation of the same model on the kernel's
    own encoder output (nvsr_pe_encode on the same depths); the relative error per layer is reported"""
    torch.manual_seed(4)
    m = hip.models.FlexibleNeRFModel().to(DEV)
    m.arithmetic = arith
    N, S = 4096, 128
    ro = torch.randn(N, 3, device=DEV)
    rd = torch.randn(N, 3, device=DEV)
    rays = hip.train_utils.pack_rays(ro, rd, 2.0, 6.0)
    z = torch.sort(2.0 + 4.0 * torch.rand(N, S, device=DEV), -1)[0]
    raw = m.pe_forward(rays, z)
    g_raw = torch.randn_like(raw)
    (raw * g_raw).sum().backward()
    x = torch.ops.nvsr.pe_encode(rays, z).cpu().double()
    gr = g_raw.reshape(-1, 4).cpu().double()
    out64, g64 = cpu_eval(m, x, gr, 39, torch.float64)
    _, g32 = cpu_eval(m, x, gr, 39, torch.float32)     # the reference's own arithmetic: the scale of the summation error over 524 288 points
    e_fwd = float((raw.detach().reshape(-1, 4).cpu().double() - out64).abs().max())
    report = ["forward max|err| %.2e" % e_fwd]
    assert e_fwd <= (1e-5 if arith == "f32" else 1e-4), report
    for k, p in m.named_parameters():
        rel = float((p.grad.cpu().double() - g64[k]).norm() / g64[k].norm().clamp_min(1e-30))
        rel32 = float((g32[k] - g64[k]).norm() / g64[k].norm().clamp_min(1e-30))
        report.append("%s %.2e (torch f32 %.2e)" % (k, rel, rel32))
        # (as tests/test_mip_nerf.py: ReLU gates that flip between f32 and f64 dominate both; the floor is the f32 summation error of a
        #  524 288-point sum, sqrt(P) 2^-24, and for bf16x3 the limbs' 2^-20 per product through the chain)
        assert rel <= 4 * rel32 + (np.sqrt(N * S) * 2.0 ** -24 if arith == "f32" else 2e-3), report
    print("pe at size (%s): " % arith + ", ".join(report))


def test_opcheck_pe_operators(hip, g24):
    g = g24
    nv = torch.ops.nvsr
    rays, z = T(g["a.rays"][:4]), T(g["a.z"][:4])
    m = models_from(hip, g, "f32")[0]
    nat = m.natural_blob()
    chk = lambda op, args: torch.library.opcheck(op, args, test_utils=("test_schema", "test_faketensor"))
    chk(nv.pe_encode, (rays, z))
    for arith in (0, 3):
        chk(nv.pe_nerf, (rays, z, nat, True, arith))
        raw, rec = nv.pe_nerf(rays, z, nat, True, arith)
        grec = nv.pe_nerf_backward(nat, rec, torch.ones_like(raw), arith)
        chk(nv.pe_nerf_backward, (nat, rec, torch.ones_like(raw), arith))
        chk(nv.pe_nerf_weight_grad, (rec, grec))
    torch.library.opcheck(nv.pe_nerf, (rays, z, nat.clone().requires_grad_(True), True, 0),
                          test_utils=("test_schema", "test_autograd_registration", "test_faketensor"))
