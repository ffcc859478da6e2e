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
import copy
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import mip_params  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ARITHS = ["f32", "bf16x3"]


def T(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def N_(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def g23():
    return load_golden("g23_mip_nerf.npz")


def models_from(hip, g, arith):
    """the two g23 models (coarse, fine): parameters from mip_params, checked against the fixture's checksums"""
    ms = []
    for i, seed in enumerate((101, 202)):
        sd = mip_params.state_dict(seed)
        flat = np.concatenate([v.reshape(-1).astype(np.float64) for v in sd.values()])
        np.testing.assert_allclose([flat.sum(), (flat * flat).sum()], g["b.m%d.checksum" % i], rtol=1e-12)
        m = hip.models.FlexibleNeRFModel(include_input_xyz=False).to(DEV)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        m.arithmetic = arith
        ms.append(m)
    return ms


def opts(perturb=False, noise=0.0, chunk=131072, nc=64, nf=64):
    from types import SimpleNamespace as NS
    mode = NS(chunksize=chunk, perturb=perturb, num_coarse=nc, num_fine=nf, white_background=False, radiance_field_noise_std=noise, lindisp=False)
    return NS(nerf=NS(use_viewdirs=True, encode_position_fn="mip", train=mode, validation=mode))


def scene(ndc):
    return {"near": 0.0 if ndc else 2.0, "far": 1.0 if ndc else 6.0, "no_ndc": not ndc}


def run(hip, g, mc, mf, o, mode, ndc=False, randoms=None):
    H, W, focal = g["c.hwf"]
    rays = torch.stack((T(g["c.ro"]).reshape(-1, 3), T(g["c.rd"]).reshape(-1, 3)))
    return hip.train_utils.run_one_iter_of_nerf(int(H), int(W), float(focal), mc, mf, rays, o, "lego_DS8", mode=mode, scene_config=scene(ndc),
                                                randoms=randoms)


def check_render(out, g, tag):
    ec = np.abs(N_(out[0]) - g[tag + "rgb_coarse"]).max()
    assert ec <= 3e-5, "%s coarse rgb max|err| %.2e" % (tag, ec)
    assert np.abs(N_(out[2]) - g[tag + "acc_coarse"]).max() <= 3e-5
    ef = np.abs(N_(out[3]) - g[tag + "rgb_fine"]).max(-1)
    mse = float(((N_(out[3]) - g[tag + "rgb_fine"]) ** 2).mean())
    psnr = 10 * np.log10(1.0 / max(mse, 1e-30))
    assert (ef <= 2e-4).mean() >= 0.95 and psnr >= 70, "%s fine: %.3f of rays within 2e-4, PSNR %.1f dB" % (tag, (ef <= 2e-4).mean(), psnr)


def check_grads(ms, g, prefix):
    for i, m in enumerate(ms):
        rl2, rmax = (1e-4, 1e-4) if i == 0 else (1e-2, 3e-2)
        if not prefix:
            # parameters after Adam: each element moves by ~lr m / sqrt(v) whatever its gradient's size, so an element whose gradient is
            # near zero moves by up to lr per step on a sign that rounding decides -- the per-element bound is 1e-3 of the largest parameter
            rmax = max(rmax, 1e-3)
        for k, p in m.named_parameters():
            ref = g["%s.m%d.grad.%s" % (prefix, i, k)] if prefix else g["e.m%d.%s" % (i, k)]
            got = mip_params.kept(k, N_(p.grad if prefix else p))
            assert np.isfinite(got).all(), k
            rel = np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-30)
            assert rel < rl2 and np.abs(got - ref).max() <= rmax * np.abs(ref).max(), "model %d %s: relative L2 %.2e" % (i, k, rel)


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


def _chain_abs_sum(g, i, x):
    """float64 sum over the layers of max_rows (|W||x| + |b|): the scale of the bf16x3 error bound"""
    sd = mip_params.state_dict((101, 202)[i])
    W = lambda k: np.abs(sd[k + ".weight"]).astype(np.float64)
    Wr = lambda k: sd[k + ".weight"].astype(np.float64)
    b = lambda k: sd[k + ".bias"].astype(np.float64)
    relu = lambda v: np.maximum(v, 0)
    xyz, view = x[:, :36].astype(np.float64), x[:, 36:].astype(np.float64)
    tot = 0.0
    h = xyz @ Wr("layer1").T + b("layer1")
    tot += (np.abs(xyz) @ W("layer1").T).max()
    for j in range(3):
        tot += (np.abs(h) @ W("layers_xyz.%d" % j).T).max()
        h = relu(h @ Wr("layers_xyz.%d" % j).T + b("layers_xyz.%d" % j))
    tot += (np.abs(h) @ W("fc_feat").T).max() + (np.abs(h) @ W("fc_alpha").T).max()
    feat = relu(h @ Wr("fc_feat").T + b("fc_feat"))
    c = np.concatenate([feat, view], -1)
    tot += (np.abs(c) @ W("layers_dir.0").T).max()
    hd = relu(c @ Wr("layers_dir.0").T + b("layers_dir.0"))
    tot += (np.abs(hd) @ W("fc_rgb").T).max()
    return tot


@pytest.mark.parametrize("arith", ARITHS)
def test_fused_forward_matches_upstream_model(hip, g23, arith):
    g = g23
    n, S = g["a.edges"].shape[0], g["a.edges"].shape[1] - 1
    for i, m in enumerate(models_from(hip, g, arith)):
        with torch.no_grad():
            raw = N_(m.mip_forward(T(g["a.rays"]), T(g["a.edges"]), float(g["radius"]))).reshape(n * S, 4)
        tol = 1e-5 if arith == "f32" else 1e-5 + 1e-6 * _chain_abs_sum(g, i, np.concatenate([g["a.ipe"], g["a.dirs"]], -1))
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

    def cpu_eval(dtype):
        ref = copy.deepcopy(m).cpu().to(dtype)
        for q in ref.parameters():
            q.grad = None
        with torch.enable_grad():
            xyz, view = x[:, :36].to(dtype), x[:, 36:].to(dtype)
            h = ref.layer1(xyz)
            for l in ref.layers_xyz:
                h = torch.relu(l(h))
            feat = torch.relu(ref.fc_feat(h))
            alpha = ref.fc_alpha(h)
            hd = torch.relu(ref.layers_dir[0](torch.cat((feat, view), -1)))
            out = torch.cat((ref.fc_rgb(hd), alpha), -1)
            (out * gr.to(dtype)).sum().backward()
        return out.detach().double(), {k: p.grad.double() for k, p in ref.named_parameters()}

    out64, g64 = cpu_eval(torch.float64)
    _, g32 = cpu_eval(torch.float32)          # the reference's own arithmetic: the scale of the summation error over 524 288 points
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
