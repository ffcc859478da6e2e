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
import copy
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import pe_params  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ARITHS = ["f32", "bf16x3"]


def T(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def N_(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def g24():
    return load_golden("g24_pe_nerf.npz")


def models_from(hip, g, arith):
    """the two g24 models (coarse, fine): parameters from pe_params, checked against the fixture's checksums"""
    ms = []
    for i, seed in enumerate(pe_params.SEEDS):
        sd = pe_params.state_dict(seed)
        np.testing.assert_allclose(pe_params.checksum(sd), g["b.m%d.checksum" % i], rtol=1e-12)
        m = hip.models.FlexibleNeRFModel().to(DEV)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        m.arithmetic = arith
        ms.append(m)
    return ms


def opts(perturb=False, noise=0.0, chunk=131072, nc=64, nf=64):
    from types import SimpleNamespace as NS
    mode = NS(chunksize=chunk, perturb=perturb, num_coarse=nc, num_fine=nf, white_background=False, radiance_field_noise_std=noise, lindisp=False)
    return NS(nerf=NS(use_viewdirs=True, encode_position_fn="positional_encoding", train=mode, validation=mode))


def scene(ndc):
    return {"near": 0.0 if ndc else 2.0, "far": 1.0 if ndc else 6.0, "no_ndc": not ndc}


def run(hip, g, mc, mf, o, mode, ndc=False, randoms=None):
    H, W, focal = g["c.hwf"]
    rays = torch.stack((T(g["c.ro"]).reshape(-1, 3), T(g["c.rd"]).reshape(-1, 3)))
    return hip.train_utils.run_one_iter_of_nerf(int(H), int(W), float(focal), mc, mf, rays, o, str(g["scene_id"]), mode=mode,
                                                scene_config=scene(ndc), randoms=randoms)


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
            rmax = max(rmax, 1e-3)      # (Adam moves an element by ~lr per step whatever its gradient's size: tests/test_mip_nerf.py)
        for k, p in m.named_parameters():
            ref = g["%s.m%d.grad.%s" % (prefix, i, k)] if prefix else g["e.m%d.%s" % (i, k)]
            got = pe_params.kept(k, N_(p.grad if prefix else p))
            assert np.isfinite(got).all(), k
            rel = np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-30)
            assert rel < rl2 and np.abs(got - ref).max() <= rmax * np.abs(ref).max(), "model %d %s: relative L2 %.2e" % (i, k, rel)


@pytest.mark.parametrize("tag", ["a.", "a.ndc."])
def test_pe_encode_matches_upstream(hip, g24, tag):
    g = g24
    out = N_(torch.ops.nvsr.pe_encode(T(g[tag + "rays"]), T(g[tag + "z"])))
    assert out.shape == (g[tag + "enc"].shape[0], 66)
    np.testing.assert_array_equal(out[:, :3], g[tag + "enc"][:, :3])              # the points, bit for bit
    err = np.abs(out[:, 3:39] - g[tag + "enc"][:, 3:])
    assert err.max() <= 2e-6, "encoding max|err| %.2e (column %d)" % (err.max(), 3 + int(err.max(0).argmax()))
    np.testing.assert_allclose(out[:, 39:], g[tag + "dirs"], rtol=0, atol=2e-6)


def _chain_abs_sum(i, x):
    """float64 sum over the layers of max_rows (|W||x| + |b|): the scale of the bf16x3 error bound"""
    sd = pe_params.state_dict(pe_params.SEEDS[i])
    W = lambda k: np.abs(sd[k + ".weight"]).astype(np.float64)
    Wr = lambda k: sd[k + ".weight"].astype(np.float64)
    b = lambda k: sd[k + ".bias"].astype(np.float64)
    relu = lambda v: np.maximum(v, 0)
    xyz, view = x[:, :39].astype(np.float64), x[:, 39:].astype(np.float64)
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
def test_fused_forward_matches_upstream_model(hip, g24, arith):
    g = g24
    for tag, key in (("a.", "raw"), ("a.ndc.", "ndc.raw")):
        n, S = g[tag + "z"].shape
        x = np.concatenate([g[tag + "enc"], g[tag + "dirs"]], -1)
        for i, m in enumerate(models_from(hip, g, arith)):
            with torch.no_grad():
                raw = N_(m.pe_forward(T(g[tag + "rays"]), T(g[tag + "z"]))).reshape(n * S, 4)
            tol = 1e-5 if arith == "f32" else 1e-5 + 1e-6 * _chain_abs_sum(i, x)
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

    def cpu_eval(dtype):
        ref = copy.deepcopy(m).cpu().to(dtype)
        for q in ref.parameters():
            q.grad = None
        with torch.enable_grad():
            xyz, view = x[:, :39].to(dtype), x[:, 39:].to(dtype)
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
