"""What the tests of the two FlexibleNeRFModel baselines share -- tests/test_mip_nerf.py and tests/test_pe_nerf.py on the GPU, the C-ABI and
configuration checks of tests/test_mip_nerf_host.py and tests/test_pe_nerf_host.py on the CPU (not collected: the name does not start with
test_).  Seeds, chunk sizes and tolerances stay with the tests."""
import copy
import os
import re
import sys
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import mip_params  # noqa: E402

DEV = "cuda:0"


def T(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def N_(t):
    return t.detach().cpu().numpy()


def models_from(hip, g, arith, params, **kwargs):
    """the two models of a fixture (coarse, fine): FlexibleNeRFModel(**kwargs) with the parameters of params.state_dict(params.SEEDS[i]),
    checked against the fixture's checksums"""
    ms = []
    for i, seed in enumerate(params.SEEDS):
        sd = params.state_dict(seed)
        np.testing.assert_allclose(params.checksum(sd), g["b.m%d.checksum" % i], rtol=1e-12)
        m = hip.models.FlexibleNeRFModel(**kwargs).to(DEV)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        m.arithmetic = arith
        ms.append(m)
    return ms


def opts(encode, perturb=False, noise=0.0, chunk=131072, nc=64, nf=64):
    mode = NS(chunksize=chunk, perturb=perturb, num_coarse=nc, num_fine=nf, white_background=False, radiance_field_noise_std=noise, lindisp=False)
    return NS(nerf=NS(use_viewdirs=True, encode_position_fn=encode, train=mode, validation=mode))


def scene(ndc):
    return {"near": 0.0 if ndc else 2.0, "far": 1.0 if ndc else 6.0, "no_ndc": not ndc}


def check_render(out, g, tag):
    ec = np.abs(N_(out[0]) - g[tag + "rgb_coarse"]).max()
    assert ec <= 3e-5, "%s coarse rgb max|err| %.2e" % (tag, ec)
    assert np.abs(N_(out[2]) - g[tag + "acc_coarse"]).max() <= 3e-5
    ef = np.abs(N_(out[3]) - g[tag + "rgb_fine"]).max(-1)
    mse = float(((N_(out[3]) - g[tag + "rgb_fine"]) ** 2).mean())
    psnr = 10 * np.log10(1.0 / max(mse, 1e-30))
    assert (ef <= 2e-4).mean() >= 0.95 and psnr >= 70, "%s fine: %.3f of rays within 2e-4, PSNR %.1f dB" % (tag, (ef <= 2e-4).mean(), psnr)


def check_grads(ms, g, prefix):
    """gradients (prefix "d") or parameters after Adam (prefix "") of both models against the fixture, at mip_params.kept_elements (the rule of
    both fixtures)"""
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


def chain_abs_sum(sd, x, enc):
    """float64 sum over the layers of max_rows (|W||x| + |b|): the scale of the bf16x3 error bound; x = [enc position columns | directions]"""
    W = lambda k: np.abs(sd[k + ".weight"]).astype(np.float64)
    Wr = lambda k: sd[k + ".weight"].astype(np.float64)
    b = lambda k: sd[k + ".bias"].astype(np.float64)
    relu = lambda v: np.maximum(v, 0)
    xyz, view = x[:, :enc].astype(np.float64), x[:, enc:].astype(np.float64)
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


def cpu_eval(m, x, gr, enc, dtype):
    """the model m on the CPU in `dtype` on encoded rows x [P, enc + 27] (float64), backward of sum(out * gr) -> (out as float64,
    {name: gradient as float64})"""
    ref = copy.deepcopy(m).cpu().to(dtype)
    for q in ref.parameters():
        q.grad = None
    with torch.enable_grad():
        xyz, view = x[:, :enc].to(dtype), x[:, enc:].to(dtype)
        h = ref.layer1(xyz)
        for l in ref.layers_xyz:
            h = torch.relu(l(h))
        feat = torch.relu(ref.fc_feat(h))
        alpha = ref.fc_alpha(h)
        hd = torch.relu(ref.layers_dir[0](torch.cat((feat, view), -1)))
        out = torch.cat((ref.fc_rgb(hd), alpha), -1)
        (out * gr.to(dtype)).sum().backward()
    return out.detach().double(), {k: p.grad.double() for k, p in ref.named_parameters()}


# ---- host checks of the C ABI (prefix "mip" / "pe") and of the configurations the kernels are not built for -------------------------------

def check_entry_points(capi, prefix, sizes):
    """the header declares the five entry points and the library exports them; the NATURAL / RECORD / GRAD_RECORD macros equal `sizes` and the
    capi constants; the weight-gradient workspace at 0, 8192 and 8193 points (one partial blob per slab of 8192)"""
    text = open(os.path.join(ROOT, "include", "nvsr.h")).read()
    for name in ("encode", "nerf_forward_arith", "nerf_backward_arith", "nerf_wgrad_workspace_floats", "nerf_weight_grad"):
        name = "nvsr_%s_%s" % (prefix, name)
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in capi.exported_symbols(), name
    for kind, value in zip(("NATURAL", "RECORD", "GRAD_RECORD"), sizes):
        macro = "NVSR_%s_NERF_%s_FLOATS" % (prefix.upper(), kind)
        assert int(re.search(r"#define %s (\d+)" % macro, text).group(1)) == value
        assert getattr(capi, macro[len("NVSR_"):]) == value
    workspace = getattr(capi.lib(), "nvsr_%s_nerf_wgrad_workspace_floats" % prefix)
    assert workspace(0) == 0
    assert workspace(8192) == sizes[0]
    assert workspace(8193) == 2 * sizes[0]


def check_bad_arguments(capi, prefix):
    """shape / arithmetic / null checks return before any launch"""
    fn = lambda name: getattr(capi.lib(), "nvsr_%s_%s" % (prefix, name))
    radius = (0.0,) if prefix == "mip" else ()                                    # (Mip's entry points take the cone radius after the depths)
    assert fn("encode")(-1, 4, None, None, *radius, None, None) == 1               # NVSR_ERR_SHAPE
    assert fn("encode")(0, 4, None, None, *radius, None, None) == 0                # nothing to do
    assert fn("nerf_forward_arith")(1, 0, None, None, *radius, None, None, None, 0, None) == 1
    assert fn("nerf_forward_arith")(1, 4, None, None, *radius, None, None, None, 7, None) == 1
    assert fn("nerf_backward_arith")(-1, None, None, None, None, 0, None) == 1
    assert fn("nerf_weight_grad")(-1, None, None, None, None, None) == 1


def host_opts(encode):
    return opts(encode, chunk=1024, nc=8, nf=8)


HOST_SCENE = {"near": 2.0, "far": 6.0, "no_ndc": True}


def check_geometry_refused(good, bad, encode, scene_id, match):
    """run_one_iter_of_nerf under `encode` refuses the geometry of `bad`, as the coarse or the fine model, before the rays are packed (CPU models
    and CPU rays: reaching a kernel would fail differently)"""
    import nvsr_amd
    rays = torch.zeros(2, 4, 3)
    for mc, mf in ((bad, good), (good, bad)):
        with pytest.raises(NotImplementedError, match=match):
            nvsr_amd.train_utils.run_one_iter_of_nerf(4, 4, 2.0, mc, mf, rays, host_opts(encode), scene_id, mode="validation",
                                                      scene_config=HOST_SCENE)
