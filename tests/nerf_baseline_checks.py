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


def cpu_eval(m, x, gr, enc, dtype, device="cpu"):
    """the model m on the CPU (or `device`) in `dtype` on encoded rows x [P, enc + 27] (float64), backward of sum(out * gr) -> (out as
    float64, {name: gradient as float64}) on that device"""
    ref = copy.deepcopy(m).to(device=device, dtype=dtype)
    for q in ref.parameters():
        q.grad = None
    with torch.enable_grad():
        x, gr = x.to(device), gr.to(device)
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


# ---- the layer engine of csrc/nerf_mlp.h restated in float64 (tests/test_nerf_baseline_edges.py) --------------------------------------------

U = 2.0 ** -24                  # f32 unit roundoff
NERF_DIR, MH, MHD = 27, 128, 64
# pre-activation gradients per point (nerf_mlp.h): [layer1 | x0 | x1 | x2 | feat (128 each) | alpha 1 | dir 64 | rgb 3]
G_L1, G_X0, G_X1, G_X2, G_FEAT, G_A, G_DIR, G_RGB, GREC = 0, 128, 256, 384, 512, 640, 641, 705, 708
NERF_F16_UP = 3                 # nerf_mlp.h: a chain's largest |dL/draw| is scaled into [2^3, 2^4)
MW_SLAB = 8192                  # nerf_mlp.h: points per weight-gradient slab, a quarter per wave


def record_columns(enc):
    """column offsets of the recording forward's record per point (nerf_mlp.h NerfLayout): [enc | dir 27 | h1 | h2 | h3 | h4 | feat | hd 64]"""
    i = enc + NERF_DIR
    return NS(enc=0, dir=enc, h1=i, h2=i + MH, h3=i + 2 * MH, h4=i + 3 * MH, feat=i + 4 * MH, hd=i + 5 * MH, width=i + 5 * MH + MHD)


def natural_blob(sd):
    """a state dict in mip_params / pe_params order -> the natural f32 blob (FlexibleNeRFModel.natural_blob's order)"""
    return np.concatenate([v.reshape(-1) for v in sd.values()]).astype(np.float32)


def bits(t):
    return t.contiguous().view(torch.int32)


def gemm_eps(arith, K):
    """The error bound of one output of a K-wide layer relative to sum_k |W_k||x_k|, with the MFMA count of nerf_mlp.h tile_layer (its zero
    padding columns add nothing):
        f32     gamma_K = K 2^-24 / (1 - K 2^-24)           the bound of a dot product whose products may be rounded (Higham, Accuracy and
                                                            Stability of Numerical Algorithms, (3.5)): at most K roundings on any term's path
        bf16x3  2^-21 + 2^-30 + 6 ceil(K / 16) 2^-24       test_limb_gemm_error_bounds (tests/test_hip_round3.py): the dropped limb products
                                                            + 6 accumulating MFMAs per 16 columns
        f16x2   2^-21 + 3 ceil(K / 16) 2^-24               test_limb_gemm_error_bounds: representation and the dropped lo x lo product + 3
                                                            MFMAs per 16 columns; plus an absolute floor for subnormal low limbs, which the
                                                            callers add
    f32 is not test_limb_gemm_error_bounds' ceil(K / 2) 2^-24 (one rounding per v_mfma_f32_32x32x2_f32, exact products): at K = 3 (fc_rgb's
    transposed product in the backward) the kernel's G_dir is off by up to 1.26 ulp of a result whose products all have one sign -- more than
    two round-to-nearest steps allow.  At K = 192 that model's bound has room enough to hide this."""
    c16 = -(-K // 16)
    return {"f32": K * U / (1 - K * U), "bf16x3": 2.0 ** -21 + 2.0 ** -30 + 6 * c16 * U, "f16x2": 2.0 ** -21 + 3 * c16 * U}[arith]


def assert_within(name, got, ref, bound):
    """|got - ref| <= bound for every element of the [P, M] arrays (a non-finite got fails) -> the worst err / bound"""
    err = (got - ref).abs()
    bound = bound.expand_as(err)
    bad = ~(err <= bound)
    if bad.any():
        pt, c = [int(v) for v in bad.nonzero()[0]]
        raise AssertionError("%s: %d of %d elements beyond the bound, the first at point %d of %d, column %d: got %r, float64 %r, bound %.3g"
                             % (name, int(bad.sum()), bad.numel(), pt, got.shape[0], c, float(got[pt, c]), float(ref[pt, c]),
                                float(bound[pt, c])))
    return float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0


def _param(sd, name, device):
    return torch.as_tensor(sd[name], device=device).double()


def check_forward_layers(arith, sd, rec, raw, enc):
    """Every layer of the recording forward (nerf_mlp.h nerf_forward_kernel) from the kernel's own record of its input, in float64:
    y = W x + b, act(y) against the kernel's record of the output (h1 .. h4, feat, hd; raw's rgb and alpha), every point and column.  Per
    element, with S = sum_k |W_k||x_k| and e = gemm_eps(arith, K) at the layer's width K (36 / 39, 128, 155, 64):
        |got - act(y)| <= (e S + floor)(1 + 2^-24) + 2^-24 |y|      the products, then one rounding of the bias add (ReLU is 1-Lipschitz)
        floor = 0; f16x2: 2^-29 sum_k |W_k| + 2^-33 sum_k |x_k|      test_limb_gemm_error_bounds' floor: a subnormal low limb of x 2^4 or of
                                                                      W 2^8 is off by up to 2^-25, 2^-29 per activation and 2^-33 per
                                                                      weight unscaled (the unscale by 2^-12 is exact)
    Taking each input from the record isolates the layer: a fault in one row of a tile cannot hide in the error of the chain.  rec [P, REC],
    raw [P, 4] (device tensors) -> {layer: worst err / bound}"""
    C = record_columns(enc)
    dev = rec.device
    r = rec.double()
    col = lambda c, n: r[:, c:c + n]
    layers = (("layer1", col(C.enc, enc), col(C.h1, MH), False), ("layers_xyz.0", col(C.h1, MH), col(C.h2, MH), True),
              ("layers_xyz.1", col(C.h2, MH), col(C.h3, MH), True), ("layers_xyz.2", col(C.h3, MH), col(C.h4, MH), True),
              ("fc_feat", col(C.h4, MH), col(C.feat, MH), True), ("fc_alpha", col(C.h4, MH), raw[:, 3:4].double(), False),
              ("layers_dir.0", torch.cat([col(C.feat, MH), col(C.dir, NERF_DIR)], 1), col(C.hd, MHD), True),
              ("fc_rgb", col(C.hd, MHD), raw[:, :3].double(), False))
    report = {}
    for name, x, got, relu in layers:
        W, b = _param(sd, name + ".weight", dev), _param(sd, name + ".bias", dev)
        e = gemm_eps(arith, W.shape[1])
        y = x @ W.T + b
        prod = e * (x.abs() @ W.abs().T)
        if arith == "f16x2":
            prod = prod + 2.0 ** -29 * W.abs().sum(1) + 2.0 ** -33 * x.abs().sum(1, keepdim=True)
        report[name] = assert_within(name, got, y.clamp_min(0) if relu else y, prod * (1 + U) + U * y.abs())
    return report


def pow2_undo(m):
    """nerf_mlp.h nerf_pow2_scale's undo factor for per-point maxima m (float32) -> float64: 2^(eu - 127), eu = clamp(biased exponent of m,
    1 + UP, 253) - UP (127 for a non-finite m: a scale of 1); the chain runs at m / undo in [2^UP, 2^(UP + 1))"""
    e = (np.ascontiguousarray(m, dtype=np.float32).view(np.uint32) >> 23) & 0xFF
    eu = np.where(e == 255, 127 + NERF_F16_UP, np.clip(e, 1 + NERF_F16_UP, 253)).astype(np.int64) - NERF_F16_UP
    return np.ldexp(1.0, eu - 127)


def check_backward_layers(arith, sd, rec, grec, g_raw, enc):
    """Every transposed layer of nerf_mlp.h nerf_backward_kernel from the kernel's own grad_record of the layer above and its recorded ReLU
    gates, in float64:
        G_rgb = dL/drgb, G_alpha = dL/dalpha                                       bit for bit (stored as read)
        G_dir = [hd > 0] G_rgb W_rgb            G_feat = [feat > 0] G_dir W_dir[:, :128]
        G_x2 = [h4 > 0] (G_feat W_feat + dL/dalpha W_alpha)
        G_x1 = [h3 > 0] G_x2 W_x2               G_x0 = [h2 > 0] G_x1 W_x1            G_1 = G_x0 W_x0 (layer1 is linear)
    Per element, with S = sum_k |W_k||G_k| over the K gradients of the layer above (K = 3, 64, 128) and e = gemm_eps(arith, K):
        e S + floor; G_x2 adds the roundings of dL/dalpha W_alpha and of the sum: + 2^-24 |dL/dalpha W_alpha| + 2^-24 (|y| + the rest)
    The f16x2 floor.  The gradient operand is not scaled by 2^4 like an activation but per point, by nerf_pow2_scale: the rgb chain (G_dir,
    G_feat and fc_feat's product) runs at 1 / un_r, which puts max |dL/drgb| into [8, 16), and from G_x2 on at 1 / un_m (max |dL/draw|); the
    rgb part enters the joint chain through an exact multiply by a power of two.  A scaled gradient g / un = hi + lo + d with
    |d| <= 2^-22 |g / un| (inside gemm_eps' 2^-21) + 2^-25 (half the spacing of subnormal f16, where lo underflows): 2^-25 un unscaled per
    gradient element.  The weight W 2^8 is off by up to 2^-25: 2^-33 unscaled.  So floor = 2^-25 un_c sum_k |W_k| + 2^-33 sum_k |G_k| with
    un_c the undo factor of the chain the operand belongs to; G_x2 adds 2^-149 un_m (the power-of-two multiply into the joint chain rounds
    only below 2^-126).  The undo factors follow from dL/draw (pow2_undo).
    rec [P, REC], grec [P, 708], g_raw [P, 4] (device tensors) -> {layer: worst err / bound}"""
    dev = rec.device
    assert torch.equal(bits(grec[:, G_RGB:G_RGB + 3]), bits(g_raw[:, :3])), "G_rgb is not dL/drgb"
    assert torch.equal(bits(grec[:, G_A]), bits(g_raw[:, 3])), "G_alpha is not dL/dalpha"
    C = record_columns(enc)
    G, g = grec.double(), g_raw.double()
    gate = lambda c, n: (rec[:, c:c + n] > 0).double()
    f16 = arith == "f16x2"
    if f16:
        gr = g_raw.cpu().numpy()
        mr = np.abs(gr[:, :3]).max(1)
        un_r, un_m = [torch.as_tensor(pow2_undo(v), device=dev)[:, None] for v in (mr, np.maximum(mr, np.abs(gr[:, 3])))]
    Wp = lambda k: _param(sd, k + ".weight", dev)
    steps = (("G_dir", G_RGB, Wp("fc_rgb"), G_DIR, gate(C.hd, MHD), "r"),
             ("G_feat", G_DIR, Wp("layers_dir.0")[:, :MH], G_FEAT, gate(C.feat, MH), "r"),
             ("G_x2", G_FEAT, Wp("fc_feat"), G_X2, gate(C.h4, MH), "r"),
             ("G_x1", G_X2, Wp("layers_xyz.2"), G_X1, gate(C.h3, MH), "m"),
             ("G_x0", G_X1, Wp("layers_xyz.1"), G_X0, gate(C.h2, MH), "m"),
             ("G_1", G_X0, Wp("layers_xyz.0"), G_L1, None, "m"))
    report = {}
    for name, xo, W, yo, gt, chain in steps:
        K, M = W.shape
        x = G[:, xo:xo + K]
        y = x @ W
        bound = gemm_eps(arith, K) * (x.abs() @ W.abs())
        if f16:
            bound = bound + 2.0 ** -25 * (un_r if chain == "r" else un_m) * W.abs().sum(0) + 2.0 ** -33 * x.abs().sum(1, keepdim=True)
        if name == "G_x2":
            ga = g[:, 3:4] * Wp("fc_alpha")[0]
            y = y + ga
            bound = bound + U * ga.abs() + U * (y.abs() + bound + U * ga.abs()) + (2.0 ** -149 * un_m if f16 else 0.0)
        report[name] = assert_within(name, G[:, yo:yo + M], y if gt is None else gt * y, bound)
    return report


def wgrad_layers(enc):
    """(G offset, rows M, record column ranges of X) of every layer, in natural-blob order (nerf_mlp.h nerf_weight_grad_launch)"""
    C = record_columns(enc)
    return ((G_L1, MH, ((C.enc, enc),)), (G_X0, MH, ((C.h1, MH),)), (G_X1, MH, ((C.h2, MH),)), (G_X2, MH, ((C.h3, MH),)),
            (G_DIR, MHD, ((C.feat, MH), (C.dir, NERF_DIR))), (G_A, 1, ((C.h4, MH),)), (G_RGB, 3, ((C.hd, MHD),)), (G_FEAT, MH, ((C.h4, MH),)))


def wgrad_reference(rec, grec, enc):
    """float64 dW = G^T X and db = sum_p G of every layer, concatenated like the natural blob, and sum_p |G||X| / sum_p |G| beside them"""
    r, G = rec.double(), grec.double()
    ref, mag = [], []
    for go, M, xs in wgrad_layers(enc):
        X = torch.cat([r[:, c:c + n] for c, n in xs], 1)
        g = G[:, go:go + M]
        ref += [(g.T @ X).reshape(-1), g.sum(0)]
        mag += [(g.abs().T @ X.abs()).reshape(-1), g.abs().sum(0)]
    return torch.cat(ref), torch.cat(mag)


def wgrad_roundings(P):
    """the most roundings a product passes through in nerf_wgrad_kernel + nerf_wgrad_reduce_kernel: one per point of its wave (up to
    MW_SLAB / 4; the f32 MFMA takes two points per step but is not one rounding per step, see gemm_eps), 3 adds of the waves' partial sums,
    slabs - 1 adds of the slabs"""
    slabs = -(-P // MW_SLAB)
    return min(P, MW_SLAB // 4) + 3 + slabs - 1


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
