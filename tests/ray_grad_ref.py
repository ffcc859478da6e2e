"""Restatements behind tests/test_ray_grad_host.py (CPU) and tests/test_ray_grad.py (GPU), no GPU needed: the four entries of csrc/ray_grad.hip
in the order include/nvsr.h states.

Every function takes `dt`: with numpy.float32 each numpy operation on float32 arrays is one correctly rounded float32 operation, like the
kernels' __f*_rn (the library is built with -ffp-contract=off) -- the bit-for-bit transcription; with numpy.float64 the same expressions are the
float64 formulas.  `*_terms` return, per component, the sum of the absolute values of the terms the stated order adds (float64): the
kernel-alone bound is K * 2^-24 * terms, K the number of roundings on the longest path:

  rays_grad       n = ceil(S / 64).  columns 0..2: n (a lane's chain onto +0) + 6 (tree).  columns 3..5: B: 1 (z .) + n + 6;  the compositor term:
                  1 (raw + noise) + 1 (g sigma) + n + 6 = n + 8 for T, + 1 (T rd_k) + 3 (rr: a product, two additions) + 1 (/): n + 13;  + 1 for
                  B + term: n + 14.  accumulate: + 1 (old + value), the old value joins the terms.
  pack_rays_bwd   relative errors add under a product or a quotient (+ 1 for its own rounding), a square root halves its operand's:
                  n2 = |v|^2, positive terms: 3;  n = sqrt: 3 / 2 + 1 = 2.5;  u_k = v_k / n: 3.5;  u_j g_j: 4.5, dot (two additions): 6.5;
                  u_k dot: 3.5 + 6.5 + 1 = 11;  g - .: 12;  / n: 12 + 2.5 + 1 = 15.5 -> K = 16;  view_is_rd, d_rd = d_rays + c: 16.5 -> K = 17.
  ray_bundle_bwd  dir_j: 2 (ii, jj are exact small integers plus a half), the product 1, tree 6, the four waves 2, the lane chain
                  ceil(slabs / 64), the last tree 6: 17 + ceil(slabs / 64).
  ndc_rays_bwd    oz = o_2 + t d_2 is a cancelling sum (its value is -near) that later divides: its relative error is not a few roundings but
                  <= 4 kappa 2^-24, kappa = (|o_2| + |t d_2|) / |oz| >= 1 per ray (t: 2 roundings, t d_2: 3, the sum: 4, relative to the sum of
                  the absolute terms).  Everything else is counted as above, relative to the absolute-term version of the same expressions
                  (every input, sx, sy by absolute value, every difference a sum, t taken as (|near| + |o_2|) / |d_2|, the divisor |oz| exact).
                  Longest path, d_rd_2 = (t g_oz - e) - t q:  ox: 4;  ox h_0: 4 + 2 + 1 = 7;  the numerator's two additions: 9;  / (oz oz): + 1 for
                  the product, + 1 for the quotient = 11, and oz twice: + 8 kappa;  g_oz d_2: 12;  g_t: 14;  q = g_t / d_2: 15;  t q: 15 + 2 + 1 =
                  18;  the last difference: 19.  K = 20 + 8 kappa (one rounding of slack for the second-order terms)."""
import numpy as np

U = 2.0 ** -24
f32, f64 = np.float32, np.float64


def tree(x):
    """balanced tree over neighbouring entries of the last axis (64, or 4): b_i = x_2i + x_2i+1, ..."""
    while x.shape[-1] > 1:
        x = x[..., 0::2] + x[..., 1::2]
    return x[..., 0]


def lane_sums(terms, lanes=64):
    """terms [N, S] -> [N, lanes]: lane l adds terms l, l + lanes, ... in ascending order onto +0 (absent terms are +0, which changes no bit)"""
    N, S = terms.shape
    n = -(-S // lanes)
    t = np.zeros((N, n * lanes), terms.dtype)
    t[:, :S] = terms
    t = t.reshape(N, n, lanes)
    acc = np.zeros((N, lanes), terms.dtype)
    for i in range(n):
        acc = acc + t[:, i]
    return acc


def k_rays_grad(S, accumulate):
    n = -(-S // 64)
    return n + 6 + bool(accumulate), n + 14 + bool(accumulate)


def rays_grad(dt, rays, z, d_points, d_viewdir, raw, noise, g_raw, accumulate=False, d_rays=None, terms=False):
    """nvsr_rays_grad -> d_rays [N,11] (terms=True: the per-component sums of absolute terms instead, float64)"""
    c = (lambda a: np.abs(np.asarray(a, f64))) if terms else (lambda a: np.asarray(a, dt))
    rays_v = np.asarray(rays, f64 if terms else dt)
    N, S = np.asarray(raw).shape[:2]
    out = np.zeros((N, 11), f64 if terms else dt)
    with np.errstate(all="ignore"):
        if d_points is not None:
            dp, zz = c(d_points).reshape(N, S, 3), c(z)
            for k in range(3):
                out[:, k] = tree(lane_sums(dp[:, :, k]))
                out[:, 3 + k] = tree(lane_sums(zz * dp[:, :, k]))
        sn = np.asarray(raw, dt)[:, :, 3] if noise is None else np.asarray(raw, dt)[:, :, 3] + np.asarray(noise, dt)
        sig = np.where(sn < 0, dt(0), sn)
        T = tree(lane_sums(c(g_raw)[:, :, 3] * c(sig)))
        rd = c(rays_v[:, 3:6])
        rr = (rd[:, 0] * rd[:, 0] + rd[:, 1] * rd[:, 1]) + rd[:, 2] * rd[:, 2]
        for k in range(3):
            out[:, 3 + k] = out[:, 3 + k] + (T * rd[:, k]) / rr
        if d_viewdir is not None:
            out[:, 8:11] = c(d_viewdir)
        if accumulate:
            old = c(d_rays)
            out[:, 0:6] = old[:, 0:6] + out[:, 0:6]
            out[:, 8:11] = old[:, 8:11] + out[:, 8:11]
    if not terms:
        bad = np.isnan(rays_v[:, [0, 1, 2, 3, 4, 5, 8, 9, 10]]).any(1)
        out[np.ix_(bad, [0, 1, 2, 3, 4, 5, 8, 9, 10])] = np.nan
    return out


def pack_rays_backward(dt, d_rays, view_src, view_is_rd, terms=False):
    """nvsr_pack_rays_backward -> (d_ro, d_rd, d_view_src or None)"""
    g, v = np.asarray(d_rays, dt), np.asarray(view_src, dt)
    with np.errstate(all="ignore"):
        n = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
        u = v / n[:, None]
        if terms:
            g, u = np.abs(g), np.abs(u)
        dot = (u[:, 0] * g[:, 8] + u[:, 1] * g[:, 9]) + u[:, 2] * g[:, 10]
        c = ((g[:, 8:11] + u * dot[:, None]) if terms else (g[:, 8:11] - u * dot[:, None])) / n[:, None]
        d_ro, d_rd = g[:, 0:3].copy(), g[:, 3:6].copy()
        if view_is_rd:
            return d_ro, d_rd + c, None
    return d_ro, d_rd, c


K_PACK, K_PACK_VIEW_IS_RD = 16, 17


def ndc_consts(dt, H, W, focal, near):
    """sx, sy, near, 2 near as nvsr_ndc_rays[_backward] form them: in double, then cast"""
    return dt(-1.0 / (W / (2.0 * focal))), dt(-1.0 / (H / (2.0 * focal))), dt(near), dt(2.0 * near)


def ndc_rays(dt, H, W, focal, near, ro, rd):
    """ndc_rays_kernel (the forward the adjoint restates)"""
    sx, sy, nr, two = ndc_consts(dt, H, W, focal, near)
    o, d = np.asarray(ro, dt), np.asarray(rd, dt)
    t = (-(nr + o[:, 2])) / d[:, 2]
    ox, oy, oz = o[:, 0] + t * d[:, 0], o[:, 1] + t * d[:, 1], o[:, 2] + t * d[:, 2]
    ro_out = np.stack([(sx * ox) / oz, (sy * oy) / oz, dt(1) + two / oz], 1)
    rd_out = np.stack([sx * (d[:, 0] / d[:, 2] - ox / oz), sy * (d[:, 1] / d[:, 2] - oy / oz), (-two) / oz], 1)
    return ro_out, rd_out


def ndc_rays_backward(dt, H, W, focal, near, ro, rd, go, gd, terms=False):
    """nvsr_ndc_rays_backward -> (d_ro, d_rd);  terms=True: (A_ro, A_rd, kappa) -- the absolute-term version of the same expressions (float64)
    and kappa [N] = (|o_2| + |t d_2|) / |oz|: the bound is (20 + 8 kappa) 2^-24 A per component (the docstring of this module derives it)"""
    if terms:
        dt = f64
    sx, sy, nr, two = ndc_consts(dt, H, W, focal, near)
    o, d, go, gd = (np.asarray(a, dt) for a in (ro, rd, go, gd))
    with np.errstate(all="ignore"):
        t = (-(nr + o[:, 2])) / d[:, 2]
        ox, oy, oz = o[:, 0] + t * d[:, 0], o[:, 1] + t * d[:, 1], o[:, 2] + t * d[:, 2]
        sub = lambda a, b: a - b
        if terms:
            kappa = (np.abs(o[:, 2]) + np.abs(t * d[:, 2])) / np.abs(oz)
            sx, sy, nr, two, o, d, go, gd, oz = (np.abs(a) for a in (sx, sy, nr, two, o, d, go, gd, oz))
            t = (nr + o[:, 2]) / d[:, 2]
            ox, oy = o[:, 0] + t * d[:, 0], o[:, 1] + t * d[:, 1]
            sub = lambda a, b: a + b
        h0, h1, h2 = sx * sub(go[:, 0], gd[:, 0]), sy * sub(go[:, 1], gd[:, 1]), two * sub(go[:, 2], gd[:, 2])
        g_ox, g_oy = h0 / oz, h1 / oz
        g_oz = ((ox * h0 + oy * h1) + h2) / (oz * oz)
        if not terms:
            g_oz = -g_oz
        k0, k1 = sx * gd[:, 0], sy * gd[:, 1]
        g_t = (g_ox * d[:, 0] + g_oy * d[:, 1]) + g_oz * d[:, 2]
        q = g_t / d[:, 2]
        d_ro = np.stack([g_ox, g_oy, sub(g_oz, q)], 1)
        e = (k0 * d[:, 0] + k1 * d[:, 1]) / (d[:, 2] * d[:, 2])
        d_rd = np.stack([k0 / d[:, 2] + t * g_ox, k1 / d[:, 2] + t * g_oy, sub(sub(t * g_oz, e), t * q)], 1)
    return (d_ro, d_rd, kappa) if terms else (d_ro, d_rd)


SLAB = 256


def bundle_dirs(dt, H, W, fx, fy, offset, row_col=None, padding=0):
    """dir [N,3] as ray_bundle_kernel / ray_bundle_at_kernel form it (float32 always: `dt` only casts the result)"""
    fx, fy, off = f32(fx), f32(fy), f32(offset)
    if row_col is None:
        Hp, Wp = H + 2 * padding, W + 2 * padding
        r, c = np.divmod(np.arange(Hp * Wp), Wp)
        ii, jj = c.astype(f32) + off, r.astype(f32) + off
        if padding > 0:
            ii, jj = ii - f32(padding), jj - f32(padding)
    else:
        rc = np.asarray(row_col)
        ii, jj = rc[:, 1].astype(f32) + off, rc[:, 0].astype(f32) + off
    d0 = (ii - f32(W * 0.5)) / fx
    d1 = -((jj - f32(H * 0.5)) / fy)
    return np.stack([d0, d1, np.full_like(d0, -1.0)], 1).astype(dt)


def k_bundle(N):
    return 17 + -(-(-(-N // SLAB)) // 64)


def ray_bundle_backward(dt, H, W, fx, fy, offset, d_ro, d_rd, row_col=None, padding=0, terms=False):
    """nvsr_ray_bundle_backward -> d_c2w [4,4] (terms=True: sums of absolute terms, float64)"""
    if terms:
        dt = f64
    dirs = bundle_dirs(dt, H, W, fx, fy, offset, row_col, padding)
    g_o, g_d = np.asarray(d_ro, dt), np.asarray(d_rd, dt)
    if terms:
        dirs, g_o, g_d = np.abs(dirs), np.abs(g_o), np.abs(g_d)
    N = dirs.shape[0]
    slabs = -(-N // SLAB)
    out = np.zeros((4, 4), dt)
    for k in range(3):
        for j in range(4):
            x = np.zeros(slabs * SLAB, dt)
            x[:N] = g_d[:, k] * dirs[:, j] if j < 3 else g_o[:, k]
            partials = tree(tree(x.reshape(slabs, 4, 64)))                       # per slab: the waves' trees, then (w0 + w1) + (w2 + w3)
            out[k, j] = tree(lane_sums(partials[None, :]))[0]
    return out


# ---- plain-torch restatements for float64 autograd (what the formulas above are the derivatives of) -------------------------------------------
def torch_composite_rgb(raw, z, rd, noise, white=False):
    """volume_render_radiance_field in plain torch: dists * |rd|, the 1e10 last interval, relu(sigma + noise) -> rgb_map, acc_map"""
    import torch
    dists = torch.cat([z[:, 1:] - z[:, :-1], torch.full_like(z[:, :1], 1e10)], 1) * rd.norm(dim=-1, keepdim=True)
    sigma = torch.relu(raw[..., 3] + (0 if noise is None else noise))
    alpha = 1.0 - torch.exp(-sigma * dists)
    trans = torch.cumprod(torch.cat([torch.ones_like(alpha[:, :1]), 1.0 - alpha + 1e-10], 1), 1)[:, :-1]
    w = alpha * trans
    rgb = (w[..., None] * torch.sigmoid(raw[..., :3])).sum(1)
    acc = w.sum(1)
    return (rgb + (1.0 - acc[:, None])) if white else rgb, acc


def torch_ray_bundle(H, W, fx, fy, c2w, offset, row_col=None, padding=0):
    """get_ray_bundle in plain torch from the float32 directions of the kernels"""
    import torch
    dirs = torch.as_tensor(bundle_dirs(f64, H, W, fx, fy, offset, row_col, padding))
    rd = (dirs[:, None, :] * c2w[:3, :3]).sum(-1)
    ro = c2w[:3, 3].expand(rd.shape)
    return ro, rd


def torch_ndc_rays(H, W, focal, near, ro, rd):
    t = -(near + ro[:, 2]) / rd[:, 2]
    o = ro + t[:, None] * rd
    import torch
    sx, sy = -1.0 / (W / (2.0 * focal)), -1.0 / (H / (2.0 * focal))
    ro_out = torch.stack([sx * o[:, 0] / o[:, 2], sy * o[:, 1] / o[:, 2], 1.0 + 2.0 * near / o[:, 2]], 1)
    rd_out = torch.stack([sx * (rd[:, 0] / rd[:, 2] - o[:, 0] / o[:, 2]), sy * (rd[:, 1] / rd[:, 2] - o[:, 1] / o[:, 2]), -2.0 * near / o[:, 2]], 1)
    return ro_out, rd_out


# ---- scenarios shared by the GPU tests and the recordings tests/ray_grad_entry_table.json, tests/training_entry_table.json ------------------------
def g27_case(ci):
    """case ci of g27_ray_grad.npz -> (g, decoders as coarse.* / fine.* arrays: g11's with this case's entries written over them, planes)"""
    from conftest import load_golden
    g, g11 = load_golden("g27_ray_grad.npz"), load_golden("g11_grads.npz")
    flat = np.concatenate([np.asarray(g11[k], dtype=f64).reshape(-1) for k in sorted(g11) if k.startswith(("coarse.", "fine."))])
    assert np.array_equal(np.array([flat.sum(), np.square(flat).sum(), flat.size]), g["g11_decoders"]), "g11_grads.npz changed: regenerate g27"
    dec = {k: v for k, v in g11.items() if k.startswith(("coarse.", "fine."))}
    pre = "c%d_" % ci
    dec.update({k[len(pre):]: v for k, v in g.items() if k.startswith((pre + "coarse.", pre + "fine."))})
    return g, dec, [g["plane%d" % d] for d in range(4)]


def _entry_record(fn, name, args, streams):
    """one capi.call as [name, arguments, stream]: every scalar argument by value, "ptr" / "null" per pointer argument (an array of pointers: one
    per element), the stream -- the last argument of every launching entry -- as an ordinal by first appearance in `streams`"""
    import ctypes as C
    types = fn.argtypes or ()
    rec, stream = [], None
    for i, a in enumerate(args):
        t = types[i] if i < len(types) else None
        pointer = t is C.c_void_p or (isinstance(t, type) and issubclass(t, C._Pointer))
        if pointer and i == len(args) - 1 and t is C.c_void_p:
            stream = streams.setdefault(a.value if isinstance(a, C.c_void_p) else a, len(streams))
        elif isinstance(a, C.Array):
            rec.append(["ptr" if v else "null" for v in a])
        elif pointer:
            rec.append("null" if a is None or (isinstance(a, C.c_void_p) and not a.value) else "ptr")
        else:
            a = getattr(a, "value", a)                          # (a ctypes scalar)
            rec.append(a if isinstance(a, (bool, int, float)) else float(a) if t in (C.c_float, C.c_double) else int(a))
    return [name, rec, stream]


def train_step_entries(hip, deterministic, iterations=2, device="cuda:0", what=("LR_planes", "decoder"), pose_grad=False, arithmetic=None,
                       fwd_max=None, sr=False, detail=False):
    """`iterations` TrainStep iterations (256 rays, 8 + 8 samples, 32^2 planes, seeded randoms) with every capi.call recorded
    -> (entry names in call order, sha256 of the planes and decoder parameters afterwards).
    what: TrainStep's what2train -- the planes / the decoders train as it names them;  pose_grad: the pose requires a gradient;  arithmetic: of
    both models (None: the library's default);  fwd_max: train_utils.RECORD_FORWARD_MAX_POINTS during the iterations;  sr: only the fine model
    super-resolves (EDSR 16 x 2 on 20^2 planes, the coarse pass under no_grad, what = {'SR'}, loss on the fine output: the construction of
    tests/test_hip_round4.py::test_default_sr_refinement_steps; the digest then covers the SR network's parameters too).
    detail: the entries as _entry_record states them instead of names, and a third result: the number of torch.zeros / zeros_like calls made
    from train_utils and ops while a backward() ran."""
    import hashlib
    import sys
    import torch
    from bench import make_synthetic_scene, render_options
    calls, streams, real = [], {}, hip.capi.call
    zeros = {"n": 0, "backward": False}

    def spy(name, *a):
        calls.append(_entry_record(getattr(hip.capi.lib(), name), name, a, streams) if detail else name)
        return real(name, *a)

    def counting(fn):
        def wrapped(*a, **kw):
            if zeros["backward"] and sys._getframe(1).f_globals.get("__name__", "").rsplit(".", 1)[-1] in ("train_utils", "ops"):
                zeros["n"] += 1
            return fn(*a, **kw)
        return wrapped

    real_backward, real_zeros, real_zeros_like = torch.Tensor.backward, torch.zeros, torch.zeros_like

    def backward(self, *a, **kw):
        zeros["backward"] = True
        try:
            return real_backward(self, *a, **kw)
        finally:
            zeros["backward"] = False

    what = set(what)
    mc, mf, sid, pose = make_synthetic_scene(device, plane_res=20 if sr else 32, view_res=8 if sr else 16, seed=27)
    for m in (mc, mf):
        for n, p in m.named_parameters():
            p.requires_grad_("rot_mats" not in n and (("LR_planes" in what) if "planes_" in n else ("decoder" in what)))
        m.train()
        if arithmetic is not None:
            m.arithmetic = arithmetic
    opts, scfg = render_options(8, 8, perturb=True, noise=0.2)
    planes = list(mc.planes_.values())
    dec = list({id(p): p for m in (mc, mf) for p in m.decoder_parameters()}.values())
    extra, kw = [], {}
    if sr:
        torch.manual_seed(8)
        net = hip.models.PlanesSR(hip.models.EDSR, 4, 48, 48, {"model": {"hidden_size": 16, "n_blocks": 2}}, "bilinear").to(device)
        net.train()
        mf.assign_SR_model(net, SR_viewdir=False)
        mf.assign_LR_planes()
        mc.optional_no_grad = torch.no_grad
        extra = list(net.parameters())
        kw = dict(SR_optimizer=torch.optim.Adam(extra, lr=2e-3), SR_model=net, sr_loss="fine")
    step = hip.training.TrainStep(mc, mf, opts, what, optimizer=torch.optim.Adam(dec, lr=5e-3) if "decoder" in what else None,
                                  planes_optimizer=torch.optim.Adam(planes, lr=5e-2) if "LR_planes" in what else None,
                                  pixel_sampler=hip.training.DevicePixelSampler(seed=5), deterministic=deterministic, **kw)
    H = W = 24
    focal = 0.5 * W / np.tan(0.5 * 0.6911112)
    gen = torch.Generator(device=device).manual_seed(3)
    img = torch.rand(H, W, 3, device=device, generator=gen)
    N, Nc, Nf = 256, 8, 8
    rnd = dict(t_rand=torch.rand(N, Nc, device=device, generator=gen), u=torch.rand(N, Nf, device=device, generator=gen),
               noise_coarse=0.2 * torch.randn(N, Nc, device=device, generator=gen), noise_fine=0.2 * torch.randn(N, Nc + Nf, device=device, generator=gen))
    if pose_grad:
        pose = pose.clone().requires_grad_(True)
    # (what a process does once, whichever call comes first, is done before the spy goes in: the registration of the library's range flag,
    #  nvsr_set_range_flag -- the sequence must not depend on what ran earlier in the process)
    hip.capi.range_flag(torch.device(device))
    limit = hip.train_utils.RECORD_FORWARD_MAX_POINTS
    hip.capi.call = spy
    torch.Tensor.backward, torch.zeros, torch.zeros_like = backward, counting(real_zeros), counting(real_zeros_like)
    try:
        if fwd_max is not None:
            hip.train_utils.RECORD_FORWARD_MAX_POINTS = fwd_max
        for it in range(iterations):
            step(it, img, pose, H, W, focal, 1, sid, scfg, N, randoms=rnd, sr_iter=sr)
        torch.cuda.synchronize()
    finally:
        hip.capi.call = real
        torch.Tensor.backward, torch.zeros, torch.zeros_like = real_backward, real_zeros, real_zeros_like
        hip.train_utils.RECORD_FORWARD_MAX_POINTS = limit
    h = hashlib.sha256()
    for p in planes + dec + extra:
        h.update(p.detach().cpu().numpy().tobytes())
    return (calls, h.hexdigest(), zeros["n"]) if detail else (calls, h.hexdigest())


# the cases of tests/training_entry_table.json (tools/training_entry_table.py records them, tests/test_ray_grad.py replays them): name ->
# (environment, deterministic, the arguments of train_step_entries, is the digest reproducible)
TRAINING_CASES = {
    "a_planes_two_streams": ({}, False, dict(what=("LR_planes",)), False),
    "b_planes_one_stream": ({"NVSR_BWD_STREAMS": "0"}, False, dict(what=("LR_planes",)), False),
    "c_planes_decoder_atomic": ({}, False, dict(), False),
    "d_planes_decoder_deterministic": ({}, True, dict(), True),
    "e_decoder_only": ({}, False, dict(what=("decoder",)), False),
    # 256 x 8 = 2048 < 3000 < 4096 = 256 x 16: the coarse pass records, the fine pass recomputes
    "f_fine_pass_recomputes": ({}, False, dict(fwd_max=3000), False),
    "g_pose_gradient_f16x2": ({}, False, dict(pose_grad=True, arithmetic="f16x2"), False),
    "g_pose_gradient_f16x2_deterministic": ({}, True, dict(pose_grad=True, arithmetic="f16x2"), True),
    "h_sr_fine_only": ({}, False, dict(what=("SR",), sr=True), False),
}


def training_case(hip, name):
    """run case `name` of TRAINING_CASES under its environment -> {"entries", "sha256" (None where float atomics order the sums), "zeros"}"""
    import os
    env, det, kw, reproducible = TRAINING_CASES[name]
    handles = ("NVSR_BWD_STREAMS", "NVSR_OPS_DISPATCH", "NVSR_DETERMINISTIC")
    saved = {h: os.environ.get(h) for h in handles}
    try:
        for h in handles:
            os.environ.pop(h, None) if h not in env else os.environ.__setitem__(h, env[h])
        calls, digest, zeros = train_step_entries(hip, det, detail=True, **kw)
    finally:
        for h, v in saved.items():
            os.environ.pop(h, None) if v is None else os.environ.__setitem__(h, v)
    return {"entries": calls, "sha256": digest if reproducible else None, "zeros": zeros}
