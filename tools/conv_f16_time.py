"""The SR convolutions in 'f16' (one f16 limb, NVSR_ARITH_F16) beside 'f16x2' (two limbs, the default): time and quality, one GPU, one process;
writes profiles/conv_f16_ab.txt.

    python tools/conv_f16_time.py [--out FILE] [--note TEXT ...]

The two arithmetics alternate three times; every figure is the median of the three rounds with min .. max.
(a) the SR stage of bench.py's scene: 3 planes of 48 channels, 200^2 -> 800^2, PlanesSR(EDSR 256 x 32), one batched pass (--workload sr)
(b) one plane's full-region training forward + backward (PlanesSR.forward in training mode on the whole 200^2 plane, gradients to the EDSR
    weights and the plane)
(c) the joint refine iteration of bench.py --workload refine (what = ['LR_planes', 'decoder', 'SR'], 4096 rays of an 800 x 800 view, 64 + 64
    samples), built from bench.py's helpers, with the SR network's arithmetic switched
Quality (figures, not thresholds): PSNR of the super-resolved planes of (a) against the 'bf16x3' planes (peak = the range of those planes), and
of one 200 x 200 frame rendered through the planes of each arithmetic against the frame through the 'bf16x3' planes (peak 1).
--note: lines copied into the file as given (the parent commit's bench.py figures of the same job, taken outside this process)."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import numpy as np
    import torch

    import nvsr_amd
    from bench import CAMERA_ANGLE_X, make_synthetic_scene, render_options

    argv = sys.argv[1:]
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(ROOT, "profiles", "conv_f16_ab.txt")
    notes = [argv[i + 1] for i, a in enumerate(argv) if a == "--note"]
    assert torch.cuda.is_available(), "conv_f16_time.py measures on a GPU; there is nothing to report without one"
    dev = "cuda:0"
    M, T = nvsr_amd.models, nvsr_amd.training
    MODES = ("f16x2", "f16")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def timed(fn, reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / reps

    def alternate(fns, warm, reps):
        """fns: {mode: callable} -> {mode: [ms of round 0, 1, 2]}"""
        for f in fns.values():
            for _ in range(warm):
                f()
        torch.cuda.synchronize()
        ms = {k: [] for k in fns}
        for _ in range(3):
            for k, f in fns.items():
                ms[k].append(timed(f, reps))
        return ms

    def report(title, ms):
        say(title)
        for k in ms:
            say("    %-6s median %.3f ms  (min %.3f .. max %.3f)" % (k, statistics.median(ms[k]), min(ms[k]), max(ms[k])))
        a, b = statistics.median(ms["f16x2"]), statistics.median(ms["f16"])
        say("    'f16' takes %.3f of 'f16x2' (%+.3f ms): %s" % (b / a, b - a, "faster" if b < a else "NOT faster"))

    def psnr(a, b, peak):
        mse = float(((a.double() - b.double()) ** 2).mean())
        return float("inf") if mse == 0 else 10.0 * np.log10(peak * peak / mse)

    say("SR convolutions: 'f16' (1 f16 limb, 1 MFMA per product block) beside 'f16x2' (2 limbs, 3 MFMAs); %s" % torch.cuda.get_device_name(0))
    for n in notes:
        say(n)

    # ---- (a) the SR stage --------------------------------------------------------------------------------------------------------------------
    torch.manual_seed(0)
    sr = M.PlanesSR(M.EDSR, 4, 48, 48, {"model": {"hidden_size": 256, "n_blocks": 32}}, "bilinear").to(dev)
    sr.eval()
    names = ["p0", "p1", "p2"]
    for n in names:
        sr.set_LR_plane(torch.randn(1, 48, 200, 200, device=dev) * 0.5, id=n, save_interpolated=False)

    def stage(mode):
        def one():
            sr.inner_model.arithmetic = mode
            sr.clear_SR_planes()
            with torch.no_grad():
                sr.super_resolve_many(names)
        return one
    report("(a) SR stage: 3 planes 48 x 200^2 -> 800^2, EDSR 256 x 32, one batched pass; 3 alternated rounds of 5", alternate({m: stage(m) for m in MODES}, 2, 5))
    # quality: the planes, and a 200 x 200 frame through the planes of each arithmetic
    mc, mf, sid, pose = make_synthetic_scene(dev, 200, 32, seed=0, theta=30.0)
    Hf = Wf = 200
    focal = 0.5 * Wf / np.tan(0.5 * CAMERA_ANGLE_X)
    ro, rd = nvsr_amd.nerf_helpers.get_ray_bundle(Hf, Wf, focal, pose)
    opts, scfg = render_options(64, 128)

    def quality(label):
        planes = {}
        for m in MODES + ("bf16x3",):
            stage(m)()
            planes[m] = torch.cat([sr.SR_planes[n] for n in names])
        peak = float(planes["bf16x3"].max() - planes["bf16x3"].min())
        lr_up = torch.cat([sr.interpolate_LR(n) for n in names])
        say("    %s: the network's share of the planes: rms(plane - bilinear(LR)) / rms(plane) = %.2e" % (
            label, float((planes["bf16x3"] - lr_up).double().pow(2).mean().sqrt() / planes["bf16x3"].double().pow(2).mean().sqrt())))
        say("      PSNR of the super-resolved planes against the 'bf16x3' planes (peak = their range %.3f): %s" % (
            peak, ", ".join("'%s' %.2f dB" % (m, psnr(planes[m], planes["bf16x3"], peak)) for m in MODES)))
        del planes, lr_up
        saved = dict(sr.LR_planes)
        sr.clear_SR_planes(all_planes=True)
        mf.assign_SR_model(sr, SR_viewdir=False)
        mf.assign_LR_planes()
        frames = {}
        for m in MODES + ("bf16x3",):
            sr.inner_model.arithmetic = m
            sr.clear_SR_planes()
            with torch.no_grad():
                frames[m] = nvsr_amd.train_utils.eval_nerf(Hf, Wf, focal, mc, mf, ro, rd, opts, scene_id=sid, scene_config=scfg)[3].clone()
        say("      PSNR of a 200 x 200 frame (64 + 128 samples) rendered through them against the frame through the 'bf16x3' planes (peak 1): %s" % (
            ", ".join("'%s' %.2f dB" % (m, psnr(frames[m], frames["bf16x3"], 1.0)) for m in MODES)))
        sr.clear_SR_planes(all_planes=True)
        sr.LR_planes = saved

    say("    quality (figures, not thresholds)")
    quality("weights as initialised (PlanesSR starts at 1/10 of He scale)")
    with torch.no_grad():
        for p_ in sr.parameters():
            p_.mul_(10.0)
    sr.inner_model.invalidate()
    quality("weights x 10 (activations O(1) through the 66 layers, as in the full-size parity tests)")
    with torch.no_grad():
        for p_ in sr.parameters():
            p_.mul_(0.1)
    sr.inner_model.invalidate()
    del mc, mf
    sr.clear_SR_planes(all_planes=True)

    # ---- (b) one plane, training forward + backward ------------------------------------------------------------------------------------------
    sr.train()
    plane = torch.nn.Parameter(torch.randn(1, 48, 200, 200, device=dev) * 0.5)
    sr.set_LR_plane(plane, id="t0", save_interpolated=False)
    g_out = torch.randn(1, 48, 800, 800, device=dev)

    def train_plane(mode):
        def one():
            sr.inner_model.arithmetic = mode
            out = sr("t0")
            torch.autograd.grad([out], [plane] + list(sr.inner_model.conv_parameters()), [g_out])
        return one
    report("(b) one plane's full-region training forward + backward (48 x 200^2 -> 800^2, gradients to the plane and the EDSR weights); 3 alternated rounds of 3",
           alternate({m: train_plane(m) for m in MODES}, 1, 3))
    del plane, g_out
    sr.clear_SR_planes(all_planes=True)
    torch.cuda.empty_cache()

    # ---- (c) the joint refine iteration of bench.py --workload refine -------------------------------------------------------------------------
    R, N, Nc, Nf = 200, 4096, 64, 64
    what = {"LR_planes", "decoder", "SR"}
    mc, mf, sid, pose = make_synthetic_scene(dev, R, 32, seed=0, theta=30.0, channels_last=True)
    torch.manual_seed(1)
    sr = M.PlanesSR(M.EDSR, 4, 48, 48, {"model": {"hidden_size": 256, "n_blocks": 32}}, "bilinear").to(dev)
    for m in (mc, mf):
        for n, p in m.named_parameters():
            p.requires_grad_("rot_mats" not in n)
        m.train()
    sr.train()
    mf.detach_LR_planes = False
    mf.assign_SR_model(sr, SR_viewdir=False)
    mf.assign_LR_planes()
    H = W = 800
    focal = 0.5 * W / np.tan(0.5 * CAMERA_ANGLE_X)
    opts, scfg = render_options(Nc, Nf, perturb=True, noise=0.2)
    g = torch.Generator(device=dev).manual_seed(100)
    target = torch.rand(H, W, 3, device=dev, generator=g)
    dec = list({id(p): p for m in (mc, mf) for p in m.decoder_parameters()}.values())
    opt = torch.optim.Adam(dec, lr=5e-4, fused=True)
    popt = torch.optim.Adam(list(mc.planes_.values()), lr=5e-4, fused=True)
    sropt = torch.optim.Adam(list(sr.parameters()), lr=5e-5, fused=True)
    step = T.TrainStep(mc, mf, opts, what, optimizer=opt, SR_optimizer=sropt, planes_optimizer=popt, SR_model=sr, sr_loss="fine",
                       pixel_sampler=T.DevicePixelSampler(seed=100))
    it = [0]

    def refine(mode):
        def one():
            sr.inner_model.arithmetic = mode
            rnd = dict(t_rand=torch.rand(N, Nc, device=dev, generator=g), u=torch.rand(N, Nf, device=dev, generator=g),
                       noise_coarse=torch.empty(N, Nc, device=dev).normal_(0.0, 0.2, generator=g),
                       noise_fine=torch.empty(N, Nc + Nf, device=dev).normal_(0.0, 0.2, generator=g))
            step(it[0], target, pose, H, W, focal, 1, sid, scfg, N, sr_iter=True, randoms=rnd)
            it[0] += 1
        return one
    report("(c) joint refine iteration (bench.py --workload refine: 4096 rays of an 800 x 800 view, 64 + 64 samples, EDSR 256 x 32 on the three regions); "
           "3 alternated rounds of 3", alternate({m: refine(m) for m in MODES}, 2, 3))
    assert all(bool(torch.isfinite(p).all()) for p in sr.parameters()), "the refine iterations left non-finite SR weights"

    # ---- the small end-to-end case of tests/test_conv_f16.py: what the arithmetic costs against the float64 oracle (computed on the CPU) ----------
    try:
        from conv_f16_ref import E2E_EREF as e
        say("tests/test_conv_f16.py, EDSR(48 -> 48, hidden 128, 2 blocks, x2) on three regions of 12^2 planes: e_ref = rms(reference - oracle) / rms(oracle) "
            "of the float64 restatement of 'f16' (CPU): output %.4e, LR-plane gradient %.4e, weight gradients per layer %s"
            % (e["out"], e["d_lr"], ", ".join("%.4e" % v for v in e["dw"])))
    except ImportError:
        pass
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
