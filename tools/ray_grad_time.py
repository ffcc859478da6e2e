"""Timing of the ray / camera-pose gradient of a training iteration (csrc/ray_grad.hip) on one GPU, device events, three
alternations, minima reported; appends to profiles/ray_grad.txt (below the accuracy figures kept there by hand).

    python tools/ray_grad_time.py [--out FILE] [--rays N] [--parent TREE]
    python tools/ray_grad_time.py --root TREE --frozen-only --label TEXT        (what --parent runs)

A 4 096-ray, 64 + 64 sample TrainStep iteration on bench.py's synthetic scene, planes + decoder training:
  iteration   with a pose that requires a gradient (the rows route once per pass + the new kernels) and with a frozen pose (today's entries in
              today's order), per arithmetic; and the frozen pose in deterministic mode -- the same ordered route without the new kernels, which
              separates the price of the ordered scatter from the price of the ray gradient
  --parent TREE: a checkout of the PARENT commit, built there.  Its frozen-pose iteration -- the only one it has -- is timed in a second process
              of the same job, on its own package and its own library, and reported next to this tree's.  Without --parent the baseline is
              THIS tree's frozen-pose route and the output says so.
  kernels     the four new entries alone on seeded inputs of the iteration's shapes"""
import os
import sys

ARGV = sys.argv[1:]
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.abspath(ARGV[ARGV.index("--root") + 1]) if "--root" in ARGV else HERE
sys.path.insert(0, ROOT)


def main():
    import numpy as np
    import torch

    import nvsr_amd as hip
    from bench import make_synthetic_scene, render_options

    out_path = ARGV[ARGV.index("--out") + 1] if "--out" in ARGV else os.path.join(HERE, "profiles", "ray_grad.txt")
    N = int(ARGV[ARGV.index("--rays") + 1]) if "--rays" in ARGV else 4096
    assert torch.cuda.is_available(), "ray_grad_time.py measures on a GPU; there is nothing to report without one"
    dev = "cuda:0"
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

    def alternate(fns, reps):
        for f in fns.values():
            f()
        torch.cuda.synchronize()
        ms = {k: [] for k in fns}
        for _ in range(3):
            for k, f in fns.items():
                ms[k].append(timed(f, reps))
        return {k: min(v) for k, v in ms.items()}

    Nc = Nf = 64
    H = W = 128
    focal = 0.5 * W / np.tan(0.5 * 0.6911112)
    say("ray / pose gradient of a training iteration: %d rays, %d + %d samples, planes + decoder, 800^2 position planes (%s)" % (
        N, Nc, Nf, torch.cuda.get_device_name(0)))
    gen = torch.Generator(device=dev).manual_seed(3)
    img = torch.rand(H, W, 3, device=dev, generator=gen)

    def iteration(arithmetic, pose_grad, deterministic):
        mc, mf, sid, pose = make_synthetic_scene(dev, seed=3)
        for m in (mc, mf):
            m.arithmetic = arithmetic
            for n, p in m.named_parameters():
                p.requires_grad_("rot_mats" not in n)
            m.train()
        opts, scfg = render_options(Nc, Nf, perturb=True, noise=0.2)
        planes = list(mc.planes_.values())
        dec = list({id(p): p for m in (mc, mf) for p in m.decoder_parameters()}.values())
        step = hip.training.TrainStep(mc, mf, opts, {"LR_planes", "decoder"}, optimizer=torch.optim.Adam(dec, lr=1e-4),
                                      planes_optimizer=torch.optim.Adam(planes, lr=1e-4), pixel_sampler=hip.training.DevicePixelSampler(seed=5),
                                      deterministic=deterministic)
        pose = pose.detach().clone().requires_grad_(pose_grad)
        rnd = dict(t_rand=torch.rand(N, Nc, device=dev, generator=gen), u=torch.rand(N, Nf, device=dev, generator=gen),
                   noise_coarse=0.2 * torch.randn(N, Nc, device=dev, generator=gen), noise_fine=0.2 * torch.randn(N, Nc + Nf, device=dev, generator=gen))
        it = [0]

        def run():
            pose.grad = None
            step(it[0], img, pose, H, W, focal, 1, sid, scfg, N, randoms=rnd)
            it[0] += 1
        return run

    if "--frozen-only" in ARGV:
        label = ARGV[ARGV.index("--label") + 1] if "--label" in ARGV else ROOT
        for arithmetic in ("f16x2", "bf16x3"):
            res = alternate({"frozen": iteration(arithmetic, False, False)}, 5)
            say("  iteration, %-6s   frozen pose %7.3f ms   on %s" % (arithmetic, res["frozen"], label))
        with open(out_path, "a") as f:
            f.write("\n".join(lines[1:]) + "\n")
        return
    for arithmetic in ("f16x2", "bf16x3"):
        res = alternate({"grad": iteration(arithmetic, True, False), "frozen": iteration(arithmetic, False, False),
                         "frozen_det": iteration(arithmetic, False, True)}, 5)
        say("  iteration, %-6s   pose.requires_grad %7.3f ms   frozen pose %7.3f ms (x%.2f)   frozen pose, deterministic mode %7.3f ms   "
            "(the ray gradient alone: +%.3f ms)" % (arithmetic, res["grad"], res["frozen"], res["grad"] / res["frozen"], res["frozen_det"],
                                                     res["grad"] - res["frozen_det"]))

    with open(out_path, "a") as f:
        f.write("\n".join(lines) + "\n")
    del lines[:]
    if "--parent" in ARGV:
        import subprocess
        tree = os.path.abspath(ARGV[ARGV.index("--parent") + 1])
        subprocess.run([sys.executable, os.path.abspath(__file__), "--root", tree, "--frozen-only", "--label", "the parent commit's package and library",
                        "--rays", str(N), "--out", out_path], check=True)
    else:
        say("  (no --parent: the frozen-pose column above is THIS tree's route, not a run of the parent commit's library)")
    nv = torch.ops.nvsr
    r = lambda *s: torch.randn(*s, device=dev, generator=gen)
    for S in (Nc, Nc + Nf):
        rays, z, d_points, d_viewdir, raw, noise, g_raw, d_rays = r(N, 11), r(N, S), r(N * S, 3), r(N, 3), r(N, S, 4), r(N, S), r(N, S, 4), r(N, 11)
        ms = alternate({"k": lambda: nv.rays_grad(rays, z, d_points, d_viewdir, raw, noise, g_raw, d_rays, True)}, 50)["k"]
        moved = N * S * (4 + 12 + 16 + 4 + 16) + N * (44 * 3 + 12)
        say("  rays_grad, S = %3d (operator call)            %7.4f ms   %6.0f GB/s over %.1f MB of touched lines" % (S, ms, moved / ms / 1e6, moved / 1e6))
    d_rays, v = r(N, 11), r(N, 3)
    ro, rd = r(N, 3), r(N, 3)
    rc = torch.randint(0, H, (N, 2), device=dev, dtype=torch.int32)
    res = alternate({"pack": lambda: nv.pack_rays_backward(d_rays, v, True), "ndc": lambda: nv.ndc_rays_backward(H, W, focal, 1.0, ro, rd, ro, rd),
                     "bundle": lambda: nv.ray_bundle_backward(H, W, focal, focal, 0.0, rc, 0, ro, rd)}, 50)
    say("  pack_rays_backward %.4f ms   ndc_rays_backward %.4f ms   ray_bundle_backward (two launches + its workspace) %.4f ms   (operator calls: "
        "host-bound at this size)" % (res["pack"], res["ndc"], res["bundle"]))
    with open(out_path, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
