"""Timing of the low-rank plane operators (csrc/lowrank.hip) on one GPU, one process; writes profiles/lowrank_time.txt.

    python tools/lowrank_time.py [--out FILE]

(a) the 4096-ray, 64 + 64 planes-only TrainStep at R = 200 (Feature_Planes_Only.yml's shape), three scenes alternated three times:
      dense     dense [1,48,200,200] planes (what the step was before low-rank planes existed)
      lowrank   planes_rank_ratio 0.1 (r = 20) on torch.ops.nvsr.lowrank_planes / lowrank_planes_backward
      torch     the same low-rank scene with gen_plane replaced, in this tool only, by a stock-torch composition (a batched matrix product
                of the two factor slices; the NCHW result then goes through plane_to_channel_last, autograd does the backward)
    per variant: ms per step (device events around 20 steps; median and min..max of the three rounds) and the kernels of one step (torch.profiler).
(b) generating three 800^2 planes at r = 80 once (evaluation), operators vs the torch composition, and the bytes/s of the generate kernel
    (factors read + planes written) beside plane_to_channel_last on the same three planes (planes read + written).
(c) the backward of (b): lowrank_planes_backward on three channels_last 800^2 gradients vs the composition's forward + autograd."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import numpy as np
    import torch

    import nvsr_amd
    from bench import render_options

    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "lowrank_time.txt")
    assert torch.cuda.is_available(), "lowrank_time.py measures on a GPU; there is nothing to report without one"
    dev = "cuda:0"
    M = nvsr_amd.models
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

    def kernels(fn):
        try:
            from torch.profiler import ProfilerActivity, profile
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                fn()
                torch.cuda.synchronize()
            return sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA") and "emcpy" not in e.name and "emset" not in e.name)
        except Exception as e:                       # (a profiler that does not work here: say so, never guess)
            return "not measured (%s)" % type(e).__name__

    def composed_plane(F, r):
        """U V^T per channel with stock torch: an NCHW-contiguous [1,C,R,R] that the step then re-lays out"""
        return F[..., :r] @ F[..., r:].transpose(-1, -2)

    def use_torch_composition(model, cache):
        """gen_plane of `model` replaced by the composition (one product per plane and step, shared through `cache` like generated_planes)"""
        def gen_plane(plane_name, detach=False):
            r = model._rank_of(plane_name)
            if r is None:
                out = model.planes_[plane_name]
            else:
                out = cache.get(plane_name)
                if out is None:
                    out = cache[plane_name] = composed_plane(model.planes_[plane_name], r)
            if detach:
                out = out.detach()
            return out
        model.gen_plane = gen_plane

    def lowrank_scene(plane_res, rank, seed):
        """the synthetic scene with its three position planes stored as rank-`rank` factors whose product has the dense scene's spread"""
        from bench import make_synthetic_scene
        mc, mf, sid, pose = make_synthetic_scene(dev, plane_res=plane_res, view_res=32, seed=seed)
        names = [M.get_plane_name(sid, d) for d in range(4)]
        gcpu = torch.Generator().manual_seed(seed + 100)
        planes = {n: torch.nn.Parameter(((0.49 / rank) ** 0.25 * torch.randn(1, 48, plane_res, 2 * rank, generator=gcpu)).to(dev)) for n in names[:3]}
        planes[names[3]] = mc.planes_[names[3]]
        planes, shared = torch.nn.ParameterDict(planes), {}
        for m in (mc, mf):
            m.planes_, m.plane_rank, m.generated_planes = planes, {n: rank for n in names[:3]}, shared
            m.invalidate()
        return mc, mf, sid, pose

    # ---- (a) training step ---------------------------------------------------------------------------------------------------------------
    H = W = 100
    focal = 0.5 * W / np.tan(0.5 * 0.6911112)
    N, R, r = 4096, 200, 20
    g = torch.Generator(device=dev).manual_seed(5)
    img = torch.rand(H, W, 3, device=dev, generator=g)
    rnd = dict(t_rand=torch.rand(N, 64, device=dev, generator=g), u=torch.rand(N, 64, device=dev, generator=g),
               noise_coarse=0.2 * torch.randn(N, 64, device=dev, generator=g), noise_fine=0.2 * torch.randn(N, 128, device=dev, generator=g))
    opts, scfg = render_options(64, 64, perturb=True, noise=0.2)

    def variant(kind):
        if kind == "dense":
            from bench import make_synthetic_scene
            mc, mf, sid, pose = make_synthetic_scene(dev, plane_res=R, view_res=32, seed=0, channels_last=True)
        else:
            mc, mf, sid, pose = lowrank_scene(R, r, seed=0)
        cache = {}
        if kind == "torch":
            for m in (mc, mf):
                use_torch_composition(m, cache)
        for m in (mc, mf):
            for n, p in m.named_parameters():
                p.requires_grad_("planes_" in n)
            m.train()
        popt = torch.optim.Adam(list(mc.planes_.values()), lr=4e-3, fused=True, capturable=True)
        step = nvsr_amd.training.TrainStep(mc, mf, opts, {"LR_planes"}, planes_optimizer=popt, pixel_sampler=nvsr_amd.training.DevicePixelSampler(seed=77))
        it = [0]

        def one():
            cache.clear()                      # (the reference clears its generated planes at every PlanesOptimizer step)
            step.run(it[0], img, pose, H, W, focal, 1, sid, scfg, N, randoms=rnd)
            it[0] += 1
        return one

    kinds = ["dense", "lowrank", "torch"]
    steps = {k: variant(k) for k in kinds}
    for k in kinds:
        for _ in range(5):
            steps[k]()
    torch.cuda.synchronize()
    ms = {k: [] for k in kinds}
    for _ in range(3):
        for k in kinds:
            ms[k].append(timed(steps[k], 20))
    say("(a) planes-only TrainStep, 4096 rays, 64 + 64 samples, R = 200 (low-rank: r = 20); ms per step, 3 alternated rounds of 20 steps")
    for k in kinds:
        say("    %-8s median %.3f ms  (min %.3f, max %.3f)   kernels per step: %s" % (k, statistics.median(ms[k]), min(ms[k]), max(ms[k]), kernels(steps[k])))
    say("    low-rank over dense: %+.3f ms; operators vs torch composition: %+.3f ms" % (
        statistics.median(ms["lowrank"]) - statistics.median(ms["dense"]), statistics.median(ms["lowrank"]) - statistics.median(ms["torch"])))

    # ---- (b) one-off generation ----------------------------------------------------------------------------------------------------------
    R, r, C = 800, 80, 48
    gc = torch.Generator().manual_seed(1)
    Fs = [(0.3 * torch.randn(1, C, R, 2 * r, generator=gc)).to(dev) for _ in range(3)]
    with torch.no_grad():
        ops_gen = lambda: torch.ops.nvsr.lowrank_planes(Fs, [r] * 3)
        mats = lambda: [composed_plane(F, r) for F in Fs]
        torch_gen = lambda: [torch.ops.nvsr.plane_to_channel_last(p) for p in mats()]
        dense = mats()
        relayout = lambda: [torch.ops.nvsr.plane_to_channel_last(p) for p in dense]
        a, b = ops_gen(), torch_gen()
        err = max(float((x.permute(0, 2, 3, 1)[0] - y).abs().max()) for x, y in zip(a, b))
        fns = {"operators": ops_gen, "torch": torch_gen, "relayout": relayout}
        for f in fns.values():
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        t = {k: [] for k in fns}
        for _ in range(3):
            for k, f in fns.items():
                t[k].append(timed(f, 10))
    plane_bytes, factor_bytes = 3 * R * R * C * 4, 3 * C * R * 2 * r * 4
    say("(b) three 800^2 planes from r = 80 factors, once; ms, 3 alternated rounds of 10 (max |operators - torch| = %.2e)" % err)
    for k, label in (("operators", "lowrank_planes (1 launch)"), ("torch", "matmul + plane_to_channel_last"), ("relayout", "plane_to_channel_last alone")):
        say("    %-32s median %.3f ms  (min %.3f, max %.3f)" % (label, statistics.median(t[k]), min(t[k]), max(t[k])))
    say("    generate kernel: %.0f GB/s (%.1f MB factors read + %.1f MB planes written); plane_to_channel_last: %.0f GB/s (%.1f MB read + as many written)" % (
        (plane_bytes + factor_bytes) / statistics.median(t["operators"]) / 1e6, factor_bytes / 1e6, plane_bytes / 1e6,
        2 * plane_bytes / statistics.median(t["relayout"]) / 1e6, plane_bytes / 1e6))
    # ---- (c) the backward of (b) -------------------------------------------------------------------------------------------------------------
    Gs = [torch.randn(1, C, R, R, generator=gc).to(dev).contiguous(memory_format=torch.channels_last) for _ in range(3)]
    Fg = [F.clone().requires_grad_() for F in Fs]

    def torch_bwd():
        planes = [composed_plane(F, r) for F in Fg]
        torch.autograd.grad(planes, Fg, Gs)
    with torch.no_grad():
        ops_bwd = lambda: torch.ops.nvsr.lowrank_planes_backward(Gs, Fs, [r] * 3)
    fns = {"operators": ops_bwd, "torch": torch_bwd}
    for f in fns.values():
        for _ in range(2):
            f()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(3):
        for k, f in fns.items():
            t[k].append(timed(f, 5))
    say("(c) gradients of the three 800^2 planes back to the r = 80 factors; ms, 3 alternated rounds of 5")
    say("    lowrank_planes_backward (1 launch)            median %.3f ms  (min %.3f, max %.3f)" % (statistics.median(t["operators"]), min(t["operators"]), max(t["operators"])))
    say("    matmul forward + autograd (channels_last G)   median %.3f ms  (min %.3f, max %.3f)" % (statistics.median(t["torch"]), min(t["torch"]), max(t["torch"])))
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
