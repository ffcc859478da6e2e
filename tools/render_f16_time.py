"""The render pass in 'f16' (one f16 limb, NVSR_ARITH_F16) beside 'f16x2' (two limbs, the default): time and quality of bench.py's frame, one
GPU, one process; writes profiles/render_f16_ab.txt.

    python tools/render_f16_time.py [--out FILE] [--res N] [--plane-res N] [--note TEXT ...] [--append FILE ...]

The frame is the benchmark's: 800 x 800 rays, 64 + 128 samples, planes 800^2 (bench.make_synthetic_scene), rendered by eval_nerf with the models'
arithmetic switched.  The two arithmetics alternate three times; every figure is the median of the three rounds with min .. max.
Quality (figures, not thresholds): PSNR of each arithmetic's fine frame against the 'f32' frame (peak 1).
--note: lines copied into the file as given (bench.py figures of the parent commit and of this tree, the ratios tests/test_render_f16.py
printed -- taken outside this process, in the same job); --append: text files copied in behind them (a per-kernel table of a rocprofv3
--kernel-trace --stats run of this tool, when one was taken)."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import numpy as np
    import torch

    import nvsr_amd
    from bench import CAMERA_ANGLE_X, make_synthetic_scene, render_options

    argv = sys.argv[1:]
    opt = lambda name, dflt: argv[argv.index(name) + 1] if name in argv else dflt
    out_path = opt("--out", os.path.join(ROOT, "profiles", "render_f16_ab.txt"))
    res, plane_res = int(opt("--res", 800)), int(opt("--plane-res", 800))
    notes = [argv[i + 1] for i, a in enumerate(argv) if a == "--note"]
    appended = [argv[i + 1] for i, a in enumerate(argv) if a == "--append"]
    assert torch.cuda.is_available(), "render_f16_time.py measures on a GPU; there is nothing to report without one"
    dev = "cuda:0"
    MODES = ("f16x2", "f16")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    mc, mf, sid, pose = make_synthetic_scene(dev, plane_res, 32, seed=0, theta=30.0)
    H = W = res
    focal = 0.5 * W / np.tan(0.5 * CAMERA_ANGLE_X)
    opts, scfg = render_options(64, 128)

    def frame(mode):
        def one():
            mc.arithmetic = mf.arithmetic = mode
            with torch.no_grad():
                ro, rd = nvsr_amd.nerf_helpers.get_ray_bundle(H, W, focal, pose)          # (ray generation is part of bench.py's step)
                return nvsr_amd.train_utils.eval_nerf(H, W, focal, mc, mf, ro, rd, opts, scene_id=sid, scene_config=scfg)
        return one

    def timed(fn, reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / reps

    say("render pass: 'f16' (1 f16 limb, 1 MFMA per product block) beside 'f16x2' (2 limbs, 3 MFMAs); %s" % torch.cuda.get_device_name(0))
    say("frame: %d x %d rays, 64 + 128 samples, planes %d^2 (bench.make_synthetic_scene), eval_nerf; 3 alternated rounds of 5 frames" % (H, W, plane_res))
    fns = {m: frame(m) for m in MODES}
    for f in fns.values():
        for _ in range(2):
            f()
    torch.cuda.synchronize()
    ms = {m: [] for m in MODES}
    for _ in range(3):
        for m, f in fns.items():
            ms[m].append(timed(f, 5))
    for m in MODES:
        say("    %-6s median %.3f ms  (min %.3f .. max %.3f)" % (m, statistics.median(ms[m]), min(ms[m]), max(ms[m])))
    a, b = statistics.median(ms["f16x2"]), statistics.median(ms["f16"])
    say("    'f16' takes %.3f of 'f16x2' (%+.3f ms per frame): %s" % (b / a, b - a, "faster" if b < a else "NOT faster"))

    def psnr(x, y):
        mse = float(((x.double() - y.double()) ** 2).mean())
        return float("inf") if mse == 0 else 10.0 * np.log10(1.0 / mse)

    frames = {m: frame(m)()[3].clone() for m in MODES + ("bf16x3", "f32")}
    flag = nvsr_amd.capi.range_flag()
    say("    PSNR of the fine frame against the 'f32' frame (peak 1; figures, not thresholds): %s; range flag %d"
        % (", ".join("'%s' %.2f dB" % (m, psnr(frames[m], frames["f32"])) for m in MODES + ("bf16x3",)), int(flag.word)))
    say("    largest pixel difference to the 'f32' frame: %s" % ", ".join("'%s' %.3e" % (m, float((frames[m] - frames["f32"]).abs().max())) for m in MODES + ("bf16x3",)))
    mc.arithmetic = mf.arithmetic = None
    for n in notes:
        say(n)
    for path in appended:
        with open(path) as f:
            for ln in f.read().splitlines():
                say(ln)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
