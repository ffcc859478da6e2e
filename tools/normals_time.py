"""Timing of a view's geometry outputs (csrc/normals.hip) on one GPU: bench.py's frame -- 800 x 800 rays, 64 + 128 samples, 800^2
position planes -- through eval_nerf (colour only, today's frame) and through eval_geometry (depth, acc and the normal map), three
alternations in one process, minima reported; writes profiles/normals.txt (appended below the accuracy figures kept there by hand).

    python tools/normals_time.py [--out FILE] [--res R] [--parent TREE]

  live share    the samples of the fine pass with a nonzero weight, the only ones the density gradient is evaluated on
  split         device-event time of the three stages of ops.normals_of_pass over the frame's slabs: decode forward with gates (both decoders:
                the density-only kernel that would skip the colour decoder is the follow-up), rows backward, normals_composite; the rest of
                eval_geometry is the two passes with weights and depth, the live list and the live points
  --parent TREE a checkout of the parent commit with its library built: its eval_nerf on the same frame, in a child process of its own"""
import os
import subprocess
import sys

ARGV = sys.argv[1:]
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)

PARENT_CODE = """
import sys, numpy as np, torch
sys.path.insert(0, %r)
import nvsr_amd
from bench import make_synthetic_scene, render_options
R = %d
mc, mf, sid, pose = make_synthetic_scene("cuda:0", 800, 32, seed=0, theta=30.0)
opts, scfg = render_options(64, 128)
focal = 0.5 * R / np.tan(0.5 * 0.6911112)
ro, rd = nvsr_amd.nerf_helpers.get_ray_bundle(R, R, focal, pose)
f = lambda: nvsr_amd.train_utils.eval_nerf(R, R, focal, mc, mf, ro, rd, opts, scene_id=sid, scene_config=scfg)
f(); torch.cuda.synchronize()
best = 1e9
for _ in range(3):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(3):
        f()
    b.record(); b.synchronize()
    best = min(best, a.elapsed_time(b) / 3)
print("PARENT_MS %%.3f" %% best)
"""


def main():
    import numpy as np
    import torch

    import nvsr_amd
    from bench import make_synthetic_scene, render_options

    out_path = ARGV[ARGV.index("--out") + 1] if "--out" in ARGV else os.path.join(HERE, "profiles", "normals.txt")
    R = int(ARGV[ARGV.index("--res") + 1]) if "--res" in ARGV else 800
    parent = ARGV[ARGV.index("--parent") + 1] if "--parent" in ARGV else None
    assert torch.cuda.is_available(), "normals_time.py measures on a GPU; there is nothing to report without one"
    dev = "cuda:0"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def timed(fn, reps=3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / reps

    tu, ops = nvsr_amd.train_utils, nvsr_amd.ops
    mc, mf, sid, pose = make_synthetic_scene(dev, 800, 32, seed=0, theta=30.0)
    opts, scfg = render_options(64, 128)
    focal = 0.5 * R / np.tan(0.5 * 0.6911112)
    ro, rd = nvsr_amd.nerf_helpers.get_ray_bundle(R, R, focal, pose)
    fns = {"eval_nerf": lambda: tu.eval_nerf(R, R, focal, mc, mf, ro, rd, opts, scene_id=sid, scene_config=scfg),
           "eval_geometry": lambda: tu.eval_geometry(R, R, focal, mc, mf, ro, rd, opts, sid, scene_config=scfg)}
    say("geometry outputs of a view: %d x %d rays, 64 + 128 samples, 800^2 position planes, arithmetic %s (%s)" % (
        R, R, nvsr_amd.capi.get_decoder_arithmetic(), torch.cuda.get_device_name(0)))
    for f in fns.values():
        f()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(3):
        for k, f in fns.items():
            ms[k].append(timed(f))
    ms = {k: min(v) for k, v in ms.items()}
    say("  eval_nerf      (rgb)                      %8.2f ms   %5.2f M rays/s" % (ms["eval_nerf"], R * R / ms["eval_nerf"] / 1e3))
    say("  eval_geometry  (depth, acc, normal)       %8.2f ms   %5.2f M rays/s   (%.2f x eval_nerf)" % (
        ms["eval_geometry"], R * R / ms["eval_geometry"] / 1e3, ms["eval_geometry"] / ms["eval_nerf"]))

    # the split: one more frame with device events around the three stages of every slab
    timers, live, real = {}, [], ops.normals_of_pass

    def spied(planes, consts, packed, packed_bwd, rays, z, weights, arith, **kw):
        live.append((int((weights != 0).sum()), weights.numel()))
        return real(planes, consts, packed, packed_bwd, rays, z, weights, arith, timers=timers, **kw)

    ops.normals_of_pass = spied
    try:
        total = timed(fns["eval_geometry"], 1)
    finally:
        ops.normals_of_pass = real
    torch.cuda.synchronize()
    stage = {k: sum(a.elapsed_time(b) for a, b in v) for k, v in timers.items()}
    n_live, n_all = sum(a for a, _ in live), sum(b for _, b in live)
    say("  live share of the fine pass: %d of %d samples = %.2f %%, %d slab(s) of at most 2^20 points" % (
        n_live, n_all, 100.0 * n_live / n_all, len(timers["composite"])))
    rest = total - sum(stage.values())
    say("  one frame with events: %.2f ms = decode forward (both decoders) %.2f + rows backward %.2f + normals_composite %.2f + the rest "
        "(two passes with weights and depth, live list, live points) %.2f" % (total, stage["decode"], stage["rows"], stage["composite"], rest))
    say("  of the %.2f ms on the live samples: decode %.0f %%, rows %.0f %%, composite %.0f %%" % (
        sum(stage.values()), *(100.0 * stage[k] / sum(stage.values()) for k in ("decode", "rows", "composite"))))
    if parent:
        env = dict(os.environ, PYTHONPATH=os.path.abspath(parent))
        out = subprocess.run([sys.executable, "-c", PARENT_CODE % (os.path.abspath(parent), R)], cwd=os.path.abspath(parent), env=env,
                             capture_output=True, text=True, timeout=600)
        got = [l for l in out.stdout.splitlines() if l.startswith("PARENT_MS")]
        if out.returncode or not got:
            say("  parent commit's eval_nerf: the child process failed (%d): %s" % (out.returncode, out.stderr.strip()[-300:]))
        else:
            p = float(got[0].split()[1])
            say("  parent commit's eval_nerf (its own tree and library, a process of its own)   %8.2f ms   (this tree: %+.2f %%)" % (
                p, 100.0 * (ms["eval_nerf"] - p) / p))
    with open(out_path, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
