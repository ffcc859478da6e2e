"""Timing of planes-only training of the generic decoder geometries in 'f16x2' (csrc/generic_fused_bwd_limb.hip, model.train_arithmetic =
'f16x2' with NVSR_GENERIC_TRAIN_FUSED=1) against this tree's two exact-f32 routes (fused: csrc/generic_fused_bwd.hip; layered:
csrc/generic.hip) on one GPU, one process, routes alternated three times; writes profiles/generic_train_limb_ab.txt.

    python tools/generic_train_limb_time.py [--out FILE] [--parent TREE]
    python tools/generic_train_limb_time.py --root TREE --append --label TEXT        (what --parent runs)

Per geometry (200^2 position planes, a 32^2 view plane, seeded weights, the decoder's parameters frozen, the planes trainable):
  fwd+bwd    model(x) on 2^19 points in train() and backward() of a fixed cotangent: ms (median, min..max of the three rounds)
  iteration  run_one_iter_of_nerf on 4 096 rays at 64 + 64 samples, an MSE loss on both passes and backward()
and the largest relative L2 distance of the limb route's plane gradients from the f32 fused route's on the 2^19 points (every ReLU gate that
the limb forward and the f32 forward decide differently -- a pre-activation within rounding of zero -- counts in it: a discontinuity).
--parent TREE: a checkout of the PARENT commit, built there.  Its two f32 routes are timed in a second process of the same job (--root imports
the package from that tree; a tree without train_arithmetic runs the f32 routes alone); the limb route is judged against the BETTER of them:
a width counts as faster only where parent's better median - limb's median exceeds the larger spread (max - min) of the two rows, in both
shapes.  GENERIC_TRAIN_LIMB_DEFAULT_HIDDEN (models.py) is set from the last lines of the file."""
import json
import os
import statistics
import subprocess
import sys

ARGV = sys.argv[1:]
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.abspath(ARGV[ARGV.index("--root") + 1]) if "--root" in ARGV else HERE
sys.path.insert(0, ROOT)

GEOMETRIES = [
    ("hidden 64, avg / concat_pos", 64, 3, dict(dec_channels=64, proj_combination="avg", viewdir_proj_combination="concat_pos", skip_connect_every=3)),
    ("hidden 128, sum / sum", 128, 3, dict(dec_channels=128, proj_combination="sum", skip_connect_every=3)),
    ("hidden 256, concat over 4 planes", 256, 4, dict(dec_channels=256, proj_combination="concat", viewdir_proj_combination="concat", skip_connect_every=3)),
]
HANDLE = "NVSR_GENERIC_TRAIN_FUSED"
SHAPES = ("fwd+bwd 2^19 points", "iteration 4096 rays, 64 + 64")


def main():
    import numpy as np
    import torch

    import nvsr_amd
    from bench import pose_spherical, render_options

    out_path = ARGV[ARGV.index("--out") + 1] if "--out" in ARGV else os.path.join(HERE, "profiles", "generic_train_limb_ab.txt")
    label = ARGV[ARGV.index("--label") + 1] if "--label" in ARGV else "this tree"
    assert torch.cuda.is_available(), "generic_train_limb_time.py measures on a GPU; there is nothing to report without one"
    dev = "cuda:0"
    M = nvsr_amd.models
    has_limb = hasattr(M.TwoDimPlanesModel, "generic_train_arithmetic")
    routes = (("limb",) if has_limb else ()) + ("fused", "layered")
    lines, result = [], {}

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
        return ms

    def scene(n_pos, kw, seed=0):
        torch.manual_seed(seed)
        np.random.seed(seed)
        sid = M.get_scene_id("lego", 1, (200, 32))
        mc = M.TwoDimPlanesModel(use_viewdirs=True, align_corners=True, num_planes_or_rot_mats=n_pos, **kw)
        mf = M.TwoDimPlanesModel(use_viewdirs=True, align_corners=True, num_planes_or_rot_mats=mc.rot_mats(), **kw)
        mc, mf = mc.to(dev), mf.to(dev)
        planes = torch.nn.ParameterDict({M.get_plane_name(sid, d): torch.nn.Parameter(0.5 * torch.randn(1, 48, 200 if d < n_pos else 32, 200 if d < n_pos else 32, device=dev))
                                         for d in range(n_pos + 1)})
        box = torch.tensor([[-4.0, -4, -4, -np.pi, -np.pi / 2], [4, 4, 4, np.pi, np.pi / 2]], dtype=torch.float64)
        for m in (mc, mf):
            m.planes_, m.box_coords = planes, {sid: box}
            m.set_cur_scene_id(sid)
            m.train()
            for p in m.decoder_parameters():
                p.requires_grad_(False)
        return mc, mf, sid, list(planes.values())

    say("generic geometries, planes-only training: 'f16x2' by name (csrc/generic_fused_bwd_limb.hip, train_arithmetic = 'f16x2', %s=1) against the "
        "exact-f32 routes fused (csrc/generic_fused_bwd.hip, %s=1) and layered (csrc/generic.hip, %s=0) -- %s%s" % (
            HANDLE, HANDLE, HANDLE, label, "" if has_limb else " (no train_arithmetic in this tree: the f32 routes alone)"))
    P = 1 << 19
    g = torch.Generator().manual_seed(1)
    x = torch.cat([torch.rand(P, 3, generator=g) * 8.4 - 4.2, torch.randn(P, 3, generator=g)], -1).to(dev)
    G = torch.randn(P, 4, generator=g).to(dev)
    H = W = 64
    focal = 0.5 * W / np.tan(0.5 * 0.6911112)
    pose = torch.from_numpy(pose_spherical(30.0, -30.0, 4.0)).to(dev)
    opts, scfg = render_options(64, 64)
    target = (torch.rand(H * W, 3, generator=g) * 0.5 + 0.25).to(dev)
    for name, hidden, n_pos, kw in GEOMETRIES:
        mc, mf, sid, plist = scene(n_pos, kw)
        ro, rd = nvsr_amd.nerf_helpers.get_ray_bundle(H, W, focal, pose)
        batch = torch.stack([ro.reshape(-1, 3), rd.reshape(-1, 3)], 0)

        def route(r, fn):
            def run():
                os.environ[HANDLE] = "0" if r == "layered" else "1"            # (read at every call)
                for m in (mc, mf):
                    m.train_arithmetic = "f16x2" if r == "limb" else None
                for p in plist:
                    p.grad = None
                fn()
                return [p.grad for p in plist]
            return run

        def fwd_bwd():
            mf(x).backward(G)

        def iteration():
            rgb_c, _, _, rgb_f, *_ = nvsr_amd.train_utils.run_one_iter_of_nerf(H, W, focal, mc, mf, batch, opts, sid, mode="train", scene_config=scfg)
            (((rgb_c - target) ** 2).mean() + ((rgb_f - target) ** 2).mean()).backward()

        shapes = ((SHAPES[0], {r: route(r, fwd_bwd) for r in routes}, 3), (SHAPES[1], {r: route(r, iteration) for r in routes}, 2))
        dist = 0.0
        if has_limb:
            os.environ[HANDLE] = "1"
            mf.train_arithmetic = "f16x2"
            assert mf.generic_train_arithmetic() == "f16x2", name
            a, b = shapes[0][1]["limb"](), shapes[0][1]["fused"]()          # (the fixed points: in an iteration the fine samples move with the coarse weights)
            dist = max(float((u - v).norm() / v.norm()) for u, v in zip(a, b))
            say("%s (largest relative L2 distance of the limb route's plane gradients from the f32 fused route's on the 2^19 points: %.2g)" % (name, dist))
        else:
            say(name)
        for what, fns, reps in shapes:
            ms = alternate(fns, reps)
            for r in routes:
                med = statistics.median(ms[r])
                result["%s | %s | %s" % (name, what, r)] = (med, min(ms[r]), max(ms[r]))
                say("    %-30s %-8s median %9.3f ms  (min %9.3f, max %9.3f)" % (what, r, med, min(ms[r]), max(ms[r])))
        del mc, mf, plist, shapes
        torch.cuda.empty_cache()
    os.environ.pop(HANDLE, None)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "a" if "--append" in ARGV else "w") as f:
        f.write("\n".join(lines) + "\n")
    print("RESULT " + json.dumps(result), flush=True)

    if "--parent" in ARGV:
        tree = os.path.abspath(ARGV[ARGV.index("--parent") + 1])
        done = subprocess.run([sys.executable, os.path.abspath(__file__), "--root", tree, "--append", "--label", "the parent commit's library", "--out", out_path],
                              capture_output=True, text=True, env={k: v for k, v in os.environ.items() if k != HANDLE})
        sys.stdout.write(done.stdout)
        if done.returncode != 0:
            sys.stderr.write(done.stderr)
            sys.exit(done.returncode)
        base = json.loads([l for l in done.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
        rows = ["the limb route against the BETTER f32 route of the parent commit (spread = the larger max - min of the two rows):"]
        faster = []
        for name, hidden, _, _ in GEOMETRIES:
            wins = []
            for what in SHAPES:
                mine = result["%s | %s | limb" % (name, what)]
                best = min((base["%s | %s | %s" % (name, what, r)] + [r] for r in ("fused", "layered")), key=lambda v: v[0])
                spread = max(mine[2] - mine[1], best[2] - best[1])
                wins.append(best[0] - mine[0] > spread)
                rows.append("    %-34s %-30s parent %-7s / limb = %.2f  (%9.3f ms against %9.3f ms, spread %.3f ms)%s" % (
                    name, what, best[3], best[0] / mine[0], best[0], mine[0], spread, "" if wins[-1] else "  -- not faster by more than the spread"))
            if all(wins):
                faster.append(hidden)
        rows.append("widths at which the limb route beats the parent's better f32 route by more than the larger spread in both shapes: %s" % (faster or "none"))
        widths = [h for _, h, _, _ in GEOMETRIES]
        run = [h for h in widths if h in faster]
        contiguous = run == widths[widths.index(run[0]):widths.index(run[-1]) + 1] if run else False
        span = (run[0], run[-1]) if contiguous else ((run[0], run[0]) if run else None)      # (a gap between measured widths: the lowest alone)
        rows.append("GENERIC_TRAIN_LIMB_DEFAULT_HIDDEN = %r" % (span,))
        print("\n".join(rows), flush=True)
        with open(out_path, "a") as f:
            f.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
