"""Timing of the fused TRAINING route of the generic decoder geometries for a frozen decoder (csrc/generic_fused_bwd.hip,
NVSR_GENERIC_TRAIN_FUSED=1) against the layered route (csrc/generic.hip, NVSR_GENERIC_TRAIN_FUSED=0) on one GPU, one process, routes
alternated three times; writes profiles/generic_train_ab.txt.

    python tools/generic_train_time.py [--out FILE] [--parent TREE]
    python tools/generic_train_time.py --root TREE --append --label TEXT        (what --parent runs)

Per geometry (200^2 position planes, a 32^2 view plane, seeded weights, the decoder's parameters frozen, the planes trainable):
  fwd+bwd    model(x) on 2^19 points in train() and backward() of a fixed cotangent: ms (median, min..max of the three rounds)
  iteration  run_one_iter_of_nerf on 4 096 rays at 64 + 64 samples, an MSE loss on both passes and backward()
the float atomics' bytes per point of both routes, computed from the geometry, and the largest relative L2 distance of the two routes'
plane gradients.
--parent TREE: a checkout of the PARENT commit, built there.  It is timed in a second process of the same job on the layered route (--root
imports the package from that tree; a tree without generic_train_route() runs the layered route alone), and every ratio is quoted against
it: no speed-up is claimed against this tree's own layered route alone."""
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
    ("hidden 64, avg / concat_pos", 3, dict(dec_channels=64, proj_combination="avg", viewdir_proj_combination="concat_pos", skip_connect_every=3)),
    ("hidden 128, sum / sum", 3, dict(dec_channels=128, proj_combination="sum", skip_connect_every=3)),
    ("hidden 256, concat over 4 planes", 4, dict(dec_channels=256, proj_combination="concat", viewdir_proj_combination="concat", skip_connect_every=3)),
]
HANDLE = "NVSR_GENERIC_TRAIN_FUSED"


def atomic_bytes_per_point(geometry, n_pos, taps=4):
    """(layered, fused) bytes of float atomics per point with every plane's gradient wanted and `taps` taps of nonzero weight: the layered
    scatter issues one dword per (decoder-input column, plane it feeds, tap); the fused one one dword per (plane, channel, tap)"""
    C, Cv, _, _, _, _, proj, view = geometry
    xd = C * n_pos                                           # every column of Xd reaches one plane ('concat') or all of them ('sum' / 'avg')
    xr = (n_pos * C + Cv) if view >= 3 else (C * n_pos + Cv)
    return 4 * taps * (xd + xr), 4 * taps * (n_pos * C + Cv)


def main():
    import numpy as np
    import torch

    import nvsr_amd
    from bench import pose_spherical, render_options

    out_path = ARGV[ARGV.index("--out") + 1] if "--out" in ARGV else os.path.join(HERE, "profiles", "generic_train_ab.txt")
    label = ARGV[ARGV.index("--label") + 1] if "--label" in ARGV else "this tree"
    assert torch.cuda.is_available(), "generic_train_time.py measures on a GPU; there is nothing to report without one"
    dev = "cuda:0"
    M = nvsr_amd.models
    has_fused = hasattr(M.TwoDimPlanesModel, "generic_train_route")
    routes = ("fused", "layered") if has_fused else ("layered",)
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

    say("generic geometries, planes-only training: fused (csrc/generic_fused_bwd.hip, %s=1) against layered (%s=0, csrc/generic.hip) -- %s%s" % (
        HANDLE, HANDLE, label, "" if has_fused else " (no fused training route in this tree: the layered route alone)"))
    P = 1 << 19
    g = torch.Generator().manual_seed(1)
    x = torch.cat([torch.rand(P, 3, generator=g) * 8.4 - 4.2, torch.randn(P, 3, generator=g)], -1).to(dev)
    G = torch.randn(P, 4, generator=g).to(dev)
    H = W = 64
    focal = 0.5 * W / np.tan(0.5 * 0.6911112)
    pose = torch.from_numpy(pose_spherical(30.0, -30.0, 4.0)).to(dev)
    opts, scfg = render_options(64, 64)
    target = (torch.rand(H * W, 3, generator=g) * 0.5 + 0.25).to(dev)
    for name, n_pos, kw in GEOMETRIES:
        mc, mf, sid, plist = scene(n_pos, kw)
        ro, rd = nvsr_amd.nerf_helpers.get_ray_bundle(H, W, focal, pose)
        batch = torch.stack([ro.reshape(-1, 3), rd.reshape(-1, 3)], 0)

        def route(r, fn):
            def run():
                os.environ[HANDLE] = "1" if r == "fused" else "0"            # (read at every call)
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

        os.environ.pop(HANDLE, None)
        taken = mf.generic_train_route() if has_fused else "layered"
        os.environ[HANDLE] = "1"
        forced = mf.generic_train_route() if has_fused else "layered"
        shapes = (("fwd+bwd 2^19 points", {r: route(r, fwd_bwd) for r in routes}, 3), ("iteration 4096 rays, 64 + 64", {r: route(r, iteration) for r in routes}, 2))
        dist = 0.0
        if has_fused:
            for _, fns, _ in shapes:
                a, b = fns["fused"](), fns["layered"]()
                dist = max([dist] + [float((u - v).norm() / v.norm()) for u, v in zip(a, b)])
        al, af = atomic_bytes_per_point(mf.generic_geometry(), n_pos)
        say("%s (route taken by default: %s, with %s=1: %s; largest relative L2 distance of the routes' plane gradients: %.2g; float atomics per point, "
            "bilinear: layered %d B, fused %d B)" % (name, taken, HANDLE, forced, dist, al, af))
        for what, fns, reps in shapes:
            ms = alternate(fns, reps)
            for r in routes:
                med = statistics.median(ms[r])
                result["%s | %s | %s" % (name, what, r)] = (med, min(ms[r]), max(ms[r]))
                say("    %-30s %-8s median %9.3f ms  (min %9.3f, max %9.3f)" % (what, r, med, min(ms[r]), max(ms[r])))
            if has_fused:
                f, l = statistics.median(ms["fused"]), statistics.median(ms["layered"])
                spread = max(max(v) - min(v) for v in ms.values())
                say("    %-30s layered / fused = %.2f  (difference %+.3f ms, largest spread of a route %.3f ms)" % (what, l / f, l - f, spread))
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
        rows = ["against the parent commit's layered route (the baseline; spread = the larger max - min of the two rows):"]
        for key, (med, lo, hi) in result.items():
            name, what, r = key.split(" | ")
            b = base.get("%s | %s | layered" % (name, what))
            if b is not None:
                rows.append("    %-34s %-30s %-8s parent layered / this = %.2f  (%9.3f ms against %9.3f ms, spread %.3f ms)" % (
                    name, what, r, b[0] / med, b[0], med, max(hi - lo, b[2] - b[1])))
        print("\n".join(rows), flush=True)
        with open(out_path, "a") as f:
            f.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
