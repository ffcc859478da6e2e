"""Timing of the generic decoder geometries' evaluation in 'f16x2' (csrc/generic_fused_limb.hip) against the two exact-f32 routes -- fused
(csrc/generic_fused.hip) and layered (csrc/generic.hip) -- on one GPU, one process, routes alternated three times; writes
profiles/generic_limb_ab.txt.  The sibling of tools/generic_fused_time.py: the same three geometries, points and frame.

    python tools/generic_limb_time.py [--out FILE] [--append] [--label TEXT] [--root TREE]

Per geometry (200^2 position planes, a 32^2 view plane, seeded weights):
  decode   model(x) on 2^22 points under no_grad: ms (median, min..max of the three rounds) and the algorithmic TFLOP/s of the geometry's layers
  frame    eval_nerf on 400 x 400 rays, 64 + 128 samples
  error    rms error of the decode against the float64 restatement (oracle/generic_decoder.py) on 4096 of the points, per route
--root TREE imports the package from another checkout (the parent commit's, built there): a tree without the limb route times the two f32
routes alone -- run it with --append --label parent in the same job and read its rows beside this tree's."""
import os
import statistics
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
ROUTES = {"f16x2-fused": ("1", "f16x2"), "f32-fused": ("1", None), "f32-layered": ("0", None)}       # NVSR_GENERIC_FUSED, model.arithmetic


def main():
    import numpy as np
    import torch

    import nvsr_amd
    from bench import pose_spherical, render_options

    out_path = ARGV[ARGV.index("--out") + 1] if "--out" in ARGV else os.path.join(HERE, "profiles", "generic_limb_ab.txt")
    label = ARGV[ARGV.index("--label") + 1] if "--label" in ARGV else "this tree"
    assert torch.cuda.is_available(), "generic_limb_time.py measures on a GPU; there is nothing to report without one"
    dev = "cuda:0"
    M = nvsr_amd.models
    has_limb = hasattr(M.TwoDimPlanesModel, "generic_arithmetic")
    routes = [r for r in ROUTES if has_limb or ROUTES[r][1] is None]
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

    def route(name, models, fn):
        def run():
            os.environ["NVSR_GENERIC_FUSED"] = ROUTES[name][0]        # (read at every call)
            for m in models:
                m.arithmetic = ROUTES[name][1]
            with torch.no_grad():
                return fn()
        return run

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
            m.eval()
        return mc, mf, sid, box

    def flop_per_point(m):
        return 2 * sum(p.numel() for p in m.decoder_parameters() if p.dim() == 2)

    say("generic geometries, evaluation: %s -- %s" % (" / ".join(routes), label))
    P = 1 << 22
    g = torch.Generator().manual_seed(1)
    x = torch.cat([torch.rand(P, 3, generator=g) * 8.4 - 4.2, torch.randn(P, 3, generator=g)], -1).to(dev)
    H = W = 400
    focal = 0.5 * W / np.tan(0.5 * 0.6911112)
    pose = torch.from_numpy(pose_spherical(30.0, -30.0, 4.0)).to(dev)
    opts, scfg = render_options(64, 128)
    for name, n_pos, kw in GEOMETRIES:
        mc, mf, sid, box = scene(n_pos, kw)
        ro, rd = nvsr_amd.nerf_helpers.get_ray_bundle(H, W, focal, pose)
        decode = {r: route(r, (mf,), lambda: mf(x)) for r in routes}
        frame = {r: route(r, (mc, mf), lambda: nvsr_amd.train_utils.eval_nerf(H, W, focal, mc, mf, ro, rd, opts, scene_id=sid, scene_config=scfg)[3]) for r in routes}
        say("%s (%.3f MFLOP per point)" % (name, flop_per_point(mf) / 1e6))
        if has_limb:
            from oracle.generic_decoder import decode as decode64
            sd = {k: v.detach().cpu().numpy() for k, v in mf.state_dict().items()}
            pl = [mf.planes_[M.get_plane_name(sid, d)].detach().cpu().numpy() for d in range(n_pos + 1)]
            n = 4096
            ref = decode64(sd, pl, box.numpy(), x[:n].cpu().numpy(), **kw)
            for r in routes:
                err = decode[r]()[:n].double().cpu().numpy() - ref
                say("    error vs float64, %d points  %-12s rms %.3g (rgb) %.3g (sigma), of output rms %.3g / %.3g" % (
                    n, r, np.sqrt((err[:, :3] ** 2).mean()), np.sqrt((err[:, 3] ** 2).mean()), np.sqrt((ref[:, :3] ** 2).mean()), np.sqrt((ref[:, 3] ** 2).mean())))
        for what, fns, reps, work in (("decode 2^22 points", decode, 3, flop_per_point(mf) * P), ("frame 400 x 400, 64 + 128", frame, 1, None)):
            ms = alternate(fns, reps)
            for r in routes:
                med = statistics.median(ms[r])
                say("    %-26s %-12s median %9.3f ms  (min %9.3f, max %9.3f)%s" % (
                    what, r, med, min(ms[r]), max(ms[r]), "" if work is None else "   %6.2f TFLOP/s" % (work / med / 1e9)))
            if has_limb:
                best = min(statistics.median(ms[r]) for r in routes if r != "f16x2-fused")
                limb = statistics.median(ms["f16x2-fused"])
                spread = max(max(v) - min(v) for v in ms.values())
                say("    %-26s better f32 route / f16x2-fused = %.2f  (difference %+.3f ms, largest spread of a route %.3f ms)" % (what, best / limb, best - limb, spread))
        del mc, mf, decode, frame
        torch.cuda.empty_cache()
    os.environ.pop("NVSR_GENERIC_FUSED", None)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "a" if "--append" in ARGV else "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
