"""Timing of the fused evaluation route of the generic decoder geometries (csrc/generic_fused.hip) against the layered route
(csrc/generic.hip, NVSR_GENERIC_FUSED=0) on one GPU, one process, routes alternated three times; writes profiles/generic_fused_ab.txt.

    python tools/generic_fused_time.py [--out FILE] [--append] [--label TEXT] [--root TREE]

Per geometry (200^2 position planes, a 32^2 view plane, seeded weights):
  decode   model(x) on 2^22 points under no_grad: ms (median, min..max of the three rounds) and the algorithmic TFLOP/s of the geometry's
           layers (2 x in x out per layer and head and point) beside the 157.3 TFLOP/s f32 MFMA peak
  frame    eval_nerf on 400 x 400 rays, 64 + 128 samples
and whether the two routes' outputs have the same bits.
--root TREE imports the package from another checkout (the parent commit's, built there): a tree without the fused operator runs the layered
route under both labels, which is the check that moving the shared code into generic_core.h left the layered route's time alone -- run it
with --append --label parent in the same job and read its 'layered' rows beside this tree's."""
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


def main():
    import numpy as np
    import torch

    import nvsr_amd
    from bench import pose_spherical, render_options

    out_path = ARGV[ARGV.index("--out") + 1] if "--out" in ARGV else os.path.join(HERE, "profiles", "generic_fused_ab.txt")
    label = ARGV[ARGV.index("--label") + 1] if "--label" in ARGV else "this tree"
    assert torch.cuda.is_available(), "generic_fused_time.py measures on a GPU; there is nothing to report without one"
    dev = "cuda:0"
    M = nvsr_amd.models
    has_fused = hasattr(M.TwoDimPlanesModel, "generic_route")
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

    def route(name, fn):
        def run():
            os.environ["NVSR_GENERIC_FUSED"] = "1" if name == "fused" else "0"        # (read at every call)
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
        return mc, mf, sid

    def flop_per_point(m):
        return 2 * sum(p.numel() for p in m.decoder_parameters() if p.dim() == 2)

    say("generic geometries, evaluation: fused (one launch, csrc/generic_fused.hip, NVSR_GENERIC_FUSED=1) against layered (NVSR_GENERIC_FUSED=0, csrc/generic.hip) -- %s%s" % (
        label, "" if has_fused else " (no fused route in this tree: both labels run the layered route)"))
    P = 1 << 22
    g = torch.Generator().manual_seed(1)
    x = torch.cat([torch.rand(P, 3, generator=g) * 8.4 - 4.2, torch.randn(P, 3, generator=g)], -1).to(dev)
    H = W = 400
    focal = 0.5 * W / np.tan(0.5 * 0.6911112)
    pose = torch.from_numpy(pose_spherical(30.0, -30.0, 4.0)).to(dev)
    opts, scfg = render_options(64, 128)
    for name, n_pos, kw in GEOMETRIES:
        mc, mf, sid = scene(n_pos, kw)
        ro, rd = nvsr_amd.nerf_helpers.get_ray_bundle(H, W, focal, pose)
        os.environ.pop("NVSR_GENERIC_FUSED", None)
        with torch.no_grad():
            taken = mf.generic_route() if has_fused else "layered"
        decode = {r: route(r, lambda: mf(x)) for r in ("fused", "layered")}
        frame = {r: route(r, lambda: nvsr_amd.train_utils.eval_nerf(H, W, focal, mc, mf, ro, rd, opts, scene_id=sid, scene_config=scfg)[3]) for r in ("fused", "layered")}
        same = all(torch.equal(fns["fused"]().view(torch.int32), fns["layered"]().view(torch.int32)) for fns in (decode, frame))
        say("%s (route taken by default: %s; outputs bit-equal: %s; %.3f MFLOP per point)" % (name, taken, same, flop_per_point(mf) / 1e6))
        for what, fns, reps, work in (("decode 2^22 points", decode, 3, flop_per_point(mf) * P), ("frame 400 x 400, 64 + 128", frame, 1, None)):
            ms = alternate(fns, reps)
            for r in ("fused", "layered"):
                med = statistics.median(ms[r])
                say("    %-26s %-8s median %9.3f ms  (min %9.3f, max %9.3f)%s" % (
                    what, r, med, min(ms[r]), max(ms[r]), "" if work is None else "   %6.2f TFLOP/s = %4.1f %% of the 157.3 f32 MFMA peak" % (work / med / 1e9, work / med / 1e9 / 1.573)))
            f, l = statistics.median(ms["fused"]), statistics.median(ms["layered"])
            spread = max(max(v) - min(v) for v in ms.values())
            say("    %-26s layered / fused = %.2f  (difference %+.3f ms, largest spread of a route %.3f ms)" % (what, l / f, l - f, spread))
        del mc, mf, decode, frame
        torch.cuda.empty_cache()
    os.environ.pop("NVSR_GENERIC_FUSED", None)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "a" if "--append" in ARGV else "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
