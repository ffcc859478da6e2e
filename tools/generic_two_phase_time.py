"""Timing of the generic decoder geometries' evaluation frame in two phases (density phase, compositing weights, live list, colour phase on
the live samples: csrc/generic_fused*.hip per phase, csrc/generic_live.hip) against the frame in one phase, on one GPU, one process, routes
alternated three times; writes profiles/generic_two_phase_ab.txt.  The sibling of tools/generic_limb_time.py: the same three geometries and
the same frame.

    python tools/generic_two_phase_time.py [--out FILE] [--append] [--label TEXT] [--root TREE]

Per geometry (200^2 position planes, a 32^2 view plane, seeded weights) and arithmetic ('f32', 'f16x2'), for the decoders as initialised and --
where their live share is near 1 -- with fc_alpha's bias shifted so that about a third of the coarse samples have a positive sigma (labelled):
  frame    eval_nerf on 400 x 400 rays, 64 + 128 samples, NVSR_GENERIC_TWO_PHASE=0 against =1 (NVSR_GENERIC_FUSED=1): ms (median, min..max of the
           three rounds), the difference against the larger of the two routes' spreads, and the frame's live share, coarse and fine
  launches the fine pass by hand from the operators: density phase, compositor for the weights, live list, colour phase, final compositor,
           beside the one-launch decode
  sweep    on 2^22 points: the one-launch decode against density phase + live list + colour phase on an ascending random list of share 1.0,
           0.5, 0.33, 0.1, and the share at which the two cost the same (linear between the measured shares)
--root TREE imports the package from another checkout (the parent commit's, built there): a tree without the phases times the one-phase frame
alone -- run it with --append --label parent in the same job and read its rows beside this tree's one-phase rows."""
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
SHARES = (1.0, 0.5, 0.33, 0.1)


def main():
    import numpy as np
    import torch

    import nvsr_amd
    from bench import pose_spherical, render_options

    out_path = ARGV[ARGV.index("--out") + 1] if "--out" in ARGV else os.path.join(HERE, "profiles", "generic_two_phase_ab.txt")
    label = ARGV[ARGV.index("--label") + 1] if "--label" in ARGV else "this tree"
    assert torch.cuda.is_available(), "generic_two_phase_time.py measures on a GPU; there is nothing to report without one"
    dev = "cuda:0"
    M, nv = nvsr_amd.models, torch.ops.nvsr
    has_phases = hasattr(M.TwoDimPlanesModel, "generic_frame_route")
    lines = []
    os.environ["NVSR_GENERIC_FUSED"] = "1"

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
        with torch.no_grad():
            for f in fns.values():
                f()
            torch.cuda.synchronize()
            ms = {k: [] for k in fns}
            for _ in range(3):
                for k, f in fns.items():
                    ms[k].append(timed(f, reps))
        return ms

    def row(what, name, v):
        say("    %-30s %-22s median %9.3f ms  (min %9.3f, max %9.3f)" % (what, name, statistics.median(v), min(v), max(v)))

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

    say("generic geometries, evaluation frame: one phase / two phases -- %s" % label)
    P = 1 << 22
    g = torch.Generator().manual_seed(1)
    x = torch.cat([torch.rand(P, 3, generator=g) * 8.4 - 4.2, torch.randn(P, 3, generator=g)], -1).to(dev)
    lists = {}
    for s in SHARES:
        idx = torch.sort(torch.randperm(P, generator=g)[:int(round(s * P))]).values.to(torch.int32).to(dev)
        lists[s] = (idx, torch.tensor([idx.numel()], dtype=torch.int32, device=dev))
    H = W = 400
    focal = 0.5 * W / np.tan(0.5 * 0.6911112)
    pose = torch.from_numpy(pose_spherical(30.0, -30.0, 4.0)).to(dev)
    opts, scfg = render_options(64, 128)
    for name, n_pos, kw in GEOMETRIES:
        for arith in ("f32", "f16x2"):
            mc, mf, sid = scene(n_pos, kw)
            mc.arithmetic = mf.arithmetic = None if arith == "f32" else "f16x2"
            ro, rd = nvsr_amd.nerf_helpers.get_ray_bundle(H, W, focal, pose)
            rays = nvsr_amd.train_utils.pack_rays(ro.reshape(-1, 3), rd.reshape(-1, 3), 2.0, 6.0, H, W, focal, no_ndc=True)
            N = rays.shape[0]

            def frame_of(two_phase):
                def run():
                    os.environ["NVSR_GENERIC_TWO_PHASE"] = two_phase      # (read at every call)
                    return nvsr_amd.train_utils.eval_nerf(H, W, focal, mc, mf, ro, rd, opts, scene_id=sid, scene_config=scfg)[3]
                return run

            def passes():
                """the one-phase passes by hand -> (fine points, z_f, raw_f, w_c, w_f)"""
                os.environ["NVSR_GENERIC_TWO_PHASE"] = "0"
                z_c = nv.coarse_z(rays, 64, False, None)
                w_c = nv.composite_rays(mc(nv.ray_points(rays, z_c)).reshape(N, 64, 4), z_c, rays, None, False, True)[3]
                z_f = nv.importance_resample(z_c, w_c, 128, None)
                pts = nv.ray_points(rays, z_f)
                raw_f = mf(pts).reshape(N, 192, 4)
                return pts, z_f, raw_f, w_c, nv.composite_rays(raw_f, z_f, rays, None, False, True)[3]

            share_of = lambda w: float((w != 0).float().mean())
            for variant in ("as initialised", "fc_alpha bias shifted: about a third of the coarse samples live"):
                with torch.no_grad():
                    if variant != "as initialised":
                        z_c = nv.coarse_z(rays, 64, False, None)
                        os.environ["NVSR_GENERIC_TWO_PHASE"] = "0"
                        for m in (mc, mf):
                            sigma = m(nv.ray_points(rays, z_c))[:, 3]
                            shift = -float(torch.quantile(sigma[::37].float(), 2.0 / 3))
                            dict(m.named_parameters())["fc_alpha.0.bias"].add_(shift)
                    pts, z_f, raw_f, w_c, w_f = passes()
                    shares = (share_of(w_c), share_of(w_f))
                say("%s, %s, %s: live share coarse %.3f, fine %.3f" % (name, arith, variant, shares[0], shares[1]))
                fns = {"one phase": frame_of("0")}
                if has_phases:
                    fns["two phases"] = frame_of("1")
                ms = alternate(fns, 1)
                for k in fns:
                    row("frame 400 x 400, 64 + 128", k, ms[k])
                if has_phases:
                    one, two = statistics.median(ms["one phase"]), statistics.median(ms["two phases"])
                    spread = max(max(v) - min(v) for v in ms.values())
                    say("    %-30s one phase / two phases = %.3f  (difference %+.3f ms, larger spread of the two routes %.3f ms: %s)" % (
                        "frame 400 x 400, 64 + 128", one / two, one - two, spread,
                        "two phases faster" if one - two > spread else "one phase faster" if two - one > spread else "within the spread"))
                if has_phases:
                    with torch.no_grad():
                        raw = mf.density_field(pts)
                        index, count = nv.generic_live_list(w_f)
                    launches = {"one-launch decode": lambda: mf(pts), "density phase": lambda: mf.density_field(pts),
                                "compositor for weights": lambda: nv.composite_rays(raw.reshape(N, 192, 4), z_f, rays, None, False, True),
                                "live list": lambda: nv.generic_live_list(w_f), "colour phase": lambda: mf.colour_field_(raw, pts, index, count),
                                "final compositor": lambda: nv.composite_rays(raw.reshape(N, 192, 4), z_f, rays, None, False, False)}
                    os.environ["NVSR_GENERIC_TWO_PHASE"] = "0"
                    ms = alternate(launches, 1)
                    for k in launches:
                        row("fine pass, %d samples" % (N * 192), k, ms[k])
                    del raw, index, count
                del pts, z_f, raw_f, w_c, w_f
                if shares[1] < 0.8:
                    break                   # (the decoders as initialised already leave dead samples: no shifted variant)
            if has_phases:
                with torch.no_grad():
                    raw = mf.density_field(x)
                wsyn = torch.rand(P, device=dev)
                fns = {"one-launch decode": lambda: mf(x), "density phase": lambda: mf.density_field(x), "live list": lambda: nv.generic_live_list(wsyn)}
                for s in SHARES:
                    fns["colour phase, share %.2f" % s] = lambda s=s: mf.colour_field_(raw, x, lists[s][0], lists[s][1])
                os.environ["NVSR_GENERIC_TWO_PHASE"] = "0"
                ms = alternate(fns, 2)
                for k in fns:
                    row("sweep, 2^22 points", k, ms[k])
                med = {k: statistics.median(v) for k, v in ms.items()}
                fixed = med["density phase"] + med["live list"]
                total = [(s, fixed + med["colour phase, share %.2f" % s]) for s in SHARES]
                say("    sweep, 2^22 points             two phases / one launch: " + ", ".join("%.3f at share %.2f" % (t / med["one-launch decode"], s) for s, t in total))
                even = None
                for (s1, t1), (s0, t0) in zip(total, total[1:]):          # shares descend
                    if (t1 - med["one-launch decode"]) * (t0 - med["one-launch decode"]) <= 0 and t1 != t0:
                        even = s0 + (s1 - s0) * (med["one-launch decode"] - t0) / (t1 - t0)
                say("    sweep, 2^22 points             break-even live share: %s" % (
                    "%.2f" % even if even is not None else "above 1.0 (two phases cheaper at every share)" if total[0][1] < med["one-launch decode"]
                    else "below %.2f (one launch cheaper at every measured share)" % SHARES[-1]))
                del raw, wsyn
            del mc, mf
            torch.cuda.empty_cache()
    os.environ.pop("NVSR_GENERIC_FUSED", None)
    os.environ.pop("NVSR_GENERIC_TWO_PHASE", None)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "a" if "--append" in ARGV else "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
