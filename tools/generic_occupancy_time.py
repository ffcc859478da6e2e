"""Timing of the generic decoder geometries' evaluation frame with an occupancy grid (models.build_occupancy on a generic geometry: the keep mask
of the sample points, their ascending list, the density phase over the list -- csrc/occupancy.hip, csrc/generic_live.hip, GF_DENSITY_LIST of
csrc/generic_fused*.hip -- then the weights, the live list and the colour phase as in a frame in two phases) against the same frame without a
grid, on one GPU, one process, routes alternated three times; writes profiles/generic_occupancy_ab.txt.  The sibling of
tools/generic_two_phase_time.py: the same frame, two of its geometries.

    python tools/generic_occupancy_time.py [--out FILE] [--append] [--label TEXT] [--root TREE]

Scene: 200^2 position planes that are ZERO outside their central block (texels 75 .. 124 of 200 along either axis: |n| < 0.25), a 32^2 view
plane, seeded weights; fc_alpha's weights are negated where the seeded decoder answers the planes with less density, and its bias puts the empty
space's sigma at -q / 2, q = the median of what the planes add to sigma at the coarse samples they reach.  Three axis-aligned planes with a block each fill three bars through the box; the grid is build_occupancy's default (128^3
cells, 2^3 probes, threshold 0, one round of dilation).  Per geometry (hidden 64 and 128) and arithmetic ('f32', 'f16x2'):
  shares   kept share of the coarse and the fine pass (the samples whose cell is set, or outside the box), and the live share of the weights
  frame    eval_nerf on 400 x 400 rays, 64 + 128 samples: no grid in one phase (NVSR_GENERIC_TWO_PHASE=0), no grid in two phases (=1), with the
           grid: ms (median, min..max of the three rounds), the ratios, and the difference against the larger spread
  launches the fine pass by hand: density phase on every sample beside keep mask + kept list + density phase over the list
--root TREE imports the package from another checkout (the parent commit's, built there): a tree without density_field_kept times the grid-less
frames alone -- run it with --append --label parent in the same job and read its rows beside this tree's grid-less rows."""
import os
import statistics
import sys

ARGV = sys.argv[1:]
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.abspath(ARGV[ARGV.index("--root") + 1]) if "--root" in ARGV else HERE
sys.path.insert(0, ROOT)

GEOMETRIES = [
    ("hidden 64, avg / concat_pos", dict(dec_channels=64, proj_combination="avg", viewdir_proj_combination="concat_pos", skip_connect_every=3)),
    ("hidden 128, sum / sum", dict(dec_channels=128, proj_combination="sum", skip_connect_every=3)),
]
RES, BLOCK = 200, (75, 125)


def main():
    import numpy as np
    import torch

    import nvsr_amd
    from bench import pose_spherical, render_options

    out_path = ARGV[ARGV.index("--out") + 1] if "--out" in ARGV else os.path.join(HERE, "profiles", "generic_occupancy_ab.txt")
    label = ARGV[ARGV.index("--label") + 1] if "--label" in ARGV else "this tree"
    assert torch.cuda.is_available(), "generic_occupancy_time.py measures on a GPU; there is nothing to report without one"
    dev = "cuda:0"
    M, nv = nvsr_amd.models, torch.ops.nvsr
    has_grid = hasattr(M.TwoDimPlanesModel, "density_field_kept")
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
        say("    %-30s %-34s median %9.3f ms  (min %9.3f, max %9.3f)" % (what, name, statistics.median(v), min(v), max(v)))

    def scene(kw, seed=0):
        torch.manual_seed(seed)
        np.random.seed(seed)
        sid = M.get_scene_id("lego", 1, (RES, 32))
        mc = M.TwoDimPlanesModel(use_viewdirs=True, align_corners=True, num_planes_or_rot_mats=3, **kw)
        mf = M.TwoDimPlanesModel(use_viewdirs=True, align_corners=True, num_planes_or_rot_mats=mc.rot_mats(), **kw)
        mc, mf = mc.to(dev), mf.to(dev)
        planes = {}
        for d in range(4):
            r = RES if d < 3 else 32
            p = 0.5 * torch.randn(1, 48, r, r, device=dev)
            if d < 3:
                mask = torch.zeros_like(p)
                mask[:, :, BLOCK[0]:BLOCK[1], BLOCK[0]:BLOCK[1]] = 1.0
                p = p * mask
            planes[M.get_plane_name(sid, d)] = torch.nn.Parameter(p)
        planes = torch.nn.ParameterDict(planes)
        box = torch.tensor([[-4.0, -4, -4, -np.pi, -np.pi / 2], [4, 4, 4, np.pi, np.pi / 2]], dtype=torch.float64)
        for m in (mc, mf):
            m.planes_, m.box_coords = planes, {sid: box}
            m.set_cur_scene_id(sid)
            m.eval()
        return mc, mf, sid

    say("generic geometries, evaluation frame: without / with an occupancy grid -- %s" % label)
    H = W = 400
    focal = 0.5 * W / np.tan(0.5 * 0.6911112)
    pose = torch.from_numpy(pose_spherical(30.0, -30.0, 4.0)).to(dev)
    opts, scfg = render_options(64, 128)
    edge = -1.0 + 2.0 * (BLOCK[0] - 1) / (RES - 1)          # the bilinear support of the block ends at the texel in front of it
    for name, kw in GEOMETRIES:
        for arith in ("f32", "f16x2"):
            mc, mf, sid = scene(kw)
            mc.arithmetic = mf.arithmetic = None if arith == "f32" else "f16x2"
            ro, rd = nvsr_amd.nerf_helpers.get_ray_bundle(H, W, focal, pose)
            rays = nvsr_amd.train_utils.pack_rays(ro.reshape(-1, 3), rd.reshape(-1, 3), 2.0, 6.0, H, W, focal, no_ndc=True)
            N = rays.shape[0]
            os.environ["NVSR_GENERIC_TWO_PHASE"] = "0"
            with torch.no_grad():
                z_c = nv.coarse_z(rays, 64, False, None)
                pts_c = nv.ray_points(rays, z_c)
                n = pts_c[:, :3] / 4.0
                inside = (n.abs() < abs(edge)).sum(1) >= 2                   # two coordinates within a block: a plane is not zero there
                far = torch.tensor([[3.5, 3.5, 3.5, 1.0, 0.0, 0.0]], device=dev)
                lift_of = lambda m: m(pts_c)[:, 3][inside][::37].float() - float(m(far)[0, 3])
                for m in (mc, mf):
                    if float(lift_of(m).median()) < 0:            # a seeded decoder may as well answer the planes with LESS density
                        m.fc_alpha["0"].weight.neg_()
                    q = float(lift_of(m).median())
                    assert q > 0, "the planes lift sigma nowhere: another seed"
                    m.fc_alpha["0"].bias.add_(-float(m(far)[0, 3]) - q / 2)
                w_c = nv.composite_rays(mc(pts_c).reshape(N, 64, 4), z_c, rays, None, False, True)[3]
                z_f = nv.importance_resample(z_c, w_c, 128, None)
                pts_f = nv.ray_points(rays, z_f)
                w_f = nv.composite_rays(mf(pts_f).reshape(N, 192, 4), z_f, rays, None, False, True)[3]
                share_of = lambda w: float((w != 0).float().mean())
                say("%s, %s: live share coarse %.3f, fine %.3f; samples the planes reach: coarse %.3f" % (
                    name, arith, share_of(w_c), share_of(w_f), float(inside.float().mean())))
                grids = {}
                if has_grid:
                    for m, pts, what in ((mc, pts_c, "coarse"), (mf, pts_f, "fine")):
                        m.build_occupancy(sid)
                        grid, G = m.occupancy_entry(sid)
                        set_share = float(sum(bin(int(v) & 0xFFFFFFFF).count("1") for v in grid.cpu().tolist())) / G ** 3
                        kept = float(nv.generic_occupancy_keep(m.scene_args(check_native=False)[1], pts, grid, G)[0].mean())
                        say("    %-30s G = %d, %.3f of the cells set; kept share of the %s pass %.3f" % ("grid", G, set_share, what, kept))
                        grids[id(m)] = m.__dict__.pop("_occupancy")

            def frame_of(two_phase, with_grid):
                def run():
                    os.environ["NVSR_GENERIC_TWO_PHASE"] = two_phase      # (read at every call)
                    for m in (mc, mf):
                        m.__dict__.pop("_occupancy", None)
                        if with_grid:
                            m.__dict__["_occupancy"] = grids[id(m)]
                    return nvsr_amd.train_utils.eval_nerf(H, W, focal, mc, mf, ro, rd, opts, scene_id=sid, scene_config=scfg)[3]
                return run

            fns = {"no grid, one phase": frame_of("0", False)}
            if hasattr(M.TwoDimPlanesModel, "generic_frame_route"):
                fns["no grid, two phases"] = frame_of("1", False)
            if has_grid:
                fns["grid"] = frame_of("1", True)
            ms = alternate(fns, 1)
            for k in fns:
                row("frame 400 x 400, 64 + 128", k, ms[k])
            if has_grid:
                med = {k: statistics.median(v) for k, v in ms.items()}
                spread = max(max(v) - min(v) for v in ms.values())
                for k in ("no grid, one phase", "no grid, two phases"):
                    d = med[k] - med["grid"]
                    say("    %-30s %s / grid = %.3f  (difference %+.3f ms, largest spread of the routes %.3f ms: %s)" % (
                        "frame 400 x 400, 64 + 128", k, med[k] / med["grid"], d, spread,
                        "the grid is faster" if d > spread else "the grid is slower" if -d > spread else "within the spread"))
                with torch.no_grad():
                    a, b = fns["grid"](), fns["no grid, two phases"]()
                    say("    %-30s largest |difference| of the fine image, grid against no grid: %.3g" % ("frame 400 x 400, 64 + 128", float((a - b).abs().max())))
                    grid, G = grids[id(mf)][sid][1], grids[id(mf)][sid][2]
                    consts = mf.scene_args(check_native=False)[1]
                    keep, _ = nv.generic_occupancy_keep(consts, pts_f, grid, G)
                launches = {"density phase, every sample": lambda: mf.density_field(pts_f),
                            "keep mask": lambda: nv.generic_occupancy_keep(consts, pts_f, grid, G),
                            "kept list": lambda: nv.generic_live_list(keep),
                            "keep mask + list + density phase": lambda: mf.density_field_kept(pts_f, grid, G)}
                ms = alternate(launches, 1)
                for k in launches:
                    row("fine pass, %d samples" % (N * 192), k, ms[k])
                del keep
            del mc, mf, pts_c, pts_f, w_c, w_f, grids
            torch.cuda.empty_cache()
    os.environ.pop("NVSR_GENERIC_FUSED", None)
    os.environ.pop("NVSR_GENERIC_TWO_PHASE", None)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "a" if "--append" in ARGV else "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
