"""Timing of training the generic decoder geometries WITH decoder gradients on the fused launches (csrc/generic_fused_bwd.hip: the recording
backward + the layered contractions on its record, NVSR_GENERIC_TRAIN_DECODER_FUSED=1) against the layered route (csrc/generic.hip,
NVSR_GENERIC_TRAIN_DECODER_FUSED=0) on one GPU, one process, routes alternated three times; writes profiles/generic_train_decoder_ab.txt.

    python tools/generic_train_decoder_time.py [--out FILE] [--parent TREE] [--no-split]
    python tools/generic_train_decoder_time.py --root TREE --append --label TEXT        (what --parent runs)
    python tools/generic_train_decoder_time.py --split-child GEOMETRY ROUTE             (what the split runs under rocprofv3)

Per geometry (200^2 position planes, a 32^2 view plane, seeded weights, planes and both decoders trained):
  fwd+bwd    model(x) on 2^19 points in train() and backward() of a fixed cotangent: ms (median, min..max of the three rounds)
  iteration  run_one_iter_of_nerf on 4 096 rays at 64 + 64 samples, an MSE loss on both passes and backward()
and the largest relative L2 distance of the two routes' gradients (planes and decoder).
--parent TREE: a checkout of the PARENT commit, built there.  It is timed in a second process of the same job on the layered route (--root
imports the package from that tree; a tree without generic_decoder_train_route() runs the layered route alone), and every ratio is quoted
against it: no speed-up is claimed against this tree's own layered route alone.
The split (unless --no-split): per geometry and route ONE `rocprofv3 --kernel-trace --stats` run of its own -- never inside the timed process --
of four calls of the route's backward operator on the 2^19 points; the kernels' total time per call goes to
  recording launch     generic_backward_fused_record_kernel
  contraction launches generic_wgrad_kernel
  everything else      every other kernel of the operator (the layered route's inputs, recomputed forward, data gradients and scatter; the
                       zero fills of the results)."""
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

ARGV = sys.argv[1:]
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.abspath(ARGV[ARGV.index("--root") + 1]) if "--root" in ARGV else HERE
sys.path.insert(0, ROOT)

GEOMETRIES = [
    ("hidden 64, avg / concat_pos", 3, dict(dec_channels=64, proj_combination="avg", viewdir_proj_combination="concat_pos", skip_connect_every=3)),
    ("hidden 128, sum / sum", 3, dict(dec_channels=128, proj_combination="sum", skip_connect_every=3)),
    ("hidden 256, concat over 4 planes", 4, dict(dec_channels=256, proj_combination="concat", viewdir_proj_combination="concat", skip_connect_every=3)),
]
HANDLE = "NVSR_GENERIC_TRAIN_DECODER_FUSED"
P = 1 << 19
SPLIT_CALLS = 4


def scene(M, np, torch, dev, n_pos, kw, seed=0):
    """coarse / fine models of a geometry on seeded planes, planes and both decoders trained -> (mc, mf, scene id, planes, decoder parameters)"""
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
            p.requires_grad_(True)
    return mc, mf, sid, list(planes.values()), list(mc.decoder_parameters()) + list(mf.decoder_parameters())


def points(torch, dev):
    g = torch.Generator().manual_seed(1)
    x = torch.cat([torch.rand(P, 3, generator=g) * 8.4 - 4.2, torch.randn(P, 3, generator=g)], -1).to(dev)
    return g, x, torch.randn(P, 4, generator=g).to(dev)


def split_child():
    """four calls of one route's backward operator on the 2^19 points of one geometry: the body of a rocprofv3 run"""
    import numpy as np
    import torch

    import nvsr_amd

    index, route = int(ARGV[ARGV.index("--split-child") + 1]), ARGV[ARGV.index("--split-child") + 2]
    dev = "cuda:0"
    _, n_pos, kw = GEOMETRIES[index]
    _, mf, _, _, _ = scene(nvsr_amd.models, np, torch, dev, n_pos, kw)
    _, x, G = points(torch, dev)
    planes = [mf.channel_last_plane(d).detach() for d in range(n_pos + 1)]
    planes, consts = mf.scene_args(planes=planes, check_native=False)
    op = torch.ops.nvsr.triplane_decode_generic_fused_backward_record if route == "fused" else torch.ops.nvsr.triplane_decode_generic_backward
    with torch.no_grad():
        for _ in range(SPLIT_CALLS):
            op(planes, consts, mf.natural_blob().detach(), mf.generic_geometry(), x, G, True, [True] * (n_pos + 1), True, None, False)
    torch.cuda.synchronize()


def split(index, route, work):
    """(recording, contraction, everything else) ms per call of the route's backward operator, from one rocprofv3 --kernel-trace --stats run"""
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    out = os.path.join(work, "g%d_%s" % (index, route))
    shutil.rmtree(out, ignore_errors=True)
    done = subprocess.run([rocprof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--", sys.executable, os.path.abspath(__file__),
                           "--split-child", str(index), route], capture_output=True, text=True, timeout=300,
                          env={k: v for k, v in os.environ.items() if k != HANDLE})
    if done.returncode != 0:
        raise RuntimeError("rocprofv3 failed: %s" % done.stderr[-2000:])
    files = glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True)
    assert files, "no kernel statistics under %s" % out
    parts = {"recording": 0.0, "contraction": 0.0, "else": 0.0}
    for f in files:
        for r in csv.DictReader(open(f)):
            total = float(r["TotalDurationNs"]) if r.get("TotalDurationNs") else float(r["AverageNs"]) * float(r["Calls"])
            key = "recording" if "generic_backward_fused_record_kernel" in r["Name"] else "contraction" if "generic_wgrad_kernel" in r["Name"] else "else"
            parts[key] += total / 1e6 / SPLIT_CALLS
    return parts["recording"], parts["contraction"], parts["else"]


def main():
    import numpy as np
    import torch

    import nvsr_amd
    from bench import pose_spherical, render_options

    out_path = ARGV[ARGV.index("--out") + 1] if "--out" in ARGV else os.path.join(HERE, "profiles", "generic_train_decoder_ab.txt")
    label = ARGV[ARGV.index("--label") + 1] if "--label" in ARGV else "this tree"
    assert torch.cuda.is_available(), "generic_train_decoder_time.py measures on a GPU; there is nothing to report without one"
    dev = "cuda:0"
    M = nvsr_amd.models
    has_fused = hasattr(M.TwoDimPlanesModel, "generic_decoder_train_route")
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

    say("generic geometries, training planes + both decoders: fused (csrc/generic_fused_bwd.hip: recording backward + the contractions on its record, "
        "%s=1) against layered (%s=0, csrc/generic.hip) -- %s%s" % (
            HANDLE, HANDLE, label, "" if has_fused else " (no fused decoder-training route in this tree: the layered route alone)"))
    g, x, G = points(torch, dev)
    H = W = 64
    focal = 0.5 * W / np.tan(0.5 * 0.6911112)
    pose = torch.from_numpy(pose_spherical(30.0, -30.0, 4.0)).to(dev)
    opts, scfg = render_options(64, 64)
    target = (torch.rand(H * W, 3, generator=g) * 0.5 + 0.25).to(dev)
    for name, n_pos, kw in GEOMETRIES:
        mc, mf, sid, plist, dlist = scene(M, np, torch, dev, n_pos, kw)
        ro, rd = nvsr_amd.nerf_helpers.get_ray_bundle(H, W, focal, pose)
        batch = torch.stack([ro.reshape(-1, 3), rd.reshape(-1, 3)], 0)

        def route(r, fn):
            def run():
                os.environ[HANDLE] = "1" if r == "fused" else "0"            # (read at every call)
                for p in plist + dlist:
                    p.grad = None
                fn()
                return [p.grad for p in plist + dlist if p.grad is not None]
            return run

        def fwd_bwd():
            mf(x).backward(G)

        def iteration():
            rgb_c, _, _, rgb_f, *_ = nvsr_amd.train_utils.run_one_iter_of_nerf(H, W, focal, mc, mf, batch, opts, sid, mode="train", scene_config=scfg)
            (((rgb_c - target) ** 2).mean() + ((rgb_f - target) ** 2).mean()).backward()

        os.environ.pop(HANDLE, None)
        taken = mf.generic_decoder_train_route() if has_fused else "layered"
        os.environ[HANDLE] = "1"
        forced = mf.generic_decoder_train_route() if has_fused else "layered"
        shapes = (("fwd+bwd 2^19 points", {r: route(r, fwd_bwd) for r in routes}, 3), ("iteration 4096 rays, 64 + 64", {r: route(r, iteration) for r in routes}, 2))
        dist = 0.0
        if has_fused:
            a, b = shapes[0][1]["fused"](), shapes[0][1]["layered"]()          # (an iteration draws its own samples: compared on the fixed points)
            dist = max([dist] + [float((u - v).norm() / v.norm()) for u, v in zip(a, b)])
        say("%s (route taken by default: %s, with %s=1: %s; largest relative L2 distance of the routes' gradients, planes and decoder: %.2g)" % (
            name, taken, HANDLE, forced, dist))
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
        del mc, mf, plist, dlist, shapes
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

    if has_fused and "--no-split" not in ARGV and "--root" not in ARGV:
        work = tempfile.mkdtemp(prefix="nvsr_decoder_split_")          # (the traces are large and of no further use: only the sums are kept)
        rows = ["the backward operator on the 2^19 points, kernel time per call from one rocprofv3 --kernel-trace --stats run per geometry and route "
                "(ms: recording launch | contraction launches | everything else | sum):"]
        for index, (name, _, _) in enumerate(GEOMETRIES):
            for r in ("layered", "fused"):
                rec, con, other = split(index, r, work)
                rows.append("    %-34s %-8s %9.3f | %9.3f | %9.3f | %9.3f" % (name, r, rec, con, other, rec + con + other))
        shutil.rmtree(work, ignore_errors=True)
        print("\n".join(rows), flush=True)
        with open(out_path, "a") as f:
            f.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    split_child() if "--split-child" in ARGV else main()
