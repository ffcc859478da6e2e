"""Timing of the two FlexibleNeRFModel baselines' kernels (csrc/mip.hip, csrc/pe.hip) on one GPU.

    python tools/nerf_baseline_time.py [--model mip|pe]        # one fresh child process per (model, arithmetic), each under `timeout -k 10 <s>`
    python tools/nerf_baseline_time.py --child mip f32         # (what the parent runs)

Per model and arithmetic, one JSON line: an 800 x 800 validation frame at 64 + 64 samples (run_one_iter_of_nerf: ms; the two model passes
alone: kernel ms, ns per point and the fraction of the roof, FLOP per point on the f32 matrix pipe at 157.3 TF, the bf16 one at 2516.6 / 6 TF or the
f16 one at 2516.6 / 3 TF)
and a 4096-ray training step (forward, backward, weight gradients: ms and the record bytes it moves).  Mip also times, as "before", the scalar
flexible_nerf_kernel on the same 4096 x 193 points with pre-encoded input.  Without --model both models run, Mip first; the first failure
ends the run."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOF = {"f32": 157.3e12, "bf16x3": 2516.6e12 / 6, "f16x2": 2516.6e12 / 3}
# per model: FlexibleNeRFModel arguments, encode_position_fn, scene id, FLOP per point (2 x multiply-adds), depths per ray of the coarse pass
# (Mip: interval edges, one more than its samples), the capi prefix of the record sizes
MODELS = {
    "mip": dict(kwargs=dict(include_input_xyz=False), encode="mip", scene="lego_DS8", flop=2 * 80384, extra=1, capi="MIP"),
    "pe": dict(kwargs=dict(), encode="positional_encoding", scene="lego", flop=2 * 80768, extra=0, capi="PE"),
}


def child(model, arith):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import nvsr_amd
    from types import SimpleNamespace as NS
    d = MODELS[model]
    dev = "cuda:0"
    tu = nvsr_amd.train_utils
    torch.manual_seed(0)
    mc = nvsr_amd.models.FlexibleNeRFModel(**d["kwargs"]).to(dev)
    mf = nvsr_amd.models.FlexibleNeRFModel(**d["kwargs"]).to(dev)
    mc.arithmetic = mf.arithmetic = arith
    ev = lambda: torch.cuda.Event(enable_timing=True)

    def timed(fn, reps=3):
        fn()
        torch.cuda.synchronize()
        best = 1e30
        for _ in range(reps):
            a, b = ev(), ev()
            a.record()
            fn()
            b.record()
            b.synchronize()
            best = min(best, a.elapsed_time(b))
        return best

    if model == "mip":
        radius = tu.mip_radius(d["scene"])
        forward = lambda m, rays, z: m.mip_forward(rays, z, radius)
    else:
        forward = lambda m, rays, z: m.pe_forward(rays, z)
    H = W = 800
    focal = 0.5 * W / np.tan(0.5 * 0.6911112)
    pose = torch.eye(4, device=dev)
    pose[2, 3] = 4.0
    ro, rd = nvsr_amd.nerf_helpers.get_ray_bundle(H, W, focal, pose)
    mode = NS(chunksize=131072, perturb=False, num_coarse=64, num_fine=64, white_background=False, radiance_field_noise_std=0.0, lindisp=False)
    opts = NS(nerf=NS(use_viewdirs=True, encode_position_fn=d["encode"], train=mode, validation=mode))
    scfg = {"near": 2.0, "far": 6.0, "no_ndc": True}
    rays_b = torch.stack((ro.reshape(-1, 3), rd.reshape(-1, 3)))
    nc = 64 + d["extra"]                      # coarse depths per ray; the fine pass sees them and as many again
    r = {"model": model, "arith": arith}
    with torch.no_grad():
        r["frame_ms"] = timed(lambda: tu.run_one_iter_of_nerf(H, W, focal, mc, mf, rays_b, opts, d["scene"], mode="validation", scene_config=scfg))
        rays = tu.pack_rays(ro, rd, 2.0, 6.0)
        zc = torch.ops.nvsr.coarse_z(rays, nc, False, None)
        zf = torch.sort(torch.cat((zc, zc + 1e-3), -1), -1)[0]
        r["frame_kernel_ms"] = timed(lambda: (forward(mc, rays, zc), forward(mf, rays, zf)))
    per_ray = 64 + 128 + d["extra"]           # points (Mip: intervals) of the two passes
    pts = rays.shape[0] * per_ray
    r["frame_tflop"] = pts * d["flop"] / 1e12
    r["frame_roof_ms"] = pts * d["flop"] / ROOF[arith] * 1e3
    r["frame_roof_frac"] = r["frame_roof_ms"] / r["frame_kernel_ms"]
    r["frame_kernel_ns_per_point"] = r["frame_kernel_ms"] * 1e6 / pts
    # training step: 4096 rays, 64 + 64
    n = 4096
    rays_t = rays[:n].contiguous()
    zc_t, zf_t = zc[:n].contiguous(), zf[:n].contiguous()

    def step():
        raw_c = forward(mc, rays_t, zc_t)
        raw_f = forward(mf, rays_t, zf_t)
        (raw_c.square().mean() + raw_f.square().mean()).backward()
    r["train_step_ms"] = timed(step)
    pts_t = n * per_ray
    # recording forward writes the record, the backward reads it and writes the gradient record, the weight gradients read both
    rec, grec = (getattr(nvsr_amd.capi, "%s_NERF_%s" % (d["capi"], k)) for k in ("RECORD_FLOATS", "GRAD_RECORD_FLOATS"))
    r["train_record_bytes"] = pts_t * 4 * (2 * rec + 2 * grec)
    r["train_tflop"] = 3 * pts_t * d["flop"] / 1e12
    if model == "mip":
        # before: the scalar kernel on the same points, pre-encoded
        x = torch.cat((torch.ops.nvsr.mip_encode(rays_t, zc_t, radius), torch.ops.nvsr.mip_encode(rays_t, zf_t, radius)), 0)
        with torch.no_grad():
            r["scalar_kernel_ms_4096rays"] = timed(lambda: mc(x))
            r["fused_kernel_ms_4096rays"] = timed(lambda: (forward(mc, rays_t, zc_t), forward(mf, rays_t, zf_t)))
    print(json.dumps(r))


def main():
    args = sys.argv[1:]
    if len(args) == 3 and args[0] == "--child":
        return child(args[1], args[2])
    if args and (len(args) != 2 or args[0] != "--model" or args[1] not in MODELS):
        sys.exit("usage: nerf_baseline_time.py [--model mip|pe]")
    for model in [args[1]] if args else list(MODELS):
        for arith in ("f32", "bf16x3", "f16x2"):
            p = subprocess.run(["timeout", "-k", "10", "600", sys.executable, os.path.abspath(__file__), "--child", model, arith])
            if p.returncode != 0:
                print(json.dumps({"model": model, "arith": arith, "exit": p.returncode}))
                return p.returncode      # (a fault or a time limit: nothing more on the GPU)
    return 0


if __name__ == "__main__":
    sys.exit(main())
