"""Timing of the positional-encoding NeRF baseline kernels (csrc/pe.hip) on one GPU; the sibling of tools/mip_time.py.

    python tools/pe_time.py                   # one fresh child process per arithmetic, each under `timeout -k 10 <s>`
    python tools/pe_time.py --child f32       # (what the parent runs)

Per arithmetic: an 800 x 800 validation frame at 64 + 64 samples (run_one_iter_of_nerf: ms; the two model passes alone: kernel ms and the
fraction of the roof, 161.5 kFLOP per point on the f32 matrix pipe at 157.3 TF or the bf16 one at 2516.6 / 6 TF) and a 4096-ray training
step (forward, backward, weight gradients: ms and the record bytes it moves)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOP = 2 * 80768
ROOF = {"f32": 157.3e12, "bf16x3": 2516.6e12 / 6}


def child(arith):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import nvsr_amd
    from types import SimpleNamespace as NS
    dev = "cuda:0"
    tu = nvsr_amd.train_utils
    torch.manual_seed(0)
    mc = nvsr_amd.models.FlexibleNeRFModel().to(dev)
    mf = nvsr_amd.models.FlexibleNeRFModel().to(dev)
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

    H = W = 800
    focal = 0.5 * W / np.tan(0.5 * 0.6911112)
    pose = torch.eye(4, device=dev)
    pose[2, 3] = 4.0
    ro, rd = nvsr_amd.nerf_helpers.get_ray_bundle(H, W, focal, pose)
    mode = NS(chunksize=131072, perturb=False, num_coarse=64, num_fine=64, white_background=False, radiance_field_noise_std=0.0, lindisp=False)
    opts = NS(nerf=NS(use_viewdirs=True, encode_position_fn="positional_encoding", train=mode, validation=mode))
    scfg = {"near": 2.0, "far": 6.0, "no_ndc": True}
    rays_b = torch.stack((ro.reshape(-1, 3), rd.reshape(-1, 3)))
    r = {"arith": arith}
    with torch.no_grad():
        r["frame_ms"] = timed(lambda: tu.run_one_iter_of_nerf(H, W, focal, mc, mf, rays_b, opts, "lego", mode="validation", scene_config=scfg))
        rays = tu.pack_rays(ro, rd, 2.0, 6.0)
        zc = torch.ops.nvsr.coarse_z(rays, 64, False, None)
        zf = torch.sort(torch.cat((zc, zc + 1e-3), -1), -1)[0]
        r["frame_kernel_ms"] = timed(lambda: (mc.pe_forward(rays, zc), mf.pe_forward(rays, zf)))
    pts = rays.shape[0] * (64 + 128)
    r["frame_tflop"] = pts * FLOP / 1e12
    r["frame_roof_ms"] = pts * FLOP / ROOF[arith] * 1e3
    r["frame_roof_frac"] = r["frame_roof_ms"] / r["frame_kernel_ms"]
    r["frame_kernel_ns_per_point"] = r["frame_kernel_ms"] * 1e6 / pts
    # training step: 4096 rays, 64 + 64
    n = 4096
    rays_t = rays[:n].contiguous()
    zc_t, zf_t = zc[:n].contiguous(), zf[:n].contiguous()

    def step():
        raw_c = mc.pe_forward(rays_t, zc_t)
        raw_f = mf.pe_forward(rays_t, zf_t)
        (raw_c.square().mean() + raw_f.square().mean()).backward()
    r["train_step_ms"] = timed(step)
    pts_t = n * (64 + 128)
    # recording forward writes the record, the backward reads it and writes the gradient record, the weight gradients read both
    r["train_record_bytes"] = pts_t * 4 * (2 * nvsr_amd.capi.PE_NERF_RECORD_FLOATS + 2 * nvsr_amd.capi.PE_NERF_GRAD_RECORD_FLOATS)
    r["train_tflop"] = 3 * pts_t * FLOP / 1e12
    print(json.dumps(r))


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        return child(sys.argv[2])
    rc = 0
    for arith in ("f32", "bf16x3"):
        p = subprocess.run(["timeout", "-k", "10", "600", sys.executable, os.path.abspath(__file__), "--child", arith])
        if p.returncode != 0:
            print(json.dumps({"arith": arith, "exit": p.returncode}))
            rc = p.returncode
            break                       # (a fault or a time limit: nothing more on the GPU)
    return rc


if __name__ == "__main__":
    sys.exit(main())
