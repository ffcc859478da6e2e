"""Frame time of the render pass's worst case for the two-phase route: a scene whose every weight is positive (both density heads: weight 0,
bias +0.05, so every live list holds all S samples and the colour pass saves nothing), benchmark size (800 x 800, 64 + 128 samples, planes
800^2), whole frames through train_utils.eval_nerf, wall clock around a synchronised frame, no profiler.  Run from the root of the tree to be
timed; the routes are chosen by the environment (NVSR_RENDER_ONE_PHASE, NVSR_COLOUR_ORDER, NVSR_COLOUR_GROUP_ORDER).  Needs the GPU.

    python tools/worst_case_frame.py [--frames 5] [--warmup 2]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.getcwd())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    import nvsr_amd
    from bench import make_synthetic_scene, render_options

    dev = "cuda:0"
    mc, mf, sid, pose = make_synthetic_scene(dev, plane_res=800, seed=0)
    for m in (mc, mf):
        m.fc_alpha["0"].weight.zero_()
        m.fc_alpha["0"].bias.fill_(0.05)
    H = W = 800
    focal = 0.5 * W / np.tan(0.5 * 0.6911112)
    ro, rd = nvsr_amd.nerf_helpers.get_ray_bundle(H, W, focal, pose)
    opts, scfg = render_options(64, 128)
    ms = []
    for i in range(a.warmup + a.frames):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = nvsr_amd.train_utils.eval_nerf(H, W, focal, mc, mf, ro, rd, opts, scene_id=sid, scene_config=scfg)
        torch.cuda.synchronize()
        if i >= a.warmup:
            ms.append(1e3 * (time.perf_counter() - t0))
    print("worst-case frame: min %.2f ms, all %s; fine image sum %.6f" % (min(ms), " ".join("%.2f" % m for m in ms), float(out[3].double().sum())))


if __name__ == "__main__":
    torch.set_grad_enabled(False)
    main()
