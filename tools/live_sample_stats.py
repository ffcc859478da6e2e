"""How much of a frame's colour-decoder work the two-phase render pass (csrc/render3.hip) can leave out, counted on the benchmark's
own frame: bench.make_synthetic_scene, the 800 x 800 view, 64 coarse + 128 fine samples, rays in train_utils.patch_order (a workgroup's 256
rays are 8 wave tiles of 16 x 2 pixels).  Needs the GPU: the scene is calibrated with the model's forward, which runs on the GPU only.

A sample is LIVE when its compositing weight is not +0.0 -- the weights are the ones the render passes write (the coarse weights of the frame;
the fine pass is run once more with its weights requested).  Printed per pass: the share of dead points, the mean live count per ray,
E[max live count] / S over a 32-ray tile, a wave's 64 rays and a workgroup's 256 rays (the colour pass runs max-live-count steps per
workgroup: that last figure is the share of the colour work that is left), and how many tiles / tile pairs are dead as a whole at a sample index
(what skipping whole tiles could save).

    python tools/live_sample_stats.py [--res 800] [--plane-res 800] [--seed 0] > profiles/live_sample_stats.txt
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=800)
    ap.add_argument("--plane-res", type=int, default=800)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--arithmetic", default="f16x2")
    a = ap.parse_args()
    import nvsr_amd
    from bench import make_synthetic_scene

    capi, tu = nvsr_amd.capi, nvsr_amd.train_utils
    dev = "cuda:0"
    mc, mf, sid, pose = make_synthetic_scene(dev, plane_res=a.plane_res, seed=a.seed)
    H = W = a.res
    N, Nc, Nf = H * W, 64, 128
    focal = 0.5 * W / np.tan(0.5 * 0.6911112)
    ro, rd = nvsr_amd.nerf_helpers.get_ray_bundle(H, W, focal, pose)
    perm, _ = tu.patch_order(N, W, dev)
    rays = tu.pack_rays(ro, rd, 2.0, 6.0)[perm].contiguous()
    lib = capi.lib()
    ws = torch.empty(int(lib.nvsr_render_workspace_floats(N, Nc, Nf)), device=dev)
    o = [torch.empty(s, device=dev) for s in ((N, 3), (N,), (N,), (N, 3), (N,), (N,))]
    sc_c, keep_c = mc.native_scene()
    sc_f, keep_f = mf.native_scene()
    arith = capi.ARITHMETIC[a.arithmetic]
    capi.call("nvsr_render_rays_arith", C.byref(sc_c), capi.ptr(mc.packed_decoder()), capi.ptr(mf.packed_decoder()), N, Nc, Nf, capi.ptr(rays),
              0, 0, None, None, None, None, *[capi.ptr(t) for t in o], capi.ptr(ws), arith, capi.stream())
    r4 = lambda n: (n + 3) // 4 * 4
    w_c = ws[r4(N * Nc):r4(N * Nc) + N * Nc].view(N, Nc)
    z_f = ws[2 * r4(N * Nc):2 * r4(N * Nc) + N * (Nc + Nf)].view(N, Nc + Nf).contiguous()
    w_f = torch.empty(N, Nc + Nf, device=dev)
    capi.call("nvsr_render_pass_arith", C.byref(sc_f), capi.ptr(mf.packed_decoder()), N, Nc + Nf, capi.ptr(rays), capi.ptr(z_f), None, 0,
              capi.ptr(o[3]), capi.ptr(o[4]), capi.ptr(o[5]), capi.ptr(w_f), None, None, arith, capi.stream())
    torch.cuda.synchronize()
    print("live-sample statistics of the benchmark frame: %d x %d view (%d rays in patch order), planes %d^2, seed %d, %s"
          % (H, W, N, a.plane_res, a.seed, a.arithmetic))
    for name, w in (("coarse pass (S = 64)", w_c), ("fine pass (S = 192)", w_f)):
        S = w.shape[1]
        live = ~(w == 0)
        cnt = live.sum(1)
        print(name)
        print("  points with w == 0                               %.1f %%" % (100 * (1 - float(live.float().mean()))))
        print("  mean live samples per ray                        %.1f" % float(cnt.float().mean()))
        for group, label in ((32, "a 32-ray tile"), (64, "a wave's 64 rays"), (256, "a workgroup's 256 rays")):
            n = N // group * group
            print("  E[max live count] / S over %-22s %.3f" % (label, float(cnt[:n].view(-1, group).max(1).values.float().mean()) / S))
        for group, label in ((32, "32-ray tiles"), (64, "64-ray tile pairs")):
            n = N // group * group
            dead = ~live[:n].view(-1, group, S).any(1)
            print("  %-18s with every w == 0 at a sample   %.1f %%" % (label, 100 * float(dead.float().mean())))


if __name__ == "__main__":
    torch.set_grad_enabled(False)
    main()
