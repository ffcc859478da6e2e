"""Steps of the colour pass on the benchmark's own frame, lockstep against point-major (csrc/render3.hip PHASE 2 and 3): per pass, the
sum over the colour workgroups of trip (the lockstep kernels run as many steps as a group's fullest ray) next to the sum of ceil(points / 256)
(the point-major kernels run a group's live points 256 at a time), both over the groups the ray order forms (32 bins, blocks of 4096 rays),
and both as a share of workgroups x S.  A sibling of tools/live_sample_stats.py: same scene, same frame, same weights.  Needs the GPU.

    python tools/point_steps_stats.py [--res 800] [--plane-res 800] [--seed 0]
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
    bins = int(lib.nvsr_internal_colour_order_bins())
    print("colour steps of the benchmark frame: %d x %d view (%d rays in patch order), planes %d^2, seed %d, %s, ray order of %d bins"
          % (H, W, N, a.plane_res, a.seed, a.arithmetic, bins))
    for name, w in (("coarse pass (S = 64)", w_c), ("fine pass (S = 192)", w_f)):
        S = w.shape[1]
        cnt = (~(w == 0)).sum(1)
        b = torch.clamp((cnt * bins + S - 1) // S, max=bins)
        key = (torch.arange(N, device=dev) // 4096) * (S + 2) + (S + 1 - b)
        c = cnt[torch.sort(key, stable=True).indices]
        G = (N + 255) // 256
        c = torch.cat([c, c.new_zeros(G * 256 - N)]).view(G, 256)
        trip, steps = int(c.max(1).values.sum()), int(((c.sum(1) + 255) // 256).sum())
        print(name)
        print("  mean live share of a ray                         %.4f" % (float(cnt.double().mean()) / S))
        print("  lockstep:    sum of trip              %8d   / (workgroups x S) = %.4f" % (trip, trip / (G * S)))
        print("  point-major: sum of ceil(points/256)  %8d   / (workgroups x S) = %.4f   (%.4f of lockstep)" % (steps, steps / (G * S), steps / trip))


if __name__ == "__main__":
    torch.set_grad_enabled(False)
    main()
