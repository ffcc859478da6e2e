"""How much of a frame's colour-decoder work the two-phase render pass (csrc/render3.hip) can leave out, counted on the benchmark's
own frame: bench.make_synthetic_scene, the 800 x 800 view, 64 coarse + 128 fine samples, rays in train_utils.patch_order (a workgroup's 256
rays are 8 wave tiles of 16 x 2 pixels).  Needs the GPU: the scene is calibrated with the model's forward, which runs on the GPU only.

A sample is LIVE when its compositing weight is not +0.0 -- the weights are the ones the render passes write (the coarse weights of the frame;
the fine pass is run once more with its weights requested).  Printed per pass: the share of dead points, the mean live count per ray,
E[max live count] / S over a 32-ray tile, a wave's 64 rays and a workgroup's 256 rays (the colour pass runs max-live-count steps per
workgroup: that last figure is the share of the colour work that is left), and how many tiles / tile pairs are dead as a whole at a sample index
(what skipping whole tiles could save).

Then, per pass, what the colour pass's ray order (live_order_kernel, csrc/colour_order.hip) can recover: the sum over workgroups of trip /
(workgroups x S) for (a) the grouping of the density pass (256 consecutive rays), (b) the rays stably sorted by live count, descending, inside
each block of 4096 consecutive rays and cut into groups of 256, (c) the same with the count quantised as the kernel does it -- bin =
ceil(count x B / S): one bin for the empty rays and B bins of equal width over 1..S -- for B = 8, 16, 32; and (d) for each of them the sum
of trips per XCD under the kernels' mapping of workgroups to XCDs (contiguous eighths of the workgroups), as max / mean over the eight.

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
        print("  colour steps left, sum of trip / (workgroups x S), and the XCDs' sums of trips as max / mean:")
        base = None
        for label, bins in (("(a) groups of the density pass", 0), ("(b) sorted by count in blocks of 4096", -1), ("(c) 32 bins", 32),
                            ("(c) 16 bins", 16), ("(c)  8 bins", 8)):
            share, xcd = grouped_trips(cnt, S, bins)
            base = share if base is None else base
            print("    %-40s %.3f  (%.3f of (a))   XCD max / mean %.3f" % (label, share, share / base, xcd))


def grouped_trips(cnt, S, bins, block=4096, group=256):
    """(sum of trip over the workgroups / (workgroups x S), max / mean of the eight XCDs' sums of trips) when the rays of every `block` are
    stably sorted by bin, fullest first: bins = 0 one bin (the order as it is), -1 the count itself, else ceil(count x bins / S)"""
    N = cnt.numel()
    b = torch.zeros_like(cnt) if bins == 0 else cnt if bins < 0 else torch.clamp((cnt * bins + S - 1) // S, max=bins)
    key = (torch.arange(N, device=cnt.device) // block) * (S + 2) + (S + 1 - b)
    c = cnt[torch.sort(key, stable=True).indices]
    G = (N + group - 1) // group
    c = torch.cat([c, c.new_zeros(G * group - N)])
    trips = c.view(G, group).max(1).values.double()
    per, rem = G // 8, G % 8
    sums = []
    for x in range(8):
        lo = x * per + min(x, rem)
        sums.append(float(trips[lo:lo + per + (1 if x < rem else 0)].sum()))
    return float(trips.sum()) / (G * S), max(sums) / (sum(sums) / 8)


if __name__ == "__main__":
    torch.set_grad_enabled(False)
    main()
