"""The benchmark's frame (800 x 800, 64 + 128 samples, planes 800^2, default arithmetic) plain and with occupancy grids built at the Python
defaults (models.build_occupancy: resolution 128, probes 2, threshold 0, dilate 1), alternating inside one process: three alternations, the
minimum of five frames each, whole frames through train_utils.eval_nerf, wall clock around a synchronised frame, no profiler.  Prints the
build time, the kept share of the coarse and the fine pass, the step share after the ordering (what the density pass over the kept lists
runs, padding included, as a share of N S), the PSNR of the occupancy frame against the plain frame and the share of pixels that differ by more
than 1/255.  Then the dense worst case of tools/worst_case_frame.py (every density +0.05: nothing is culled), which shows what the cull and
the lists cost when they save nothing.  Run from the root of the tree to be timed.  Needs the GPU.

    python tools/occupancy_frame.py [--frames 5] [--warmup 2] [--alternations 3] [--resolution 128] [--probes 2] [--dilate 1]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.getcwd())


def frames(nv, n, warmup, render):
    ms, out = [], None
    for i in range(warmup + n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = render()
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append(1e3 * (time.perf_counter() - t0))
    return ms, out


def shares(nv, mc, mf, rays, Nc, Nf, sid):
    """kept share and step share of the two passes of one occupancy frame, from the kept counts the launches leave (packed entries of the ray order)"""
    capi = nv.capi
    ops = torch.ops.nvsr
    N = rays.shape[0]
    planes, consts = mc.scene_args()
    code = capi.resolve_decoder_arithmetic(mc.arithmetic)
    (gc, Gc), (gf, Gf) = mc.occupancy_entry(sid), mf.occupancy_entry(sid)

    def kept(S):
        t = torch.empty(N, dtype=torch.int32, device=rays.device)
        capi.call("nvsr_internal_copy_kept_counts", capi.ptr(t), N, capi.stream())
        torch.cuda.synchronize()
        c = (t.cpu().numpy() >> 12).astype(np.int64)
        pad = (-N) % 256
        trips = np.concatenate([c, np.zeros(pad, np.int64)]).reshape(-1, 256).max(1)
        return c.sum() / (N * S), 256 * trips.sum() / (N * S)

    _, _, _, w_c = ops.render_pass_occupancy(planes, consts, mc.packed_decoder(), rays, None, Nc, False, True, True, gc, Gc, code)
    coarse = kept(Nc)
    z_f = torch.empty(N, Nc + Nf, device=rays.device)
    capi.call("nvsr_importance_resample_rays", N, Nc, Nf, capi.ptr(rays), 0, capi.ptr(w_c), None, capi.ptr(z_f), capi.stream())
    planes_f, _ = mf.scene_args()
    ops.render_pass_occupancy(planes_f, consts, mf.packed_decoder(), rays, z_f, Nc + Nf, False, True, False, gf, Gf, code)
    return coarse, kept(Nc + Nf)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--resolution", type=int, default=128)
    ap.add_argument("--probes", type=int, default=2)
    ap.add_argument("--dilate", type=int, default=1)
    ap.add_argument("--threshold", type=float, default=0.0)
    a = ap.parse_args()
    import nvsr_amd as nv
    from bench import make_synthetic_scene, render_options

    dev = "cuda:0"
    H = W = 800
    Nc, Nf = 64, 128
    focal = 0.5 * W / np.tan(0.5 * 0.6911112)
    opts, scfg = render_options(Nc, Nf)

    def scene(dense):
        mc, mf, sid, pose = make_synthetic_scene(dev, plane_res=800, seed=0)
        if dense:
            for m in (mc, mf):
                m.fc_alpha["0"].weight.zero_()
                m.fc_alpha["0"].bias.fill_(0.05)
        ro, rd = nv.nerf_helpers.get_ray_bundle(H, W, focal, pose)
        return mc, mf, sid, ro, rd

    for dense in (False, True):
        name = "dense worst case" if dense else "benchmark frame"
        mc, mf, sid, ro, rd = scene(dense)
        render = lambda: nv.train_utils.eval_nerf(H, W, focal, mc, mf, ro, rd, opts, scene_id=sid, scene_config=scfg)
        render()                                  # (pack the decoders, allocate the scratch)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for m in (mc, mf):
            m.build_occupancy(sid, a.resolution, a.probes, a.threshold, a.dilate)
        torch.cuda.synchronize()
        build_ms = 1e3 * (time.perf_counter() - t0)
        grids = {m: m.__dict__["_occupancy"] for m in (mc, mf)}
        set_bits = [int(sum(bin(int(w) & 0xffffffff).count("1") for w in m.occupancy(sid).cpu().numpy())) for m in (mc, mf)]
        best = {"plain": [], "occupancy": []}
        imgs = {}
        for _ in range(a.alternations):
            for route in ("plain", "occupancy"):
                for m in (mc, mf):
                    if route == "plain":
                        m.__dict__.pop("_occupancy", None)
                    else:
                        m.__dict__["_occupancy"] = grids[m]
                ms, out = frames(nv, a.frames, a.warmup, render)
                best[route].append(min(ms))
                imgs[route] = out[3].float().clamp(0, 1)
        rays = nv.train_utils.pack_rays(ro, rd, 2.0, 6.0)
        perm, _ = nv.train_utils.patch_order(H * W, W, rays.device)
        (kc, sc), (kf, sf) = shares(nv, mc, mf, rays[perm].contiguous(), Nc, Nf, sid)
        d = (imgs["plain"] - imgs["occupancy"]).abs()
        mse = float((d.double() ** 2).mean())
        psnr = float("inf") if mse == 0 else -10.0 * np.log10(mse)
        print("%s: grids %d^3, %d^3 probes, threshold %g, dilate %d; build %.1f ms (both models); occupied cells coarse %.1f %%, fine %.1f %%"
              % (name, a.resolution, a.probes, a.threshold, a.dilate, build_ms, 100.0 * set_bits[0] / a.resolution ** 3, 100.0 * set_bits[1] / a.resolution ** 3))
        for route in ("plain", "occupancy"):
            print("  %-9s frame: min %.2f ms; minima of the alternations %s" % (route, min(best[route]), " ".join("%.2f" % m for m in best[route])))
        print("  kept share: coarse %.1f %%, fine %.1f %%; step share after the ordering: coarse %.1f %%, fine %.1f %%" % (100 * kc, 100 * kf, 100 * sc, 100 * sf))
        print("  occupancy frame against the plain frame: PSNR %.2f dB; pixels that differ by more than 1/255: %.4f %%"
              % (psnr, 100.0 * float((d.max(-1).values > 1.0 / 255.0).double().mean())))


if __name__ == "__main__":
    torch.set_grad_enabled(False)
    main()
