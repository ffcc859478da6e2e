"""Golden fixture of a view's geometry outputs -- expected depth, acc and the composited surface normal -- computed by the
UPSTREAM code on the CPU in float64.

Re-run:  NVSR_REFERENCE_DIR=<upstream checkout> python tests/golden/gen_normals.py

Upstream renders the frame (run_one_iter_of_nerf, validation mode: no perturbation, no noise); its volume_render_radiance_field returns the
weights and the depth map that predict_and_render_radiance drops, recorded here through a wrapper.  The per-sample density gradient is
upstream's own autograd through the fine model's forward, with the two shims of gen_points_grad.py: Tensor.cpu -> detach (normalize_coords
calls .cpu().numpy() on a tensor that requires grad) and, for that ONE forward, torch.no_grad -> nullcontext (CoordProjector.forward projects
under no_grad and would return 0).  The compositing of the normals is not upstream's -- it has none -- but three lines of float64 numpy.

  g28_normals.npz
    scene lego_DS8_PlRes7_4: position planes 7x7, view plane 4x3 (H x W), 48 channels, N(0, 0.5^2) entries; a 6x5 frame, Nc = 8, Nf = 8
    coarse.* / fine.*   the entries of the two decoders' state dicts that DIFFER from g11_grads.npz's: g11's decoders with fc_alpha calibrated
                        on this scene as gen_golden.build_models does; g11_decoders: its checksum as this fixture was made from it
    plane0..3, box, hwf, seed
    rays [30,11]        float32 origins / directions of get_ray_bundle as float64, near, far, viewdir = rd / |rd| in float64
    z_fine, weights_fine [30,16], depth, acc [30]    the fine pass
    index [M], g [M,3]  the samples with weights_fine != 0 in ascending flat order and d sigma_raw / d p there
    normal [30,3]       sum_s w_s n_s,  n_s = -g_s / |g_s|

The seed is raised until, for every sample with w > 1e-6: every hidden pre-activation of the density decoder is at least 1e-4 of its layer's
rms away from 0, every tap coordinate at least 1e-4 texel away from an integer, and |g| at least 1e-3 of the median -- a flipped ReLU gate or
bilinear cell must not hide in a tolerance.  No ray is dropped."""
import contextlib
import os
import sys

import numpy as np
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as gg  # noqa: E402  (imports the upstream modules behind the shims of SURVEY Appendix A)
from gen_golden_lowrank import decoder_checksum  # noqa: E402

models, tu, nh = gg.models, gg.tu, gg.nh
H, W, NC, NF = 6, 5, 8, 8
VIEW_SHAPE = (4, 3)


def build(seed, g11):
    sid, mc, mf, planes, box = gg.build_models(7, 4, 0.5, seed=seed)
    for prefix, m in (("coarse.", mc), ("fine.", mf)):
        m.load_state_dict({k[len(prefix):]: torch.from_numpy(v) for k, v in g11.items() if k.startswith(prefix)}, strict=False)
    names = [models.get_plane_name(sid, d) for d in range(4)]
    torch.manual_seed(seed)
    planes[names[3]] = nn.Parameter(0.5 * torch.randn(1, 48, *VIEW_SHAPE))
    with torch.no_grad():
        g = torch.Generator().manual_seed(seed + 1)
        pts = torch.rand(4096, 3, generator=g) * 6 - 3
        d = torch.randn(4096, 3, generator=g)
        xc = torch.cat([pts, d / d.norm(dim=-1, keepdim=True)], -1)
        for m in (mc, mf):
            m.eval()
            scale = 1.0 / float(m(xc)[:, 3].std())
            m.fc_alpha["0"].weight.mul_(scale)
            m.fc_alpha["0"].bias.mul_(scale)
            m.fc_alpha["0"].bias.add_(-float(m(xc)[:, 3].mean()) - 0.5)
    state = {}
    for prefix, m in (("coarse.", mc), ("fine.", mf)):
        for k, v in gg.state_arrays(prefix, m).items():
            assert k in g11 and v.shape == g11[k].shape, k
            if not np.array_equal(v, g11[k]):
                state[k] = v.copy()
    plane_arrays = [planes[n].detach().numpy().copy() for n in names]
    for m in (mc, mf):
        m.double()
    for n in names:
        planes[n].data = planes[n].data.double()
    return sid, mc, mf, plane_arrays, box, state


def render(sid, mc, mf):
    """upstream's frame in float64 -> rays [N,11], z_fine, weights_fine, depth, acc"""
    focal = 0.5 * W / np.tan(0.5 * 0.6911112)
    ro, rd = nh.get_ray_bundle(H, W, focal, torch.from_numpy(gg.POSE))
    ro, rd = ro.reshape(-1, 3).double(), rd.reshape(-1, 3).double()
    v = gg.mode_cfg(NC, NF)
    cfg = gg.make_cfg(v, v)
    zrec, vrec = [], []
    real_rn, real_vr = tu.run_network, tu.volume_render_radiance_field

    def rec_rn(*a, **k):
        zrec.append(k["z_vals"].clone())
        return real_rn(*a, **k)

    def rec_vr(*a, **k):
        out = real_vr(*a, **k)
        vrec.append([t.clone() for t in out])
        return out

    tu.run_network, tu.volume_render_radiance_field = rec_rn, rec_vr
    try:
        with torch.no_grad():
            out = tu.run_one_iter_of_nerf(H, W, focal, mc, mf, torch.stack([ro, rd], 0), cfg, scene_id=sid, mode="validation",
                                          scene_config=cfg.dataset["synt"])
    finally:
        tu.run_network, tu.volume_render_radiance_field = real_rn, real_vr
    assert len(zrec) == 2 and len(vrec) == 2 and out[5].dtype == torch.float64
    _, _, acc, weights, depth = vrec[1]
    assert torch.equal(acc, out[5])
    ones = torch.ones_like(rd[:, :1])
    rays = torch.cat([ro, rd, 2.0 * ones, 6.0 * ones, rd / rd.norm(p=2, dim=-1).unsqueeze(-1)], -1)
    return gg.npy(rays), gg.npy(zrec[1]), gg.npy(weights), gg.npy(depth), gg.npy(acc), focal


def gradient(mf, plane_shapes, rays, z, index):
    """upstream's d sigma_raw / d p on the listed samples (both shims), with the density decoder's pre-activations and the pixel coordinates of
    the taps -> (g [M,3], [pre-activations per layer], [pixel coordinates per plane [M,2]])"""
    S = z.shape[1]
    ray = index // S
    p = rays[ray, 0:3] + rays[ray, 3:6] * z.reshape(-1)[index][:, None]
    x = torch.from_numpy(np.concatenate([p, rays[ray, 8:11]], 1)).requires_grad_(True)
    pre, grids = [], []
    hooks = [l.register_forward_hook(lambda mod, inp, out: pre.append(out.detach().numpy().copy())) for l in mf.density_dec["0"]]
    hooks.append(mf.coord_projector.register_forward_hook(lambda mod, inp, out: grids.append(out.detach().numpy().copy())))
    real_cpu, real_no_grad = torch.Tensor.cpu, torch.no_grad
    torch.Tensor.cpu = lambda s, *a, **k: s.detach()                  # shim A
    torch.no_grad = contextlib.nullcontext                            # shim B
    try:
        mf.eval()
        mf(x)[:, 3].sum().backward()
    finally:
        torch.Tensor.cpu, torch.no_grad = real_cpu, real_no_grad
        for h in hooks:
            h.remove()
    assert len(pre) == 4 and len(grids) == 3
    pix = [(grids[d] + 1) * (np.array([plane_shapes[d][1], plane_shapes[d][0]]) - 1) / 2 for d in range(3)]
    return x.grad.numpy()[:, :3].copy(), pre, pix


def well_separated(weights, index, g, pre, pix):
    sel = weights.reshape(-1)[index] > 1e-6
    why = []
    for l, a in enumerate(pre):
        a = a[sel]
        if np.abs(a).min() < 1e-4 * np.sqrt(np.square(a).mean()):
            why.append("pre-activation of density layer %d" % l)
    for d, c in enumerate(pix):
        c = c[sel]
        if np.abs(c - np.round(c)).min() < 1e-4:
            why.append("tap coordinate of plane %d" % d)
    mag = np.linalg.norm(g[sel], axis=1)
    if mag.min() < 1e-3 * np.median(mag):
        why.append("|g|")
    return why, int(sel.sum())


def main():
    g11 = dict(np.load(os.path.join(gg.HERE, "g11_grads.npz")))
    seed = 2800
    while True:
        sid, mc, mf, planes, box, state = build(seed, g11)
        rays, z, weights, depth, acc, focal = render(sid, mc, mf)
        index = np.nonzero(~(weights.reshape(-1) == 0))[0].astype(np.int32)
        g, pre, pix = gradient(mf, [p.shape[-2:] for p in planes], rays, z, index.astype(np.int64))
        why, n = well_separated(weights, index, g, pre, pix)
        if not why:
            break
        print("   seed %d: too close to a kink: %s" % (seed, ", ".join(why)))
        seed += 1
    assert np.isfinite(g).all() and sid == "lego_DS8_PlRes7_4"
    nrm = -g / np.linalg.norm(g, axis=1, keepdims=True)
    normal = np.zeros((H * W, 3))
    np.add.at(normal, index // z.shape[1], weights.reshape(-1)[index][:, None] * nrm)
    print("   seed %d: %d live samples of %d, %d with w > 1e-6; acc %.3f .. %.3f; |normal| %.3f .. %.3f" % (
        seed, len(index), weights.size, n, acc.min(), acc.max(), np.linalg.norm(normal, axis=1).min(), np.linalg.norm(normal, axis=1).max()))
    arrs = dict(box=gg.npy(box), hwf=np.array([H, W, focal]), seed=np.array(seed), rays=rays, z_fine=z, weights_fine=weights, depth=depth, acc=acc,
                index=index, g=g, normal=normal, g11_decoders=decoder_checksum(g11), **state)
    print("   decoder entries that differ from g11:", sorted(state))
    for d in range(4):
        arrs["plane%d" % d] = planes[d]
    gg.save("g28_normals.npz", **arrs)


if __name__ == "__main__":
    main()
