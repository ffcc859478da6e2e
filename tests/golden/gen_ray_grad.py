"""Golden fixture of the RAY and CAMERA-POSE gradients of a training render, computed by the UPSTREAM code on the CPU.

Re-run:  NVSR_REFERENCE_DIR=<upstream checkout> python tests/golden/gen_ray_grad.py

Upstream is driven as it stands, behind the two shims of gen_points_grad.py: A, torch.Tensor.cpu = detach (normalize_coords calls
.cpu().numpy() on a tensor that requires grad), and B, for the differentiated forward, torch.no_grad = a null context, so that the sample
positions carry their gradient through CoordProjector (upstream's own pose gradient lacks that term; ours is the true derivative).

  g27_ray_grad.npz, per case c0 (synthetic: no_ndc True, near 2, far 6) and c1 (forward-facing: no_ndc False, near 0, far 1):
    pose [4,4] requires grad -> get_ray_bundle at H x W = 6 x 8 -> 24 selected pixels, some of them twice -> batch_rays [2,24,3]
    (retain_grad) -> run_one_iter_of_nerf(mode='train'), 8 + 8 samples, perturb, density noise 0.2 -> mse(coarse) + mse(fine) -> backward.
    planes 12 x 12 (view plane 8 x 8), N(0, 0.5^2); the decoders are g11_grads.npz's with fc_alpha calibrated per case as
    gen_golden.build_models does (stored: the entries that differ from g11's, `g11_decoders` its checksum).
    cN_sel, cN_target, cN_t_rand, cN_noise_coarse, cN_u, cN_noise_fine   the inputs (the random draws as upstream drew them)
    cN_z_fine, cN_rgb_coarse, cN_rgb_fine, cN_loss                       float32 run
    cN_rays_grad [2,24,3], cN_pose_grad [4,4], cN_grad_plane0..3         float32 run
    cN_rays_grad64, cN_pose_grad64 (float64), cN_grad64_plane0..3 (rounded to float32 for size), cN_z_fine64, cN_loss64:
                                                                         the same upstream code with models, planes and inputs in float64"""
import contextlib
import os
import sys

import numpy as np
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as gg  # noqa: E402  (imports the upstream modules behind the shims of SURVEY Appendix A)
from gen_golden_lowrank import decoder_checksum  # noqa: E402

models, nh, tu = gg.models, gg.nh, gg.tu
H, W, N, NC, NF, STD = 6, 8, 24, 8, 8, 0.2
R, RV = 12, 8
NDC_BOX = [[-1.2, -1.2, -1.05, -np.pi, -np.pi / 2], [1.2, 1.2, 1.05, np.pi, np.pi / 2]]


def ndc_pose():
    pose = np.eye(4, dtype=np.float32)
    pose[:3, 3] = (0.05, -0.03, 0.1)
    c, s = np.cos(0.1), np.sin(0.1)
    pose[:3, :3] = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], dtype=np.float32)
    return pose


CASES = [dict(ndc=False, pose=gg.POSE, focal=0.5 * W / np.tan(0.5 * 0.6911112), near=2.0, far=6.0, box=gg.BOX, span=3.0, sigma_scale=1.0, shift=0.5),
         dict(ndc=True, pose=ndc_pose(), focal=7.0, near=0.0, far=1.0, box=NDC_BOX, span=1.0, sigma_scale=8.0, shift=3.0)]


def build(case, g11, seed):
    """coarse + fine model wired as gen_golden.build_models wires them, g11's decoders, this fixture's planes and box, fc_alpha calibrated"""
    sid, mc, mf, _, _ = gg.build_models(R, RV, 0.5, seed=27)
    mc.load_state_dict({k[len("coarse."):]: torch.from_numpy(v) for k, v in g11.items() if k.startswith("coarse.")}, strict=False)
    mf.load_state_dict({k[len("fine."):]: torch.from_numpy(v) for k, v in g11.items() if k.startswith("fine.")}, strict=False)
    names = [models.get_plane_name(sid, d) for d in range(4)]
    torch.manual_seed(270)
    planes = nn.ParameterDict([(names[d], nn.Parameter(0.5 * torch.randn(1, 48, *((R, R) if d < 3 else (RV, RV))))) for d in range(4)])
    box = torch.tensor(case["box"], dtype=torch.float64)
    for m in (mc, mf):
        m.planes_ = planes
        m.box_coords = {sid: box}
        m.set_cur_scene_id(sid)
    with torch.no_grad():
        g = torch.Generator().manual_seed(seed)
        pts = (torch.rand(4096, 3, generator=g) * 2 - 1) * case["span"]
        d = torch.randn(4096, 3, generator=g)
        x = torch.cat([pts, d / d.norm(dim=-1, keepdim=True)], -1)
        for m in (mc, mf):
            m.eval()
            scale = case["sigma_scale"] / float(m(x)[:, 3].std())
            m.fc_alpha["0"].weight.mul_(scale)
            m.fc_alpha["0"].bias.mul_(scale)
            m.fc_alpha["0"].bias.add_(-float(m(x)[:, 3].mean()) - case["shift"])
    return sid, mc, mf, planes, names, box


def run(case, sid, mc, mf, planes, names, sel, target, dtype, seed):
    """one differentiated training render in `dtype` -> dict of results"""
    for m in (mc, mf):
        m.to(dtype)
        m.train()
    for p in planes.values():
        p.grad = None
    vt = gg.mode_cfg(NC, NF, perturb=True, noise=STD)
    key = "llff" if case["ndc"] else "synt"
    cfg = gg.CfgNode({"nerf": {"use_viewdirs": True, "train": vt, "validation": vt},
                      "dataset": {key: {"near": case["near"], "far": case["far"], "no_ndc": not case["ndc"]}}})
    pose = torch.tensor(case["pose"], dtype=dtype, requires_grad=True)
    ro, rd = nh.get_ray_bundle(H, W, case["focal"], pose)
    batch_rays = torch.stack([ro.reshape(-1, 3)[sel], rd.reshape(-1, 3)[sel]], 0)
    batch_rays.retain_grad()
    zrec = []
    real_rn, real_no_grad = tu.run_network, torch.no_grad

    def rec_rn(*a, **k):
        zrec.append(k["z_vals"].detach().clone())
        return real_rn(*a, **k)

    tu.run_network = rec_rn
    torch.no_grad = contextlib.nullcontext                            # shim B
    try:
        torch.manual_seed(seed)
        rc, dc, ac, rf, df, af, *_ = tu.run_one_iter_of_nerf(H, W, case["focal"], mc, mf, batch_rays, cfg, scene_id=sid, mode="train",
                                                             scene_config=cfg.dataset[key])
    finally:
        tu.run_network, torch.no_grad = real_rn, real_no_grad
    tgt = target.to(dtype)
    loss = torch.nn.functional.mse_loss(rc, tgt) + torch.nn.functional.mse_loss(rf, tgt)
    loss.backward()
    assert zrec[1].shape == (N, NC + NF) and zrec[1].dtype == dtype and rc.dtype == dtype
    return dict(z_fine=gg.npy(zrec[1]), rgb_coarse=gg.npy(rc), rgb_fine=gg.npy(rf), loss=np.array(float(loss)), rays_grad=gg.npy(batch_rays.grad),
                pose_grad=gg.npy(pose.grad), planes=[gg.npy(planes[n].grad) for n in names])


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b))


def main():
    g11 = dict(np.load(os.path.join(gg.HERE, "g11_grads.npz")))
    torch.Tensor.cpu = lambda s, *a, **k: s.detach()                  # shim A
    arrs = dict(g11_decoders=decoder_checksum(g11), hw=np.array([H, W]), params=np.array([NC, NF, STD]))
    for ci, case in enumerate(CASES):
        sid, mc, mf, planes, names, box = build(case, g11, seed=271 + ci)
        pre = "c%d_" % ci
        rng = np.random.default_rng(2700 + ci)
        sel = rng.permutation(H * W)[:N]
        sel[[5, 17]] = sel[[2, 2]]                                    # pixels drawn twice (and three times)
        sel[21] = sel[9]
        torch.manual_seed(272 + ci)
        target = torch.rand(N, 3)
        seed = 273 + 10 * ci
        sel_t = torch.from_numpy(sel)
        r32 = run(case, sid, mc, mf, planes, names, sel_t, target, torch.float32, seed)
        state32 = {**gg.state_arrays("coarse.", mc), **gg.state_arrays("fine.", mf)}
        planes32 = [gg.npy(planes[n]) for n in names]
        r64 = run(case, sid, mc, mf, planes, names, sel_t, target, torch.float64, seed)
        for m in (mc, mf):
            m.to(torch.float32)
        torch.manual_seed(seed)                                       # the draws, in upstream's order
        arrs[pre + "t_rand"] = gg.npy(torch.rand(N, NC))
        arrs[pre + "noise_coarse"] = gg.npy(torch.randn(N, NC) * STD)
        arrs[pre + "u"] = gg.npy(torch.rand(N, NF))
        arrs[pre + "noise_fine"] = gg.npy(torch.randn(N, NC + NF) * STD)
        arrs.update({pre + "sel": sel.astype(np.int32), pre + "target": gg.npy(target), pre + "pose": case["pose"], pre + "box": gg.npy(box),
                     pre + "scene": np.array([case["focal"], case["near"], case["far"], float(case["ndc"])])})
        for k in ("z_fine", "rgb_coarse", "rgb_fine", "loss", "rays_grad", "pose_grad"):
            arrs[pre + k] = r32[k]
        for k in ("z_fine", "loss", "rays_grad", "pose_grad"):
            arrs[pre + k + "64"] = r64[k]
        for d in range(4):
            arrs[pre + "grad_plane%d" % d] = r32["planes"][d]
            arrs[pre + "grad64_plane%d" % d] = r64["planes"][d].astype(np.float32)
            if ci == 0:
                arrs["plane%d" % d] = planes32[d]
            else:
                assert np.array_equal(arrs["plane%d" % d], planes32[d])
        for k, v in state32.items():
            assert k in g11 and v.shape == g11[k].shape, k
            if not np.array_equal(v, g11[k]):
                arrs[pre + k] = v.copy()
        flips = np.abs(r32["z_fine"] - r64["z_fine"]).max(1) > 1e-5 * np.abs(r64["z_fine"]).max(1)
        print("   case %d (%s): loss %.5f; float32 vs float64 relative L2: rays %.3g, pose %.3g, plane0 %.3g; rays whose fine depths differ: %d; "
              "|rays_grad| %.3g, |pose_grad| %.3g; decoder entries that differ from g11: %s" % (
                  ci, "ndc" if case["ndc"] else "synthetic", float(r32["loss"]), rel(r32["rays_grad"], r64["rays_grad"]),
                  rel(r32["pose_grad"], r64["pose_grad"]), rel(r32["planes"][0], r64["planes"][0]), int(flips.sum()),
                  float(np.abs(r64["rays_grad"]).mean()), float(np.abs(r64["pose_grad"]).mean()),
                  sorted(k for k in arrs if k.startswith(pre + "coarse.") or k.startswith(pre + "fine."))))
    gg.save("g27_ray_grad.npz", **arrs)


if __name__ == "__main__":
    main()
