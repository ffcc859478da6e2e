"""Golden fixture of the low-rank feature planes (models.py:223-230, 541-548), computed by the UPSTREAM code on the CPU.

Re-run:  NVSR_REFERENCE_DIR=<upstream checkout> python tests/golden/gen_golden_lowrank.py

  g26_lowrank.npz
    scene lego_DS8_PlRes12_6, 48 channels; the three position planes are stored as factor tensors [1,48,12,2r] with
    plane_rank = {D0: 3, D1: 5, D2: 12} (N(0, 0.5^2) entries), the view-direction plane [1,48,6,6] dense
    coarse.* / fine.*     the entries of both decoders' state dicts that DIFFER from g11_grads.npz's: the decoders are g11's (two full state
                          dicts are 1 MB, over the size limit of a committed file) with fc_alpha calibrated ON THE LOW-RANK SCENE the way
                          gen_golden.build_models does for g11 (sigma straddles zero, so the fine pass has importance samples to place);
                          a reader takes g11's coarse.* / fine.* and overwrites them with these.  box, hwf
    g11_decoders          [float64 sum, sum of squares, element count] over g11's coarse.* / fine.* arrays in sorted key order, as this fixture was
                          made from them: g26 DEPENDS on g11_grads.npz, and a reader checks these three numbers first (decoder_checksum below), so
                          that a regenerated g11 fails loudly here instead of quietly changing the scene -- regenerate g26 after g11
    plane0..3             the `planes_` entries (factors for 0..2), ranks
    generated0..2         the planes upstream's gen_plane made of them (torch.matmul on the CPU)
    rays, target          8 x 8 rays of POSE, a seeded target
    rgb_coarse, rgb_fine, loss    run_one_iter_of_nerf(mode='train'), 8 + 8 samples, perturb off, noise 0; loss = MSE(coarse) + MSE(fine)
    grad_plane0..3        the gradient of the loss for every `planes_` entry (the factors' for 0..2)"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as gg  # noqa: E402  (imports the upstream modules behind the shims)

nh, models, tu = gg.nh, gg.models, gg.tu
RANKS = (3, 5, 12)


def decoder_checksum(arrays):
    """[sum, sum of squares, count] in float64 over the coarse.* / fine.* entries of an npz dict, sorted by key"""
    vals = [np.asarray(arrays[k], dtype=np.float64).reshape(-1) for k in sorted(arrays) if k.startswith(("coarse.", "fine."))]
    flat = np.concatenate(vals)
    return np.array([flat.sum(), np.square(flat).sum(), flat.size], dtype=np.float64)


def main():
    R, Rv, H, W, nc, nf = 12, 6, 8, 8, 8, 8
    sid, mc, mf, planes, box = gg.build_models(R, Rv, 0.5, seed=26)
    g11 = dict(np.load(os.path.join(gg.HERE, "g11_grads.npz")))
    for prefix, m in (("coarse.", mc), ("fine.", mf)):
        m.load_state_dict({k[len(prefix):]: torch.from_numpy(v) for k, v in g11.items() if k.startswith(prefix)}, strict=False)
    names = [models.get_plane_name(sid, d) for d in range(4)]
    torch.manual_seed(260)
    factors = nn.ParameterDict([(names[d], models.create_plane([R, 2 * RANKS[d]], 48, 0.5)) for d in range(3)] + [(names[3], planes[names[3]])])
    rank = {names[d]: RANKS[d] for d in range(3)}
    generated = {}
    for m in (mc, mf):
        m.planes_, m.plane_rank, m.generated_planes = factors, rank, generated
    # fc_alpha was calibrated for the dense planes build_models drew: once more, for the planes this scene generates
    with torch.no_grad():
        g = torch.Generator().manual_seed(27)
        pts = torch.rand(4096, 3, generator=g) * 6 - 3
        d = torch.randn(4096, 3, generator=g)
        x = torch.cat([pts, d / d.norm(dim=-1, keepdim=True)], -1)
        for m in (mc, mf):
            m.eval()
            scale = 1.0 / float(m(x)[:, 3].std())
            m.fc_alpha["0"].weight.mul_(scale)
            m.fc_alpha["0"].bias.mul_(scale)
            m.fc_alpha["0"].bias.add_(-float(m(x)[:, 3].mean()) - 0.5)
    generated.clear()

    focal = 0.5 * W / np.tan(0.5 * 0.6911112)
    ro, rd = nh.get_ray_bundle(H, W, focal, torch.from_numpy(gg.POSE))
    rays = torch.stack([ro.reshape(-1, 3), rd.reshape(-1, 3)], 0)
    torch.manual_seed(261)
    target = torch.rand(H * W, 3)
    arrs = dict(box=gg.npy(box), hwf=np.array([H, W, focal], dtype=np.float64), ranks=np.array(RANKS), samples=np.array([nc, nf]),
                rays=gg.npy(rays), target=gg.npy(target), g11_decoders=decoder_checksum(g11))
    for prefix, m in (("coarse.", mc), ("fine.", mf)):
        for k, v in gg.state_arrays(prefix, m).items():
            assert k in g11 and v.shape == g11[k].shape, k
            if not np.array_equal(v, g11[k]):
                arrs[k] = v.copy()
    print("   decoder entries that differ from g11:", sorted(k for k in arrs if k.startswith(("coarse.", "fine."))))
    for dnum in range(4):
        arrs["plane%d" % dnum] = gg.npy(factors[names[dnum]]).copy()
    vt = gg.mode_cfg(nc, nf, perturb=False, noise=0.0)
    cfg = gg.make_cfg(vt, vt)
    mc.train(); mf.train()
    rc, _, _, rf, *_ = tu.run_one_iter_of_nerf(H, W, focal, mc, mf, rays, cfg, scene_id=sid, mode="train", scene_config=cfg.dataset["synt"])
    loss = torch.nn.functional.mse_loss(rc, target) + torch.nn.functional.mse_loss(rf, target)
    loss.backward()
    for dnum in range(3):
        arrs["generated%d" % dnum] = gg.npy(generated[names[dnum]]).copy()
    arrs.update(rgb_coarse=gg.npy(rc), rgb_fine=gg.npy(rf), loss=np.array(float(loss.detach())))
    for dnum in range(4):
        arrs["grad_plane%d" % dnum] = gg.npy(factors[names[dnum]].grad).copy()
    print("   loss %.5f; rgb_fine spread %.3f; nonzero factor-gradient fraction %s" % (
        float(loss), float(rf.std()), ["%.2f" % float((factors[names[d]].grad != 0).float().mean()) for d in range(3)]))
    gg.save("g26_lowrank.npz", **arrs)


if __name__ == "__main__":
    main()
