"""Golden fixture of both FlexibleNeRFModel baselines at ragged sample counts, computed by the UPSTREAM code on the CPU.

Re-run:  NVSR_REFERENCE_DIR=<upstream checkout> python tests/golden/gen_golden_nerf_ragged.py

  g25_nerf_ragged.npz     keys mip.* (the Mip-NeRF baseline of gen_golden_mip.py) and pe.* (the positional-encoding one of gen_golden_pe.py)
    *.b.m*.checksum   the two models: mip_params / pe_params.state_dict(SEEDS) (not stored: their float64 sum and sum of squares)
    *.c.*             run_one_iter_of_nerf in validation mode, 7 x 11 rays, 33 + 17 samples, without NDC (c.*) and with NDC (c.ndc.*): rgb /
                      disp / acc of both passes and the depths each pass was evaluated at (run_network wrapped; Mip: interval edges), every
                      ray.  No pass has a multiple of 32 points: Mip 77 x 33 = 2 541 and 77 x 51 = 3 927, PE 77 x 33 and 77 x 50 = 3 850
    *.d.*             train mode (perturb, noise 0.2) with torch.manual_seed(25 / 26) before the call: the outputs and the gradient of
                      MSE(coarse) + MSE(fine) against a seeded target for every parameter of both models (at mip_params.kept_elements)
    *.chunksize       128 (Mip, which divides it by 4) and 32 (PE): the reference draws its random numbers per 32 rays, chunks of 32, 32, 13
    *.num_coarse / *.num_fine
The models are m0 (coarse) and m1 (fine) throughout."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as gg  # noqa: E402  (imports the upstream modules behind the shims)
import gen_golden_mip as gmip  # noqa: E402
import gen_golden_pe as gpe  # noqa: E402
import mip_params  # noqa: E402
import pe_params  # noqa: E402

H, W = 7, 11
NC, NF = 33, 17
BASELINES = (("mip", gmip, mip_params, 128, 25), ("pe", gpe, pe_params, 32, 26))
OUTS = ("rgb_coarse", "disp_coarse", "acc_coarse", "rgb_fine", "disp_fine", "acc_fine")


def record(gen, params, chunk, seed):
    npy = gen.npy
    out = {"chunksize": np.array(chunk), "num_coarse": np.array(NC), "num_fine": np.array(NF)}
    ms = [gen.model(s) for s in params.SEEDS]
    for i, m in enumerate(ms):
        out["b.m%d.checksum" % i] = params.checksum({k: npy(v) for k, v in m.state_dict().items()})
    mc, mf = ms
    focal = 0.5 * W / np.tan(0.5 * 0.6911112)
    ro, rd = gg.nh.get_ray_bundle(H, W, focal, torch.from_numpy(gg.POSE))
    out.update({"c.ro": npy(ro.contiguous()), "c.rd": npy(rd.contiguous()), "c.hwf": np.array([H, W, focal])})
    for tag, ndc in (("c.", False), ("c.ndc.", True)):
        z = []
        with torch.no_grad():
            o = gen.run(mc, mf, H, W, focal, ro, rd, gen.cfg(NC, NF, chunk=chunk, ndc=ndc), "validation", z)
        for j, key in enumerate(OUTS):
            out[tag + key] = npy(o[j])
        # (run_network is called per ray chunk, coarse then fine)
        out[tag + "z_coarse"], out[tag + "z_fine"] = npy(torch.cat(z[0::2])), npy(torch.cat(z[1::2]))
    target = torch.rand(H * W, 3, generator=torch.Generator().manual_seed(seed))
    out["d.target"] = npy(target)
    torch.manual_seed(seed)
    o = gen.run(mc, mf, H, W, focal, ro, rd, gen.cfg(NC, NF, perturb=True, noise=0.2, chunk=chunk), "train")
    loss = torch.nn.functional.mse_loss(o[0], target) + torch.nn.functional.mse_loss(o[3], target)
    loss.backward()
    for j, key in enumerate(OUTS):
        out["d." + key] = npy(o[j])
    out["d.loss"] = npy(loss)
    for i, m in enumerate(ms):
        for k, p in m.named_parameters():
            out["d.m%d.grad.%s" % (i, k)] = params.kept(k, npy(p.grad))
    return out


def main():
    torch.set_num_threads(8)
    out = {}
    for name, gen, params, chunk, seed in BASELINES:
        out.update({"%s.%s" % (name, k): v for k, v in record(gen, params, chunk, seed).items()})
    path = os.path.join(HERE, "g25_nerf_ragged.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, len(out), "arrays, %.1f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
