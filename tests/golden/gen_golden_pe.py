"""Golden fixture of the positional-encoding NeRF baseline (MipNeRF_baseline.yml with encode_position_fn: positional_encoding), computed by
the UPSTREAM code on the CPU.

Re-run:  NVSR_REFERENCE_DIR=<upstream checkout> python tests/golden/gen_golden_pe.py

  g24_pe_nerf.npz
    a.*   seeded packed rays and sample depths without NDC (24 x 16; |x| up to ~6: degree-5 arguments near 200 rad) and with NDC (a.ndc.*,
          12 x 16); positional_encoding(pts, 6, True) of the points ro + rd z as the reference forms them (train_utils.py:111; 39 columns, the
          first 3 are the points) and positional_encoding(viewdir, 4, True) (27 columns)
    b.*   two FlexibleNeRFModel(num_encoding_fn_xyz=6, num_encoding_fn_dir=4, include_input_xyz=True, include_input_dir=True) with the
          parameters of pe_params.state_dict(303 / 404) (not stored: b.m*.checksum holds their float64 sum and sum of squares) and their
          forward on the rows of (a), without and with NDC
    c.*   run_one_iter_of_nerf in validation mode, 16 x 16 rays, scene lego, 64 + 64 samples: without NDC (c.*) and with NDC (c.ndc.*);
          rgb / disp / acc of both passes, and the depths each pass was evaluated at (run_network wrapped) for the first 32 rays
    d.*   train mode (perturb, noise 0.2, chunksize 100 -> reference ray chunks of 100, 100 and 56) with torch.manual_seed(24) before the call:
          outputs and the gradient of MSE(coarse) + MSE(fine) against a seeded target for every parameter of both models (at
          pe_params.kept_elements)
    e.*   three Adam steps (lr 1e-3, all parameters of both models) of that loss, fresh draws per step after torch.manual_seed(31): the loss per
          step and the parameters afterwards (at pe_params.kept_elements)
The models are b.m0 (coarse) and b.m1 (fine) throughout."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as gg  # noqa: E402  (imports the upstream modules behind the shims)
import pe_params  # noqa: E402

nh, models, tu, CfgNode = gg.nh, gg.models, gg.tu, gg.CfgNode


def npy(t):
    return gg.npy(t).copy()         # (a CPU tensor's numpy() shares its memory: the Adam steps of (e) must not rewrite the arrays of (b))


SID = "lego"


def pack(ro, rd, near, far, viewsrc=None):
    v = rd if viewsrc is None else viewsrc
    vd = v / v.norm(p=2, dim=-1, keepdim=True)
    n = ro.shape[0]
    return torch.cat((ro, rd, near * torch.ones(n, 1), far * torch.ones(n, 1), vd), -1)


def pos_enc(x):
    return nh.positional_encoding(x, 6, True)


def dir_enc(x):
    return nh.positional_encoding(x, 4, True)


def model(seed):
    m = models.FlexibleNeRFModel(num_encoding_fn_xyz=6, num_encoding_fn_dir=4, include_input_xyz=True, include_input_dir=True, use_viewdirs=True)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in pe_params.state_dict(seed).items()})
    m.optional_no_grad = _Null
    return m


class _Null:
    def __enter__(self):
        return None

    def __exit__(self, *a):
        return False


def cfg(nc, nf, perturb=False, noise=0.0, chunk=131072, ndc=False):
    mode = dict(chunksize=chunk, perturb=perturb, num_coarse=nc, num_fine=nf, white_background=False, radiance_field_noise_std=noise, lindisp=False)
    return CfgNode({"nerf": {"use_viewdirs": True, "encode_position_fn": "positional_encoding", "train": mode, "validation": mode},
                    "dataset": {"synt": {"near": 0.0 if ndc else 2.0, "far": 1.0 if ndc else 6.0, "no_ndc": not ndc}}})


def run(mc, mf, H, W, focal, ro, rd, opts, mode, record=None):
    real = tu.run_network

    def rec(network_fn, *a, **k):
        if record is not None:
            record.append(k["z_vals"].detach().clone())
        return real(network_fn, *a, **k)

    tu.run_network = rec
    try:
        return tu.run_one_iter_of_nerf(H, W, focal, mc, mf, torch.stack((ro.reshape(-1, 3), rd.reshape(-1, 3))), opts, SID, mode=mode,
                                       encode_position_fn=pos_enc, encode_direction_fn=dir_enc, scene_config=opts.dataset.synt)
    finally:
        tu.run_network = real


def encode(rays, z):
    """the reference's points and rows for packed rays [n,11] and depths z [n,S] (train_utils.py:111, run_network's encoders)"""
    n, S = z.shape
    ro, rd = rays[..., :3], rays[..., 3:6]
    pts = ro[..., None, :] + rd[..., None, :] * z[..., :, None]
    enc = pos_enc(pts.reshape(-1, 3))
    dirs = dir_enc(rays[:, None, 8:11].expand(n, S, 3).reshape(-1, 3))
    return pts, enc, dirs


def main():
    torch.set_num_threads(8)
    out = {"scene_id": np.array(SID)}
    # (a) rays: random origins in [-1, 1]^3, unit directions, depths in [2, 5] (|x| <= 6); one ray far out; and NDC rays of a forward view
    g = torch.Generator().manual_seed(12)
    n, S = 24, 16
    ro = (torch.rand(n, 3, generator=g) - 0.5) * 2.0
    rd = torch.randn(n, 3, generator=g)
    rd = rd / rd.norm(dim=-1, keepdim=True)
    ro[1] = torch.tensor([1.0, -1.0, 1.0])
    rd[1] = torch.tensor([1.0, -1.0, 1.0]) / np.sqrt(3.0)
    rays = pack(ro, rd, 2.0, 6.0)
    z = torch.sort(2.0 + 3.0 * torch.rand(n, S, generator=g), -1)[0]
    z[1, -1] = 5.0
    _, enc, dirs = encode(rays, z)
    out.update({"a.rays": npy(rays), "a.z": npy(z), "a.enc": npy(enc), "a.dirs": npy(dirs)})
    Hn = Wn = 16
    focal_n = 0.5 * Wn / np.tan(0.5 * 0.6911112)
    nn = 12
    ro_n = torch.zeros(nn, 3) + torch.tensor([0.1, -0.2, 0.3])
    rd_n = torch.cat((0.4 * (torch.rand(nn, 2, generator=g) - 0.5), -torch.ones(nn, 1)), -1)
    o_ndc, d_ndc = nh.ndc_rays(Hn, Wn, focal_n, 1.0, ro_n, rd_n)
    rays_n = pack(o_ndc, d_ndc, 0.0, 1.0, viewsrc=rd_n)
    z_n = torch.sort(torch.rand(nn, S, generator=g), -1)[0]
    _, enc_n, dirs_n = encode(rays_n, z_n)
    out.update({"a.ndc.rays": npy(rays_n), "a.ndc.z": npy(z_n), "a.ndc.enc": npy(enc_n), "a.ndc.dirs": npy(dirs_n)})
    # (b) two models on the rows of (a)
    ms = [model(s) for s in pe_params.SEEDS]
    for i, m in enumerate(ms):
        out["b.m%d.checksum" % i] = pe_params.checksum({k: npy(v) for k, v in m.state_dict().items()})
        with torch.no_grad():
            out["b.m%d.raw" % i] = npy(m(torch.cat((enc, dirs), -1)))
            out["b.m%d.ndc.raw" % i] = npy(m(torch.cat((enc_n, dirs_n), -1)))
    mc, mf = ms
    # (c) validation renders
    H = W = 16
    focal = 0.5 * W / np.tan(0.5 * 0.6911112)
    ro_v, rd_v = nh.get_ray_bundle(H, W, focal, torch.from_numpy(gg.POSE))
    out.update({"c.ro": npy(ro_v.contiguous()), "c.rd": npy(rd_v), "c.hwf": np.array([H, W, focal])})
    for tag, ndc in (("c.", False), ("c.ndc.", True)):
        zs = []
        with torch.no_grad():
            o = run(mc, mf, H, W, focal, ro_v, rd_v, cfg(64, 64, ndc=ndc), "validation", zs)
        for j, key in enumerate(("rgb_coarse", "disp_coarse", "acc_coarse", "rgb_fine", "disp_fine", "acc_fine")):
            out[tag + key] = npy(o[j])
        out[tag + "z_coarse"], out[tag + "z_fine"] = npy(zs[0][:32]), npy(zs[1][:32])
    # (d) one training iteration
    target = torch.rand(H * W, 3, generator=torch.Generator().manual_seed(6))
    out["d.target"] = npy(target)
    opts = cfg(64, 64, perturb=True, noise=0.2, chunk=100)
    torch.manual_seed(24)
    o = run(mc, mf, H, W, focal, ro_v, rd_v, opts, "train")
    loss = torch.nn.functional.mse_loss(o[0], target) + torch.nn.functional.mse_loss(o[3], target)
    loss.backward()
    for j, key in enumerate(("rgb_coarse", "disp_coarse", "acc_coarse", "rgb_fine", "disp_fine", "acc_fine")):
        out["d." + key] = npy(o[j])
    out["d.loss"] = npy(loss)
    for i, m in enumerate(ms):
        for k, p in m.named_parameters():
            out["d.m%d.grad.%s" % (i, k)] = pe_params.kept(k, npy(p.grad))
    # (e) three Adam steps from the (b) parameters
    for m in ms:
        m.zero_grad()
    params = list(mc.parameters()) + list(mf.parameters())
    opt = torch.optim.Adam(params, lr=1e-3)
    torch.manual_seed(31)
    losses = []
    for _ in range(3):
        opt.zero_grad()
        o = run(mc, mf, H, W, focal, ro_v, rd_v, opts, "train")
        loss = torch.nn.functional.mse_loss(o[0], target) + torch.nn.functional.mse_loss(o[3], target)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    out["e.losses"] = np.array(losses, dtype=np.float64)
    for i, m in enumerate(ms):
        for k, p in m.named_parameters():
            out["e.m%d.%s" % (i, k)] = pe_params.kept(k, npy(p))
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "g24_pe_nerf.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, len(out), "arrays; losses", losses)


if __name__ == "__main__":
    main()
