"""Golden fixture of the Mip-NeRF baseline (MipNeRF_baseline.yml), computed by the UPSTREAM code on the CPU.

Re-run:  NVSR_REFERENCE_DIR=<upstream checkout> python tests/golden/gen_golden_mip.py

  g23_mip_nerf.npz
    a.*   cast_rays means / covariances (mip.py:9-44) and IntegratedPositionalEncoding(3, 7) (mip.py:154-199) on seeded packed rays and interval
          edges -- a near-axis direction, very short intervals, degree-5 arguments above 100 rad -- plus positional_encoding(viewdir, 4) (27 columns)
    b.*   two FlexibleNeRFModel(include_input_xyz=False) with the parameters of mip_params.state_dict(101 / 202) (not stored: b.m*.checksum
          holds their float64 sum and sum of squares) and their forward on the rows of (a)
    c.*   run_one_iter_of_nerf in validation mode, 16 x 16 rays, scene lego_DS8, 64 + 64 samples: without NDC (c.*) and with NDC (c.ndc.*);
          rgb / disp / acc of both passes, and the edges each pass was evaluated at (run_network wrapped) for the first 32 rays
    d.*   train mode (perturb, noise 0.2, chunksize 400 -> reference ray chunks of 100) with torch.manual_seed(23) before the call: outputs and the
          gradient of MSE(coarse) + MSE(fine) against a seeded target for every parameter of both models (at mip_params.kept_elements)
    e.*   three Adam steps (lr 1e-3, all parameters of both models) of that loss, fresh draws per step after torch.manual_seed(29): the loss per
          step and the parameters afterwards (at mip_params.kept_elements)
The models are b.m0 (coarse) and b.m1 (fine) throughout."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as gg  # noqa: E402  (imports the upstream modules behind the shims)
import mip_params  # noqa: E402

import mip  # noqa: E402  (upstream, on sys.path after import_reference)

nh, models, tu, CfgNode = gg.nh, gg.models, gg.tu, gg.CfgNode


def npy(t):
    return gg.npy(t).copy()         # (a CPU tensor's numpy() shares its memory: the Adam steps of (e) must not rewrite the arrays of (b))


SID = "lego_DS8"
RADIUS = 8 * 0.00135 * 2 / np.sqrt(12.0)


def pack(ro, rd, near, far, viewsrc=None):
    v = rd if viewsrc is None else viewsrc
    vd = v / v.norm(p=2, dim=-1, keepdim=True)
    n = ro.shape[0]
    return torch.cat((ro, rd, near * torch.ones(n, 1), far * torch.ones(n, 1), vd), -1)


def ipe():
    return mip.IntegratedPositionalEncoding(3, 7)


def dir_enc(x):
    return nh.positional_encoding(x, 4, True)


def model(seed):
    m = models.FlexibleNeRFModel(num_encoding_fn_xyz=6, num_encoding_fn_dir=4, include_input_xyz=False, include_input_dir=True, use_viewdirs=True)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in mip_params.state_dict(seed).items()})
    m.optional_no_grad = tu.__dict__.get("null_with") or _Null
    return m


class _Null:
    def __enter__(self):
        return None

    def __exit__(self, *a):
        return False


def cfg(nc, nf, perturb=False, noise=0.0, chunk=131072, ndc=False):
    mode = dict(chunksize=chunk, perturb=perturb, num_coarse=nc, num_fine=nf, white_background=False, radiance_field_noise_std=noise, lindisp=False)
    return CfgNode({"nerf": {"use_viewdirs": True, "encode_position_fn": "mip", "train": mode, "validation": mode},
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
                                       encode_position_fn=ipe(), encode_direction_fn=dir_enc, scene_config=opts.dataset.synt)
    finally:
        tu.run_network = real


def main():
    torch.set_num_threads(8)
    out = {"radius": np.array(RADIUS), "scene_id": np.array(SID)}
    # (a) rays: random origins / directions, one near-axis direction, one ray far out (degree-5 arguments > 100 rad)
    g = torch.Generator().manual_seed(11)
    n, S = 24, 16
    ro = (torch.rand(n, 3, generator=g) - 0.5) * 4.0
    rd = torch.randn(n, 3, generator=g)
    rd[0] = torch.tensor([1e-4, -2e-4, 1.0])
    ro[1] = torch.tensor([3.5, -3.0, 2.0])
    rays = pack(ro, rd, 2.0, 6.0)
    edges = torch.sort(2.0 + 4.0 * torch.rand(n, S + 1, generator=g), -1)[0]
    edges[2] = 2.0 + torch.arange(S + 1) * 1e-5              # very short intervals
    edges[3, 5:] = edges[3, 5:] + 1e-6
    means, covs = mip.cast_rays(edges, rays[:, :3], rays[:, 3:6], RADIUS, None)
    enc = ipe()((means, covs)).reshape(n * S, 36)
    dirs = dir_enc(rays[:, None, 8:11].expand(n, S, 3).reshape(-1, 3))
    out.update({"a.rays": npy(rays), "a.edges": npy(edges), "a.means": npy(means), "a.covs": npy(covs), "a.ipe": npy(enc), "a.dirs": npy(dirs)})
    # (b) two models on the rows of (a)
    ms = [model(s) for s in mip_params.SEEDS]
    for i, m in enumerate(ms):
        out["b.m%d.checksum" % i] = mip_params.checksum({k: npy(v) for k, v in m.state_dict().items()})
        with torch.no_grad():
            out["b.m%d.raw" % i] = npy(m(torch.cat((enc, dirs), -1)))
    mc, mf = ms
    # (c) validation renders
    H = W = 16
    focal = 0.5 * W / np.tan(0.5 * 0.6911112)
    ro_v, rd_v = nh.get_ray_bundle(H, W, focal, torch.from_numpy(gg.POSE))
    out.update({"c.ro": npy(ro_v.contiguous()), "c.rd": npy(rd_v), "c.hwf": np.array([H, W, focal])})
    for tag, ndc in (("c.", False), ("c.ndc.", True)):
        z = []
        with torch.no_grad():
            o = run(mc, mf, H, W, focal, ro_v, rd_v, cfg(64, 64, ndc=ndc), "validation", z)
        for j, key in enumerate(("rgb_coarse", "disp_coarse", "acc_coarse", "rgb_fine", "disp_fine", "acc_fine")):
            out[tag + key] = npy(o[j])
        out[tag + "edges_coarse"], out[tag + "edges_fine"] = npy(z[0][:32]), npy(z[1][:32])
    # (d) one training iteration
    target = torch.rand(H * W, 3, generator=torch.Generator().manual_seed(5))
    out["d.target"] = npy(target)
    opts = cfg(64, 64, perturb=True, noise=0.2, chunk=400)
    torch.manual_seed(23)
    o = run(mc, mf, H, W, focal, ro_v, rd_v, opts, "train")
    loss = torch.nn.functional.mse_loss(o[0], target) + torch.nn.functional.mse_loss(o[3], target)
    loss.backward()
    for j, key in enumerate(("rgb_coarse", "disp_coarse", "acc_coarse", "rgb_fine", "disp_fine", "acc_fine")):
        out["d." + key] = npy(o[j])
    out["d.loss"] = npy(loss)
    for i, m in enumerate(ms):
        for k, p in m.named_parameters():
            out["d.m%d.grad.%s" % (i, k)] = mip_params.kept(k, npy(p.grad))
    # (e) three Adam steps from the (b) parameters
    for m in ms:
        m.zero_grad()
    params = list(mc.parameters()) + list(mf.parameters())
    opt = torch.optim.Adam(params, lr=1e-3)
    torch.manual_seed(29)
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
            out["e.m%d.%s" % (i, k)] = mip_params.kept(k, npy(p))
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "g23_mip_nerf.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, len(out), "arrays; losses", losses)


if __name__ == "__main__":
    main()
