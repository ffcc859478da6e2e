"""float64 restatement of TwoDimPlanesModel.forward for ANY decoder geometry in torch on the CPU, so that torch.autograd gives reference
PLANE gradients for a cotangent.  A helper of the training tests of the generic geometries (tests/test_generic_train_fused*.py), not a test.

It is oracle/generic_decoder.py's forward (the float32 normalisation and projection matrices, then float64: grid_sample in double -- bilinear or
bicubic, padding_mode='border', either align_corners --, combine_pos_planes, combine_all_planes, skip layers, heads) on torch tensors; the
planes are leaves.  Pinned against the reference's own float32 autograd (tests/golden/g19_decoder_variant_grads.npz) in
tests/test_generic_train_fused_host.py."""
import numpy as np
import torch
import torch.nn.functional as F


def is_skip_layer(layer_num, skip_connect_every):
    return skip_connect_every is not None and layer_num % skip_connect_every == 0 and layer_num > 0


def forward(sd, planes, box, x, dec_density_layers=4, dec_rgb_layers=4, skip_connect_every=None, proj_combination="sum",
            viewdir_proj_combination=None, align_corners=True, coord_noise=None, plane_interp="bilinear", **_ignored):
    """sd: state dict (numpy arrays, reference key names); planes: float64 torch tensors [1,C,H,W], the position planes then the view plane;
    box [2,5]; x [P,6] numpy -> [P,4] float64 torch tensor (differentiable in the planes)"""
    view_rule = viewdir_proj_combination or proj_combination
    x = np.asarray(x, np.float32)
    d = x[:, 3:]
    az = np.arctan2(d[:, 1], d[:, 0])
    el = np.arctan2(d[:, 2], np.sqrt(d[:, 0] ** 2 + d[:, 1] ** 2))
    x5 = np.concatenate([x[:, :3], az[:, None], el[:, None]], 1).astype(np.float32)
    box = np.asarray(box, np.float64)
    lo, rng = box[0].astype(np.float32), (box[1] - box[0]).astype(np.float32)
    n5 = 2 * (x5 - lo) / rng - 1
    if coord_noise is not None:
        n5[:, :3] = n5[:, :3] + np.asarray(coord_noise, np.float32)
    n5 = n5.astype(np.float64)
    n_pos = len(planes) - 1

    def sample(plane, g):
        grid = torch.as_tensor(np.ascontiguousarray(g), dtype=torch.float64).reshape(1, 1, -1, 2)
        out = F.grid_sample(plane, grid, mode=plane_interp, padding_mode="border", align_corners=bool(align_corners))      # [1,C,1,P]
        return out[0, :, 0, :].T

    pos = []
    for dnum in range(n_pos):
        rot = np.asarray(sd["coord_projector.rot_mats_NON_LEARNED.%d" % dnum]).astype(np.float32).astype(np.float64)
        pos.append(sample(planes[dnum], n5[:, :3] @ rot[:, 1:]))
    view = sample(planes[n_pos], n5[:, 3:5])

    def combine_pos():
        if proj_combination == "sum":
            return torch.stack(pos, 0).sum(0)
        if proj_combination == "avg":
            return torch.stack(pos, 0).mean(0)
        return torch.cat(pos, 1)

    def w(key):
        return torch.as_tensor(np.asarray(sd[key], np.float64))

    def mlp(inp, name, nlayers, head):
        h = inp
        for l in range(nlayers):
            if is_skip_layer(l - 1, skip_connect_every):
                h = torch.cat([h, inp], 1)
            h = torch.relu(h @ w("%s.0.%d.weight" % (name, l)).T + w("%s.0.%d.bias" % (name, l)))
        return h @ w(head + ".0.weight").T + w(head + ".0.bias")

    alpha = mlp(combine_pos(), "density_dec", dec_density_layers, "fc_alpha")
    if view_rule == "concat_pos":
        rgb_in = torch.cat(pos + [view], 1)
    elif view_rule == "concat":
        rgb_in = torch.cat([combine_pos(), view], 1)
    else:
        pp = combine_pos()
        assert pp.shape[1] == view.shape[1]
        rgb_in = pp + view if view_rule == "sum" else (pp + view) / 2 if view_rule == "avg" else pp * (1 + view)
        assert view_rule in ("sum", "avg", "mult")
    return torch.cat([mlp(rgb_in, "rgb_dec", dec_rgb_layers, "fc_rgb"), alpha], 1)


def plane_gradients(sd, planes, box, x, cotangent, **kw):
    """-> (out [P,4] float64 numpy, [d sum(out * cotangent) / d plane] as float64 numpy [1,C,H,W]); planes: numpy arrays"""
    leaves = [torch.as_tensor(np.asarray(p, np.float64)).clone().requires_grad_(True) for p in planes]
    out = forward(sd, leaves, box, x, **kw)
    if out.shape[0]:
        (out * torch.as_tensor(np.asarray(cotangent, np.float64))).sum().backward()
    return out.detach().numpy(), [np.zeros(tuple(p.shape)) if p.grad is None else p.grad.numpy() for p in leaves]


def rel_l2(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b))
