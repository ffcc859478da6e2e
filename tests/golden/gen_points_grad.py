"""Golden fixture of the tri-plane model's INPUT gradient (x.grad of model(x)), computed by the UPSTREAM code on the CPU.

Re-run:  NVSR_REFERENCE_DIR=<upstream checkout> python tests/golden/gen_points_grad.py

Two facts about upstream shape this file:
  1. CoordProjector.forward runs under torch.no_grad() (models.py:495-497): upstream's x.grad is exactly 0 in the position columns.
  2. normalize_coords calls .cpu().numpy() on a tensor that requires grad (models.py:266-267) and raises.  Shim A, for this script only:
     torch.Tensor.cpu = detach.  Then upstream's forward runs and autograd gives the view-direction columns.
Shim B, for the duration of ONE forward: torch.no_grad = contextlib.nullcontext.  The same upstream code then also gives the position columns,
through torch's own grid_sampler_2d_backward.  The forward's bits are the same with and without shim B (asserted below).

  g23_points_grad.npz
    scene lego_DS8_PlRes7_4, 48 channels: position planes 5x7, 6x4, 7x5 (H x W: a swapped axis shows), view plane 4x3, N(0, 0.5^2) entries
    coarse.*            the entries of the decoder's state dict that DIFFER from g11_grads.npz's coarse.*: g11's decoder with fc_alpha calibrated
                        on this scene as gen_golden.build_models does (sigma straddles zero: mixed ReLU gates); a reader takes g11's coarse.* and
                        overwrites.  g11_decoders: gen_golden_lowrank.decoder_checksum of g11 as this fixture was made from it (checked first)
    plane0..3, box
    x [67,6]            rows 0..7 interior hand-picked, then: beyond the box on one axis (3 rows), exactly on the low / high border of an axis
                        (6 rows: pixel 0 and W - 1 exactly in float32 for the box +-4), on an interior texel line (x_k = 0: 3 rows), view directions
                        along an axis but not a pole (4 rows, position interior), then seeded interior points.  `kinds` names every row.
    g_out [67,4], out [67,4]
    x_grad_reference    upstream as it runs (shim A): position columns exactly 0
    x_grad_full         with shim B as well: the true derivative"""
import contextlib
import os
import sys

import numpy as np
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as gg  # noqa: E402  (imports the upstream modules behind the shims of SURVEY Appendix A)
from gen_golden_lowrank import decoder_checksum  # noqa: E402

models = gg.models
SHAPES = ((5, 7), (6, 4), (7, 5), (4, 3))            # H x W of planes 0..3
P = 67


def points():
    rng = np.random.default_rng(2300)
    rows, kinds = [], []

    def add(kind, xyz, v=None):
        v = rng.standard_normal(3) if v is None else np.asarray(v, dtype=np.float64)
        rows.append(np.concatenate([np.asarray(xyz, dtype=np.float64), v / np.linalg.norm(v)]))
        kinds.append(kind)

    for _ in range(8):
        add("interior", rng.uniform(-3.7, 3.7, 3))
    for k in range(3):
        p = rng.uniform(-3.0, 3.0, 3)
        p[k] = (4.75, -5.5, 6.25)[k]
        add("beyond%d" % k, p)
    for k in range(3):
        for name, val in (("low", -4.0), ("high", 4.0)):
            p = rng.uniform(-3.0, 3.0, 3)
            p[k] = val
            add("%s%d" % (name, k), p)
    for k in range(3):
        p = rng.uniform(-3.0, 3.0, 3)
        p[k] = 0.0
        add("line%d" % k, p)
    for v in ((1.0, 0.0, 0.0), (0.0, -1.0, 0.0), (0.0, 1.0, 0.0), (0.6, 0.0, 0.8)):
        add("axis_view", rng.uniform(-3.0, 3.0, 3), v)
    while len(rows) < P:
        add("interior", rng.uniform(-3.9, 3.9, 3))
    return np.stack(rows).astype(np.float32), np.array(kinds)


def main():
    sid, mc, _, planes0, box = gg.build_models(7, 4, 0.5, seed=23)
    g11 = dict(np.load(os.path.join(gg.HERE, "g11_grads.npz")))
    mc.load_state_dict({k[len("coarse."):]: torch.from_numpy(v) for k, v in g11.items() if k.startswith("coarse.")}, strict=False)
    names = [models.get_plane_name(sid, d) for d in range(4)]
    torch.manual_seed(230)
    planes = nn.ParameterDict([(names[d], nn.Parameter(0.5 * torch.randn(1, 48, *SHAPES[d]))) for d in range(4)])
    mc.planes_ = planes
    with torch.no_grad():
        g = torch.Generator().manual_seed(231)
        pts = torch.rand(4096, 3, generator=g) * 6 - 3
        d = torch.randn(4096, 3, generator=g)
        xc = torch.cat([pts, d / d.norm(dim=-1, keepdim=True)], -1)
        mc.eval()
        scale = 1.0 / float(mc(xc)[:, 3].std())
        mc.fc_alpha["0"].weight.mul_(scale)
        mc.fc_alpha["0"].bias.mul_(scale)
        mc.fc_alpha["0"].bias.add_(-float(mc(xc)[:, 3].mean()) - 0.5)

    x_np, kinds = points()
    torch.manual_seed(232)
    g_out = torch.randn(P, 4)
    mc.train()
    torch.Tensor.cpu = lambda s, *a, **k: s.detach()                  # shim A

    def run():
        x = torch.from_numpy(x_np.copy()).requires_grad_(True)
        out = mc(x)
        (out * g_out).sum().backward()
        return out.detach().numpy().copy(), x.grad.numpy().copy()

    out_ref, grad_ref = run()
    real_no_grad = torch.no_grad
    torch.no_grad = contextlib.nullcontext                            # shim B
    try:
        out_full, grad_full = run()
    finally:
        torch.no_grad = real_no_grad
    assert np.array_equal(out_ref.view(np.uint32), out_full.view(np.uint32)), "shim B changed the forward"
    assert np.array_equal(grad_ref[:, 3:].view(np.uint32), grad_full[:, 3:].view(np.uint32)), "shim B changed the view half"
    assert not grad_ref[:, :3].any(), "upstream returned a position gradient"
    assert np.isfinite(grad_full).all()
    for k in range(3):
        for kind in ("beyond%d" % k, "low%d" % k, "high%d" % k):
            assert not grad_full[kinds == kind][:, k].any(), kind
    sig = out_ref[:, 3]
    print("   sigma_raw > 0 on %d of %d points; |x_grad_full| position / view: %.3g / %.3g" % (
        int((sig > 0).sum()), P, float(np.abs(grad_full[:, :3]).mean()), float(np.abs(grad_full[:, 3:]).mean())))

    arrs = dict(box=gg.npy(box), x=x_np, kinds=kinds, g_out=g_out.numpy(), out=out_ref, x_grad_reference=grad_ref, x_grad_full=grad_full,
                g11_decoders=decoder_checksum(g11))
    for k, v in gg.state_arrays("coarse.", mc).items():
        assert k in g11 and v.shape == g11[k].shape, k
        if not np.array_equal(v, g11[k]):
            arrs[k] = v.copy()
    print("   decoder entries that differ from g11:", sorted(k for k in arrs if k.startswith("coarse.")))
    for dnum in range(4):
        arrs["plane%d" % dnum] = planes[names[dnum]].detach().numpy().copy()
    gg.save("g23_points_grad.npz", **arrs)


if __name__ == "__main__":
    main()
