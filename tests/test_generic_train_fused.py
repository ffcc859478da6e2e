"""The fused TRAINING route of the generic decoder geometries for a decoder that takes no gradient (csrc/generic_fused_bwd.hip,
torch.ops.nvsr.triplane_decode_generic_fused_backward, TwoDimPlanesModel.generic_train_route()): the planes' gradients in one launch, exact
f32.  Held to the reference's own autograd (g19), to the float64 restatement tests/generic_train_ref.py (pinned against g19 in
test_generic_train_fused_host.py) and -- where the atomics cannot reorder anything -- to the BITS of the layered route (csrc/generic.hip),
which stays the reference implementation and runs every decoder-weight gradient."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import load_golden
from test_hip_parity import DEV, N_, T, make_options
from test_oracle import G18_VARIANTS, G22_BOX

import generic_train_ref as ref64

pytestmark = pytest.mark.gpu
SID = "lego_DS8_PlRes10_6"
HANDLE = "NVSR_GENERIC_TRAIN_FUSED"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def seeded_model(hip, seed, n_pos=3, size=16, view_size=8, **kw):
    """a seeded model on size x size position planes and a view_size x view_size view plane, decoder frozen, planes trainable, in train():
    (model, state dict and planes as numpy for the float64 helper)"""
    kw.setdefault("align_corners", True)
    torch.manual_seed(seed)
    np.random.seed(seed)                      # (more than three position planes: CoordProjector draws its frames from NumPy's generator)
    m = hip.models.TwoDimPlanesModel(use_viewdirs=True, num_planes_or_rot_mats=n_pos, **kw)
    with torch.no_grad():                     # (He weights and mostly positive biases: no layer whose ReLUs are all shut, at any width)
        for p in m.decoder_parameters():
            p.normal_(0.0, float(np.sqrt(2.0 / p.shape[1]))) if p.dim() == 2 else p.uniform_(-0.1, 0.4)
    rng = np.random.default_rng(seed)
    c = kw.get("num_plane_channels", 48)
    planes = [rng.standard_normal((1, c, size, size)).astype(np.float32) for _ in range(n_pos)] + \
             [rng.standard_normal((1, c, view_size, view_size)).astype(np.float32)]
    m = m.to(DEV).train()
    m.planes_ = torch.nn.ParameterDict({hip.models.get_plane_name(SID, d): torch.nn.Parameter(T(planes[d])) for d in range(n_pos + 1)})
    m.box_coords = {SID: torch.as_tensor(G22_BOX, dtype=torch.float64)}
    m.set_cur_scene_id(SID)
    freeze_decoder(m)
    return m, planes


def state_dict_of(m):
    return {k: N_(v) for k, v in m.state_dict().items() if "planes_" not in k}


def freeze_decoder(m):
    for p in m.decoder_parameters():
        p.requires_grad_(False)


def plane_list(hip, m, sid=SID):
    return [m.planes_[hip.models.get_plane_name(sid, d)] for d in range(m.num_density_planes + 1)]


def points(P, seed=3):
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.uniform(-4.3, 4.3, (P, 3)), rng.standard_normal((P, 3))], 1).astype(np.float32)


def op_args(m):
    planes = [m.channel_last_plane(d).detach() for d in range(m.num_density_planes + 1)]
    planes, consts = m.scene_args(planes=planes, check_native=False)
    return planes, consts, m.natural_blob().detach(), m.generic_geometry()


def both_ops(m, x, G, noise=None, need=None):
    """(fused, layered) plane gradients of the two backward operators, [H,W,C] numpy each"""
    planes, consts, nat, geometry = op_args(m)
    need = [True] * len(planes) if need is None else need
    tail = (bool(m.align_corners), None if noise is None else T(noise), m.plane_interp == "bicubic")
    with torch.no_grad():
        f = torch.ops.nvsr.triplane_decode_generic_fused_backward(planes, consts, nat, geometry, T(x), T(G), need, *tail)
        l = torch.ops.nvsr.triplane_decode_generic_backward(planes, consts, nat, geometry, T(x), T(G), False, need, *tail)[1:]
    return [N_(t) for t in f], [N_(t) for t in l]


def model_grads(hip, m, x, G, monkeypatch, handle, sid=SID):
    """(out, plane gradients [1,C,H,W]) of a training-mode model call under NVSR_GENERIC_TRAIN_FUSED = handle"""
    monkeypatch.setenv(HANDLE, handle)
    pl = plane_list(hip, m, sid)
    for p in pl:
        p.grad = None
    out = m(T(x))
    (out * T(G)).sum().backward()
    return N_(out), [None if p.grad is None else N_(p.grad) for p in pl]


class Spy:
    """counts the calls of operators of torch.ops.nvsr by name"""

    def __init__(self, monkeypatch, names):
        self.calls = {n: 0 for n in names}
        for n in names:
            real = getattr(torch.ops.nvsr, n)

            def wrapped(*a, _n=n, _real=real, **k):
                self.calls[_n] += 1
                return _real(*a, **k)

            monkeypatch.setattr(torch.ops.nvsr, n, wrapped, raising=False)


def test_planes_only_training_takes_the_fused_backward(hip, monkeypatch):
    """fails without the feature: with the handle at 1 and only the planes requiring gradients, a g18 'avg_mult' model in train() answers
    'fused' and its backward is ONE call of triplane_decode_generic_fused_backward, none of the layered operator"""
    from test_hip_round2 import _variant_model
    g = load_golden("g18_decoder_variants.npz")
    m, sid, *_ = _variant_model(hip, g, "avg_mult")
    m.train()
    freeze_decoder(m)
    monkeypatch.setenv(HANDLE, "1")
    assert m.generic_train_route() == "fused"
    spy = Spy(monkeypatch, ["triplane_decode_generic_fused_backward", "triplane_decode_generic_backward"])
    out = m(T(g["avg_mult.x"]))
    out.sum().backward()
    assert spy.calls == {"triplane_decode_generic_fused_backward": 1, "triplane_decode_generic_backward": 0}
    assert all(p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0 for p in plane_list(hip, m, sid))


def test_reference_gradients_of_the_five_geometries(hip, monkeypatch):
    """g19, the reference's own autograd, with the decoder frozen: the training forward is the layered training forward bit for bit; the four
    plane gradients stay inside the tolerances of test_generic_decoder_gradients_vs_reference (relative L2 < 2e-5, atol 3e-5 max|ref|); with
    only plane 1 requiring a gradient, only plane 1 gets one"""
    from test_hip_round2 import _variant_model
    g, gg = load_golden("g18_decoder_variants.npz"), load_golden("g19_decoder_variant_grads.npz")
    names = [n for n in G18_VARIANTS if n + ".gout" in gg]
    assert len(names) == 5
    for name in names:
        m, sid, *_ = _variant_model(hip, g, name)
        m.train()
        freeze_decoder(m)
        x, G = g[name + ".x"], gg[name + ".gout"]
        out_l, _ = model_grads(hip, m, x, G, monkeypatch, "0", sid)
        assert m.generic_train_route() == "layered"
        out_f, grads = model_grads(hip, m, x, G, monkeypatch, "1", sid)
        assert m.generic_train_route() == "fused"
        assert torch.equal(torch.as_tensor(out_f), torch.as_tensor(out_l)), name
        for d in range(4):
            refp = gg[name + ".gplane%d" % d]
            assert grads[d].shape == refp.shape
            err = np.linalg.norm(grads[d] - refp) / np.linalg.norm(refp)
            print("%s plane %d: relative L2 %.3g" % (name, d, err))
            assert err < 2e-5, (name, d, err)
            np.testing.assert_allclose(grads[d], refp, rtol=0, atol=3e-5 * float(np.abs(refp).max()), err_msg="%s plane %d" % (name, d))
        pl = plane_list(hip, m, sid)
        for p in pl:
            p.requires_grad_(False)
        pl[1].requires_grad_(True)
        _, only = model_grads(hip, m, x, G, monkeypatch, "1", sid)
        assert m.generic_train_route() == "fused"
        np.testing.assert_allclose(only[1], gg[name + ".gplane1"], rtol=0, atol=3e-5 * float(np.abs(gg[name + ".gplane1"]).max()))
        assert only[0] is None and only[2] is None and only[3] is None and all(p.grad is None for p in m.decoder_parameters())


# ---- bit equality with the layered route on points whose tap footprints are pairwise disjoint --------------------------------------------
def disjoint_points(m, count):
    """`count` interior points whose bilinear 2 x 2 footprints are pairwise disjoint and unclamped on every plane of model m (16 x 16
    position planes on the three axis pairs, 8 x 8 view plane): asserted in numpy on the float32 grid coordinates"""
    consts = m.scene_args(planes=[m.channel_last_plane(d).detach() for d in range(4)], check_native=False)[1]
    lo, rng = np.array(consts[:5], np.float32), np.array(consts[5:10], np.float32)
    # texel coordinates: every axis of point i sits in its own slot of three texels; the view coordinates on a 2 x 2 lattice of the 8 x 8 plane
    tex = np.array([[2.5 + 3 * i + 0.13 * a for a in range(3)] for i in range(count)], np.float32)
    vtex = np.array([[1.5 + 3 * (i % 2), 1.4 + 3 * (i // 2)] for i in range(count)], np.float32)
    n3 = tex / np.float32(7.5) - 1                                        # align_corners: texel = (g + 1) * 15 / 2
    xyz = lo[:3] + (n3 + 1) / 2 * rng[:3]
    nv = vtex / np.float32(3.5) - 1
    az, el = lo[3] + (nv[:, 0] + 1) / 2 * rng[3], lo[4] + (nv[:, 1] + 1) / 2 * rng[4]
    dirs = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], 1)
    x = np.concatenate([xyz, dirs], 1).astype(np.float32)
    # the check, from x as the kernels see it
    n = (2 * (x[:, :3] - lo[:3]) / rng[:3] - 1).astype(np.float32)
    a2 = np.arctan2(x[:, 4], x[:, 3]).astype(np.float32)
    e2 = np.arctan2(x[:, 5], np.sqrt(x[:, 3] ** 2 + x[:, 4] ** 2)).astype(np.float32)
    grids = [(n @ np.array(consts[10 + 6 * d:16 + 6 * d], np.float32).reshape(3, 2), 16) for d in range(3)]
    grids.append((np.stack([2 * (a2 - lo[3]) / rng[3] - 1, 2 * (e2 - lo[4]) / rng[4] - 1], 1).astype(np.float32), 8))
    for grid, size in grids:
        t = (grid + 1) * np.float32((size - 1) / 2)
        fl = np.floor(t)
        assert np.all(fl >= 1) and np.all(fl + 1 <= size - 2) and np.all(t - fl > 0.05) and np.all(t - fl < 0.95)      # interior, no tap of weight 0
        texels = [{(int(fl[i, 1]) + dy, int(fl[i, 0]) + dx) for dy in (0, 1) for dx in (0, 1)} for i in range(count)]
        for i in range(count):
            for j in range(i):
                assert not (texels[i] & texels[j])
    return x


BIT_CASES = {
    "concat24": dict(skip_connect_every=3, **G18_VARIANTS["concat24"]),
    "skip2": dict(G18_VARIANTS["skip2"]),
    "avg_mult": dict(skip_connect_every=3, **G18_VARIANTS["avg_mult"]),
    "hidden33": dict(dec_channels=33, dec_density_layers=5, dec_rgb_layers=3, skip_connect_every=1, proj_combination="avg", viewdir_proj_combination="concat_pos"),
    "hidden31": dict(dec_channels=31, dec_density_layers=5, dec_rgb_layers=3, skip_connect_every=2, proj_combination="sum", viewdir_proj_combination="sum"),
}


@pytest.mark.parametrize("case", list(BIT_CASES))
def test_bits_of_the_layered_route_on_disjoint_footprints(hip, case):
    """1 and then 4 points whose footprints share no texel: a texel channel of a zeroed plane receives at most the density decoder's and the
    colour decoder's addend, and 0 + a + b does not depend on the order -- so the fused gradients must be torch.equal to the layered ones.
    One hidden unit of the density decoder has a zero weight row and a zero bias: its gate is closed at exactly 0.  One unit of the colour
    decoder has a NaN bias: its pre-activation is NaN (closed as well: fmaxf), at the single point of the first run and at every point of
    the second; outside 'mult' (where 0 x NaN reaches the position planes in both routes) a NaN texel of the view plane under point 0 alone
    also makes every first-layer pre-activation of the colour decoder NaN at that one point.  (NaN at one point of ONE unit alone needs a
    non-finite weight or an overflow, and then the layered route's own gradients are no longer finite and nonzero.)  A zero cotangent gives
    exactly +0 everywhere."""
    m, _ = seeded_model(hip, 31, **BIT_CASES[case])
    with torch.no_grad():
        m.density_dec["0"][1].weight[2].zero_()
        m.density_dec["0"][1].bias[2] = 0.0
        m.rgb_dec["0"][1].bias[3] = float("nan")
        if BIT_CASES[case].get("viewdir_proj_combination") != "mult":
            plane_list(hip, m)[3][0, 5, 1, 1] = float("nan")          # (texel (1, 1) of the view plane: point 0's footprint, disjoint_points)
    rng = np.random.default_rng(17)
    for count in (1, 4):
        x = disjoint_points(m, count)
        G = rng.standard_normal((count, 4)).astype(np.float32)
        fused, layered = both_ops(m, x, G)
        for d in range(4):
            assert np.isfinite(layered[d]).all(), (case, count, d)
            if d < 3 or count == 4:               # (the NaN texel shuts the colour decoder, the view plane's only source, at point 0)
                assert np.abs(layered[d]).max() > 0, (case, count, d)
            assert torch.equal(torch.as_tensor(fused[d]), torch.as_tensor(layered[d])), (case, count, d)
            assert not np.signbit(fused[d][fused[d] == 0]).any()
        fused, layered = both_ops(m, x, np.zeros((count, 4), np.float32))
        for d in range(4):
            assert np.all(fused[d] == 0) and not np.signbit(fused[d]).any() and torch.equal(torch.as_tensor(fused[d]), torch.as_tensor(layered[d]))


# ---- ragged point counts against float64 ---------------------------------------------------------------------------------------------------
RAGGED = {
    "bilinear-mult": (3, dict(dec_channels=40, proj_combination="avg", viewdir_proj_combination="mult", skip_connect_every=3, align_corners=True), False),
    "bilinear-noalign-sum": (3, dict(dec_channels=40, proj_combination="sum", viewdir_proj_combination="sum", skip_connect_every=2, align_corners=False), True),
    "bicubic-planes5": (5, dict(dec_channels=64, num_plane_channels=24, proj_combination="avg", viewdir_proj_combination="concat_pos", skip_connect_every=2,
                                align_corners=True, plane_interp="bicubic"), True),
    "bicubic-noalign-concat": (3, dict(dec_channels=96, num_plane_channels=24, proj_combination="concat", viewdir_proj_combination="concat",
                                       align_corners=False, plane_interp="bicubic"), False),
}


@pytest.mark.parametrize("case", list(RAGGED))
def test_ragged_point_counts_against_float64(hip, case):
    """P in {0, 1, 31, 32, 33, 129, 300} on random 16 x 16 planes (8 x 8 view plane): bilinear and bicubic taps, align_corners both ways, five
    position planes, a given coord_noise, the 'mult' and 'sum' view rules.  The layered route's relative L2 error against the float64 helper
    is checked first (< 2e-5, the project's bound for these gradients); then the fused route's: below 2e-5, and no more than 1.5 x the
    layered route's on the same inputs + 1e-7 (the atomics' arrival order; both run the same chains)."""
    n_pos, kw, with_noise = RAGGED[case]
    m, planes = seeded_model(hip, 41, n_pos=n_pos, **kw)
    sd = state_dict_of(m)
    rng = np.random.default_rng(43)
    x_all, G_all = points(300, seed=47), rng.standard_normal((300, 4)).astype(np.float32)
    noise_all = (rng.standard_normal((300, 3)) * 0.02).astype(np.float32) if with_noise else None
    helper_kw = {k: v for k, v in kw.items() if k not in ("dec_channels", "num_plane_channels")}
    for P in (0, 1, 31, 32, 33, 129, 300):
        x, G = x_all[:P], G_all[:P]
        noise = None if noise_all is None else noise_all[:P]
        fused, layered = both_ops(m, x, G, noise)
        if P == 0:
            assert all(np.all(f == 0) and f.shape == l.shape for f, l in zip(fused, layered))
            continue
        _, want = ref64.plane_gradients(sd, planes, G22_BOX, x, G, coord_noise=noise, **helper_kw)
        for d in range(n_pos + 1):
            w = want[d][0].transpose(1, 2, 0)
            el, ef = ref64.rel_l2(layered[d], w), ref64.rel_l2(fused[d], w)
            print("%s P=%d plane %d: layered %.3g fused %.3g" % (case, P, d, el, ef))
            assert el < 2e-5, (case, P, d, el)
            assert ef < 2e-5 and ef <= 1.5 * el + 1e-7, (case, P, d, ef, el)


def test_beyond_the_capacity_the_entry_refuses_and_the_model_trains_layered(hip, monkeypatch):
    monkeypatch.setenv(HANDLE, "1")
    m, _ = seeded_model(hip, 9, size=4, view_size=4, dec_channels=4096, dec_density_layers=1, dec_rgb_layers=1, proj_combination="sum")
    planes, consts, nat, geometry = op_args(m)
    x, G = T(points(40)), T(np.ones((40, 4), np.float32))
    geo, n_pos, _, sc = hip.ops._generic_setup(planes, consts, nat, geometry, True, None, 40)
    assert hip.capi.lib().nvsr_generic_backward_fused_supported(C.byref(geo), n_pos) == 0
    gpl = [torch.zeros_like(p) for p in planes]
    d_planes = (C.c_void_p * 4)(*[t.data_ptr() for t in gpl])
    status = hip.capi.lib().nvsr_generic_decode_backward_fused_ext(C.byref(sc), C.byref(geo), hip.capi.ptr(nat), 40, hip.capi.ptr(x), None, hip.capi.ptr(G),
                                                                   d_planes, hip.capi.stream())
    assert status == hip.capi.lib().nvsr_generic_decode_fused_ext(C.byref(sc), C.byref(geo), hip.capi.ptr(nat), 40, hip.capi.ptr(x), None, hip.capi.ptr(G),
                                                                  hip.capi.stream()) != 0          # NVSR_ERR_SHAPE, like the forward entry
    assert all(float(t.abs().max()) == 0 for t in gpl)
    with pytest.raises(Exception, match="capacity"):
        torch.ops.nvsr.triplane_decode_generic_fused_backward(planes, consts, nat, geometry, x, G, [True] * 4)
    assert m.generic_train_route() == "layered"
    spy = Spy(monkeypatch, ["triplane_decode_generic_fused_backward", "triplane_decode_generic_backward"])
    m(x).sum().backward()
    assert spy.calls == {"triplane_decode_generic_fused_backward": 0, "triplane_decode_generic_backward": 1}
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in plane_list(hip, m))


def test_planes_only_iteration_through_run_one_iter_of_nerf(hip, monkeypatch):
    """64 rays, 16 + 16 samples, the 'skip2' coarse / fine pair with frozen decoders: the pixels of the fused route are the layered route's
    bits, the plane gradients within a relative L2 of 2e-5, and five Adam steps on the planes lower the loss"""
    from test_hip_round2 import _variant_model
    g = load_golden("g18_decoder_variants.npz")
    mc, sid, *_ = _variant_model(hip, g, "skip2")
    mf, *_ = _variant_model(hip, g, "skip2")
    mf.planes_ = mc.planes_
    opts, scfg = make_options(16, 16)
    for mm in (mc, mf):
        mm.train()
        freeze_decoder(mm)
    H = W = 8
    focal = 0.5 * W / np.tan(0.5 * 0.6911112)
    ro, rd = hip.nerf_helpers.get_ray_bundle(H, W, focal, T(g["pose"]))
    batch = torch.stack([ro.reshape(-1, 3), rd.reshape(-1, 3)], 0)
    target = torch.rand((H * W, 3), generator=torch.Generator().manual_seed(4)).to(DEV) * 0.5 + 0.25
    pl = plane_list(hip, mc, sid)

    def iteration(handle):
        monkeypatch.setenv(HANDLE, handle)
        for p in pl:
            p.grad = None
        rgb_c, _, _, rgb_f, *_ = hip.train_utils.run_one_iter_of_nerf(H, W, focal, mc, mf, batch, opts, sid, mode="validation", scene_config=scfg)
        loss = ((rgb_c - target) ** 2).mean() + ((rgb_f - target) ** 2).mean()
        loss.backward()
        return rgb_c.detach().clone(), rgb_f.detach().clone(), [N_(p.grad) for p in pl], float(loss.detach())

    lc, lf, lg, _ = iteration("0")
    spy = Spy(monkeypatch, ["triplane_decode_generic_fused_backward", "triplane_decode_generic_backward"])
    fc, ff, fg, _ = iteration("1")
    assert spy.calls["triplane_decode_generic_fused_backward"] >= 2 and spy.calls["triplane_decode_generic_backward"] == 0
    assert torch.equal(fc, lc) and torch.equal(ff, lf)
    for d in range(4):
        err = np.linalg.norm(fg[d] - lg[d]) / np.linalg.norm(lg[d])
        assert err < 2e-5, (d, err)
    opt = torch.optim.Adam(pl, lr=2e-3)
    losses = []
    for it in range(6):
        opt.zero_grad()
        losses.append(iteration("1")[3])
        opt.step()
    assert losses[5] < losses[0], losses


def test_training_through_super_resolved_planes(hip, monkeypatch):
    """the configuration of test_training_through_super_resolved_planes_on_a_generic_geometry with the decoder frozen: the training forward
    is the layered one bit for bit, and the EDSR weight gradients (and one LR plane's) of the fused route agree with the layered route's in
    that test's own measure and tolerance -- <gradient, direction> along a random direction, within 2e-2 relative + 1e-6"""
    rng = np.random.default_rng(71)
    R, Rv, hid, nb, C_ = 20, 6, 16, 2, 48
    kw = dict(skip_connect_every=3, proj_combination="sum", viewdir_proj_combination="concat_pos")
    torch.manual_seed(8)
    m = hip.models.TwoDimPlanesModel(use_viewdirs=True, dec_channels=64, **kw).to(DEV)
    sid = "lego_DS8_PlRes20_6"
    planes = [rng.standard_normal((1, C_, R, R), dtype=np.float32) * 0.5 for _ in range(3)] + [rng.standard_normal((1, C_, Rv, Rv), dtype=np.float32) * 0.5]
    m.planes_ = torch.nn.ParameterDict({hip.models.get_plane_name(sid, d): torch.nn.Parameter(T(planes[d])) for d in range(4)})
    m.box_coords = {sid: torch.as_tensor(G22_BOX, dtype=torch.float64)}
    m.set_cur_scene_id(sid)
    sr = hip.models.PlanesSR(hip.models.EDSR, 4, C_, C_, {"model": {"hidden_size": hid, "n_blocks": nb}}, "bilinear").to(DEV)
    with torch.no_grad():
        for p_ in sr.parameters():
            p_.mul_(10.0)
    m.assign_SR_model(sr, SR_viewdir=False)
    m.assign_LR_planes()
    for p_ in list(m.decoder_parameters()) + list(m.planes_.values()):
        p_.requires_grad_(False)
    lr_names = [hip.models.get_plane_name(sid, d) for d in range(3)]
    for n_ in lr_names:
        sr.LR_planes[n_].requires_grad_(True)
    m.train(); sr.train()
    P = 300
    x = np.concatenate([rng.uniform(-1.5, 2.0, (P, 3)), rng.standard_normal((P, 3))], 1).astype(np.float32)
    G = rng.standard_normal((P, 4)).astype(np.float32)

    def run(handle):
        monkeypatch.setenv(HANDLE, handle)
        for w in list(sr.inner_model.conv_weights()) + [sr.LR_planes[n_] for n_ in lr_names]:
            w.grad = None
        out = m(T(x))
        (out * T(G)).sum().backward()
        return (N_(out), np.concatenate([N_(w.grad).reshape(-1) for w in sr.inner_model.conv_weights()]).astype(np.float64),
                N_(sr.LR_planes[lr_names[1]].grad).astype(np.float64))

    out_l, w_l, lr_l = run("0")
    assert m.generic_train_route() == "layered"
    spy = Spy(monkeypatch, ["triplane_decode_generic_fused_backward", "triplane_decode_generic_backward"])
    out_f, w_f, lr_f = run("1")
    assert m.generic_train_route() == "fused"
    assert spy.calls == {"triplane_decode_generic_fused_backward": 1, "triplane_decode_generic_backward": 0}
    assert np.array_equal(out_f, out_l)
    assert np.isfinite(w_f).all() and np.abs(w_f).max() > 0 and np.isfinite(lr_f).all() and np.abs(lr_f).max() > 0
    blob = np.concatenate([N_(w).reshape(-1) for w in sr.inner_model.conv_weights()])
    dw = rng.standard_normal(blob.shape) * np.abs(blob).mean()
    dl = rng.standard_normal(lr_l.shape) * 0.5
    assert abs(w_f @ dw - w_l @ dw) <= 2e-2 * abs(w_l @ dw) + 1e-6
    assert abs((lr_f * dl).sum() - (lr_l * dl).sum()) <= 2e-2 * abs((lr_l * dl).sum()) + 1e-6
    print("SR weights: relative L2 fused vs layered %.3g; LR plane 1: %.3g" % (np.linalg.norm(w_f - w_l) / np.linalg.norm(w_l),
                                                                              np.linalg.norm(lr_f - lr_l) / np.linalg.norm(lr_l)))


def test_opcheck(hip):
    m, _ = seeded_model(hip, 3, dec_channels=64, proj_combination="avg", viewdir_proj_combination="concat_pos", skip_connect_every=3, align_corners=True)
    args = op_args(m) + (T(points(50)), T(np.ones((50, 4), np.float32)), [True, False, True, True], True, None, False)
    torch.library.opcheck(torch.ops.nvsr.triplane_decode_generic_fused_backward, args, test_utils=("test_schema", "test_faketensor"))


def test_kernel_resources_gate_covers_the_new_kernel(hip):
    """no scratch and no spilled vector registers in any instantiation: tools/kernel_resources.py --check, with the kernel in its list"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_resources
    finally:
        sys.path.pop(0)
    assert "generic_backward_fused_kernel" in kernel_resources.BENCHMARKED
    table = kernel_resources.kernel_table()
    mine = [k for k in table if "generic_backward_fused_kernel" in k["name"]]
    assert len(mine) == 18 and all(k["scratch"] == 0 and k["vgpr_spill"] == 0 for k in mine), mine
    done = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "--check"], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
