"""Planes-only training of the generic decoder geometries in 'f16x2' (csrc/generic_fused_bwd_limb.hip,
torch.ops.nvsr.triplane_decode_generic_fused_backward_arith, TwoDimPlanesModel.train_arithmetic / generic_train_arithmetic()): the planes'
gradients in one launch on two f16 limbs.  Held to float64 autograd (tests/generic_train_ref.py), to the numpy restatement
tests/generic_train_limb_ref.py under a derived accumulation bound, to exact scale invariance, to the range contract, and at the model level."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import load_golden
from test_generic_limb import flag_of
from test_generic_train_fused import (DEV, HANDLE, N_, RAGGED, ROOT, SID, Spy, T, both_ops, freeze_decoder, make_options, op_args, plane_list, points,
                                      seeded_model, state_dict_of)
from test_oracle import G22_BOX

import generic_limb_ref as fwd
import generic_train_limb_ref as ref
import generic_train_ref as ref64

pytestmark = pytest.mark.gpu
F32, F16X2 = 0, 2
NEW, OLD, LAYERED = "triplane_decode_generic_fused_backward_arith", "triplane_decode_generic_fused_backward", "triplane_decode_generic_backward"


def blobs(m):
    _, _, nat, geometry = op_args(m)
    n_pos = int(m.num_density_planes)
    return torch.ops.nvsr.pack_generic_decoder(nat, geometry, n_pos), torch.ops.nvsr.pack_generic_decoder_bwd(nat, geometry, n_pos)


def limb_grads(m, x, G, noise=None, need=None, arith=F16X2):
    """the plane gradients [H,W,C] of the new operator"""
    planes, consts, nat, geometry = op_args(m)
    need = [True] * len(planes) if need is None else need
    packed, packed_bwd = blobs(m)
    with torch.no_grad():
        g = torch.ops.nvsr.triplane_decode_generic_fused_backward_arith(planes, consts, nat, packed, packed_bwd, geometry, T(x), T(G), need,
                                                                        bool(m.align_corners), None if noise is None else T(noise),
                                                                        m.plane_interp == "bicubic", arith)
    return [N_(t) for t in g]


def helper_kw(kw):
    return {k: v for k, v in kw.items() if k not in ("dec_channels", "num_plane_channels")}


# ---- the transposed blob ----------------------------------------------------------------------------------------------------------------------
PACK = {
    "hidden33-skip1": dict(dec_channels=33, dec_density_layers=5, dec_rgb_layers=3, skip_connect_every=1, proj_combination="avg", viewdir_proj_combination="concat_pos"),
    "hidden160-skip2": dict(dec_channels=160, proj_combination="avg", viewdir_proj_combination="concat_pos", skip_connect_every=2),
    "c24-concat": dict(dec_channels=96, num_plane_channels=24, proj_combination="concat", viewdir_proj_combination="concat"),
}


@pytest.mark.parametrize("case", list(PACK))
def test_pack_kernel_is_the_numpy_layout(hip, case):
    kw = PACK[case]
    m, _ = seeded_model(hip, 7, **kw)
    sd = state_dict_of(m)
    parts = ref.layer_parts(sd, kw["dec_channels"], dec_density_layers=m.dec_density_layers, dec_rgb_layers=m.dec_rgb_layers,
                            skip_connect_every=kw.get("skip_connect_every"))
    want = ref.pack_bwd(parts, kw["dec_channels"])
    got = N_(blobs(m)[1]).view(np.uint32)
    assert got.size == want.size and np.array_equal(got, want), np.flatnonzero(got != want)[:8]


# ---- 1. ragged point counts against float64 ----------------------------------------------------------------------------------------------------
CASES = dict(RAGGED)
CASES.update({
    "hidden33": (3, dict(dec_channels=33, dec_density_layers=5, dec_rgb_layers=3, skip_connect_every=1, proj_combination="avg",
                         viewdir_proj_combination="concat_pos", align_corners=True), False),
    "hidden31": (3, dict(dec_channels=31, dec_density_layers=5, dec_rgb_layers=3, skip_connect_every=2, proj_combination="sum",
                         viewdir_proj_combination="sum", align_corners=True), True),
    # one tile per layer (NT = 1) under Kr = 192, Kd = 144: six and five groups of the input gradients
    "groups": (3, dict(dec_channels=32, proj_combination="concat", viewdir_proj_combination="concat", skip_connect_every=2, align_corners=True), False),
})
# seeds of the models at which the limb forward and float64 agree on every gate of the 300 points (asserted below on the CPU, before any launch)
# and no float64 pre-activation lies within 1e-5 of zero (chosen so on the CPU: the kernel's f32 accumulation then cannot flip a gate either)
SEEDS = {"bilinear-mult": 48, "bilinear-noalign-sum": 41, "bicubic-planes5": 44, "bicubic-noalign-concat": 71, "hidden33": 41, "hidden31": 42,
         "groups": 45}


def ragged_inputs(case):
    n_pos, kw, with_noise = CASES[case]
    rng = np.random.default_rng(43)
    x, G = points(300, seed=47), rng.standard_normal((300, 4)).astype(np.float32)
    noise = (rng.standard_normal((300, 3)) * 0.02).astype(np.float32) if with_noise else None
    return n_pos, kw, x, G, noise


@pytest.mark.parametrize("case", list(CASES))
def test_ragged_point_counts_against_float64(hip, case):
    """P in {0, 1, 31, 32, 33, 129, 300}: relative L2 of every plane's gradient against float64 autograd below 2e-5, the project's bound for
    these gradients; the f32 fused route's error is printed beside it.  A ReLU gate that differs between the limb forward and float64 is a
    discontinuity, not an arithmetic error: the numpy references must agree on every gate at this seed -- asserted first, never masked.
    Measured (MI355X), over all cases, counts and planes: the limb route 1.3e-7 .. 2.0e-6, the f32 fused route 1.3e-7 .. 2.0e-6."""
    n_pos, kw, x_all, G_all, noise_all = ragged_inputs(case)
    m, planes = seeded_model(hip, SEEDS[case], n_pos=n_pos, **kw)
    sd = state_dict_of(m)
    hk = helper_kw(kw)
    ga = ref.gates(sd, planes, G22_BOX, x_all, fwd.layer, coord_noise=noise_all, **hk)
    gb = ref.gates(sd, planes, G22_BOX, x_all, fwd.layer_f64, coord_noise=noise_all, **hk)
    assert all(np.array_equal(u, v) for u, v in zip(ga, gb)), "seed %d of %s: a gate differs between the limb forward and float64" % (SEEDS[case], case)
    for P in (0, 1, 31, 32, 33, 129, 300):
        x, G = x_all[:P], G_all[:P]
        noise = None if noise_all is None else noise_all[:P]
        (got, bits), f32 = flag_of(hip, lambda: limb_grads(m, x, G, noise)), both_ops(m, x, G, noise)[0]
        assert bits == 0
        if P == 0:
            assert all(np.all(a == 0) and a.shape == b.shape for a, b in zip(got, f32))
            continue
        _, want = ref64.plane_gradients(sd, planes, G22_BOX, x, G, coord_noise=noise, **hk)
        for d in range(n_pos + 1):
            w = want[d][0].transpose(1, 2, 0)
            el, ef = ref64.rel_l2(got[d], w), ref64.rel_l2(f32[d], w)
            print("%s P=%d plane %d: f16x2 %.3g f32 fused %.3g" % (case, P, d, el, ef))
            assert el < 2e-5, (case, P, d, el)


# ---- 2. against the numpy limb reference: the derived accumulation bound ----------------------------------------------------------------------
@pytest.mark.parametrize("hidden", [33, 64])
def test_one_hidden_layer_within_the_derived_accumulation_bound(hip, hidden):
    """test_generic_limb.test_one_hidden_layer_within_the_derived_accumulation_bound's construction, transposed.  One hidden layer per decoder;
    9 x 9 position planes of multiples of 1/64 sampled at their texel centres (tap weights (1, 0, 0, 0)), 'sum' / 'concat_pos'; the 81 points
    (a, b, (a + b) mod 9) meet every texel of every position plane exactly once; a cotangent with ONE nonzero colour channel per point, so
    each head gradient is a single product, rounded once in the kernel and in the reference alike.  The gates are asserted equal (limb forward
    against float64).  Kernel and numpy reference then hold the same dZ, the same scale and the same limbs, and differ by the order of the
    f32 accumulation alone:
      decoder-input gradient:  e_x = 1.01 n 2^-24 sum_m |w^||z^| 2^(-8 - e),  n = 3 ceil(hidden / 16) accumulating MFMAs (one f32 rounding of at
                               most the absolute sum per MFMA: conv_f16_ref.bound's model)
      texel (plane d, c):      e_x[dXd[c]] + e_x[dXr[d C + c]] + 2 x 2^-24 |texel|: the two addends, their one rounded addition in front of the
                               atomic on a zeroed texel, and the rounding of the float64 sums to f32 values."""
    m, _ = seeded_model(hip, 17, size=9, view_size=9, dec_channels=hidden, dec_density_layers=1, dec_rgb_layers=1, proj_combination="sum",
                        viewdir_proj_combination="concat_pos")
    rng = np.random.default_rng(hidden)
    planes = [(rng.integers(-128, 129, (1, 48, 9, 9)) / 64.0).astype(np.float32) for _ in range(3)] + [np.zeros((1, 48, 9, 9), np.float32)]
    with torch.no_grad():
        for d, p in enumerate(plane_list(hip, m)):
            p.copy_(T(planes[d]))
    sd = state_dict_of(m)
    kw = dict(dec_density_layers=1, dec_rgb_layers=1, proj_combination="sum", viewdir_proj_combination="concat_pos")
    ab = np.array([(a, b) for a in range(9) for b in range(9)])
    x = np.concatenate([np.stack([ab[:, 0], ab[:, 1], (ab[:, 0] + ab[:, 1]) % 9], 1) - 4, rng.standard_normal((81, 3))], 1).astype(np.float32)
    G = np.zeros((81, 4), np.float32)
    G[np.arange(81), rng.integers(0, 3, 81)] = rng.standard_normal(81)
    G[:, 3] = rng.standard_normal(81)
    Xd, _ = fwd.inputs(sd, planes, G22_BOX, x, **kw)
    assert np.array_equal(Xd * 64, np.round(Xd * 64)) and np.abs(Xd).max() > 1                      # exact inputs, as designed
    ga, gb = ref.gates(sd, planes, G22_BOX, x, fwd.layer, **kw), ref.gates(sd, planes, G22_BOX, x, fwd.layer_f64, **kw)
    assert all(np.array_equal(u, v) for u, v in zip(ga, gb))
    dXd, dXr, ad, ar = ref.decoder_input_gradients(sd, planes, G22_BOX, x, G, **kw)
    want = ref.pull_back(sd, planes, G22_BOX, x, dXd, dXr, **kw)
    absum = ref.pull_back(sd, planes, G22_BOX, x, ad, ar, **kw)
    got = limb_grads(m, x, G, need=[True, True, True, False])
    n = 3 * -(-hidden // 16)
    for d in range(3):
        w, a = want[d][0].transpose(1, 2, 0), absum[d][0].transpose(1, 2, 0)
        assert (np.abs(w).sum(2) > 0).sum() == 81                                                  # every texel from exactly one point
        bound = 1.01 * n * ref.U24 * a + 2 * ref.U24 * np.abs(w)
        err = np.abs(got[d] - w)
        print("hidden %d plane %d: worst error / bound %.3f" % (hidden, d, float((err[bound > 0] / bound[bound > 0]).max())))
        assert (err <= bound).all(), (d, float((err[bound > 0] / bound[bound > 0]).max()))
    assert got[3].size == 0


# ---- 3. scale invariance -----------------------------------------------------------------------------------------------------------------------
def lattice_points(m, count, with_view):
    """test_generic_train_fused.disjoint_points for up to 64 points: point i = (a, b) takes the 2 x 2 texel slots (a, b, (a + b) mod 8) of
    the three axes of the 16 x 16 position planes -- every pair of axes meets every slot pair once -- and, with_view (count <= 16), slot
    (i % 4, i // 4) of the 8 x 8 view plane.  -> (x, owner): owner[d][row, col] = the point whose footprint holds that texel, -1 for none;
    disjointness is asserted from the float32 grid coordinates"""
    consts = m.scene_args(planes=[m.channel_last_plane(d).detach() for d in range(4)], check_native=False)[1]
    lo, rng = np.array(consts[:5], np.float32), np.array(consts[5:10], np.float32)
    i = np.arange(count)
    a, b = i % 8, i // 8
    tex = (2 * np.stack([a, b, (a + b) % 8], 1) + 0.3 + 0.05 * np.arange(3)).astype(np.float32)
    vtex = (2 * np.stack([i % 4, (i // 4) % 4], 1) + np.array([0.4, 0.6])).astype(np.float32)
    n3 = tex / np.float32(7.5) - 1                                            # align_corners: texel = (g + 1) * 15 / 2
    xyz = lo[:3] + (n3 + 1) / 2 * rng[:3]
    nv = vtex / np.float32(3.5) - 1
    az, el = lo[3] + (nv[:, 0] + 1) / 2 * rng[3], lo[4] + (nv[:, 1] + 1) / 2 * rng[4]
    dirs = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], 1)
    x = np.concatenate([xyz, dirs], 1).astype(np.float32)
    n = (2 * (x[:, :3] - lo[:3]) / rng[:3] - 1).astype(np.float32)
    a2 = np.arctan2(x[:, 4], x[:, 3]).astype(np.float32)
    e2 = np.arctan2(x[:, 5], np.sqrt(x[:, 3] ** 2 + x[:, 4] ** 2)).astype(np.float32)
    grids = [(n @ np.array(consts[10 + 6 * d:16 + 6 * d], np.float32).reshape(3, 2), 16) for d in range(3)]
    if with_view:
        assert count <= 16
        grids.append((np.stack([2 * (a2 - lo[3]) / rng[3] - 1, 2 * (e2 - lo[4]) / rng[4] - 1], 1).astype(np.float32), 8))
    owners = []
    for grid, size in grids:
        t = (grid + 1) * np.float32((size - 1) / 2)
        fl = np.floor(t).astype(int)
        assert np.all(fl >= 0) and np.all(fl + 1 <= size - 1) and np.all(t - fl > 0.05) and np.all(t - fl < 0.95)
        owner = -np.ones((size, size), int)
        for p in range(count):
            for dy in (0, 1):
                for dx in (0, 1):
                    assert owner[fl[p, 1] + dy, fl[p, 0] + dx] == -1
                    owner[fl[p, 1] + dy, fl[p, 0] + dx] = p
        owners.append(owner)
    return x, owners


def test_scale_invariance_on_disjoint_footprints(hip):
    """P = 64 on pairwise disjoint footprints of the three 16 x 16 position planes: the cotangent of point p times 2^k[p], k in [-40, 40], gives
    the unscaled run's gradient times 2^k[p] at p's texels BIT FOR BIT (no value underflows: asserted); points with a zero cotangent leave
    exact zeros.  An 8 x 8 view plane holds 16 disjoint footprints, not 64: its gradient is not requested in the run of 64 and is held to the
    same equality in a second run on the first 16 points."""
    kw = dict(dec_channels=40, proj_combination="avg", viewdir_proj_combination="concat_pos", skip_connect_every=2)
    m, _ = seeded_model(hip, 23, **kw)
    rng = np.random.default_rng(5)
    for count, with_view in ((64, False), (16, True)):
        x, owners = lattice_points(m, count, with_view)
        G = rng.standard_normal((count, 4)).astype(np.float32)
        G[[3, 10]] = 0
        k = rng.integers(-40, 41, count)
        k[:2] = (-40, 40)
        need = [True, True, True, with_view]
        (base, bits0), (scaled, bits1) = flag_of(hip, lambda: limb_grads(m, x, G, need=need)), flag_of(
            hip, lambda: limb_grads(m, x, np.ldexp(G, k[:, None]).astype(np.float32), need=need))
        assert bits0 == 0 and bits1 == 0
        for d, owner in enumerate(owners):
            live = owner >= 0
            assert np.isfinite(base[d]).all() and np.abs(base[d][live]).max() > 0
            nz = np.abs(base[d][base[d] != 0])
            assert nz.min() > 2.0 ** -80 and nz.max() < 2.0 ** 80                                  # times 2^+-40: normal f32 numbers, no underflow
            want = np.ldexp(base[d], np.where(live, k[np.maximum(owner, 0)], 0)[:, :, None]).astype(np.float32)
            assert torch.equal(torch.as_tensor(scaled[d]), torch.as_tensor(want)), (count, d)
            assert not base[d][~live].any() and not scaled[d][~live].any()
            for p in (3, 10):
                assert not base[d][owner == p].any() and not scaled[d][owner == p].any() and not np.signbit(scaled[d][owner == p]).any()


# ---- 4. range ----------------------------------------------------------------------------------------------------------------------------------
def test_range_contract(hip):
    """a hidden weight of 300 (>= 255: its limbs are (inf, -inf)): NaN gradients wherever the weight's column reaches, and the flag; an inf cotangent at one point: NaN at that point's
    texels and the flag; a finite cotangent of 1e30: finite gradients, the flag clear, within 2e-5 of float64"""
    kw = dict(dec_channels=40, proj_combination="avg", viewdir_proj_combination="concat_pos", skip_connect_every=2)
    m, planes = seeded_model(hip, 23, **kw)
    x, owners = lattice_points(m, 16, True)
    G = np.random.default_rng(8).standard_normal((16, 4)).astype(np.float32)
    base, bits = flag_of(hip, lambda: limb_grads(m, x, G))
    assert bits == 0 and all(np.isfinite(g).all() for g in base)
    big, bits = flag_of(hip, lambda: limb_grads(m, x, G * np.float32(1e30)))
    assert bits == 0 and all(np.isfinite(g).all() and np.abs(g).max() > 1e20 for g in big)
    _, want = ref64.plane_gradients(state_dict_of(m), planes, G22_BOX, x, G.astype(np.float64) * float(np.float32(1e30)), **helper_kw(kw))
    for d in range(4):
        assert ref64.rel_l2(big[d], want[d][0].transpose(1, 2, 0)) < 2e-5
    Ginf = G.copy()
    Ginf[5, 3] = np.inf
    Ginf[6, 1] = -np.inf
    got, bits = flag_of(hip, lambda: limb_grads(m, x, Ginf))
    assert bits & 1
    for d in range(3):                                    # point 5: the density decoder reaches every position plane; point 6: the colour decoder
        for p in (5, 6):
            assert np.isnan(got[d][owners[d] == p]).all(), (d, p)
        rest = ~np.isin(owners[d], (5, 6))
        assert torch.equal(torch.as_tensor(got[d][rest]), torch.as_tensor(base[d][rest]))
    assert np.isnan(got[3][owners[3] == 6]).all() and np.isfinite(got[3][owners[3] != 6]).all()
    # W[5][7] of the density decoder's layer 1 feeds column 7 of that layer's input gradient: NaN at every point; it survives layer 0's gate
    # where unit 7 of layer 0 is open (the forward of layer 0 does not read the weight), and a NaN in a row makes the row's gradients NaN
    open7 = ref.gates(state_dict_of(m), planes, G22_BOX, x, fwd.layer, **helper_kw(kw))[0][:, 7]
    assert open7.any() and not open7.all()
    with torch.no_grad():
        m.density_dec["0"][1].weight[5, 7] = 300.0
    got, bits = flag_of(hip, lambda: limb_grads(m, x, G))
    assert bits & 1
    for d in range(3):
        for p in range(16):
            mine = got[d][owners[d] == p]
            assert np.isnan(mine).all() if open7[p] else np.isfinite(mine).all(), (d, p)
    assert torch.equal(torch.as_tensor(got[3]), torch.as_tensor(base[3]))          # (the colour decoder alone feeds the view plane)


# ---- 5. the training forward ---------------------------------------------------------------------------------------------------------------------
def test_training_forward_is_the_limb_evaluation_launch(hip, monkeypatch):
    n_pos, kw, x, G, noise = ragged_inputs("bicubic-planes5")
    m, _ = seeded_model(hip, SEEDS["bicubic-planes5"], n_pos=n_pos, **kw)
    m.train_arithmetic = "f16x2"
    monkeypatch.setenv(HANDLE, "1")
    assert m.generic_train_arithmetic() == "f16x2"
    planes, consts, nat, geometry = op_args(m)
    with torch.no_grad():
        want = torch.ops.nvsr.triplane_decode_generic_fused_arith(planes, consts, nat, blobs(m)[0], geometry, T(x), True, None, True, F16X2)
    spy = Spy(monkeypatch, [NEW, OLD, LAYERED])
    out = m(T(x))
    assert out.requires_grad and torch.equal(out.detach(), want)
    (out * T(G)).sum().backward()
    assert spy.calls == {NEW: 1, OLD: 0, LAYERED: 0}
    got = [N_(p.grad)[0].transpose(1, 2, 0) for p in plane_list(hip, m)]
    direct = limb_grads(m, x, G)
    for d in range(n_pos + 1):
        assert ref64.rel_l2(got[d], direct[d].astype(np.float64)) < 1e-6          # (the same launch twice: the atomics' order alone)
    m.train_arithmetic = None
    assert m.generic_train_arithmetic() == "f32"


# ---- 6. model level ------------------------------------------------------------------------------------------------------------------------------
def test_planes_only_iteration_through_run_one_iter_of_nerf(hip, monkeypatch):
    """test_generic_train_fused's iteration with train_arithmetic = 'f16x2' on both models: the backward is the new operator alone, the plane
    gradients agree with the f32 fused route's within 2e-5 (relative L2), and five Adam steps on the planes lower the loss"""
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
    monkeypatch.setenv(HANDLE, "1")

    def iteration(train_arithmetic):
        for mm in (mc, mf):
            mm.train_arithmetic = train_arithmetic
        for p in pl:
            p.grad = None
        rgb_c, _, _, rgb_f, *_ = hip.train_utils.run_one_iter_of_nerf(H, W, focal, mc, mf, batch, opts, sid, mode="validation", scene_config=scfg)
        loss = ((rgb_c - target) ** 2).mean() + ((rgb_f - target) ** 2).mean()
        loss.backward()
        return [N_(p.grad) for p in pl], float(loss.detach())

    spy = Spy(monkeypatch, [NEW, OLD, LAYERED])
    fg, _ = iteration(None)
    assert spy.calls[OLD] >= 2 and spy.calls[NEW] == 0 and spy.calls[LAYERED] == 0
    before = dict(spy.calls)
    (lg, _), bits = flag_of(hip, lambda: iteration("f16x2"))
    assert bits == 0
    assert spy.calls[NEW] >= 2 and spy.calls[OLD] == before[OLD] and spy.calls[LAYERED] == 0
    for d in range(4):
        err = np.linalg.norm(lg[d] - fg[d]) / np.linalg.norm(fg[d])
        print("plane %d: f16x2 against f32 fused %.3g" % (d, err))
        assert err < 2e-5, (d, err)
    opt = torch.optim.Adam(pl, lr=2e-3)
    losses = []
    for it in range(6):
        opt.zero_grad()
        losses.append(iteration("f16x2")[1])
        opt.step()
    assert losses[5] < losses[0], losses


def test_training_through_super_resolved_planes_reaches_the_sr_weights(hip, monkeypatch):
    """test_generic_train_fused.test_training_through_super_resolved_planes with the new attribute: one call of the new backward, finite nonzero
    EDSR weight gradients that agree with the f32 fused route's along a random direction within that test's 2e-2 relative + 1e-6"""
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
    m.train(); sr.train()
    P = 300
    x = np.concatenate([rng.uniform(-1.5, 2.0, (P, 3)), rng.standard_normal((P, 3))], 1).astype(np.float32)
    G = rng.standard_normal((P, 4)).astype(np.float32)
    monkeypatch.setenv(HANDLE, "1")

    def run(train_arithmetic):
        m.train_arithmetic = train_arithmetic
        for w in sr.inner_model.conv_weights():
            w.grad = None
        out = m(T(x))
        (out * T(G)).sum().backward()
        return np.concatenate([N_(w.grad).reshape(-1) for w in sr.inner_model.conv_weights()]).astype(np.float64)

    w_f = run(None)
    spy = Spy(monkeypatch, [NEW, OLD, LAYERED])
    w_l = run("f16x2")
    assert m.generic_train_arithmetic() == "f16x2" and spy.calls == {NEW: 1, OLD: 0, LAYERED: 0}
    assert np.isfinite(w_l).all() and np.abs(w_l).max() > 0
    dw = rng.standard_normal(w_f.shape)
    assert abs(w_l @ dw - w_f @ dw) <= 2e-2 * abs(w_f @ dw) + 1e-6
    print("SR weights: relative L2 f16x2 vs f32 fused %.3g" % (np.linalg.norm(w_l - w_f) / np.linalg.norm(w_f)))


def test_decoder_gradients_the_deterministic_scope_and_the_capacity_train_as_today(hip, monkeypatch):
    monkeypatch.setenv(HANDLE, "1")
    kw = dict(dec_channels=40, proj_combination="avg", viewdir_proj_combination="concat_pos", skip_connect_every=2)
    m, _ = seeded_model(hip, 23, **kw)
    m.train_arithmetic = "f16x2"
    x = T(points(40))
    spy = Spy(monkeypatch, [NEW, OLD, LAYERED])
    for p in m.decoder_parameters():                       # unfrozen: the layered route, exact f32, decoder gradients included
        p.requires_grad_(True)
    assert m.generic_train_arithmetic() == "f32"
    m(x).sum().backward()
    assert spy.calls == {NEW: 0, OLD: 0, LAYERED: 1} and all(p.grad is not None for p in m.decoder_parameters())
    freeze_decoder(m)
    with hip.capi.deterministic_scope(True):              # the deterministic mode: refused before any launch, as today
        assert m.generic_train_arithmetic() == "f32"
        with pytest.raises(Exception, match="[Dd]eterministic"):
            m(x)
    assert spy.calls == {NEW: 0, OLD: 0, LAYERED: 1}
    big, _ = seeded_model(hip, 9, size=4, view_size=4, dec_channels=4096, dec_density_layers=1, dec_rgb_layers=1, proj_combination="sum")
    big.train_arithmetic = "f16x2"
    assert big.generic_train_arithmetic() == "f32"
    big(x).sum().backward()
    assert spy.calls == {NEW: 0, OLD: 0, LAYERED: 2} and all(p.grad is not None and torch.isfinite(p.grad).all() for p in plane_list(hip, big))


# ---- the entry's refusals, 7. opcheck and the resources gate ---------------------------------------------------------------------------------
def test_entry_refusals(hip):
    m, _ = seeded_model(hip, 3, dec_channels=64, proj_combination="avg", viewdir_proj_combination="concat_pos")
    big, _ = seeded_model(hip, 9, size=4, view_size=4, dec_channels=4096, dec_density_layers=1, dec_rgb_layers=1, proj_combination="sum")
    x, G = T(points(40)), T(np.ones((40, 4), np.float32))
    fn, ptr = hip.capi.lib().nvsr_generic_decode_backward_fused_arith_ext, hip.capi.ptr
    for mdl, arith, null, status in ((m, 1, None, 1), (m, 3, None, 1), (m, -1, None, 1), (big, F16X2, None, 1), (m, F16X2, "packed", 3),
                                     (m, F16X2, "packed_bwd", 3), (m, F32, "packed", 0), (m, F16X2, None, 0)):
        planes, consts, nat, geometry = op_args(mdl)
        geo, n_pos, _, sc = hip.ops._generic_setup(planes, consts, nat, geometry, True, None, 40)
        packed, packed_bwd = blobs(mdl) if mdl is m else (nat, nat)
        gpl = [torch.zeros_like(p) for p in planes]
        d_planes = (C.c_void_p * 4)(*[t.data_ptr() for t in gpl])
        got = fn(C.byref(sc), C.byref(geo), ptr(nat), None if null == "packed" else ptr(packed), None if null else ptr(packed_bwd), 40, ptr(x), None,
                 ptr(G), d_planes, arith, hip.capi.stream())
        assert got == status, (arith, null, got)
        assert all((float(t.abs().max()) == 0) == (status != 0) for t in gpl[:3])
    planes, consts, nat, geometry = op_args(m)
    assert fn(C.byref(sc), C.byref(geo), ptr(nat), ptr(packed), ptr(packed_bwd), 0, ptr(x), None, ptr(G), d_planes, F16X2, hip.capi.stream()) == 0
    assert fn(C.byref(sc), C.byref(geo), ptr(nat), ptr(packed), ptr(packed_bwd), 40, ptr(x), None, ptr(G), None, F16X2, hip.capi.stream()) == 0
    with pytest.raises(Exception, match="arithmetic"):
        torch.ops.nvsr.triplane_decode_generic_fused_backward_arith(planes, consts, nat, packed, packed_bwd, geometry, x, G, [True] * 4, True, None, False, 3)
    same = limb_grads(m, N_(x), N_(G), arith=F32)
    assert all(ref64.rel_l2(a, b.astype(np.float64)) < 1e-6 for a, b in zip(same, both_ops(m, N_(x), N_(G))[0]))


def test_opcheck(hip):
    m, _ = seeded_model(hip, 3, dec_channels=64, proj_combination="avg", viewdir_proj_combination="concat_pos", skip_connect_every=3, align_corners=True)
    planes, consts, nat, geometry = op_args(m)
    packed, packed_bwd = blobs(m)
    torch.library.opcheck(torch.ops.nvsr.pack_generic_decoder_bwd, (nat, geometry, 3), test_utils=("test_schema", "test_faketensor"))
    args = (planes, consts, nat, packed, packed_bwd, geometry, T(points(50)), T(np.ones((50, 4), np.float32)), [True, False, True, True], True, None,
            False, F16X2)
    torch.library.opcheck(torch.ops.nvsr.triplane_decode_generic_fused_backward_arith, args, test_utils=("test_schema", "test_faketensor"))
    assert "pack_generic_decoder_bwd" in hip.ops.FORWARD_OPS


def test_kernel_resources_gate_covers_the_new_kernels(hip):
    """no scratch and no spilled vector registers in any instantiation: tools/kernel_resources.py --check, with both kernels in its list"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_resources
    finally:
        sys.path.pop(0)
    assert "generic_backward_fused_limb_kernel" in kernel_resources.BENCHMARKED and "generic_pack_limb_bwd_kernel" in kernel_resources.BENCHMARKED
    table = kernel_resources.kernel_table()
    mine = [k for k in table if "generic_backward_fused_limb_kernel" in k["name"]]
    assert len(mine) == 18 and all(k["scratch"] == 0 and k["vgpr_spill"] == 0 for k in mine), mine
    pack = [k for k in table if "generic_pack_limb_bwd_kernel" in k["name"]]
    assert len(pack) == 1 and pack[0]["scratch"] == 0 and pack[0]["vgpr_spill"] == 0
    done = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "--check"], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
