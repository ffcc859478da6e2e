"""Training the generic decoder geometries WITH decoder gradients on the fused launches (csrc/generic_fused_bwd.hip,
nvsr_generic_decode_backward_fused_record_ext, torch.ops.nvsr.triplane_decode_generic_fused_backward_record,
TwoDimPlanesModel.generic_decoder_train_route()): per chunk one launch that scatters the planes' gradients and records the operands of the
weight-gradient contraction, then the layered route's contractions on the record.  Held to the reference's own autograd (g19), to the float64
restatement tests/generic_train_decoder_ref.py and -- where the atomics cannot reorder anything -- to the BITS of the layered route
(csrc/generic.hip), which stays the reference implementation."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import load_golden
from test_generic_train_fused import (BIT_CASES, RAGGED, ROOT, SID, Spy, disjoint_points, op_args, plane_list, points, seeded_model, state_dict_of)
from test_hip_parity import DEV, N_, T, make_options
from test_oracle import G18_VARIANTS, G22_BOX

import generic_train_decoder_ref as ref64

pytestmark = pytest.mark.gpu
HANDLE = "NVSR_GENERIC_TRAIN_DECODER_FUSED"
OPS = ["triplane_decode_generic_fused_backward_record", "triplane_decode_generic_backward"]


def train_decoder(m, flag=True):
    for p in m.decoder_parameters():
        p.requires_grad_(flag)


def both_ops(m, x, G, noise=None, need=None, want_natural=True):
    """(fused, layered) results of the two backward operators: [d_natural, plane gradients [H,W,C] ...] as numpy"""
    planes, consts, nat, geometry = op_args(m)
    need = [True] * len(planes) if need is None else need
    args = (planes, consts, nat, geometry, T(x), T(G), want_natural, need, bool(m.align_corners), None if noise is None else T(noise),
            m.plane_interp == "bicubic")
    with torch.no_grad():
        f = torch.ops.nvsr.triplane_decode_generic_fused_backward_record(*args)
        l = torch.ops.nvsr.triplane_decode_generic_backward(*args)
    return [N_(t) for t in f], [N_(t) for t in l]


def model_grads(hip, m, x, G, monkeypatch, handle, sid=SID):
    """(out, d_natural or None, plane gradients [1,C,H,W] or None) of a training-mode model call under the handle"""
    monkeypatch.setenv(HANDLE, handle)
    pl, params = plane_list(hip, m, sid), list(m.decoder_parameters())
    for p in pl + params:
        p.grad = None
    out = m(T(x))
    (out * T(G)).sum().backward()
    gnat = None if all(p.grad is None for p in params) else np.concatenate([N_(p.grad).reshape(-1) for p in params])
    return N_(out), gnat, [None if p.grad is None else N_(p.grad) for p in pl]


def bits_equal(a, b):
    """torch.equal on the words: what torch.equal asks, and in addition the same sign of a zero and the same NaN where the layered route has one"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and torch.equal(torch.as_tensor(a.view(np.int32)), torch.as_tensor(b.view(np.int32)))


def colour_input_weights(m):
    """mask over the natural blob of the colour decoder's hidden weight matrices that read the decoder's input Xr -- layer 0 and the skip
    layers: the only parameters whose gradient contracts dZ with the view plane's features"""
    geometry = [int(v) for v in m.generic_geometry()]
    nd, nr, skip = geometry[3], geometry[4], geometry[5]
    params = list(m.decoder_parameters())                        # natural_blob order: density layers, fc_alpha, rgb layers, fc_rgb; weight then bias
    mask, o = np.zeros(sum(p.numel() for p in params), bool), 0
    for i, p in enumerate(params):
        l = (i - (2 * nd + 2)) // 2                              # the colour decoder's layer of parameter i
        if i >= 2 * nd + 2 and i % 2 == 0 and l < nr and (l == 0 or (skip > 0 and l - 1 > 0 and (l - 1) % skip == 0)):
            mask[o:o + p.numel()] = True
        o += p.numel()
    return mask


def test_training_with_decoder_gradients_takes_the_recording_backward(hip, monkeypatch):
    """fails without the feature: with the handle at 1 and decoder and planes requiring gradients, a g18 'avg_mult' model in train() answers
    'fused' and its backward is ONE call of triplane_decode_generic_fused_backward_record, none of the layered operator; with the handle at 0
    it is the other way round; in the deterministic mode the predicate answers 'layered' and the forward raises before any launch"""
    from test_hip_round2 import _variant_model
    g = load_golden("g18_decoder_variants.npz")
    m, sid, *_ = _variant_model(hip, g, "avg_mult")
    m.train()
    train_decoder(m)
    params = list(m.decoder_parameters())

    def run(handle):
        monkeypatch.setenv(HANDLE, handle)
        for p in plane_list(hip, m, sid) + params:
            p.grad = None
        spy = Spy(monkeypatch, OPS)
        m(T(g["avg_mult.x"])).sum().backward()
        assert all(p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0 for p in plane_list(hip, m, sid) + params)
        return {k: spy.calls[k] for k in OPS}

    monkeypatch.setenv(HANDLE, "1")
    assert m.generic_decoder_train_route() == "fused"
    assert run("1") == {OPS[0]: 1, OPS[1]: 0}
    monkeypatch.setenv(HANDLE, "0")
    assert m.generic_decoder_train_route() == "layered"
    assert run("0") == {OPS[0]: 0, OPS[1]: 1}
    monkeypatch.setenv(HANDLE, "1")
    launches = Spy(monkeypatch, OPS + ["triplane_decode_generic_fused", "triplane_decode_generic"])
    with hip.capi.deterministic_scope(True):
        assert m.generic_decoder_train_route() == "layered"
        with pytest.raises(hip.capi.DeterministicModeError):
            m(T(g["avg_mult.x"]))
    assert not any(launches.calls.values())
    monkeypatch.delenv(HANDLE)
    span = m.GENERIC_TRAIN_DECODER_FUSED_DEFAULT_HIDDEN
    assert m.generic_decoder_train_route() == ("fused" if span is not None and span[0] <= 64 <= span[1] else "layered")


def test_reference_gradients_of_the_five_geometries(hip, monkeypatch):
    """g19, the reference's own autograd: the training forward is the layered training forward bit for bit; gnat and the four plane gradients
    stay inside the bounds of test_generic_decoder_gradients_vs_reference (relative L2 < 2e-5, atol 3e-5 max|ref|); with only plane 1 requiring
    a gradient only plane 1 gets one; with only the decoder requiring gradients no plane gets one and gnat keeps the bounds"""
    from test_hip_round2 import _variant_model
    g, gg = load_golden("g18_decoder_variants.npz"), load_golden("g19_decoder_variant_grads.npz")
    names = [n for n in G18_VARIANTS if n + ".gout" in gg]
    assert len(names) == 5

    def held(got, ref, what):
        assert got.shape == ref.shape, what
        err = np.linalg.norm(got - ref) / np.linalg.norm(ref)
        print("%s: relative L2 %.3g" % (what, err))
        assert err < 2e-5, (what, err)
        np.testing.assert_allclose(got, ref, rtol=0, atol=3e-5 * float(np.abs(ref).max()), err_msg=what)

    for name in names:
        m, sid, *_ = _variant_model(hip, g, name)
        m.train()
        train_decoder(m)
        x, G = g[name + ".x"], gg[name + ".gout"]
        out_l, _, _ = model_grads(hip, m, x, G, monkeypatch, "0", sid)
        assert m.generic_decoder_train_route() == "layered"
        out_f, gnat, grads = model_grads(hip, m, x, G, monkeypatch, "1", sid)
        assert m.generic_decoder_train_route() == "fused"
        assert bits_equal(out_f, out_l), name
        held(gnat, gg[name + ".gnat"], name + " decoder")
        for d in range(4):
            held(grads[d], gg[name + ".gplane%d" % d], "%s plane %d" % (name, d))
        pl = plane_list(hip, m, sid)
        for p in pl:                                       # the decoder alone
            p.requires_grad_(False)
        spy = Spy(monkeypatch, OPS)
        _, gnat, only = model_grads(hip, m, x, G, monkeypatch, "1", sid)
        assert spy.calls == {OPS[0]: 1, OPS[1]: 0} and only == [None] * 4
        held(gnat, gg[name + ".gnat"], name + " decoder alone")
        pl[1].requires_grad_(True)                         # the decoder and plane 1
        _, gnat, only = model_grads(hip, m, x, G, monkeypatch, "1", sid)
        assert only[0] is None and only[2] is None and only[3] is None
        held(only[1], gg[name + ".gplane1"], name + " plane 1 alone")
        held(gnat, gg[name + ".gnat"], name + " decoder with plane 1")


@pytest.mark.parametrize("case", list(BIT_CASES))
def test_bits_of_the_layered_route(hip, case):
    """test_generic_train_fused's disjoint footprints (1 and 4 points; a gate closed at exactly 0, a NaN bias, a NaN view texel): d_natural -- one
    wave of one slab has points, every other addend is +0 -- and all planes are torch.equal to the layered operator's; a zero cotangent gives
    exactly +0 everywhere.  On hidden 31 / 33 also P in {31, 33, 300, 512} random points: d_natural is the layered route's bit for bit (the
    planes there share texels: test_ragged_point_counts_against_float64 holds them)."""
    m, _ = seeded_model(hip, 31, **BIT_CASES[case])
    with torch.no_grad():
        m.density_dec["0"][1].weight[2].zero_()
        m.density_dec["0"][1].bias[2] = 0.0
        m.rgb_dec["0"][1].bias[3] = float("nan")
        nan_texel = BIT_CASES[case].get("viewdir_proj_combination") != "mult"
        if nan_texel:
            plane_list(hip, m)[3][0, 5, 1, 1] = float("nan")
    rng = np.random.default_rng(17)
    for count in (1, 4):
        x = disjoint_points(m, count)
        G = rng.standard_normal((count, 4)).astype(np.float32)
        fused, layered = both_ops(m, x, G)
        # The NaN texel is an OPERAND of the contractions with Xr: the colour decoder's first (and skip) weight matrices take dZ[point 0] x
        # Xr[point 0] = 0 x NaN in both routes (the layered route's own result: its wgrad kernel multiplies the gated zero with the feature).
        # Every other parameter's gradient is finite.
        nan_ok = colour_input_weights(m) if nan_texel else np.zeros(layered[0].shape, bool)
        assert not np.isnan(layered[0][~nan_ok]).any() and np.isfinite(layered[0]).any() and np.nanmax(np.abs(layered[0])) > 0, (case, count)
        assert bits_equal(fused[0], layered[0]), (case, count)
        for d in range(1, 5):
            assert np.isfinite(layered[d]).all() and bits_equal(fused[d], layered[d]), (case, count, d)
        for want_natural, need in ((True, [False] * 4), (False, [True] * 4), (True, [False, True, False, False])):
            f2, l2 = both_ops(m, x, G, need=need, want_natural=want_natural)
            assert all(bits_equal(a, b) for a, b in zip(f2, l2)), (case, count, want_natural, need)
            assert bits_equal(f2[0], fused[0] if want_natural else fused[0][:0])
        fused, layered = both_ops(m, x, np.zeros((count, 4), np.float32))
        for i, (f, l) in enumerate(zip(fused, layered)):
            zero = ~np.isnan(l) if i == 0 else np.ones(l.shape, bool)
            assert not np.isnan(l[~nan_ok]).any() if i == 0 else zero.all()
            assert np.all(f[zero] == 0) and not np.signbit(f[zero]).any() and bits_equal(f, l), (case, count, i)
    if case in ("hidden31", "hidden33"):
        x_all, G_all = points(512, seed=5), rng.standard_normal((512, 4)).astype(np.float32)
        for P in (31, 33, 300, 512):
            fused, layered = both_ops(m, x_all[:P], G_all[:P])
            assert np.nanmax(np.abs(layered[0])) > 0 and bits_equal(fused[0], layered[0]), (case, P)


COUNTS = (0, 1, 31, 32, 33, 129, 300, 513, 2049)


def float64_rule(case, P, what, layered, fused, want, bound=2e-5):
    """the project's rule for these gradients: the layered route within `bound` of float64 first; the fused route within it and no more than
    1.5 x the layered route's error + 1e-7 (the two differ by the order of their float atomics only)"""
    el, ef = ref64.rel_l2(layered, want), ref64.rel_l2(fused, want)
    print("%s P=%d %s: layered %.3g fused %.3g" % (case, P, what, el, ef))
    if bound is not None:
        assert el < bound, (case, P, what, el)
        assert ef < bound, (case, P, what, ef)
    assert ef <= 1.5 * el + 1e-7, (case, P, what, ef, el)
    return el, ef


@pytest.mark.parametrize("case", list(RAGGED))
def test_ragged_point_counts_against_float64(hip, case):
    """P in {0, 1, 31, 32, 33, 129, 300, 513, 2049} on random 16 x 16 planes: the last two put a second wave and a second slab of the
    contraction to work.  d_natural and every plane against tests/generic_train_decoder_ref.py under float64_rule."""
    n_pos, kw, with_noise = RAGGED[case]
    m, planes = seeded_model(hip, 41, n_pos=n_pos, **kw)
    sd = state_dict_of(m)
    rng = np.random.default_rng(43)
    top = max(COUNTS)
    x_all, G_all = points(top, seed=47), rng.standard_normal((top, 4)).astype(np.float32)
    noise_all = (rng.standard_normal((top, 3)) * 0.02).astype(np.float32) if with_noise else None
    helper_kw = {k: v for k, v in kw.items() if k not in ("dec_channels", "num_plane_channels")}
    for P in COUNTS:
        x, G = x_all[:P], G_all[:P]
        noise = None if noise_all is None else noise_all[:P]
        fused, layered = both_ops(m, x, G, noise)
        if P == 0:
            assert all(np.all(f == 0) and f.shape == l.shape for f, l in zip(fused, layered))
            assert fused[0].shape == (m.natural_blob().numel(),) and [f.shape for f in fused[1:]] == [tuple(p.shape) for p in op_args(m)[0]]
            continue
        _, want_nat, want = ref64.gradients(sd, planes, G22_BOX, x, G, coord_noise=noise, **helper_kw)
        float64_rule(case, P, "d_natural", layered[0], fused[0], want_nat)
        for d in range(n_pos + 1):
            float64_rule(case, P, "plane %d" % d, layered[1 + d], fused[1 + d], want[d][0].transpose(1, 2, 0))


def test_chunk_boundary(hip):
    """P = chunk + 33 on the hidden-33 geometry, 16 x 16 planes: a second chunk of 33 points reuses the record.  Against the float64 helper the
    layered route's error is measured first; the fused route stays within 1.5 x that + 1e-7.  No absolute bound is fixed for this size (2^17
    points accumulate on 16 x 16 texels); measured on an MI355X, layered / fused: d_natural 6.59e-4 / 6.59e-4, planes 4.88e-4 / 4.88e-4,
    7.13e-4 / 7.13e-4, 5.82e-4 / 5.82e-4, 6.10e-4 / 6.10e-4 -- the same to three digits on both routes, which share one float32 forward
    (presumably its ReLU gates that float64 opens or shuts differently at a few of 2^17 points x 264 units; not examined further)."""
    chunk = hip.capi.generic_backward_chunk()
    P = chunk + 33
    m, planes = seeded_model(hip, 41, **BIT_CASES["hidden33"])
    sd = state_dict_of(m)
    rng = np.random.default_rng(59)
    x, G = points(P, seed=61), rng.standard_normal((P, 4)).astype(np.float32)
    fused, layered = both_ops(m, x, G)
    helper_kw = {k: v for k, v in BIT_CASES["hidden33"].items() if k != "dec_channels"}
    _, want_nat, want = ref64.gradients(sd, planes, G22_BOX, x, G, **helper_kw)
    float64_rule("chunk", P, "d_natural", layered[0], fused[0], want_nat, bound=None)
    for d in range(4):
        float64_rule("chunk", P, "plane %d" % d, layered[1 + d], fused[1 + d], want[d][0].transpose(1, 2, 0), bound=None)
    # the second chunk alone, through the same entry: its 33 points are the tail of the large call's d_natural in exact arithmetic
    tail_f, tail_l = both_ops(m, x[chunk:], G[chunk:])
    assert bits_equal(tail_f[0], tail_l[0])


def _skip2_pair(hip, g):
    from test_hip_round2 import _variant_model
    mc, sid, *_ = _variant_model(hip, g, "skip2")
    mf, *_ = _variant_model(hip, g, "skip2")
    mf.planes_ = mc.planes_
    for mm in (mc, mf):
        mm.train()
        train_decoder(mm)
    return mc, mf, sid


def test_iteration_through_run_one_iter_of_nerf_and_train_step(hip, monkeypatch):
    """64 rays, 16 + 16 samples, the 'skip2' coarse / fine pair, planes and both decoders trained: the pixels of the fused route are the
    layered route's bits; the first step's gradients of every plane and of both decoders lie within a relative L2 of 2e-5 of the handle-0
    run's (the bound both routes keep against float64); six TrainStep iterations with Adam lower the loss on the new operator alone"""
    g = load_golden("g18_decoder_variants.npz")
    mc, mf, sid = _skip2_pair(hip, g)
    opts, scfg = make_options(16, 16)
    H = W = 8
    focal = 0.5 * W / np.tan(0.5 * 0.6911112)
    ro, rd = hip.nerf_helpers.get_ray_bundle(H, W, focal, T(g["pose"]))
    batch = torch.stack([ro.reshape(-1, 3), rd.reshape(-1, 3)], 0)
    target = torch.rand((H * W, 3), generator=torch.Generator().manual_seed(4)).to(DEV) * 0.5 + 0.25
    pl = plane_list(hip, mc, sid)
    decs = [list(mc.decoder_parameters()), list(mf.decoder_parameters())]

    def iteration(handle):
        monkeypatch.setenv(HANDLE, handle)
        for p in pl + decs[0] + decs[1]:
            p.grad = None
        rgb_c, _, _, rgb_f, *_ = hip.train_utils.run_one_iter_of_nerf(H, W, focal, mc, mf, batch, opts, sid, mode="validation", scene_config=scfg)
        (((rgb_c - target) ** 2).mean() + ((rgb_f - target) ** 2).mean()).backward()
        return (rgb_c.detach().clone(), rgb_f.detach().clone(),
                [N_(p.grad) for p in pl] + [np.concatenate([N_(p.grad).reshape(-1) for p in ps]) for ps in decs])

    lc, lf, lg = iteration("0")
    spy = Spy(monkeypatch, OPS)
    fc, ff, fg = iteration("1")
    assert spy.calls[OPS[0]] >= 2 and spy.calls[OPS[1]] == 0
    assert torch.equal(fc, lc) and torch.equal(ff, lf)
    for i, (a, b) in enumerate(zip(fg, lg)):
        err = np.linalg.norm(a - b) / np.linalg.norm(b)
        print("gradient %d: relative L2 fused vs layered %.3g" % (i, err))
        assert np.isfinite(a).all() and err < 2e-5, (i, err)
    opt = torch.optim.Adam(decs[0] + decs[1], lr=2e-3)
    popt = torch.optim.Adam(pl, lr=2e-3)
    step = hip.training.TrainStep(mc, mf, opts, {"LR_planes", "decoder"}, optimizer=opt, planes_optimizer=popt)
    np.random.seed(3)
    torch.manual_seed(3)
    img = target.reshape(H, W, 3)
    monkeypatch.setenv(HANDLE, "1")
    spy = Spy(monkeypatch, OPS)
    losses = [step(it, img, T(g["pose"]), H, W, focal, 1, sid, scfg, H * W)["loss"] for it in range(6)]
    assert spy.calls[OPS[0]] >= 12 and spy.calls[OPS[1]] == 0
    assert all(np.isfinite(losses)) and losses[5] < losses[0], losses


def test_training_through_super_resolved_planes(hip, monkeypatch):
    """test_generic_train_fused.test_training_through_super_resolved_planes with the decoder trained as well: the training forward is the layered
    one bit for bit, the decoder's gradient lies within 2e-5 of the layered route's, and the EDSR weight gradients (and one LR plane's) agree
    in that test's own measure and tolerance -- <gradient, direction> along a random direction, within 2e-2 relative + 1e-6"""
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
    for p_ in m.planes_.values():
        p_.requires_grad_(False)
    train_decoder(m)
    params = list(m.decoder_parameters())
    lr_names = [hip.models.get_plane_name(sid, d) for d in range(3)]
    for n_ in lr_names:
        sr.LR_planes[n_].requires_grad_(True)
    m.train(); sr.train()
    P = 300
    x = np.concatenate([rng.uniform(-1.5, 2.0, (P, 3)), rng.standard_normal((P, 3))], 1).astype(np.float32)
    G = rng.standard_normal((P, 4)).astype(np.float32)

    def run(handle):
        monkeypatch.setenv(HANDLE, handle)
        for w in list(sr.inner_model.conv_weights()) + [sr.LR_planes[n_] for n_ in lr_names] + params:
            w.grad = None
        out = m(T(x))
        (out * T(G)).sum().backward()
        return (N_(out), np.concatenate([N_(w.grad).reshape(-1) for w in sr.inner_model.conv_weights()]).astype(np.float64),
                N_(sr.LR_planes[lr_names[1]].grad).astype(np.float64), np.concatenate([N_(p.grad).reshape(-1) for p in params]))

    out_l, w_l, lr_l, nat_l = run("0")
    assert m.generic_decoder_train_route() == "layered"
    spy = Spy(monkeypatch, OPS)
    out_f, w_f, lr_f, nat_f = run("1")
    assert m.generic_decoder_train_route() == "fused"
    assert spy.calls == {OPS[0]: 1, OPS[1]: 0}
    assert np.array_equal(out_f, out_l)
    assert bits_equal(nat_f, nat_l)                     # 300 points: one wave of one slab
    assert np.isfinite(w_f).all() and np.abs(w_f).max() > 0 and np.isfinite(lr_f).all() and np.abs(lr_f).max() > 0
    blob = np.concatenate([N_(w).reshape(-1) for w in sr.inner_model.conv_weights()])
    dw = rng.standard_normal(blob.shape) * np.abs(blob).mean()
    dl = rng.standard_normal(lr_l.shape) * 0.5
    assert abs(w_f @ dw - w_l @ dw) <= 2e-2 * abs(w_l @ dw) + 1e-6
    assert abs((lr_f * dl).sum() - (lr_l * dl).sum()) <= 2e-2 * abs((lr_l * dl).sum()) + 1e-6


def test_beyond_the_capacity_the_entry_refuses_and_the_model_trains_layered(hip, monkeypatch):
    monkeypatch.setenv(HANDLE, "1")
    m, _ = seeded_model(hip, 9, size=4, view_size=4, dec_channels=4096, dec_density_layers=1, dec_rgb_layers=1, proj_combination="sum")
    train_decoder(m)
    planes, consts, nat, geometry = op_args(m)
    x, G = T(points(40)), T(np.ones((40, 4), np.float32))
    geo, n_pos, n, sc = hip.ops._generic_setup(planes, consts, nat, geometry, True, None, 40)
    lib = hip.capi.lib()
    assert lib.nvsr_generic_backward_fused_supported(C.byref(geo), n_pos) == 0
    gpl, gnat = [torch.zeros_like(p) for p in planes], torch.zeros(n, device=DEV)
    ws = torch.zeros(lib.nvsr_generic_backward_fused_record_workspace_floats_ext(C.byref(geo), n_pos, 40), device=DEV)
    d_planes = (C.c_void_p * 4)(*[t.data_ptr() for t in gpl])
    status = lib.nvsr_generic_decode_backward_fused_record_ext(C.byref(sc), C.byref(geo), hip.capi.ptr(nat), 40, hip.capi.ptr(x), None, hip.capi.ptr(G),
                                                               hip.capi.ptr(gnat), d_planes, hip.capi.ptr(ws), hip.capi.stream())
    assert status == 1                                                     # NVSR_ERR_SHAPE
    assert all(float(t.abs().max()) == 0 for t in gpl + [gnat])
    with pytest.raises(Exception, match="capacity"):
        torch.ops.nvsr.triplane_decode_generic_fused_backward_record(planes, consts, nat, geometry, x, G, True, [True] * 4)
    assert m.generic_decoder_train_route() == "layered"
    spy = Spy(monkeypatch, OPS)
    m(x).sum().backward()
    assert spy.calls == {OPS[0]: 0, OPS[1]: 1}
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in plane_list(hip, m) + list(m.decoder_parameters()))


def test_strided_inputs_give_the_bits_of_contiguous_ones(hip):
    """x, d_out, coord_noise and the natural blob as views with strides (every other row of a column slice, every other column, a transpose, one
    column of a matrix): the operator makes them dense, and on four points of disjoint footprints -- nothing the atomics could reorder -- every
    result is the contiguous call's bit for bit"""
    m, _ = seeded_model(hip, 13, **BIT_CASES["hidden33"])
    planes, consts, nat, geometry = op_args(m)
    P = 4
    x = disjoint_points(m, P)
    rng = np.random.default_rng(3)
    G = rng.standard_normal((P, 4)).astype(np.float32)
    noise = np.zeros((P, 3), np.float32)
    dense = torch.ops.nvsr.triplane_decode_generic_fused_backward_record(planes, consts, nat, geometry, T(x), T(G), True, [True] * 4, True, T(noise), False)
    wide = torch.zeros((2 * P, 9), device=DEV)
    wide[::2, 2:8] = T(x)
    xs = wide[::2, 2:8]
    Gs = torch.zeros((P, 8), device=DEV)
    Gs[:, ::2] = T(G)
    ns = torch.zeros((3, P), device=DEV).t()
    nats = torch.zeros((nat.numel(), 2), device=DEV)
    nats[:, 1] = nat
    assert not xs.is_contiguous() and not Gs[:, ::2].is_contiguous() and not ns.is_contiguous() and not nats[:, 1].is_contiguous()
    strided = torch.ops.nvsr.triplane_decode_generic_fused_backward_record(planes, consts, nats[:, 1], geometry, xs, Gs[:, ::2], True, [True] * 4, True, ns, False)
    assert float(dense[0].abs().max()) > 0
    for a, b in zip(dense, strided):
        assert torch.equal(a, b)


def test_opcheck(hip):
    m, _ = seeded_model(hip, 3, dec_channels=64, proj_combination="avg", viewdir_proj_combination="concat_pos", skip_connect_every=3, align_corners=True)
    args = op_args(m) + (T(points(50)), T(np.ones((50, 4), np.float32)), True, [True, False, True, True], True, None, False)
    torch.library.opcheck(torch.ops.nvsr.triplane_decode_generic_fused_backward_record, args, test_utils=("test_schema", "test_faketensor"))


def test_kernel_resources_gate_covers_the_recording_kernel(hip):
    """no scratch and no spilled vector registers in any of the 18 recording instantiations: tools/kernel_resources.py --check, with the kernel
    in its list; the 18 instantiations of generic_backward_fused_kernel are still there beside them"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_resources
    finally:
        sys.path.pop(0)
    assert "generic_backward_fused_record_kernel" in kernel_resources.BENCHMARKED
    table = kernel_resources.kernel_table()
    mine = [k for k in table if "generic_backward_fused_record_kernel" in k["name"]]
    assert len(mine) == 18 and all(k["scratch"] == 0 and k["vgpr_spill"] == 0 for k in mine), mine
    assert len([k for k in table if "generic_backward_fused_kernel" in k["name"]]) == 18
    done = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "--check"], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
