"""GPU tests (-m gpu) of the SR convolutions' one-limb arithmetic 'f16' (NVSR_ARITH_F16 = 1, include/nvsr.h): operands rounded once to f16,
f32 accumulation -- conv3x3_limb16_kernel<PB, 4, 1> forward and data gradient, conv3x3_wgrad_limb_kernel<1>, through the C ABI, EDSR / PlanesSR,
TrainStep and the evaluation fall-back.  The arithmetic is restated in float64 by tests/conv_f16_ref.py.

Shapes: Cin 32 | 64 (one and two channel chunks: the patch double buffer), Cout 128 | 256 (one and two co-groups), inputs 8 x 40 and 7 x 37 (two
32-pixel column tiles with a ragged edge, row counts no multiple of any tile height), every rows_per_tile the entry points accept."""
import numpy as np
import pytest
import torch

import conv_f16_ref as R
from test_hip_parity import DEV, N_, T

pytestmark = pytest.mark.gpu
F16, F16X2, BF16X3 = 1, 2, 3
ROWS = (0, 2, 3, 4, 8, 16, 18, 19, 20, 22)          # 0 | 16 | 18 | 19 | 20 | 22: the 16x16x32 kernel (its choice, 2 | 3 | 4 | 6 rows); the others: bf16 limbs
ROWS_ONE_LIMB = (0, 16, 18, 19, 20, 22)
LAYERS = ((32, 128, 8, 40), (64, 256, 7, 37), (64, 128, 7, 37), (32, 256, 8, 40))          # Cin, Cout, H, W


def _pack(capi, w, dgrad=False):
    Cout, Cin = w.shape[:2]
    ci, co = (Cout, Cin) if dgrad else (Cin, Cout)          # the packed convolution's own channels
    pk = torch.empty(capi.lib().nvsr_conv3x3_packed_floats(ci, co), device=DEV)
    wd = T(w)
    capi.call("nvsr_pack_conv3x3_dgrad" if dgrad else "nvsr_pack_conv3x3", capi.ptr(wd), Cin, Cout, capi.ptr(pk), capi.stream())
    return pk


def _conv(capi, xd, pk, Cin, Cout, H, W, epi, skd, arith, rows):
    shape = (Cout // 4, 2 * (H - 2), 2 * (W - 2)) if epi == 3 else (Cout, H - 2, W - 2)
    out = torch.full(shape, -7.0, device=DEV)
    capi.call("nvsr_conv3x3_arith", capi.ptr(xd), Cin, H, W, capi.ptr(pk), Cout, epi, capi.ptr(skd), capi.ptr(out), arith, rows, capi.stream())
    return out


def _dgrad(capi, dyd, pk, Cin, Cout, H, W, arith, rows):
    dx = torch.full((Cin, H, W), -7.0, device=DEV)
    capi.call("nvsr_conv3x3_dgrad_arith", capi.ptr(dyd), Cin, H, W, capi.ptr(pk), Cout, capi.ptr(dx), arith, rows, capi.stream())
    return dx


def _wgrad(capi, dyd, xd, Cin, Cout, H, W, arith):
    ws = torch.empty(capi.lib().nvsr_conv3x3_wgrad_workspace_floats(Cin, H, W, Cout), device=DEV)
    dw = torch.zeros((Cout, Cin, 3, 3), device=DEV)
    capi.call("nvsr_conv3x3_wgrad_arith", capi.ptr(dyd), capi.ptr(xd), Cin, H, W, Cout, 1.0, capi.ptr(dw), capi.ptr(ws), arith, capi.stream())
    return dw


def test_equals_f16x2_on_representable_operands(hip):
    """Operands that are f16 numbers after their scale: 'f16x2''s low limbs are all zero, its two extra MFMAs per product block add exact zeros,
    and the order of chunks, taps and output blocks is the same -- so 'f16' must give 'f16x2''s numbers (torch.equal) with the same rows_per_tile:
    the forward with every epilogue (none, ReLU, residual, PixelShuffle), the data gradient (virtual border of 2), the weight gradient."""
    capi = hip.capi
    rng = np.random.default_rng(11)
    for Cin, Cout, H, W in LAYERS:
        x, w = R.representable_activations(rng, (Cin, H, W)), R.representable_weights(rng, (Cout, Cin, 3, 3))
        skip = rng.standard_normal((Cout, H + 2, W + 2), dtype=np.float32)
        xd, skd, pk = T(x), T(skip), _pack(capi, w)
        for epi in (0, 1, 2, 3):
            for rows in (r for r in ROWS if r != 8 or Cout % 256 == 0):          # (the 8-row wave tile exists for multiples of 256 output channels)
                one, two = (_conv(capi, xd, pk, Cin, Cout, H, W, epi, skd if epi == 2 else None, a, rows) for a in (F16, F16X2))
                assert torch.isfinite(one).all() and float(one.abs().max()) > 0 and torch.equal(one, two), (Cin, Cout, H, W, epi, rows)
        # weight gradient of this layer
        dy = R.representable_gradient(rng, (Cout, H - 2, W - 2), exponent=int(rng.integers(-24, 8)))
        dyd = T(dy)
        one, two = (_wgrad(capi, dyd, xd, Cin, Cout, H, W, a) for a in (F16, F16X2))
        assert float(one.abs().max()) > 0 and torch.equal(one, two), (Cin, Cout, H, W, "wgrad")
        # data gradient of the TRANSPOSED layer (Cout -> Cin channels of the forward: the gradient's convolution maps Cin -> Cout like the forward above)
        wt = R.representable_weights(rng, (Cin, Cout, 3, 3))                 # a layer with Cout inputs and Cin outputs
        g = R.representable_gradient(rng, (Cin, H - 2, W - 2), exponent=int(rng.integers(-24, 8)))
        gd, pkd = T(g), _pack(capi, wt, dgrad=True)
        for rows in (0, 2, 3, 4, 16, 18, 19, 20, 22):
            one, two = (_dgrad(capi, gd, pkd, Cout, Cin, H, W, a, rows) for a in (F16, F16X2))
            assert float(one.abs().max()) > 0 and torch.equal(one, two), (Cin, Cout, H, W, "dgrad", rows)
    # a layer the one-limb kernels do not take, asked for by name: refused, nothing written (inside a network it runs what 'f16x2' runs there)
    out = torch.full((256, 6, 38), -7.0, device=DEV)
    xn, pkn = T(rng.standard_normal((48, 8, 40), dtype=np.float32)), torch.zeros(capi.lib().nvsr_conv3x3_packed_floats(48, 256), device=DEV)
    assert capi.lib().nvsr_conv3x3_arith(capi.ptr(xn), 48, 8, 40, capi.ptr(pkn), 256, 0, None, capi.ptr(out), F16, 0, capi.stream()) == 1
    assert float(out.min()) == -7.0


def test_outputs_are_within_the_error_model(hip):
    """General operands, spread over several binades inside the normal f16 range of both scales.  Every output of the forward, the data gradient
    and the weight gradient lies within 1.01 n 2^-24 sum |w^||x^| of conv_f16_ref's value (n = 9 Cin; the contracted pixels for a weight
    gradient), and within (2^-10 + 2^-22 + 1.01 n 2^-24) sum |w||x| of float64 on the unquantised operands.
    Measured worst |error| / bound on an MI355X: forward 0.0081, data gradient 0.0068, weight gradient 0.0145 (the f32 sums behave like a random
    walk, the bound is their worst case); against float64 0.19 / 0.37 / 0.22."""
    capi = hip.capi
    rng = np.random.default_rng(12)
    spread = lambda shape, lo, hi: (rng.choice([-1.0, 1.0], shape) * np.exp2(rng.uniform(lo, hi, shape))).astype(np.float32)
    worst = dict(fwd=0.0, dgrad=0.0, wgrad=0.0, fwd64=0.0, dgrad64=0.0, wgrad64=0.0)

    def check(kind, got, ref, ref64, tag):
        v, absum, n = ref
        v64, abs64 = ref64
        r1 = float((np.abs(got - v) / R.bound(absum, n)).max())
        r2 = float((np.abs(got - v64) / R.bound_f64(abs64, n)).max())
        worst[kind], worst[kind + "64"] = max(worst[kind], r1), max(worst[kind + "64"], r2)
        print("%s %s: worst |error| / bound %.3f (reference), %.3f (float64)" % (kind, tag, r1, r2))
        assert r1 <= 1.0 and r2 <= 1.0, (kind, tag, r1, r2)

    for Cin, Cout, H, W in LAYERS:
        x, w = spread((Cin, H, W), -5, 3), spread((Cout, Cin, 3, 3), -9, -2)
        xd, pk = T(x), _pack(capi, w)
        ref, ref64 = R.conv_f16(x, w), R.conv_f64(x, w)
        for rows in ROWS_ONE_LIMB:
            check("fwd", N_(_conv(capi, xd, pk, Cin, Cout, H, W, 0, None, F16, rows)).astype(np.float64), ref, ref64, (Cin, Cout, H, W, rows))
        dy = spread((Cout, H - 2, W - 2), -20, -14) * np.float32(2.0 ** int(rng.integers(-20, 20)))
        assert np.abs(dy).min() * R.tensor_scale(dy) >= 2.0 ** -14                                     # (normal f16 numbers after the tensor's scale)
        dyd = T(dy)
        check("wgrad", N_(_wgrad(capi, dyd, xd, Cin, Cout, H, W, F16)).astype(np.float64), R.wgrad_f16(dy, x), R.wgrad_f64(dy, x), (Cin, Cout, H, W))
        wt = spread((Cin, Cout, 3, 3), -9, -2)                                                         # data gradient of a layer Cout -> Cin
        g = spread((Cin, H - 2, W - 2), -20, -14) * np.float32(2.0 ** int(rng.integers(-20, 20)))
        gd, pkd = T(g), _pack(capi, wt, dgrad=True)
        ref, ref64 = R.dgrad_f16(g, wt), R.conv_f64(g, R._flip(wt), pad=2)
        for rows in ROWS_ONE_LIMB:
            check("dgrad", N_(_dgrad(capi, gd, pkd, Cout, Cin, H, W, F16, rows)).astype(np.float64), ref, ref64, (Cin, Cout, H, W, rows))
    print("worst |error| / bound:", worst)


def test_it_is_not_f16x2(hip):
    """Operands with full 24-bit mantissas: the forward differs from 'f16x2''s somewhere, and from float64 by more than 'f16x2''s documented
    bound -- 2^-21 |W||x| per product, plus its f32 accumulation -- allows.  Guards against plumbing that silently runs the old mode."""
    capi = hip.capi
    rng = np.random.default_rng(13)
    Cin, Cout, H, W = 32, 128, 8, 40
    x = rng.standard_normal((Cin, H, W), dtype=np.float32)
    w = (rng.standard_normal((Cout, Cin, 3, 3), dtype=np.float32) / np.sqrt(9 * Cin)).astype(np.float32)
    xd, pk = T(x), _pack(capi, w)
    v64, abs64 = R.conv_f64(x, w)
    allowed = (2.0 ** -21 + 1.01 * 9 * Cin * R.U24) * abs64
    for rows in ROWS_ONE_LIMB:
        one, two = (N_(_conv(capi, xd, pk, Cin, Cout, H, W, 0, None, a, rows)).astype(np.float64) for a in (F16, F16X2))
        assert (np.abs(two - v64) <= allowed).all(), rows
        assert not np.array_equal(one, two) and (np.abs(one - v64) > allowed).any(), rows


def test_range_is_f16x2s(hip):
    """A weight of 300 or an activation of 5000 does not fit the lone limb: NaN in exactly the outputs it reaches (never a wrong number; the ReLU
    lets the NaN through), every other output untouched; through PlanesSR the range flag's bit 2 is raised, and in-range launches leave it zero."""
    capi = hip.capi
    rng = np.random.default_rng(14)
    Cin, Cout, H, W = 64, 128, 12, 40
    x = rng.standard_normal((Cin, H, W), dtype=np.float32)
    w = (rng.standard_normal((Cout, Cin, 3, 3), dtype=np.float32) / np.sqrt(9 * Cin)).astype(np.float32)
    conv = lambda xa, wa, arith, epi: N_(_conv(capi, T(xa), _pack(capi, wa), Cin, Cout, H, W, epi, None, arith, 0))
    for epi in (0, 1):
        base = conv(x, w, F16, epi)
        assert np.isfinite(base).all()
        xb = x.copy()
        xb[5, 6, 20] = 5000.0                            # reaches outputs (.., 4..6, 18..20)
        bad = conv(xb, w, F16, epi)
        hit = np.zeros_like(bad, bool)
        hit[:, 4:7, 18:21] = True
        assert np.isnan(bad[hit]).all() and np.array_equal(bad[~hit], base[~hit]), epi
        assert np.isfinite(conv(xb, w, BF16X3, epi)).all()
        wb = w.copy()
        wb[17, 3, 1, 1] = 300.0                          # output channel 17
        bad = conv(x, wb, F16, epi)
        assert np.isnan(bad[17]).all() and np.array_equal(np.delete(bad, 17, 0), np.delete(base, 17, 0)), epi
    # the SR range flag (bit 2), through the entry point that raises it
    torch.manual_seed(3)
    sr = hip.models.PlanesSR(hip.models.EDSR, 2, 48, 48, {"model": {"hidden_size": 128, "n_blocks": 1}}, "bilinear").to(DEV)
    sr.eval()
    sr.inner_model.arithmetic = "f16"
    sr.set_LR_plane(T(rng.standard_normal((1, 48, 12, 12), dtype=np.float32) * 0.5), id="p0", save_interpolated=False)
    flag = capi.range_flag(torch.device(DEV))
    flag.reset()
    with torch.no_grad():
        out = sr("p0")
    assert torch.isfinite(out).all() and capi.RangeFlag.raised(flag.read_async()) == 0
    with torch.no_grad():
        sr.inner_model.residual[0].conv1.weight[17, 3, 1, 1] = 300.0
    sr.inner_model.invalidate()
    sr.clear_SR_planes()
    flag.reset()
    with torch.no_grad():
        out = sr("p0")
    assert torch.isnan(out).any() and capi.RangeFlag.raised(flag.read_async()) == 2
    flag.reset()


@pytest.fixture(scope="module")
def e2e(hip, oracle):
    """the small PlanesSR(EDSR) case of conv_f16_ref: its oracle values (computed once) and the GPU run in 'f16'"""
    sr, lrs, d_outs = R.e2e_case(hip.models)
    orc = R.e2e_oracle(oracle, sr, lrs, d_outs, with_crops=False)
    sr = sr.to(DEV)
    sr.train()
    sr.inner_model.arithmetic = "f16"
    reqs = [("p%d" % k, R.E2E["rois"][k]) for k in range(3)]

    def run():
        planes = [torch.nn.Parameter(T(lr)[None]) for lr in lrs]
        sr.clear_SR_planes(all_planes=True)
        for k, t in enumerate(planes):
            sr.set_LR_plane(t, id="p%d" % k, save_interpolated=False)
        for p_ in sr.parameters():
            p_.grad = None
        outs = sr.forward_many(reqs)
        sum((torch.nan_to_num(o) * T(w)[None]).sum() for o, w in zip(outs, d_outs)).backward()
        dw = torch.cat([(w.grad if w.grad is not None else torch.zeros_like(w)).reshape(-1) for w in sr.inner_model.conv_parameters()])
        return dict(out=[o.detach()[0] for o in outs], d_lr=[t.grad.detach()[0] for t in planes], dw=dw.detach().clone())
    return dict(sr=sr, orc=orc, run=run, lrs=lrs, reqs=reqs)


def test_small_network_end_to_end_vs_oracle(hip, e2e):
    """EDSR(48 -> 48, hidden 128, 2 blocks, x2) inside PlanesSR on 12 x 12 planes, three regions of different sizes through the batched ragged
    route (PlanesSRBatchFn), forward and backward.  Yardstick: the project's float64 oracle.  e_ref = rms(reference - oracle) / rms(oracle), with
    conv_f16_ref's chain of the arithmetic, was computed on the CPU (conv_f16_ref.E2E_EREF; tests/test_conv_f16_host.py recomputes it):
    output 1.0192e-05, LR-plane gradient 1.1677e-05, the 8 layers' weight gradients 4.8535e-04, 1.4708e-02, 6.1395e-04, 1.3653e-02, 5.9305e-04,
    4.1573e-04, 4.1446e-04, 4.1328e-04.  The GPU stays within 2 x e_ref for each (a rounding flip at an f16 boundary moves single elements by
    2^-11, not the rms); its weight gradients are the same bits in two identical runs."""
    a = e2e["run"]()
    got = dict(out=[N_(o).astype(np.float64) for o in a["out"]], d_lr=[N_(g).astype(np.float64) for g in a["d_lr"]], dw=N_(a["dw"]).astype(np.float64))
    orc = e2e["orc"]
    for o, g in zip(orc["out"], got["out"]):
        assert np.array_equal(np.isnan(o), np.isnan(g))
    e, rec = R.e2e_errors(got, orc), R.E2E_EREF
    print("GPU vs oracle: out %.4e (e_ref %.4e)  d_lr %.4e (%.4e)  dw %s (%s)" % (e["out"], rec["out"], e["d_lr"], rec["d_lr"],
          ", ".join("%.4e" % v for v in e["dw"]), ", ".join("%.4e" % v for v in rec["dw"])))
    assert e["out"] <= 2 * rec["out"] and e["d_lr"] <= 2 * rec["d_lr"], e
    assert len(e["dw"]) == len(rec["dw"]) and all(x <= 2 * y for x, y in zip(e["dw"], rec["dw"])), e["dw"]
    b = e2e["run"]()
    assert float(a["dw"].abs().max()) > 0 and torch.equal(a["dw"], b["dw"]) and all(torch.equal(torch.nan_to_num(x), torch.nan_to_num(y)) for x, y in zip(a["out"], b["out"]))


def test_one_plane_route_gives_the_batched_routes_outputs(hip, e2e):
    """the same three regions plane by plane (PlanesSR.forward in training mode: nvsr_planes_sr_train, one launch per layer and plane): the forward
    has a static scale, so its outputs are the batched route's bits; the backward runs and leaves finite gradients on the weights and the plane"""
    a = e2e["run"]()
    sr = e2e["sr"]
    for k, req in enumerate(e2e["reqs"]):
        plane = torch.nn.Parameter(T(e2e["lrs"][k])[None])
        sr.clear_SR_planes(all_planes=True)
        sr.set_LR_plane(plane, id=req[0], save_interpolated=False)
        for p_ in sr.parameters():
            p_.grad = None
        out = sr(req)
        assert out.requires_grad and torch.equal(torch.nan_to_num(out.detach()[0]), torch.nan_to_num(a["out"][k])), k
        torch.nan_to_num(out).square().sum().backward()
        gw = [w.grad for w in sr.inner_model.conv_parameters()]
        assert all(g_ is not None and torch.isfinite(g_).all() and float(g_.abs().max()) > 0 for g_ in gw) and torch.isfinite(plane.grad).all()
        assert float(plane.grad.abs().max()) > 0


def _tiny_sr_scene(hip, hid=128, nb=1, train=False):
    """a 24^2-texel synthetic scene whose fine model samples planes super-resolved x4 by a one-block EDSR of 128 channels (the wide kernels run);
    train: set up like an SR-refinement run (what = ['SR']: only the SR network receives gradients, the coarse pass under torch.no_grad)"""
    from bench import make_synthetic_scene, render_options
    mc, mf, sid, pose = make_synthetic_scene(DEV, plane_res=24, view_res=8, seed=9)
    torch.manual_seed(3)
    sr = hip.models.PlanesSR(hip.models.EDSR, 4, 48, 48, {"model": {"hidden_size": hid, "n_blocks": nb}}, "bilinear").to(DEV)
    if train:
        for m in (mc, mf):
            for p_ in m.parameters():
                p_.requires_grad_(False)
            m.train()
        sr.train()
        mf.detach_LR_planes = False
        mc.optional_no_grad = torch.no_grad
    mf.assign_SR_model(sr, SR_viewdir=False)
    mf.assign_LR_planes()
    H = W = 40
    focal = 0.5 * W / np.tan(0.5 * 0.6911112)
    opts, scfg = render_options(16, 16)
    return mc, mf, sr, sid, pose, H, W, focal, opts, scfg


def test_train_step_refines_the_sr_network_in_f16(hip):
    """training.TrainStep with what2train = ['SR'] and inner_model.arithmetic = 'f16' on a tiny scene: the iterations run, the SR optimizer steps,
    the parameters stay finite and the network's arithmetic is what it was set to"""
    mc, mf, sr, sid, pose, H, W, focal, opts, scfg = _tiny_sr_scene(hip, train=True)
    sr.inner_model.arithmetic = "f16"
    img = torch.rand(H, W, 3, generator=torch.Generator().manual_seed(5)).to(DEV)
    sr_opt = torch.optim.Adam(sr.parameters(), lr=1e-3)
    step = hip.training.TrainStep(mc, mf, opts, {"SR"}, SR_optimizer=sr_opt, SR_model=sr, sr_loss="fine")
    np.random.seed(4)
    before = [p_.detach().clone() for p_ in sr.parameters()]
    for it in range(3):
        r = step(it, img, pose, H, W, focal, 1, sid, scfg, 200, sr_iter=True)
        assert r["fine_loss"] is not None and np.isfinite(r["loss"])
    assert any(not torch.equal(a, b.detach()) for a, b in zip(before, sr.parameters()))
    assert all(torch.isfinite(p_).all() for p_ in sr.parameters()) and sr.inner_model.arithmetic == "f16"


def test_evaluation_falls_back_from_f16_like_from_f16x2(hip):
    """An evaluation frame through an SR network beyond the range (a trunk weight of 300) in 'f16': one warning, the SR stage runs again in 'bf16x3',
    the pixels are finite, and the network is back in 'f16' afterwards; a second frame of the same parameters neither warns nor super-resolves again"""
    import warnings
    mc, mf, sr, sid, pose, H, W, focal, opts, scfg = _tiny_sr_scene(hip)
    sr.eval()
    sr.inner_model.arithmetic = "f16"
    ro, rd = hip.nerf_helpers.get_ray_bundle(H, W, focal, pose)
    ev = lambda: hip.train_utils.eval_nerf(H, W, focal, mc, mf, ro, rd, opts, scene_id=sid, scene_config=scfg)
    with torch.no_grad():
        sr.inner_model.residual[0].conv1.weight[17, 3, 1, 1] = 300.0
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        first = ev()
        second = ev()
    ours = [c for c in caught if "bf16x3" in str(c.message)]
    assert len(ours) == 1, [str(c.message)[:80] for c in caught]
    assert torch.isfinite(first[3]).all() and torch.equal(first[3], second[3])
    assert sr.inner_model.arithmetic == "f16" and sr.__dict__.get("_planes_arith") == "bf16x3"
    sr.inner_model.arithmetic = "bf16x3"          # the fall-back's frame is what 'bf16x3' renders in the first place
    sr.clear_SR_planes()
    assert torch.equal(ev()[3], first[3])
