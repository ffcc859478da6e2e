"""GPU parity tests added in round 2 (-m gpu): every row-tile instantiation of the SR convolutions and the full-size 256 x 32 EDSR
against the oracle, the stated error bound of the bf16x3 limb arithmetic on adversarial operands, per-call arithmetic on concurrent
streams, and the torch.library operators (torch.ops.nvsr.*, opcheck)."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_hip_parity import DEV, N_, T, build_model

pytestmark = pytest.mark.gpu
ARITH = {"f32": 0, "bf16x3": 3, "f16x2": 2}


# ---------------------------------------------------------------------------------------------------------------------------------
# SR convolutions: every row-tile variant (models.py:769-822 -> csrc/sr.hip launch_conv)
# ---------------------------------------------------------------------------------------------------------------------------------
def test_conv3x3_every_row_tile_variant_vs_oracle(hip, oracle):
    """The wide (multiple-of-256 output channels) conv kernels exist in 2-, 3- and 4-row tile instantiations, and at 200^2 -> 800^2 the
    launcher's cost model picks the 3- and 4-row ones for most layers, while every small test shape gets 2 rows.  Force each
    instantiation (rows_per_tile of nvsr_conv3x3_arith / nvsr_conv3x3_dgrad_arith) of both kernels (exact f32 / bf16x3 limbs), with
    every fused epilogue, on shapes whose row count is ragged for 2, 3 and 4 rows, against the oracle.  Tolerance as in
    test_conv3x3_shapes_vs_oracle: 3e-5 on O(1) outputs."""
    rng = np.random.default_rng(41)
    capi = hip.capi
    #        Cin  Cout  H   W   epilogue (0 none, 1 ReLU, 2 residual, 3 PixelShuffle)
    cases = [(48, 256, 15, 45, 0), (256, 256, 15, 70, 1), (256, 256, 13, 40, 2), (256, 1024, 9, 37, 3), (256, 512, 7, 33, 0)]
    for Cin, Cout, H, W, epi in cases:
        x = rng.standard_normal((Cin, H, W), dtype=np.float32)
        w = (rng.standard_normal((Cout, Cin, 3, 3), dtype=np.float32) / np.sqrt(9 * Cin)).astype(np.float32)
        skip = rng.standard_normal((Cout, H + 2, W + 2), dtype=np.float32) if epi == 2 else None
        xd, wd = T(x), T(w)
        pk = torch.empty(capi.lib().nvsr_conv3x3_packed_floats(Cin, Cout), device=DEV)
        capi.call("nvsr_pack_conv3x3", capi.ptr(wd), Cin, Cout, capi.ptr(pk), capi.stream())
        ref = oracle.conv3x3(x, w, relu=(epi == 1))
        if epi == 2:      # _Residual_Block: conv * 0.1 + centre-cropped identity (models.py:781-785)
            ref = (ref.astype(np.float64) * np.float64(np.float32(0.1)) + skip[:, 2:-2, 2:-2]).astype(np.float32)
        if epi == 3:
            ref = ref.reshape(Cout // 4, 2, 2, H - 2, W - 2).transpose(0, 3, 1, 4, 2).reshape(Cout // 4, 2 * (H - 2), 2 * (W - 2))
        skd = None if skip is None else T(skip)
        results = {}
        for mode in ("bf16x3", "f32"):
            # (8: round 3's one-output-block x 8-row wave tile; 16: the 16x16x32-MFMA kernel -- limb arithmetic only, 16 only where Cin % 32 == 0
            #  and Cout % 128 == 0; 0 = what the launcher picks, i.e. 16 for those layers)
            limb16 = mode == "bf16x3" and Cin % 32 == 0 and Cout % 128 == 0
            for rows in ((2, 3, 4, 8) + ((16, 0) if limb16 else ()) if mode == "bf16x3" else (2, 3, 4)):
                out = torch.full(ref.shape, -7.0, device=DEV)
                capi.call("nvsr_conv3x3_arith", capi.ptr(xd), Cin, H, W, capi.ptr(pk), Cout, epi, capi.ptr(skd), capi.ptr(out), ARITH[mode],
                          rows, capi.stream())
                np.testing.assert_allclose(N_(out), ref, rtol=0, atol=3e-5, err_msg=str((Cin, Cout, H, W, epi, mode, rows)))
                results[(mode, rows)] = out
            # the row tiling does not change the arithmetic of an output element: the instantiations agree bit for bit (the 16x16x32 kernel sums
            # 32 input channels per instruction instead of 16: same products, another f32 accumulation order)
            assert all(torch.equal(results[(mode, 2)], results[k]) for k in results if k[0] == mode and k[1] in (2, 3, 4, 8))
            if limb16:
                assert torch.equal(results[(mode, 16)], results[(mode, 0)]) and not torch.equal(results[(mode, 16)], results[(mode, 4)])
        # NVSR_ARITH_F16X2 (round 3): the 16x16x32 kernel on 2 f16 limbs for the eligible layers -- every row instantiation, same tolerance, bit-identical
        # to each other, and at least as close to the (double-accumulating) oracle as the 3-bf16-limb kernel; other layers run the bf16x3 kernels
        if Cin % 32 == 0 and Cout % 128 == 0:
            f16 = {}
            for rows in (0, 16, 18, 19, 20, 22):            # (22: the 6-row tile, f16 limbs only)
                out = torch.full(ref.shape, -7.0, device=DEV)
                capi.call("nvsr_conv3x3_arith", capi.ptr(xd), Cin, H, W, capi.ptr(pk), Cout, epi, capi.ptr(skd), capi.ptr(out), ARITH["f16x2"],
                          rows, capi.stream())
                np.testing.assert_allclose(N_(out), ref, rtol=0, atol=3e-5, err_msg=str((Cin, Cout, H, W, epi, "f16x2", rows)))
                f16[rows] = out
            assert all(torch.equal(f16[0], v) for v in f16.values())
            e16, e3 = np.abs(N_(f16[0]).astype(np.float64) - ref).max(), np.abs(N_(results[("bf16x3", 16)]).astype(np.float64) - ref).max()
            print("conv %s: max |out - oracle|  f16x2 %.3g  bf16x3 %.3g  f32 %.3g" % ((Cin, Cout, H, W, epi), e16, e3,
                                                                                        np.abs(N_(results[("f32", 4)]).astype(np.float64) - ref).max()))
            assert e16 <= 1.25 * e3 + 1e-7
        else:
            out = torch.full(ref.shape, -7.0, device=DEV)
            capi.call("nvsr_conv3x3_arith", capi.ptr(xd), Cin, H, W, capi.ptr(pk), Cout, epi, capi.ptr(skd), capi.ptr(out), ARITH["f16x2"], 0, capi.stream())
            assert torch.equal(out, results[("bf16x3", 4)])
    # invalid rows_per_tile / arithmetic are refused, nothing is written
    out = torch.full((256, 13, 43), -7.0, device=DEV)
    x = T(rng.standard_normal((48, 15, 45), dtype=np.float32))
    pk = torch.zeros(capi.lib().nvsr_conv3x3_packed_floats(48, 256), device=DEV)
    for arith, rows in ((3, 5), (3, 1), (7, 0), (1, 0), (0, 8), (3, 16), (0, 16), (2, 16), (2, 21)):   # (8 / 16 exist in the limb kernel only; 16 needs Cin % 32 == 0: 48 is not)
        st = capi.lib().nvsr_conv3x3_arith(capi.ptr(x), 48, 15, 45, capi.ptr(pk), 256, 0, None, capi.ptr(out), arith, rows, capi.stream())
        assert st == 1 and float(out.min()) == -7.0
    # data gradient (virtual zero border, flipped + transposed kernel): every row-tile variant, both kernels
    for Cin, Cout, H, W in ((256, 256, 15, 38), (48, 256, 11, 70), (256, 1024, 8, 35)):
        w = (rng.standard_normal((Cout, Cin, 3, 3), dtype=np.float32) / np.sqrt(9 * Cin)).astype(np.float32)
        dy = rng.standard_normal((Cout, H - 2, W - 2), dtype=np.float32)
        pk = torch.empty(capi.lib().nvsr_conv3x3_packed_floats(Cout, Cin), device=DEV)
        capi.call("nvsr_pack_conv3x3_dgrad", capi.ptr(T(w)), Cin, Cout, capi.ptr(pk), capi.stream())
        wt = np.ascontiguousarray(w.transpose(1, 0, 2, 3)[:, :, ::-1, ::-1])
        ref = oracle.conv3x3(np.pad(dy, ((0, 0), (2, 2), (2, 2))), wt)
        dyd = T(dy)
        for mode in ("bf16x3", "f32"):
            for rows in (0, 2, 3, 4) + ((16,) if (mode == "bf16x3" and Cout % 32 == 0 and Cin % 128 == 0) else ()):
                dx = torch.full((Cin, H, W), -7.0, device=DEV)
                capi.call("nvsr_conv3x3_dgrad_arith", capi.ptr(dyd), Cin, H, W, capi.ptr(pk), Cout, capi.ptr(dx), ARITH[mode], rows, capi.stream())
                np.testing.assert_allclose(N_(dx), ref, rtol=0, atol=3e-5 * max(1.0, np.sqrt(Cout / Cin)),
                                           err_msg="dgrad " + str((Cin, Cout, H, W, mode, rows)))


def _full_size_sr(hip, seed=21):
    torch.manual_seed(seed)
    sr = hip.models.PlanesSR(hip.models.EDSR, 4, 48, 48, {"model": {"hidden_size": 256, "n_blocks": 32}}, "bilinear").to(DEV)
    with torch.no_grad():
        for p_ in sr.parameters():
            p_.mul_(10.0)          # PlanesSR initialises at 1/10 of He scale (models.py:843-848); x10 keeps 66 layers of activations O(1)
    return sr


def test_full_size_edsr_windows_vs_oracle(hip, oracle):
    """BASELINE config 3 at its real size: PlanesSR(EDSR 256 channels x 32 blocks, x4) on the three 200^2 position planes of a scene in
    one batched pass (the product path of a render: models.native_scene -> super_resolve_many) -- the shapes at which the launcher picks
    the 3- and 4-row conv tiles.  Three 8x8-texel LR windows (32x32 HR) are compared with the oracle run on exactly the input that
    determines them: the window plus the network's 68-texel receptive-field halo (models.py:836-842) cut out of the replicate-padded
    plane, 144^2 -> 34^2 -> centre 32^2, plus the bilinear x4 residual of the full plane (models.py:918-919).  Windows: the top-left
    corner (halo = replicate padding), an interior window at odd offsets (inside different row / column tiles of every layer), the
    bottom-right corner.  Both arithmetic modes.  Then the ROI (training-mode) path at this size against the full-plane values."""
    sr = _full_size_sr(hip)
    sr.eval()
    rng = np.random.default_rng(22)
    R, sf, pad, over = 200, 4, 68, 1
    assert sr.inner_model.required_padding == pad and sr.HR_overpadding == over
    lrs = [(rng.standard_normal((48, R, R), dtype=np.float32) * 0.5) for _ in range(3)]
    names = ["p0", "p1", "p2"]
    sd = {k: N_(v) for k, v in sr.state_dict().items()}
    blob, nblocks = oracle.edsr_blob(sd)
    assert nblocks == 32
    windows = [(0, 0, 0), (1, 96, 57), (2, R - 8, R - 8)]              # (plane, first LR row, first LR column)
    refs = []
    for pl, ay, ax in windows:
        padded = np.pad(lrs[pl], ((0, 0), (pad, pad), (pad, pad)), mode="edge")
        crop = np.ascontiguousarray(padded[:, ay: ay + 8 + 2 * pad, ax: ax + 8 + 2 * pad])          # [48,144,144]
        diff = oracle.edsr_forward(crop, blob, 48, 256, 32, 2)
        assert diff.shape == (48, 34, 34)
        up = oracle.upsample_bilinear(lrs[pl], sf)
        refs.append(diff[:, over:-over, over:-over] + up[:, sf * ay: sf * ay + 32, sf * ax: sf * ax + 32])
    scale = max(float(np.abs(r).max()) for r in refs)
    for mode, tol in (("f16x2", 1e-4), ("bf16x3", 1e-4), ("f32", 1e-4)):
        sr.inner_model.arithmetic = mode
        sr.clear_SR_planes(all_planes=True)
        for n, lr in zip(names, lrs):
            sr.set_LR_plane(T(lr)[None], id=n, save_interpolated=False)
        with torch.no_grad():
            sr.super_resolve_many(names)
        assert sorted(sr.SR_planes) == names
        worst = 0.0
        for (pl, ay, ax), ref in zip(windows, refs):
            got = N_(sr.SR_planes[names[pl]][0, :, sf * ay: sf * ay + 32, sf * ax: sf * ax + 32])
            err = float(np.abs(got - ref).max())
            worst = max(worst, err)
            # 66 chained convolutions with K = 2304 f32 products each, outputs O(1): stated tolerance 1e-4 of the output range
            assert err <= tol * max(1.0, scale), (mode, pl, ay, ax, err, scale)
        print("full-size EDSR windows, %s: max |err| %.2e (output range %.2f)" % (mode, worst, scale))
    # ROI path at full size (what a band-sharded SR stage and an SR training step run): identical values inside the ROI, NaN outside
    sr.inner_model.arithmetic = None
    sr.clear_SR_planes()
    with torch.no_grad():
        full = sr("p1").clone()
        sr.clear_SR_planes()
        sr.train()
        roi = torch.tensor([[-0.31, 0.12], [0.07, 0.55]])            # [[ymin, xmin], [ymax, xmax]] in [-1, 1]
        part = sr(("p1", roi.to(DEV)))
    valid = ~torch.isnan(part)
    frac = float(valid.float().mean())
    assert 0.03 < frac < 0.2 and torch.equal(part[valid], full[valid])
    # ... and through the differentiable training forward (torch.ops.nvsr.planes_sr_train keeps the activations): same values
    lr_p = torch.nn.Parameter(T(lrs[1])[None])
    sr.clear_SR_planes(all_planes=True)
    sr.set_LR_plane(lr_p, id="p1", save_interpolated=False)
    small = torch.tensor([[-0.05, -0.02], [0.04, 0.06]])
    out = sr(("p1", small.to(DEV)))
    assert out.requires_grad
    v2 = ~torch.isnan(out)
    assert torch.equal(out.detach()[v2], full[v2]) and int(v2.sum()) > 0


# ---------------------------------------------------------------------------------------------------------------------------------
# The real bound of the bf16x3 limb arithmetic (include/nvsr.h, csrc/limb_core.h)
# ---------------------------------------------------------------------------------------------------------------------------------
def _adversarial(rng, shape, pattern, sign=None):
    """f32 values with chosen mantissa bits: 'ones' = all 23 stored bits set (1.9999999 x 2^e); 'low16' = the 7 leading stored bits
    clear and the 16 low bits set (1.0078124 x 2^e: the leading limb is 2^e exactly, the middle and low limbs take their largest
    possible share, 2^-7 and 2^-15 of the value)"""
    mant = {"ones": 0x7FFFFF, "low16": 0x00FFFF}[pattern]
    e = rng.integers(124, 128, size=shape).astype(np.uint32)            # 2^-3 .. 2^0
    s = rng.integers(0, 2, size=shape).astype(np.uint32) if sign is None else ((sign < 0).astype(np.uint32))
    return ((s << 31) | (e << 23) | np.uint32(mant)).astype(np.uint32).view(np.float32)


def test_limb_error_bound(hip):
    """Measured worst case of the bf16x3 decoder arithmetic against its stated bound (include/nvsr.h).  One decoder layer with K = 192
    -- rgb layer 0 (models.py:409-413) -- is isolated with the layer-input record of the training forward: the record holds the exact f32
    layer input X [P,192] the kernel multiplied and the layer's post-ReLU output H [P,128]; the weights W are ours.  Operands are
    adversarial: every mantissa is all ones or (the true worst case of truncation limbs) has its low 16 bits set, and the signs are
    arranged so that all 192 products of a row are positive -- the dropped limb products Wm xl + Wl xm + Wl xl then all have the same sign
    and add up instead of averaging out.  Reported: max over all outputs of |H - float64(W x)| / sum_k |W_k x_k| for exact f32 and for
    bf16x3 (and the mean SIGNED error: a one-sided bias shows as |mean| ~ max).  Asserted, per output:
        |err| / sum|w||x|  <=  2^-21 + 2^-30                    the three dropped limb products at their largest (2^-7 * 2^-15 twice,
                                                                 2^-15 * 2^-15; zero for the exact-f32 kernel)
                              + n_acc * 2^-24                    one f32 rounding of the running sum per MFMA that adds into it:
                                                                 n_acc = 6 K / 16 = 72 for bf16x3, K / 2 = 96 for v_mfma_f32_32x32x2_f32
    The second term is the worst case of round-to-nearest accumulation and is what dominates the MEASURED limb error (printed below,
    recorded in DESIGN.md 4): the products are exact up to the dropped terms, the sums are ordinary f32 sums of 6x as many, partly much smaller, terms."""
    capi = hip.capi
    rng = np.random.default_rng(77)
    g = torch.Generator().manual_seed(5)
    K = 192
    BOUND = {"bf16x3": 2.0 ** -21 + 2.0 ** -30 + (6 * K // 16) * 2.0 ** -24, "f32": (K // 2) * 2.0 ** -24}
    report = {}
    for pattern in ("ones", "low16"):
        for signs in ("same", "mixed"):
            # planes 3x3 texels: the points below sit exactly on texel centres, so a feature IS a texel value (blend weights 1, 0, 0, 0)
            planes = [_adversarial(rng, (1, 48, 3, 3), pattern) for _ in range(4)]
            m = hip.models.TwoDimPlanesModel(use_viewdirs=True, skip_connect_every=3, proj_combination="avg",
                                             viewdir_proj_combination="concat_pos", align_corners=True)
            state = {k: torch.randn(v.shape, generator=g) * 0.1 for k, v in m.state_dict().items() if "rot_mats" not in k}
            box = np.array([[-1, -1, -1, -np.pi, -np.pi / 2], [1, 1, 1, np.pi, np.pi / 2]], np.float64)
            state.update({k: v for k, v in m.state_dict().items() if "rot_mats" in k})
            m, sid = build_model(hip, {k: N_(v) for k, v in state.items()}, planes, box, sid="adv_DS1_PlRes3_3")
            # points on the 27 texel-centre combinations; view direction +x -> (az, el) = (0, 0) = the centre texel of the view plane
            pts = np.array([[x, y, z] for x in (-1.0, 0.0, 1.0) for y in (-1.0, 0.0, 1.0) for z in (-1.0, 0.0, 1.0)], np.float32)
            P = pts.shape[0]
            rays = np.zeros((P, 11), np.float32)
            rays[:, 0:3] = pts
            rays[:, 8] = 1.0
            raysd, z = T(rays), torch.zeros((P, 1), device=DEV)
            sc, keep = m.native_scene()
            nrec = capi.lib().nvsr_decoder_record_floats(P, 1)
            Pp = nrec // 2308                      # (allocated rows: N * S rounded up to 8 + the 32 dump rows of round 6)

            def run(mode):
                raw = torch.empty((P, 1, 4), device=DEV)
                gates = torch.empty((P, 1, 32), dtype=torch.int32, device=DEV)
                rec = torch.full((nrec,), float("nan"), device=DEV)
                capi.call("nvsr_decode_rays_arith", C.byref(sc), capi.ptr(m.packed_decoder()), P, 1, capi.ptr(raysd), capi.ptr(z), capi.ptr(raw),
                          capi.ptr(gates), capi.ptr(rec), ARITH[mode], capi.stream())
                r = N_(rec)
                off_xr = 64 * Pp + 2 * 4 * 128 * Pp
                Xr = r[off_xr: off_xr + 192 * Pp].reshape(Pp, 192)[:P]
                Hr0 = r[off_xr + 192 * Pp: off_xr + 192 * Pp + 128 * Pp].reshape(Pp, 128)[:P]
                return Xr, Hr0

            X, _ = run("f32")
            assert np.isfinite(X).all() and (np.abs(X) >= 0.124).all()              # texel values, untouched by the blend
            assert np.array_equal(X.view(np.uint32) & 0x7FFFFF, np.full(X.shape, {"ones": 0x7FFFFF, "low16": 0x00FFFF}[pattern], np.uint32))
            # weights of rgb layer 0: adversarial mantissas; 'same': the sign of each weight follows its input of point 0 -> for the
            # points that share point 0's signs every product is positive; judge every row by its own sum |w||x| anyway
            sgn = np.sign(X[0])[None, :].repeat(128, 0) if signs == "same" else None
            W = _adversarial(rng, (128, 192), pattern, sign=sgn) * np.float32(1.0 / 64)      # (a power of two: mantissas unchanged)
            with torch.no_grad():
                m.rgb_dec["0"][0].weight.copy_(T(W))
                m.rgb_dec["0"][0].bias.zero_()
            res = {}
            for mode in ("f32", "bf16x3"):
                Xm, H = run(mode)
                assert np.array_equal(Xm, X)
                pre = W.astype(np.float64) @ X.astype(np.float64).T                   # [128, P]
                mag = np.abs(W.astype(np.float64)) @ np.abs(X.astype(np.float64)).T
                ref = np.maximum(pre, 0.0).T                                          # [P, 128]
                rel = (H.astype(np.float64) - ref) / mag.T
                res[mode] = float(np.abs(rel).max())
                res[mode + "_mean_signed"] = float(rel[ref > 0].mean())
                assert res[mode] <= BOUND[mode], (pattern, signs, mode, res)
            report[(pattern, signs)] = res
    for k, v in report.items():
        print("limb bound %-5s mantissas, %-5s signs: max |err| / sum|w||x|   f32 %.3e (mean signed %+.2e)   bf16x3 %.3e (mean signed %+.2e)"
              % (k + (v["f32"], v["f32_mean_signed"], v["bf16x3"], v["bf16x3_mean_signed"])))
    print("stated bounds: bf16x3 %.3e, f32 %.3e; 2^-21 = %.3e" % (BOUND["bf16x3"], BOUND["f32"], 2.0 ** -21))
    # the limb arithmetic is NOT bit-grade f32: its worst error exceeds the exact-f32 kernel's on every operand set, and with equal signs
    # the dropped products show as a one-sided (negative: truncation limbs under-estimate) mean error inside their 2^-21 bound
    for k, v in report.items():
        assert v["bf16x3"] > v["f32"], k
    for pattern in ("ones", "low16"):
        m_ = report[(pattern, "same")]["bf16x3_mean_signed"]
        assert -(2.0 ** -21 + 2.0 ** -30) <= m_ < 0.0, (pattern, m_)
    assert report[("low16", "same")]["bf16x3_mean_signed"] < 2 * report[("ones", "same")]["bf16x3_mean_signed"]      # the worst-case mantissas


# ---------------------------------------------------------------------------------------------------------------------------------
# per-call arithmetic: nothing process-global, re-entrant across streams
# ---------------------------------------------------------------------------------------------------------------------------------
def test_two_streams_two_arithmetic_modes(hip):
    """Two streams of one process run the same render pass and the same convolution concurrently, one in exact f32 and one in bf16x3
    (the arithmetic is an argument of the call): each stream's result equals, bit for bit, that mode's result computed alone -- and
    the process default (nvsr_set_decoder_arithmetic) is neither consulted nor changed."""
    from bench import make_synthetic_scene

    capi = hip.capi
    nv = torch.ops.nvsr
    mc, mf, sid, pose = make_synthetic_scene(DEV, plane_res=128, view_res=16, seed=9)
    H = W = 144                                           # 20 736 rays: the fused two-tile kernels (N >= 16 384)
    focal = 0.5 * W / np.tan(0.5 * 0.6911112)
    ro, rd = hip.nerf_helpers.get_ray_bundle(H, W, focal, pose)
    rays = hip.train_utils.pack_rays(ro, rd, 2.0, 6.0)
    N, S = rays.shape[0], 48
    z = torch.sort(torch.rand((N, S), device=DEV) * 4 + 2, -1)[0].contiguous()
    planes, consts = mf.scene_args()
    packed = mf.packed_decoder()
    x = torch.randn((1, 256, 40, 75), device=DEV)
    net = hip.models.EDSR(256, 256, 256, 1, 2, 0).to(DEV)
    geom, wts = list(net.geometry), net.packed_weights()
    default_before = capi.get_decoder_arithmetic(), capi.get_conv_arithmetic()
    alone = {}
    for mode in ("f32", "bf16x3"):
        alone[mode] = (nv.render_pass(planes, consts, packed, rays, z, None, False, True, ARITH[mode]), nv.edsr(x, wts, geom, ARITH[mode]))
    torch.cuda.synchronize()
    assert not torch.equal(alone["f32"][0][0], alone["bf16x3"][0][0]) and not torch.equal(alone["f32"][1], alone["bf16x3"][1])
    streams = {"f32": torch.cuda.Stream(), "bf16x3": torch.cuda.Stream()}
    got = {}
    for rep in range(3):                                  # interleave the enqueues: both streams have work in flight at the same time
        for mode in ("f32", "bf16x3"):
            with torch.cuda.stream(streams[mode]):
                got[mode] = (nv.render_pass(planes, consts, packed, rays, z, None, False, True, ARITH[mode]), nv.edsr(x, wts, geom, ARITH[mode]))
    torch.cuda.synchronize()
    bits = lambda t: t.contiguous().view(torch.int32)              # (disparity is NaN where a ray hits nothing: compare bit patterns)
    for mode in ("f32", "bf16x3"):
        for a, b in zip(got[mode][0], alone[mode][0]):
            assert torch.equal(bits(a), bits(b)), mode
        assert torch.equal(got[mode][1], alone[mode][1]), mode
    assert (capi.get_decoder_arithmetic(), capi.get_conv_arithmetic()) == default_before
    # the host mirror carries the mode per model: two models, two modes, same process
    mf.arithmetic, mc.arithmetic = "f32", "f32"
    opts_scfg = __import__("bench").render_options(16, 16)
    a = hip.train_utils.run_one_iter_of_nerf(H, W, focal, mc, mf, torch.stack([ro.reshape(-1, 3), rd.reshape(-1, 3)]), opts_scfg[0], sid,
                                             mode="validation", scene_config=opts_scfg[1])[3]
    mf.arithmetic, mc.arithmetic = "bf16x3", "bf16x3"
    b = hip.train_utils.run_one_iter_of_nerf(H, W, focal, mc, mf, torch.stack([ro.reshape(-1, 3), rd.reshape(-1, 3)]), opts_scfg[0], sid,
                                             mode="validation", scene_config=opts_scfg[1])[3]
    # (end to end the importance depths are regenerated by each mode: a few rays sit on the sampler's discontinuities)
    assert not torch.equal(a, b) and float(((a - b).abs().max(-1)[0] < 2e-4).float().mean()) >= 0.98


# ---------------------------------------------------------------------------------------------------------------------------------
# torch.library registration
# ---------------------------------------------------------------------------------------------------------------------------------
def test_torch_library_ops_exist_and_opcheck(hip):
    """torch.ops.nvsr.* are registered custom operators (schema, fake / meta implementation, autograd where differentiable):
    torch.library.opcheck on the forward operators, FakeTensor tracing of a render, and gradients through the registered formulas."""
    from bench import make_synthetic_scene

    nv = torch.ops.nvsr
    for name in hip.ops.FORWARD_OPS + ["decode_rays_backward", "decoder_weight_grad", "composite_backward", "edsr_train", "edsr_backward",
                                       "planes_sr_train", "planes_sr_backward", "pack_edsr", "pack_decoder_bwd"]:
        assert hasattr(nv, name), name
    mc, mf, sid, pose = make_synthetic_scene(DEV, plane_res=32, view_res=8, seed=4)
    H = W = 12
    focal = 0.5 * W / np.tan(0.5 * 0.6911112)
    ro, rd = hip.nerf_helpers.get_ray_bundle(H, W, focal, pose)
    rays = hip.train_utils.pack_rays(ro, rd, 2.0, 6.0)
    N = rays.shape[0]
    planes, consts = mf.scene_args()
    packed = mf.packed_decoder()
    z = nv.coarse_z(rays, 16, False, None)
    raw, _, _ = nv.decode_rays(planes, consts, packed, rays, z, False, False, 3)
    pts = torch.cat([rays[:, 0:3] + rays[:, 3:6] * z[:, :1], rays[:, 8:11]], -1).contiguous()
    tests = ("test_schema", "test_faketensor", "test_autograd_registration")
    chk = lambda op, args: torch.library.opcheck(op, args, test_utils=tests)
    chk(nv.plane_to_channel_last, (mf.planes_[hip.models.get_plane_name(sid, 0)].detach(),))
    chk(nv.plane_from_channel_last, (planes[0],))
    chk(nv.pack_decoder, (mf.natural_blob(),))
    chk(nv.coarse_z, (rays, 16, False, None))
    chk(nv.triplane_decode, (planes, consts, packed, pts))
    chk(nv.render_pass, (planes, consts, packed, rays, z, None, False, True, 3))
    chk(nv.ray_points, (rays, z))
    chk(nv.triplane_decode_generic, (planes, consts, mf.natural_blob(), mf.generic_geometry(), pts))     # (the shipped geometry is one of the geometries)
    chk(nv.render_rays, (planes, consts, mc.packed_decoder(), packed, rays, 16, 8, False, False, None, None, None, None, 0))
    chk(nv.decode_rays, (planes, consts, packed, rays, z, True, True, 3))
    w = nv.composite_rays(raw, z, rays, None, False, True)[3]
    chk(nv.importance_resample, (z, w, 8, None))
    chk(nv.composite_rays, (raw, z, rays, None, False, True))
    rd3 = rays[:, 3:6].contiguous()
    chk(nv.composite, (raw.clone().requires_grad_(True), z, rd3, None, True, False))
    net = hip.models.EDSR(48, 48, 32, 1, 4, 0).to(DEV)
    x = torch.randn((2, 48, 20, 23), device=DEV)
    chk(nv.edsr, (x, net.packed_weights(), list(net.geometry), 3))
    sr = hip.models.PlanesSR(hip.models.EDSR, 4, 48, 48, {"model": {"hidden_size": 32, "n_blocks": 1}}, "bilinear").to(DEV)
    lr = [torch.randn((48, 21, 19), device=DEV) for _ in range(2)]
    pad, over = int(sr.inner_model.required_padding), int(sr.HR_overpadding)
    chk(nv.planes_sr, (lr, sr.inner_model.packed_weights(), list(sr.inner_model.geometry), pad, over, None, None, None, 3))
    chk(nv.planes_sr, (lr[:1], sr.inner_model.packed_weights(), list(sr.inner_model.geometry), pad, over, [-0.5, -0.4, 0.3, 0.6], None, None, 0))
    # differentiable operators: gradients flow through the registered formulas
    rawp = raw.clone().requires_grad_(True)
    rgb, disp, acc, wts, depth = nv.composite(rawp, z, rd3, None, False, False)
    assert rgb.requires_grad and acc.requires_grad and disp.requires_grad and depth.requires_grad and not wts.requires_grad      # (round 3: disp / depth carry gradients)
    gout = torch.randn_like(rgb)
    (rgb * gout).sum().backward()
    # the registered autograd formula IS the backward operator (whose numerics the golden / oracle tests of test_hip_parity.py pin)
    assert torch.equal(rawp.grad, nv.composite_backward(raw, z, rd3, None, False, False, gout, None))
    xg = torch.randn((1, 48, 20, 23), device=DEV, requires_grad=True)
    for w_ in net.conv_weights():
        w_.requires_grad_(True)
    y = net(xg)
    assert y.requires_grad
    gy = torch.randn_like(y)
    (y * gy).sum().backward()
    ca = hip.capi.resolve_conv_arithmetic(None)          # the arithmetic net(xg) ran in (the process default)
    o_, acts = nv.edsr_train(xg.detach(), net.natural_blob(), net.packed_weights(), net.packed_dgrad_weights(), list(net.geometry), ca)
    gnat, dx = nv.edsr_backward(xg.detach(), acts, net.packed_dgrad_weights(), list(net.geometry), gy, True, ca)
    assert torch.equal(o_, y.detach()) and torch.equal(dx, xg.grad)
    assert torch.equal(gnat, torch.cat([w_.grad.reshape(-1) for w_ in net.conv_weights()]))
    # the operators trace with FakeTensors (what torch.compile / export see): shapes and dtypes without touching the GPU
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode(allow_non_fake_inputs=False) as fm:
        f = lambda t: fm.from_tensor(t)
        out = nv.render_rays([f(p) for p in planes], consts, f(mc.packed_decoder()), f(packed), f(rays), 16, 8, False, False, None, None, None, None, -1)
        assert [tuple(o.shape) for o in out] == [(N, 3), (N,), (N,), (N, 3), (N,), (N,)]
        o2 = nv.planes_sr([f(t) for t in lr], f(sr.inner_model.packed_weights()), list(sr.inner_model.geometry), pad, over, None, None, None, -1)
        assert [tuple(o.shape) for o in o2] == [(1, 48, 84, 76)] * 2


# ---------------------------------------------------------------------------------------------------------------------------------
# plane store / checkpoints written by the reference
# ---------------------------------------------------------------------------------------------------------------------------------
def test_render_from_reference_written_store(hip):
    """The files under tests/golden/g17_store/ were written by the reference's own PlanesOptimizer.save_params / safe_saving and
    checkpoint code (gen_golden.py::g17_store).  Read them with the mirror (plane_store.load_scene, find_latest_checkpoint,
    load_decoder_checkpoint, load_sr_checkpoint), render with eval_nerf and super-resolve a plane: the pixels the reference rendered
    from the same files (after reading them back itself) within the end-to-end tolerance, the SR plane within 1e-5."""
    import os
    from conftest import GOLDEN, load_golden

    g = load_golden("g17_store.npz")
    store = os.path.join(GOLDEN, "g17_store")
    sid = str(g["sid"])
    H, W, Nc, Nf, R, Rv, Cc, hidden, nblocks, sf = [int(v) for v in g["cfg"]]
    M, ps = hip.models, hip.plane_store
    kw = dict(use_viewdirs=True, skip_connect_every=3, proj_combination="avg", viewdir_proj_combination="concat_pos", align_corners=True)
    torch.manual_seed(1234)                                   # fresh random modules: everything must come from the files
    mc = M.TwoDimPlanesModel(**kw)
    mf = M.TwoDimPlanesModel(num_planes_or_rot_mats=mc.rot_mats(), **kw)
    ps.load_decoder_checkpoint(ps.find_latest_checkpoint(store, sr=False), mc, mf)
    mc, mf = mc.to(DEV).eval(), mf.to(DEV).eval()
    content = ps.load_scene([mc, mf], os.path.join(store, "planes"), sid, device=DEV)
    assert mc.planes_ is mf.planes_ and all(p.is_cuda for p in mc.planes_.values())
    from test_hip_parity import make_options, psnr
    opts, scfg = make_options(Nc, Nf)
    ro, rd = hip.nerf_helpers.get_ray_bundle(H, W, float(g["focal"]), T(g["pose"]))
    rgb_c, _, _, rgb_f, *_ = hip.train_utils.eval_nerf(H, W, float(g["focal"]), mc, mf, ro, rd, opts, scene_id=sid, scene_config=scfg)
    np.testing.assert_allclose(N_(rgb_c), g["rgb_coarse"], rtol=0, atol=2e-5)
    ef = np.abs(N_(rgb_f) - g["rgb_fine"]).max(-1)
    assert (ef <= 2e-4).mean() >= 0.98 and psnr(N_(rgb_f), g["rgb_fine"]) >= 80.0
    # a second load of the same scene replaces the parameters: the renderer must not serve stale channel-last copies
    with torch.no_grad():
        for p_ in mc.planes_.values():
            p_.data.mul_(0.0)                                 # a write through .data: no version bump ...
    mc.invalidate()                                           # ... so the caches are told; the fine model shares them
    mf.invalidate()
    z0 = hip.train_utils.eval_nerf(H, W, float(g["focal"]), mc, mf, ro, rd, opts, scene_id=sid, scene_config=scfg)[3]
    ps.load_scene([mc, mf], os.path.join(store, "planes"), sid, device=DEV)
    again = hip.train_utils.eval_nerf(H, W, float(g["focal"]), mc, mf, ro, rd, opts, scene_id=sid, scene_config=scfg)[3]
    assert torch.equal(again, rgb_f) and not torch.equal(z0, rgb_f)
    # SR checkpoint -> PlanesSR -> the plane the reference super-resolved
    sr = M.PlanesSR(M.EDSR, sf, Cc, Cc, {"model": {"hidden_size": hidden, "n_blocks": nblocks}}, "bilinear")
    ps.load_sr_checkpoint(ps.find_latest_checkpoint(store, sr=True), sr)
    sr = sr.to(DEV).eval()
    name0 = M.get_plane_name(sid, 0)
    sr.set_LR_plane(mc.planes_[name0].detach(), id=name0, save_interpolated=False)
    with torch.no_grad():
        # (the stored planes are O(10) and this SR net amplifies: outputs reach +-300 -- tolerance relative to the output range)
        np.testing.assert_allclose(N_(sr(name0)), g["sr_plane0"], rtol=0, atol=5e-6 * float(np.abs(g["sr_plane0"]).max()))
    # the mirror's writer produces a file the same reader accepts, with the reference's keys (round trip on the device tensors)
    assert sorted(content) == ["coords_normalization", "opt_states", "params"]


def test_render_rays_odd_sizes_keep_workspace_alignment(hip, oracle):
    """N * Nc not a multiple of 4 (odd ray counts with odd sample counts): the sub-buffers of the caller's workspace are rounded up to
    16 bytes each (the raw scratch used to land unaligned and the call failed with NVSR_ERR_ALIGN)."""
    from bench import make_synthetic_scene
    from oracle.oracle import decoder_blob

    mc, mf, sid, pose = make_synthetic_scene(DEV, plane_res=32, view_res=8, seed=6)
    H, W = 3, 7
    focal = 0.5 * W / np.tan(0.5 * 0.6911112)
    ro, rd = hip.nerf_helpers.get_ray_bundle(H, W, focal, pose)
    for nc, nf in ((5, 3), (7, 6), (9, 0)):
        from test_hip_parity import make_options
        opts, scfg = make_options(nc, nf)
        rgb_c, _, _, rgb_f, *_ = hip.train_utils.eval_nerf(H, W, focal, mc, mf, ro, rd, opts, scene_id=sid, scene_config=scfg)
        planes = [N_(mc.planes_[hip.models.get_plane_name(sid, d)]) for d in range(4)]
        sc = oracle.scene(planes, mc.box_coords[sid].numpy())
        sdn = lambda m: {k: N_(v) for k, v in m.state_dict().items()}
        rays = oracle.pack_rays(N_(ro), N_(rd), 2.0, 6.0)
        o = oracle.render_rays(sc, oracle.decoder(decoder_blob(sdn(mc))), oracle.decoder(decoder_blob(sdn(mf))), rays, nc, nf)
        np.testing.assert_allclose(N_(rgb_c).reshape(-1, 3), o["rgb_coarse"], rtol=0, atol=2e-5)
        if nf:
            assert (np.abs(N_(rgb_f).reshape(-1, 3) - o["rgb_fine"]).max(-1) <= 2e-4).mean() >= 0.9


# ---------------------------------------------------------------------------------------------------------------------------------
# multi-GPU partitions with the HIP renderer, rehearsed with two ranks on this box's one GPU
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("partition,res,self_launch", [("frame", 384, False), ("rows", 160, True)])
def test_sharded_render_is_bit_identical_to_one_rank(partition, res, self_launch):
    """`bench.py --gpus 2` with the rays of a frame sharded by row blocks over two ranks (both on cuda:0, gloo: NVSR_BENCH_REHEARSAL=1):
    inside the run every rank compares the frames assembled by distributed.render_image_sharded / render_views_sharded -- rendered by the
    HIP kernels on its row block, gathered with one all_gather -- with the frames it renders alone: torch.equal, coarse and fine
    (bench.py prints SHARDED_RENDER_IDENTICAL per rank and exits non-zero otherwise).  res 384: 73 728 rays per rank, the fused
    two-tile passes on both sides (the identity holds while the per-rank ray count stays on the same side of NVSR_FUSED_MIN_RAYS = 65 536:
    an 800^2 frame on up to 9 GPUs); res 160: the sample-parallel kernels.
    'rows' is launched the way a user would -- plain `python bench.py --gpus 2`, which spawns its own ranks -- 'frame' the way the
    driver does (torch.distributed.run)."""
    import json, os, socket, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, NVSR_BENCH_REHEARSAL="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    tail = [os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--res", str(res), "--plane-res", "128", "--full",
            "--no-cpu-baseline", "--no-modes", "--partition", partition]
    if self_launch:
        cmd = [sys.executable] + tail
    else:
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port",
               str(port)] + tail
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-4000:]
    for r in (0, 1):
        assert "SHARDED_RENDER_IDENTICAL rank %d partition %s" % (r, partition) in p.stderr, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    r = json.loads(lines[0])
    assert r["n_gpus"] == 2 and r["config"]["partition"] == partition and r["scaling"] == ("strong" if partition == "frame" else "weak")
    assert r["sharded_frame_identical_to_one_gpu"] is True          # (round 6: the N > 1 line says that its frames are the one-GPU frames)
    frames = 1 if partition == "frame" else 2
    assert abs(r["value"] - frames * res * res * 2 / (r["ms_per_step"] * 2e-3)) <= 1e-6 * r["value"]


# ---------------------------------------------------------------------------------------------------------------------------------
# BASELINE configs[4] at its real size: LLFF 'fern'-like forward-facing view, NDC rays, 64 + 128 samples, planes super-resolved by the
# full EDSR(256 x 32) -- rendering and one SR-refinement optimisation step
# ---------------------------------------------------------------------------------------------------------------------------------
def test_config5_llff_ndc_real_size_render_and_sr_refinement_step(hip, oracle):
    """378 x 504 view (LLFF at 1/8), scene_config.no_ndc = False (train_utils.py:215-218), LR planes 200^2 super-resolved to
    800^2 by PlanesSR(EDSR 256 x 32) on first use (models.py:270-284), 64 + 128 samples: 190 512 rays through the fused passes.
    2 048 randomly chosen rays are checked against the oracle rendering the SAME super-resolved planes (their values are pinned by
    test_full_size_edsr_windows_vs_oracle); then one `what: ['SR']` refinement step at this size (4 096 rays, ROI super-resolution of
    the three planes in training mode, gradients through the renderer into all 43 M SR weights) must run, give finite gradients for
    every conv, and a second evaluation must serve freshly super-resolved planes."""
    from oracle.oracle import decoder_blob
    from test_hip_parity import Opt, make_options
    from bench import make_synthetic_scene

    mc, mf, sid, _ = make_synthetic_scene(DEV, plane_res=200, view_res=32, seed=11)
    sr = _full_size_sr(hip, seed=31)
    with torch.no_grad():
        for p_ in sr.parameters():
            p_.mul_(0.3)                     # keep the super-resolved planes in the range of the LR ones
    sr.eval()
    for m in (mc, mf):
        m.assign_SR_model(sr, SR_viewdir=False)
        # forward-facing NDC scene: the box spans the NDC cube
        m.box_coords = {sid: torch.tensor([[-1.5, -1.5, -1.5, -np.pi, -np.pi / 2], [1.5, 1.5, 1.5, np.pi, np.pi / 2]], dtype=torch.float64)}
        m.invalidate()
    mf.assign_LR_planes()
    H, W, focal = 378, 504, 407.6
    pose = torch.tensor([[1.0, 0.0, 0.0, 0.03], [0.0, 1.0, 0.0, -0.02], [0.0, 0.0, 1.0, 0.1], [0.0, 0.0, 0.0, 1.0]], device=DEV)
    ro, rd = hip.nerf_helpers.get_ray_bundle(H, W, focal, pose)
    opts, _ = make_options(64, 128)
    scfg = Opt(near=0, far=1, no_ndc=False)
    with torch.no_grad():
        rgb_c, _, _, rgb_f, *_ = hip.train_utils.eval_nerf(H, W, focal, mc, mf, ro, rd, opts, scene_id=sid, scene_config=scfg)
    assert rgb_f.shape == (H, W, 3) and torch.isfinite(rgb_f).all()
    names = [hip.models.get_plane_name(sid, d) for d in range(4)]
    assert sorted(sr.SR_planes) == sorted(names[:3]) and all(sr.SR_planes[n].shape[-1] == 800 for n in names[:3])
    # oracle on a sample of the rays, from the same HR planes
    rng = np.random.default_rng(5)
    ids = np.sort(rng.choice(H * W, 2048, replace=False))
    planes = [N_(sr.SR_planes[n]) for n in names[:3]] + [N_(mc.planes_[names[3]])]
    osc = oracle.scene(planes, mc.box_coords[sid].numpy())
    sdn = lambda m: {k: N_(v) for k, v in m.state_dict().items() if "SR_model" not in k}
    ro_n, rd_n = hip.nerf_helpers.ndc_rays(H, W, focal, 1.0, ro.reshape(-1, 3), rd.reshape(-1, 3))
    rays = oracle.pack_rays(N_(ro_n)[ids], N_(rd_n)[ids], 0.0, 1.0, dirs_for_view=N_(rd.reshape(-1, 3))[ids])
    o = oracle.render_rays(osc, oracle.decoder(decoder_blob(sdn(mc))), oracle.decoder(decoder_blob(sdn(mf))), rays, 64, 128)
    np.testing.assert_allclose(N_(rgb_c).reshape(-1, 3)[ids], o["rgb_coarse"], rtol=0, atol=3e-5)
    err = np.abs(N_(rgb_f).reshape(-1, 3)[ids] - o["rgb_fine"]).max(-1)
    assert (err <= 2e-4).mean() >= 0.97, ((err <= 2e-4).mean(), err.max())
    # SR refinement step at this size
    for m in (mc, mf):
        for n_, p_ in m.named_parameters():           # (the SR model is a registered sub-module of both: leave its weights trainable)
            if "SR_model" not in n_:
                p_.requires_grad_(False)
    for p_ in mc.planes_.values():
        p_.requires_grad_(False)
    sr_opt = torch.optim.Adam(sr.parameters(), lr=1e-4)
    step = hip.training.TrainStep(mc, mf, opts, {"SR"}, SR_optimizer=sr_opt, SR_model=sr, sr_loss="fine")
    np.random.seed(3)
    before = [w_.detach().clone() for w_ in sr.inner_model.conv_weights()[:2]]
    r = step(0, rgb_f.detach() * 0.9, pose, H, W, focal, 1, sid, scfg, 4096, sr_iter=True)
    assert np.isfinite(r["loss"]) and r["coarse_loss"] is None
    grads = [w_.grad for w_ in sr.inner_model.conv_weights()]
    assert all(g_ is not None and torch.isfinite(g_).all() for g_ in grads) and float(grads[0].abs().max()) > 0 and float(grads[-1].abs().max()) > 0
    assert not torch.equal(before[0], sr.inner_model.conv_weights()[0]) and not torch.equal(before[1], sr.inner_model.conv_weights()[1])
    sr.eval()
    sr.clear_SR_planes()
    with torch.no_grad():
        again = hip.train_utils.eval_nerf(H, W, focal, mc, mf, ro, rd, opts, scene_id=sid, scene_config=scfg)[3]
    assert torch.isfinite(again).all() and not torch.equal(again, rgb_f)          # the refined network was used


# ---------------------------------------------------------------------------------------------------------------------------------
# decoder geometries other than the shipped one (csrc/generic.hip)
# ---------------------------------------------------------------------------------------------------------------------------------
def _variant_model(hip, g, name, state_prefix=None):
    from test_oracle import G18_VARIANTS, g18_variant
    kw, sd_, planes = g18_variant(g, name)
    if state_prefix is not None:
        sd_ = {k[len(state_prefix):]: v for k, v in g.items() if k.startswith(state_prefix)}
    m = hip.models.TwoDimPlanesModel(use_viewdirs=True, align_corners=True, **kw)
    m.load_state_dict({k: torch.as_tensor(v) for k, v in sd_.items()}, strict=True)
    m = m.to(DEV).eval()
    sid = "lego_DS8_PlRes10_6"
    m.planes_ = torch.nn.ParameterDict({hip.models.get_plane_name(sid, d): torch.nn.Parameter(T(planes[d])) for d in range(4)})
    m.box_coords = {sid: torch.as_tensor(g["box"], dtype=torch.float64)}
    m.set_cur_scene_id(sid)
    return m, sid, kw, sd_, planes


def test_generic_decoder_geometries_vs_reference_and_oracle(hip):
    """TwoDimPlanesModel for geometries the MFMA kernels are not compiled for -- dec_channels 256 / 64 / 96, 24-channel planes,
    proj_combination sum / concat, viewdir_proj_combination sum / mult / concat, skip layers, 5 + 3 layers (config/TrainModels.yml lists such
    alternatives) -- through torch.ops.nvsr.triplane_decode_generic: the reference's own outputs (g18) within 2e-5 of the output range,
    the numpy restatement on a large ragged point list that crosses the kernel's chunk boundary, a render through eval_nerf against the
    reference's pixels; geometries the reference's own layer sizes do not admit are refused loudly."""
    from conftest import load_golden
    from oracle.generic_decoder import decode
    from test_oracle import G18_VARIANTS
    from test_hip_parity import make_options, psnr
    g = load_golden("g18_decoder_variants.npz")
    for name in G18_VARIANTS:
        m, sid, kw, sd_, planes = _variant_model(hip, g, name)
        assert not m.is_native_geometry()
        with torch.no_grad():
            out = N_(m(T(g[name + ".x"])))
        ref = g[name + ".out"]
        np.testing.assert_allclose(out, ref, rtol=0, atol=2e-5 * max(1.0, float(np.abs(ref).max())), err_msg=name)
    # a point list that is not a multiple of anything and crosses the 2^20-point chunk of the layer stack
    m, sid, kw, sd_, planes = _variant_model(hip, g, "avg_mult")
    rng = np.random.default_rng(3)
    P = (1 << 20) + 77
    x = np.concatenate([rng.uniform(-4.3, 4.3, (P, 3)), rng.standard_normal((P, 3))], 1).astype(np.float32)
    with torch.no_grad():
        out = N_(m(T(x)))
    sel = np.concatenate([np.arange(0, 5000), np.arange((1 << 20) - 2500, P)])
    ref = decode(sd_, planes, g["box"], x[sel], **kw)
    np.testing.assert_allclose(out[sel], ref, rtol=0, atol=2e-5 * max(1.0, float(np.abs(ref).max())))
    with torch.no_grad():
        assert N_(m(T(x[:1]))).shape == (1, 4) and m(T(x[:0])).shape == (0, 4)
    # render (8 x 8 rays, 16 + 16 samples) with a coarse / fine pair of the 'concat24' geometry
    mc, sid, *_ = _variant_model(hip, g, "concat24", state_prefix="concat24.render.coarse.")
    mf, *_ = _variant_model(hip, g, "concat24", state_prefix="concat24.render.fine.")
    mf.planes_ = mc.planes_
    H, W, focal = int(g["concat24.render.hwf"][0]), int(g["concat24.render.hwf"][1]), float(g["concat24.render.hwf"][2])
    ro, rd = hip.nerf_helpers.get_ray_bundle(H, W, focal, T(g["pose"]))
    opts, scfg = make_options(16, 16)
    rgb_c, _, _, rgb_f, *_ = hip.train_utils.eval_nerf(H, W, focal, mc, mf, ro, rd, opts, scene_id=sid, scene_config=scfg)
    np.testing.assert_allclose(N_(rgb_c), g["concat24.render.rgb_coarse"], rtol=0, atol=3e-5)
    ef = np.abs(N_(rgb_f) - g["concat24.render.rgb_fine"]).max(-1)
    assert (ef <= 2e-4).mean() >= 0.95 and psnr(N_(rgb_f), g["concat24.render.rgb_fine"]) >= 70.0, ((ef <= 2e-4).mean(), ef.max())
    # loud refusal
    bad = hip.capi.DecoderGeometry(48, 48, 128, 4, 4, 0, 0, 3)          # 'concat' view features on summed position features (models.py:186-190)
    assert hip.capi.lib().nvsr_generic_decoder_natural_floats(C.byref(bad)) == -1


def test_generic_decoder_gradients_vs_reference(hip):
    """Training on decoder geometries other than the shipped one (csrc/generic.hip backward: forward recomputed with every layer's output
    kept, weight / data gradient kernels, scatter through combination rule and bilinear taps): the reference's own torch.autograd
    gradients of the four planes and of every decoder parameter (g19) for a fixed cotangent -- 'avg' + 'mult', 'sum' + 'sum', 'concat' +
    'concat' on 24-channel planes, skip layers, 5 + 3 layers; then a few Adam steps through run_one_iter_of_nerf (pass by pass:
    differentiable model call + differentiable compositing) must lower the loss."""
    from conftest import load_golden
    from test_oracle import G18_VARIANTS
    from test_hip_parity import make_options
    g, gg = load_golden("g18_decoder_variants.npz"), load_golden("g19_decoder_variant_grads.npz")
    names = [n for n in G18_VARIANTS if n + ".gout" in gg]
    assert len(names) == 5
    for name in names:
        m, sid, kw, sd_, planes = _variant_model(hip, g, name)
        m.train()
        params = m.decoder_parameters()
        plist = [m.planes_[hip.models.get_plane_name(sid, d)] for d in range(4)]
        for t_ in list(params) + plist:
            t_.requires_grad_(True)
        out = m(T(g[name + ".x"]))
        np.testing.assert_allclose(N_(out), g[name + ".out"], rtol=0, atol=2e-5 * max(1.0, float(np.abs(g[name + ".out"]).max())), err_msg=name)
        (out * T(gg[name + ".gout"])).sum().backward()
        gnat = np.concatenate([N_(t_.grad).reshape(-1) for t_ in params])
        ref = gg[name + ".gnat"]
        assert gnat.shape == ref.shape
        assert np.linalg.norm(gnat - ref) / np.linalg.norm(ref) < 2e-5, (name, np.linalg.norm(gnat - ref) / np.linalg.norm(ref))
        np.testing.assert_allclose(gnat, ref, rtol=0, atol=3e-5 * float(np.abs(ref).max()), err_msg=name + " decoder")
        for d in range(4):
            got, refp = N_(plist[d].grad), gg[name + ".gplane%d" % d]
            assert got.shape == refp.shape
            assert np.linalg.norm(got - refp) / np.linalg.norm(refp) < 2e-5, (name, d)
            np.testing.assert_allclose(got, refp, rtol=0, atol=3e-5 * float(np.abs(refp).max()), err_msg="%s plane %d" % (name, d))
        # only what asks for a gradient gets one
        for t_ in list(params) + plist:
            t_.grad = None
            t_.requires_grad_(False)
        plist[1].requires_grad_(True)
        (m(T(g[name + ".x"])) * T(gg[name + ".gout"])).sum().backward()
        np.testing.assert_allclose(N_(plist[1].grad), gg[name + ".gplane1"], rtol=0, atol=3e-5 * float(np.abs(gg[name + ".gplane1"]).max()))
        assert all(t_.grad is None for t_ in params) and plist[0].grad is None
    # training through run_one_iter_of_nerf: 64 rays, 16 + 16 samples, planes + both decoders of the 'skip2' geometry
    mc, sid, *_ = _variant_model(hip, g, "skip2")
    mf, *_ = _variant_model(hip, g, "skip2")
    mf.planes_ = mc.planes_
    opts, scfg = make_options(16, 16)
    for mm in (mc, mf):
        mm.train()
        for t_ in mm.decoder_parameters():
            t_.requires_grad_(True)
    for t_ in mc.planes_.values():
        t_.requires_grad_(True)
    opt = torch.optim.Adam(list(mc.decoder_parameters()) + list(mf.decoder_parameters()) + list(mc.planes_.values()), lr=2e-3)
    H = W = 8
    focal = 0.5 * W / np.tan(0.5 * 0.6911112)
    ro, rd = hip.nerf_helpers.get_ray_bundle(H, W, focal, T(g["pose"]))
    batch = torch.stack([ro.reshape(-1, 3), rd.reshape(-1, 3)], 0)
    target = torch.rand((H * W, 3), generator=torch.Generator().manual_seed(4)).to(DEV) * 0.5 + 0.25
    losses = []
    for it in range(12):
        opt.zero_grad()
        rgb_c, _, _, rgb_f, *_ = hip.train_utils.run_one_iter_of_nerf(H, W, focal, mc, mf, batch, opts, sid, mode="validation", scene_config=scfg)
        loss = ((rgb_c - target) ** 2).mean() + ((rgb_f - target) ** 2).mean()
        loss.backward()
        assert all(t_.grad is not None and torch.isfinite(t_.grad).all() for t_ in opt.param_groups[0]["params"])
        opt.step()
        losses.append(float(loss.detach()))
    assert losses[-1] < 0.8 * losses[0], losses


def test_patch_ordered_render_is_bit_identical_to_row_order(hip, monkeypatch):
    """eval_nerf renders a frame's rays in 16 x 2 pixel patches inside 128 x 32 pixel blocks (train_utils.patch_order: a wave tile of the
    fused passes is then a compact patch instead of 32 pixels of a row -- 3 % faster on the 800 x 800 frame): every ray is independent, so the image must be the same
    bits as in row order (NVSR_ROW_ORDER=1), also for sizes that leave ragged patches at the right and bottom edges; and the order itself
    is a permutation that visits the grid patch by patch"""
    from test_hip_parity import make_options
    tu = hip.train_utils
    perm, inv = tu.patch_order(12 * 19, 19, DEV)
    assert sorted(N_(perm).tolist()) == list(range(12 * 19)) and torch.equal(perm[inv], torch.arange(12 * 19, device=DEV))
    pw, ph = tu.PATCH_W, tu.PATCH_H
    assert pw * ph == 32 and (pw, ph) == (16, 2)
    assert N_(perm[:32]).tolist() == [y * 19 + x for y in range(ph) for x in range(pw)]               # the first patch: 16 x 2 pixels, row-major
    assert N_(perm[32:38]).tolist() == [y * 19 + x for y in range(ph) for x in range(16, 19)]         # the ragged second patch: 3 x 2
    assert N_(perm[38:70]).tolist() == [y * 19 + x for y in range(2, 4) for x in range(pw)]           # then the next patch row of the block
    # a grid wider and taller than a super-block: the first block (128 x 32 pixels) is visited completely before the second
    Wb, Hb = tu.PATCH_W * tu.SUPER_W, tu.PATCH_H * tu.SUPER_H
    perm2, _ = tu.patch_order((Hb + 2) * (Wb + 16), Wb + 16, DEV)
    head = N_(perm2[:Wb * Hb])
    assert sorted(head.tolist()) == sorted(y * (Wb + 16) + x for y in range(Hb) for x in range(Wb))
    bench = __import__("bench")
    mc, mf, sid, pose = bench.make_synthetic_scene(DEV, 96, 16, seed=2)
    opts, scfg = make_options(16, 16)
    for H, W in ((256, 264), (250, 267)):
        focal = 0.5 * W / np.tan(0.5 * 0.6911112)
        ro, rd = hip.nerf_helpers.get_ray_bundle(H, W, focal, pose)
        with torch.no_grad():
            a = tu.eval_nerf(H, W, focal, mc, mf, ro, rd, opts, scene_id=sid, scene_config=scfg)
            monkeypatch.setenv("NVSR_ROW_ORDER", "1")
            b = tu.eval_nerf(H, W, focal, mc, mf, ro, rd, opts, scene_id=sid, scene_config=scfg)
            monkeypatch.delenv("NVSR_ROW_ORDER")
        assert torch.equal(a[0], b[0]) and torch.equal(a[3], b[3]) and tuple(a[3].shape) == (H, W, 3)
        assert float(a[3].std()) > 0.01


def test_cumprod_exclusive_kernel(hip, oracle):
    """nerf_helpers.cumprod_exclusive (nerf_helpers.py:409-430) runs a HIP kernel too (round 1 used torch.cumprod): the reference's golden
    values (g05) and the oracle's left-to-right products, bit for bit"""
    from conftest import load_golden
    g = load_golden("g05_composite.npz")
    got = N_(hip.nerf_helpers.cumprod_exclusive(T(g["cumprod_in"])))
    np.testing.assert_allclose(got, g["cumprod_out"], rtol=1e-6, atol=1e-7)
    rng = np.random.default_rng(9)
    a = rng.uniform(0.2, 1.3, (1001, 193)).astype(np.float32)
    np.testing.assert_array_equal(N_(hip.nerf_helpers.cumprod_exclusive(T(a))), oracle.cumprod_exclusive(a))
    assert hip.nerf_helpers.cumprod_exclusive(T(a[:, :1])).eq(1.0).all() and hip.nerf_helpers.cumprod_exclusive(T(a[:0])).shape == (0, 193)


def test_inference_frame_computes_coarse_depths_in_kernel(hip):
    """An inference frame (no stratified jitter) on the fused passes never stores its coarse depths: the coarse pass
    (render_pass3_coarse_z_kernel) and the resampler (nvsr_importance_resample_rays) recompute z = near (1 - t) + far t (or the lindisp
    form, train_utils.py:95-100) from the ray in registers.  The frame must equal, bit for bit, the explicit sequence coarse_z ->
    render pass -> importance_resample -> render pass on stored depths, for both spacings; NVSR_STORE_COARSE_Z=1 selects the stored form."""
    import os
    from bench import make_synthetic_scene, render_options
    nv = torch.ops.nvsr
    mc, mf, sid, pose = make_synthetic_scene(DEV, plane_res=96, view_res=16, seed=13)
    H = W = 272                                       # 73 984 rays >= NVSR_FUSED_MIN_RAYS
    focal = 0.5 * W / np.tan(0.5 * 0.6911112)
    ro, rd = hip.nerf_helpers.get_ray_bundle(H, W, focal, pose)
    rays = hip.train_utils.pack_rays(ro, rd, 2.0, 6.0)
    planes, consts = mc.scene_args()
    bits = lambda t: t.contiguous().view(torch.int32)
    arith = hip.capi.ARITHMETIC[hip.capi.get_decoder_arithmetic()]          # the explicit passes below in the arithmetic eval_nerf runs in
    for lindisp in (False, True):
        opts, scfg = render_options(64, 128)
        opts.nerf.validation.lindisp = lindisp
        got = hip.train_utils.eval_nerf(H, W, focal, mc, mf, ro, rd, opts, scene_id=sid, scene_config=scfg)
        z_c = nv.coarse_z(rays, 64, lindisp, None)
        rgb_c, disp_c, acc_c, w_c = nv.render_pass(planes, consts, mc.packed_decoder(), rays, z_c, None, False, True, arith)
        z_f = nv.importance_resample(z_c, w_c, 128, None)
        rgb_f, *_ = nv.render_pass(planes, consts, mf.packed_decoder(), rays, z_f, None, False, False, arith)
        assert torch.equal(bits(got[0].reshape(-1, 3)), bits(rgb_c)) and torch.equal(bits(got[3].reshape(-1, 3)), bits(rgb_f)), lindisp
        # the resampler alone: depths recomputed from the rays == depths read
        z_f2 = torch.empty_like(z_f)
        hip.capi.call("nvsr_importance_resample_rays", rays.shape[0], 64, 128, hip.capi.ptr(rays), int(lindisp), hip.capi.ptr(w_c), None,
                      hip.capi.ptr(z_f2), hip.capi.stream())
        assert torch.equal(z_f, z_f2)
    os.environ["NVSR_STORE_COARSE_Z"] = "1"
    try:
        stored = hip.train_utils.eval_nerf(H, W, focal, mc, mf, ro, rd, opts, scene_id=sid, scene_config=scfg)
    finally:
        del os.environ["NVSR_STORE_COARSE_Z"]
    assert torch.equal(bits(stored[3]), bits(got[3]))


# ---------------------------------------------------------------------------------------------------------------------------------
# property tests ("property tests with hypothesis for sample_pdf monotonicity / range and compositing weight sum <= 1")
# ---------------------------------------------------------------------------------------------------------------------------------
def test_properties_of_sampling_and_compositing(hip):
    from hypothesis import given, settings, strategies as st

    @settings(max_examples=30, deadline=None)
    @given(st.integers(1, 300), st.integers(3, 96), st.integers(1, 160), st.integers(0, 2 ** 31 - 1), st.booleans())
    def sample_pdf_props(N, nb, ns, seed, det):
        """sample_pdf_2 (nerf_helpers.py:668-702): every sample lies inside [bins[0], bins[-1]]; with sorted u (det) the samples are
        non-decreasing; a row of zero weights still gives finite samples"""
        g = torch.Generator().manual_seed(seed)
        bins = torch.sort(torch.rand(N, nb, generator=g) * 4 + 2, -1)[0].to(DEV)
        w = torch.rand(N, nb - 1, generator=g).pow(4).to(DEV)
        w[0] = 0.0
        u = None if det else torch.rand(N, ns, generator=g).to(DEV)
        out = hip.nerf_helpers.sample_pdf_2(bins, w, ns, det=det, u=u)
        assert out.shape == (N, ns) and torch.isfinite(out).all()
        assert (out >= bins[:, :1] - 1e-6).all() and (out <= bins[:, -1:] + 1e-6).all()
        if det:
            assert (out[:, 1:] >= out[:, :-1] - 1e-6).all()

    @settings(max_examples=30, deadline=None)
    @given(st.integers(1, 200), st.integers(1, 300), st.integers(0, 2 ** 31 - 1), st.booleans())
    def composite_props(N, S, seed, white):
        """volume_render_radiance_field (volume_rendering_utils.py:6-51): weights >= 0, acc = sum(weights) <= 1 (+ rounding), rgb inside
        [0, 1] without a background and <= 1 + rounding with one"""
        g = torch.Generator().manual_seed(seed)
        raw = (torch.randn(N, S, 4, generator=g) * 3).to(DEV)
        z = torch.sort(torch.rand(N, S, generator=g) * 4 + 2, -1)[0].to(DEV)
        rd = torch.randn(N, 3, generator=g).to(DEV)
        rgb, disp, acc, w, depth = hip.volume_rendering_utils.volume_render_radiance_field(raw, z, rd, white_background=white)
        assert (w >= 0).all() and torch.allclose(acc, w.sum(-1), atol=1e-5)
        assert (acc <= 1 + 1e-4).all() and (rgb >= -1e-6).all() and (rgb <= 1 + 1e-4).all()
        assert (depth >= -1e-6).all() and (depth <= 6 * (1 + 1e-4)).all()

    sample_pdf_props()
    composite_props()
