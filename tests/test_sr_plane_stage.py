"""PlanesSR's plane stage on the device against float64 (-m gpu): sr_prepare_kernel, sr_finish_kernel (csrc/sr.hip), sr_finish_backward_kernel,
sr_residual_backward_gather_kernel<2|4|8>, sr_prepare_backward_kernel (csrc/sr_bwd.hip) and their tap / region helpers (csrc/sr_core.h), through the
C ABI in the exact-f32 convolution arithmetic, per element, at every border of the region table and every scale factor -- against
tests/sr_plane_ref.py (float64 autograd) within its a-priori bounds.  tests/test_sr_plane_stage_host.py checks on the CPU that the reference
reproduces the committed goldens, that the case tables cover what they promise and that every one-line mutant of the reference exceeds the
bounds.  Every test prints the worst |error| / bound per tensor and asserts each <= 1.

Which checks are tight.  The a-priori bounds are tight for the residual (one short sum: section A, measured ratios up to 0.65) and exact for the
NaN mask and the guards.  For the network path they grow with the depth of the chain and exceed the values themselves from x4 upward and in
the ReLU case (an all-zero gradient would pass): there they are only the necessary condition, and the check that can fail is the tight
random-walk yardstick of tests/sr_plane_ref.py (`*_tight`: about 1e-5 .. 1e-4 of the values), which sections B and C assert for every
network-path tensor.  The host test shows the network-path mutants exceeding it at x8 and in the ReLU case."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

import sr_plane_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32 = 0                       # NVSR_ARITH_F32
GUARD = 64                    # sentinel floats on both sides of a guarded buffer (256 bytes: the payload stays 16-byte aligned)
SENTINEL = 12345.678


def _guarded(n, fill):
    whole = torch.full((n + 2 * GUARD,), SENTINEL, device=DEV)
    view = whole[GUARD: GUARD + n]
    view.fill_(fill)
    return whole, view


def _guards_intact(whole):
    s = torch.tensor(SENTINEL, device=DEV)
    return bool((whole[:GUARD] == s).all() and (whole[-GUARD:] == s).all())


def _dev(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a, np.float32), device=DEV)


def _roi_c(roi):
    return None if roi is None else (C.c_float * len(roi))(*[float(v) for v in roi])


@contextlib.contextmanager
def _residual_settings(lib, align, mode):
    """nvsr_set_sr_align_corners / nvsr_set_sr_plane_interp around a call of a one-plane entry point; both restored"""
    a0, m0 = lib.nvsr_get_sr_align_corners(), lib.nvsr_get_sr_plane_interp()
    try:
        assert lib.nvsr_set_sr_align_corners(int(align)) == 0 and lib.nvsr_set_sr_plane_interp(1 if mode == "bicubic" else 0) == 0
        yield
    finally:
        lib.nvsr_set_sr_align_corners(a0)
        lib.nvsr_set_sr_plane_interp(m0)


class Stage:
    """one network's packed blobs on the device, and the C ABI's PlanesSR calls in NVSR_ARITH_F32"""

    def __init__(self, hip, ws, hid, nblocks, n_up):
        self.capi, self.lib = hip.capi, hip.capi.lib()
        self.net = (hid, nblocks, n_up)
        self.geom = (ref.C, ref.C, hid, nblocks, n_up)
        capi, lib = self.capi, self.lib
        nat = _dev(ref.join_blob(ws))
        assert nat.numel() == lib.nvsr_edsr_natural_floats(*self.geom)
        self.n_nat = nat.numel()
        self.packed = torch.zeros(lib.nvsr_edsr_packed_floats(*self.geom), device=DEV)
        self.packed_dgrad = torch.zeros(lib.nvsr_edsr_packed_dgrad_floats(*self.geom), device=DEV)
        capi.call("nvsr_pack_edsr_arith", capi.ptr(nat), *self.geom, capi.ptr(self.packed), F32, capi.stream())
        capi.call("nvsr_pack_edsr_dgrad_arith", capi.ptr(nat), *self.geom, capi.ptr(self.packed_dgrad), F32, capi.stream())
        torch.cuda.synchronize()

    def forward(self, lr, pad, over, roi, mean, std, mode, align, train):
        """-> (out [C, sf R0, sf R1] as an array, keep or None); the output buffer is guarded"""
        capi, lib = self.capi, self.lib
        Cc, R0, R1 = lr.shape
        hid, nb, n_up = self.net
        sf = 1 << n_up
        roi_c = _roi_c(roi)
        nws = lib.nvsr_planes_sr_workspace_floats(Cc, R0, R1, hid, nb, n_up, pad, roi_c)
        assert nws > 0
        ws = torch.zeros(nws, device=DEV)
        whole, out = _guarded(Cc * R0 * sf * R1 * sf, 0.0)
        with _residual_settings(lib, align, mode):
            if train:
                keep = torch.zeros(lib.nvsr_planes_sr_keep_floats(Cc, R0, R1, hid, nb, n_up, pad, roi_c), device=DEV)
                capi.call("nvsr_planes_sr_train_arith", capi.ptr(lr), Cc, R0, R1, capi.ptr(self.packed), hid, nb, n_up, pad, over, roi_c, capi.ptr(mean),
                          capi.ptr(std), capi.ptr(out), capi.ptr(ws), capi.ptr(keep), F32, capi.stream())
            else:
                keep = None
                capi.call("nvsr_planes_sr_arith", capi.ptr(lr), Cc, R0, R1, capi.ptr(self.packed), hid, nb, n_up, pad, over, roi_c, capi.ptr(mean),
                          capi.ptr(std), capi.ptr(out), capi.ptr(ws), F32, capi.stream())
            torch.cuda.synchronize()
        assert _guards_intact(whole)
        return out.reshape(Cc, R0 * sf, R1 * sf).cpu().numpy(), keep

    def backward(self, shape, keep, pad, over, roi, std, d_out, mode, align, d_lr=None, d_lr_fill=None):
        """-> (the weight-gradient blob added to zeros, d_lr).  d_lr: a guarded (whole, view) pair to accumulate into; d_lr_fill: a fresh one filled
        with it; neither: the call gets d_lr = NULL"""
        capi, lib = self.capi, self.lib
        Cc, R0, R1 = shape
        hid, nb, n_up = self.net
        roi_c = _roi_c(roi)
        ws = torch.zeros(lib.nvsr_planes_sr_backward_workspace_floats(Cc, R0, R1, hid, nb, n_up, pad, roi_c), device=DEV)
        gw_whole, gw = _guarded(self.n_nat, 0.0)
        if d_lr is None and d_lr_fill is not None:
            d_lr = _guarded(Cc * R0 * R1, d_lr_fill)
        with _residual_settings(lib, align, mode):
            capi.call("nvsr_planes_sr_backward_arith", Cc, R0, R1, capi.ptr(keep), capi.ptr(self.packed_dgrad), hid, nb, n_up, pad, over, roi_c, capi.ptr(std),
                      capi.ptr(d_out), capi.ptr(gw), None if d_lr is None else capi.ptr(d_lr[1]), capi.ptr(ws), F32, capi.stream())
            torch.cuda.synchronize()
        assert _guards_intact(gw_whole) and (d_lr is None or _guards_intact(d_lr[0]))
        return gw.cpu().numpy(), d_lr


_REFS = {}


def _reference(key, lr, ws, nblocks, n_up, pad, over, roi, mean, std, mode, align, d_out):
    """the float64 reference of a case, computed once per distinct region (the reference depends on the roi through its bounds alone)"""
    lo, hi = ref.roi_bounds(lr.shape[1], lr.shape[2], roi)
    key = key + (tuple(lo), tuple(hi))
    if key not in _REFS:
        _REFS[key] = ref.reference(lr, ws, nblocks, n_up, pad, over, roi, mean, std, mode, align, d_out=d_out)
    return _REFS[key]


class Worst:
    """worst |error| / bound per tensor, and where it was"""

    def __init__(self):
        self.r = {}

    def add(self, name, got, want, bound, where):
        ratio, at = ref.worst_ratio(got, want, bound)
        if ratio > self.r.get(name, (-1.0,))[0]:
            self.r[name] = (ratio, where, at)

    def out(self, name, got, r, where):
        """an output plane: the NaN mask is the reference's exactly, the values inside within the bound"""
        assert np.array_equal(np.isnan(got), np.isnan(r["out"])), (name, where, "NaN mask", r["lo"], r["hi"])
        self.add(name, np.nan_to_num(got), np.nan_to_num(r["out"]), r["out_bound"], where)

    def out_tight(self, name, got, r, where):
        self.add(name, np.nan_to_num(got), np.nan_to_num(r["out"]), r["out_tight"], where)

    def check(self, label):
        print("%s: worst |error| / bound  %s" % (label, "  ".join("%s %.3g" % (k, v[0]) for k, v in sorted(self.r.items()))))
        bad = {k: v for k, v in self.r.items() if not v[0] <= 1.0}
        assert not bad, bad


# ---- A. the residual alone: a zero-weight network ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_up", ref.RESIDUAL["n_ups"])
@pytest.mark.parametrize("align", ref.RESIDUAL["aligns"])
@pytest.mark.parametrize("mode", ref.RESIDUAL["modes"])
def test_residual_alone(hip, mode, align, n_up):
    """out = the up-sampled plane inside the region (NaN mask = roi_bounds exactly), d_lr = the residual's transpose: the gather at x2 / x4 / x8, the
    scatter of sr_finish_backward_kernel at x1 / x16 and for bicubic.  Three backward passes per (plane, region): into a d_lr pre-filled with 1.0;
    again into the same buffer (it must add the same amount); with d_out outside the region overwritten by 1e30 (the region is all it may read).
    With zero weights the clamped gather and its transpose contribute nothing here: this section pins the finish kernels, the gather and the taps;
    sr_prepare_kernel / sr_prepare_backward_kernel are pinned by sections B and C.

    Worst |error| / bound measured on the MI355X, at x1, x2, x4, x8, x16:
        bilinear, align_corners 1    out 0, 0.386, 0.609, 0.653, 0.397       d_lr 0.077, 0.369, 0.337, 0.192, 0.012
        bilinear, align_corners 0    out 0, 0.139, 0.153, 0.250, 0.187       d_lr 0.072, 0.371, 0.058, 0.015, 0.0078
        bicubic,  align_corners 1    out 0, 0.025, 0.035, 0.043, 0.023       d_lr 0.0024, 0.259, 0.076, 0.191, 0.0044
        bicubic,  align_corners 0    out 0, 0.0028, 0.0030, 0.0029, 0.0024   d_lr 0.0024, 0.219, 0.081 .. 0.125, 0.021, 0.0017
    (x1 is the identity: exact.)  The inference forward gives the training forward's figures; the second pass and the pass with 1e30 outside
    the region give d_lr's to the second digit (largest: 0.370 and 0.371); where the residual is scattered by atomics their order, and with it
    the last digits, varies from run to run (x16, bicubic).  The weight gradient of the zero-weight network is exactly zero."""
    c = ref.RESIDUAL
    planes = ref.SMALLEST_PLANES if n_up == 4 else ref.PLANES
    ws, lrs, d_outs = ref.make_case(100 + n_up, c["hid"], c["nblocks"], n_up, planes, zero_weights=True)
    pad, over = ref.pad_over(c["nblocks"], n_up)
    stage = Stage(hip, ws, c["hid"], c["nblocks"], n_up)
    sf = 1 << n_up
    w = Worst()
    for (R0, R1), lr, d_out in zip(planes, lrs, d_outs):
        lr_d, d_out_d = _dev(lr), _dev(d_out)
        for name, roi in ref.REGIONS.items():
            where = ((R0, R1), name)
            r = _reference(("A", mode, align, n_up, R0, R1), lr, ws, c["nblocks"], n_up, pad, over, roi, None, None, mode, align, d_out)
            out, keep = stage.forward(lr_d, pad, over, roi, None, None, mode, align, train=True)
            w.out("out", out, r, where)
            w.out("out_inference", stage.forward(lr_d, pad, over, roi, None, None, mode, align, train=False)[0], r, where)
            args = ((ref.C, R0, R1), keep, pad, over, roi, None)
            gw, d_lr = stage.backward(*args, d_out_d, mode, align, d_lr_fill=1.0)
            first = d_lr[1].cpu().numpy().astype(np.float64).reshape(lr.shape)
            w.add("d_lr", first - 1.0, r["d_lr"], ref.d_lr_bound(r, 1.0), where)
            w.add("gw", gw, r["gw"], ref.gw_bound([r]), where)
            stage.backward(*args, d_out_d, mode, align, d_lr=d_lr)
            second = d_lr[1].cpu().numpy().astype(np.float64).reshape(lr.shape)
            w.add("d_lr_second_pass", second - first, r["d_lr"], ref.d_lr_bound(r, first), where)
            lo, hi = r["lo"], r["hi"]
            poisoned = torch.full_like(d_out_d, 1e30)
            box = (slice(None), slice(lo[0] * sf, hi[0] * sf), slice(lo[1] * sf, hi[1] * sf))
            poisoned[box] = d_out_d[box]
            _, d_lr3 = stage.backward(*args, poisoned, mode, align, d_lr_fill=1.0)
            w.add("d_lr_poisoned_outside", d_lr3[1].cpu().numpy().astype(np.float64).reshape(lr.shape) - 1.0, r["d_lr"], ref.d_lr_bound(r, 1.0), where)
    w.check("residual alone %s align %d x%d" % (mode, align, sf))


# ---- B. a linear network ---------------------------------------------------------------------------------------------------------------------
def _linear(hip, n_up, mode, align, normalised, extra_pad=0):
    c = ref.LINEAR
    ws, lrs, d_outs = ref.make_case(200 + 10 * n_up + align, c["hid"], c["nblocks"], n_up, c["planes"])
    sf = 1 << n_up
    pad, over = ref.pad_over(c["nblocks"], n_up)
    pad, over = pad + extra_pad, over + extra_pad * sf
    mean, std = (np.array(c["mean"]), np.array(c["std"])) if normalised else (None, None)
    mean_d, std_d = _dev(mean), _dev(std)
    stage = Stage(hip, ws, c["hid"], c["nblocks"], n_up)
    w = Worst()
    for (R0, R1), lr, d_out in zip(c["planes"], lrs, d_outs):
        lr_d, d_out_d = _dev(lr), _dev(d_out)
        for name, roi in ref.REGIONS.items():
            where = ((R0, R1), name)
            r = _reference(("B", mode, align, n_up, normalised, extra_pad, R0, R1), lr, ws, c["nblocks"], n_up, pad, over, roi, mean, std, mode, align, d_out)
            out, keep = stage.forward(lr_d, pad, over, roi, mean_d, std_d, mode, align, train=True)
            w.out("out", out, r, where)
            w.out_tight("out_tight", out, r, where)
            out_inf = stage.forward(lr_d, pad, over, roi, mean_d, std_d, mode, align, train=False)[0]
            w.out("out_inference", out_inf, r, where)
            w.out_tight("out_inference_tight", out_inf, r, where)
            args = ((ref.C, R0, R1), keep, pad, over, roi, std_d)
            gw, d_lr = stage.backward(*args, d_out_d, mode, align, d_lr_fill=1.0)
            added = d_lr[1].cpu().numpy().astype(np.float64).reshape(lr.shape) - 1.0
            w.add("d_lr", added, r["d_lr"], ref.d_lr_bound(r, 1.0), where)
            w.add("d_lr_tight", added, r["d_lr"], ref.d_lr_tight(r, 1.0), where)
            w.add("gw", gw, r["gw"], ref.gw_bound([r]), where)
            w.add("gw_tight", gw, r["gw"], ref.gw_tight([r]), where)
            # d_lr = NULL (the LR plane detached): the same blob, and nothing else written (Stage.backward asserts the guards)
            gw0, none = stage.backward(*args, d_out_d, mode, align)
            assert none is None
            w.add("gw_without_d_lr", gw0, r["gw"], ref.gw_bound([r]), where)
            w.add("gw_without_d_lr_tight", gw0, r["gw"], ref.gw_tight([r]), where)
    return w


@pytest.mark.parametrize("normalised", [False, True])
@pytest.mark.parametrize("n_up,mode,align", ref.LINEAR["cases"])
def test_linear_network(hip, n_up, mode, align, normalised):
    """hid 8, 0 blocks, random weights: the clamped gather (replicate padding, planes narrower than the padding, R0 != R1) with and without
    (x - mean) / std, the crop of the over-padding and the zero ring of d_diff, the transposed gather with its division by std -- out, d_lr
    (pre-filled with 1.0) and the whole weight-gradient blob per element, and the blob again with d_lr = NULL.

    Every tensor is held to two yardsticks: the a-priori bound (necessary; slack here -- it exceeds the gradients themselves from x4 upward) and
    the tight random-walk yardstick of tests/sr_plane_ref.py (about 1e-5 .. 1e-4 of the values: the check that can fail for a wrong kernel).
    Worst |error| / yardstick measured on the MI355X, largest over the cases of a scale factor, plain / normalised:
        tight       x2    out 0.12 / 0.14       d_lr 0.19 / 0.29         blob 0.086 / 0.13
                    x4    out 0.20 / 0.20       d_lr 0.11 / 0.31         blob 0.080 / 0.077
                    x8    out 0.22 / 0.17       d_lr 0.12 / 0.12         blob 0.095 / 0.070
        a-priori    x2    out 1.1e-4 / 6.9e-5   d_lr 6.1e-3 / 8.9e-3     blob 6.0e-5 / 7.1e-5
                    x4    out 2.6e-5 / 9.0e-6   d_lr 1.2e-4 / 5.7e-4     blob 3.3e-6 / 2.7e-6
                    x8    out 2.4e-6 / 1.0e-6   d_lr 3.6e-6 / 2.2e-6     blob 1.9e-7 / 1.1e-7
    The blob with d_lr = NULL has the same figures."""
    _linear(hip, n_up, mode, align, normalised).check("linear network %s align %d x%d%s" % (mode, align, 1 << n_up, " normalised" if normalised else ""))


def test_linear_network_with_a_wider_over_padding(hip):
    """pad + 1 and over + sf at x4 (over = 5), which the entry points' consistency check accepts: the crop diff[over:-over] and the zero ring of
    d_diff beyond one texel.

    Worst |error| / yardstick measured on the MI355X: tight out 0.20, d_lr 0.11, blob 0.071; a-priori (slack) out 1.8e-5, d_lr 1.2e-4, blob 2.6e-6."""
    c = ref.LINEAR_WIDE
    pad, over = ref.pad_over(0, c["n_up"])
    assert (pad + c["extra_pad"], over + c["extra_pad"] * (1 << c["n_up"])) == (5, 5)
    _linear(hip, c["n_up"], "bilinear", 1, False, c["extra_pad"]).check("linear network, over-padding 5")


# ---- C. ReLU and the residual epilogue, a ragged batch ------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", ref.RELU["seeds"])
def test_relu_block_in_a_ragged_batch(hip, seed):
    """hid 8, 1 block, x4, three 9 x 13 planes with three different regions through ONE nvsr_planes_sr_train_batch_arith /
    nvsr_planes_sr_backward_batch_arith pair: the three outputs, the three d_lr and the summed weight gradient per element.  The host test
    certifies that no pre-activation of these seeds is within 2 x its bound of zero, so no ReLU gate can differ from float64's and both
    yardsticks apply to every element.  The a-priori bound of this seven-layer chain exceeds its gradients (necessary only); the tight
    random-walk yardstick is the check that can fail.

    Worst |error| / yardstick measured on the MI355X, seeds 19 / 25: tight out 0.15 / 0.14, d_lr 0.13 / 0.14, blob 0.046 / 0.060;
    a-priori (slack) out 2.4e-6 / 2.9e-6, d_lr 1.7e-6 / 1.7e-6, blob 4.1e-8 / 3.1e-8."""
    capi = hip.capi
    lib = capi.lib()
    c = ref.RELU
    hid, nb, n_up, pad, over = c["hid"], c["nblocks"], c["n_up"], c["pad"], c["over"]
    R0, R1 = c["plane"]
    B, sf = 3, 1 << n_up
    ws, lrs, d_outs = ref.make_case(seed, hid, nb, n_up, [c["plane"]] * B)
    rois = [ref.REGIONS[n] for n in c["regions"]]
    refs = [_reference(("C", seed, b), lr, ws, nb, n_up, pad, over, roi, None, None, "bilinear", 1, d) for b, (lr, roi, d) in enumerate(zip(lrs, rois, d_outs))]
    assert min(ref.relu_margins(r)[0] for r in refs) >= 2.0
    stage = Stage(hip, ws, hid, nb, n_up)
    rois_c = _roi_c([v for roi in rois for v in roi])
    size = (B, ref.C, R0, R1, hid, nb, n_up, pad, rois_c)
    keep = torch.zeros(lib.nvsr_planes_sr_batch_keep_floats(*size), device=DEV)
    fws = torch.zeros(lib.nvsr_planes_sr_batch_workspace_floats(*size), device=DEV)
    bws = torch.zeros(lib.nvsr_planes_sr_batch_backward_workspace_floats(*size), device=DEV)
    lr_d, d_out_d = [_dev(a) for a in lrs], [_dev(a) for a in d_outs]
    outs = [_guarded(ref.C * R0 * sf * R1 * sf, 0.0) for _ in range(B)]
    d_lrs = [_guarded(ref.C * R0 * R1, 0.0) for _ in range(B)]
    gw_whole, gw = _guarded(stage.n_nat, 0.0)
    ptrs = lambda ts: (C.c_void_p * B)(*[t.data_ptr() for t in ts])
    capi.call("nvsr_planes_sr_train_batch_arith", ptrs(lr_d), B, ref.C, R0, R1, capi.ptr(stage.packed), hid, nb, n_up, pad, over, rois_c, None, None,
              ptrs([o[1] for o in outs]), capi.ptr(fws), capi.ptr(keep), F32, 1, 0, capi.stream())
    capi.call("nvsr_planes_sr_backward_batch_arith", B, ref.C, R0, R1, capi.ptr(keep), capi.ptr(stage.packed_dgrad), hid, nb, n_up, pad, over, rois_c, None,
              ptrs(d_out_d), capi.ptr(gw), ptrs([d[1] for d in d_lrs]), capi.ptr(bws), F32, 1, 0, capi.stream())
    torch.cuda.synchronize()
    assert _guards_intact(gw_whole) and all(_guards_intact(t[0]) for t in outs + d_lrs)
    w = Worst()
    for b, r in enumerate(refs):
        where = (b, c["regions"][b])
        out, d_lr = outs[b][1].cpu().numpy().reshape(r["out"].shape), d_lrs[b][1].cpu().numpy().reshape(lrs[b].shape)
        w.out("out", out, r, where)
        w.out_tight("out_tight", out, r, where)
        w.add("d_lr", d_lr, r["d_lr"], ref.d_lr_bound(r, 0.0), where)
        w.add("d_lr_tight", d_lr, r["d_lr"], ref.d_lr_tight(r, 0.0), where)
    w.add("gw", gw.cpu().numpy(), sum(r["gw"] for r in refs), ref.gw_bound(refs), "sum of the planes")
    w.add("gw_tight", gw.cpu().numpy(), sum(r["gw"] for r in refs), ref.gw_tight(refs), "sum of the planes")
    w.check("ReLU block, ragged batch, seed %d" % seed)

