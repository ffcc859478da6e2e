"""Float64 restatement of the SR convolutions' one-limb arithmetic NVSR_ARITH_F16 (include/nvsr.h), for tests/test_conv_f16*.py.

The arithmetic: w^ = RN_f16(w 2^8) and x^ = RN_f16(x s) are exact inputs of the matrix instruction, their products are exact in f32, the sum is
an f32 accumulation in some order, and the scales are undone afterwards.  Here the operands are quantised with np.float16 (round to nearest
even, subnormals kept, overflow to inf: what v_cvt_pk_f16_f32 does), the sums are formed in float64 and the scales applied:

    value = (sum w^ x^) / (2^8 s)          absum = (sum |w^||x^|) / (2^8 s)

A float64 sum of n <= 2^16 products of 22 significant bits is exact when their exponents span less than ~15 binades and otherwise off by at
most n 2^-53 absum -- a 2^-29 of the error model's own n 2^-24 absum, which its factor 1.01 covers 300 000 times over.

s = 2^4 for activations; for a data-gradient input and for the dy operand of a weight gradient the power of two that puts the largest |dy| of
the whole tensor (all planes of a launch) into [2^12, 2^13) (csrc/sr_core.h: f16_gradient_scale).

Also here: builders of operands that ARE f16 numbers after their scale (on which the two-limb arithmetic 'f16x2' has zero low limbs), and the
chain of a small EDSR inside PlanesSR, forward and backward, layer by layer, in this arithmetic or in plain float64."""
import numpy as np

SW, SX = 8, 4                      # csrc/limb_core.h: F16_SW, F16_SX
W_SCALE, X_SCALE = 2.0 ** SW, 2.0 ** SX
U24 = 2.0 ** -24                   # unit roundoff of an f32 addition


def q16(a, scale=1.0):
    """RN_f16(a * scale) as float64.  a is f32 data, scale a power of two: the product is exact in f32 (as on the device), the conversion
    rounds once."""
    with np.errstate(over="ignore"):
        return (np.asarray(a, np.float32) * np.float32(scale)).astype(np.float16).astype(np.float64)


def gradient_scale(absmax):
    """csrc/sr_core.h f16_gradient_scale on the f32 value max |dy|: 2^(12 - floor(log2 absmax)); 1 for zero, subnormal or non-finite maxima;
    the exponent field clamped to 254"""
    bits = int(np.asarray(absmax, np.float32).view(np.uint32))
    e = (bits >> 23) & 0xFF
    if e == 0 or e == 255:
        return 1.0
    return float(np.array(min(254 + 12 - e, 254) << 23, np.uint32).view(np.float32))


def tensor_scale(*tensors):
    """the scale of a gradient tensor that spans these planes (one magnitude word for all planes of a launch)"""
    return gradient_scale(max(float(np.abs(np.asarray(t, np.float32)).max()) for t in tensors))


# ---- operands that are f16 numbers after their scale ------------------------------------------------------------------------------------
def is_representable(a, scale):
    """every a * scale is a finite f16 number"""
    v = np.asarray(a, np.float32).astype(np.float64) * scale
    return bool(np.isfinite(q16(a, scale)).all() and np.array_equal(q16(a, scale), v))


def representable_weights(rng, shape):
    """integers of at most 11 bits times 2^-16: |w| < 2^-5, w 2^8 = m 2^-8 < 8 (f16 spacing 2^-8 below 8)"""
    w = (rng.integers(-2047, 2048, shape).astype(np.float64) * 2.0 ** -16).astype(np.float32)
    assert is_representable(w, W_SCALE)
    return w


def representable_activations(rng, shape):
    """integers of at most 11 bits times 2^-10: |x| < 2, x 2^4 = m 2^-6 < 32 (f16 spacing 2^-6 below 32)"""
    x = (rng.integers(-2047, 2048, shape).astype(np.float64) * 2.0 ** -10).astype(np.float32)
    assert is_representable(x, X_SCALE)
    return x


def representable_gradient(rng, shape, exponent=-9):
    """integers of at most 11 bits times 2^exponent, one of them +-2047: the tensor's maximum 2047 2^exponent goes to 2047 * 4 in [2^12, 2^13),
    every element to m * 4 (f16 spacing 4 below 2^13)"""
    m = rng.integers(-2047, 2048, shape).astype(np.float64)
    m.reshape(-1)[int(rng.integers(m.size))] = 2047.0 * (1 if rng.integers(2) else -1)
    g = (m * 2.0 ** exponent).astype(np.float32)
    s = tensor_scale(g)
    assert 2.0 ** 12 <= float(np.abs(g).max()) * s < 2.0 ** 13 and is_representable(g, s)
    return g


# ---- the three operations ---------------------------------------------------------------------------------------------------------------
def _corr(x, w):
    """valid 3x3 correlation in float64: x [Ci,H,W], w [Co,Ci,3,3] -> [Co,H-2,W-2]"""
    Ci, H, W = x.shape
    wt = np.ascontiguousarray(np.asarray(w, np.float64).transpose(2, 3, 0, 1))          # (contiguous [Co,Ci] taps: the products go to BLAS)
    out = np.zeros((w.shape[0], (H - 2) * (W - 2)))
    for ky in range(3):
        for kx in range(3):
            out += wt[ky, kx] @ np.ascontiguousarray(x[:, ky: ky + H - 2, kx: kx + W - 2]).reshape(Ci, -1)
    return out.reshape(w.shape[0], H - 2, W - 2)


def _wcorr(dy, x):
    """dW[co,ci,ky,kx] = sum_pixels dy[co,y,x] x[ci,y+ky,x+kx] in float64"""
    Co, Ho, Wo = dy.shape
    dw = np.empty((Co, x.shape[0], 3, 3))
    d2 = dy.reshape(Co, -1)
    for ky in range(3):
        for kx in range(3):
            dw[:, :, ky, kx] = d2 @ np.ascontiguousarray(x[:, ky: ky + Ho, kx: kx + Wo]).reshape(x.shape[0], -1).T
    return dw


def _flip(w):
    """the data gradient's kernel: w'[ci][co][ky][kx] = w[co][ci][2-ky][2-kx]"""
    return np.ascontiguousarray(np.asarray(w).transpose(1, 0, 2, 3)[:, :, ::-1, ::-1])


def conv_f16(x, w, pad=0, s=X_SCALE, absum=True):
    """-> (value, absum, n) of the valid 3x3 convolution of x [Ci,H,W] (virtual zero border `pad`) with w [Co,Ci,3,3]; absum=False: None in its place"""
    xq = np.pad(q16(x, s), ((0, 0), (pad, pad), (pad, pad)))
    wq = q16(w, W_SCALE)
    return _corr(xq, wq) / (W_SCALE * s), (_corr(np.abs(xq), np.abs(wq)) / (W_SCALE * s) if absum else None), 9 * x.shape[0]


def dgrad_f16(dy, w, s=None):
    """data gradient of the convolution with w [Co,Ci,3,3]: dy [Co,H-2,W-2] -> dx [Ci,H,W]; s: the scale of dy's tensor (default: from dy alone)"""
    return conv_f16(dy, _flip(w), pad=2, s=tensor_scale(dy) if s is None else s)


def wgrad_f16(dy, x, s=None, absum=True):
    """-> (value, absum, n) of dW = sum_pixels dy (x) X: X at the static scale, dy at its tensor's; n = the contracted pixels"""
    s = tensor_scale(dy) if s is None else s
    dq, xq = q16(dy, s), q16(x, X_SCALE)
    return _wcorr(dq, xq) / (X_SCALE * s), (_wcorr(np.abs(dq), np.abs(xq)) / (X_SCALE * s) if absum else None), dy.shape[1] * dy.shape[2]


def conv_f64(x, w, pad=0, absum=True):
    """the same on the unquantised operands -> (value, sum |w||x|)"""
    x64 = np.pad(np.asarray(x, np.float64), ((0, 0), (pad, pad), (pad, pad)))
    w64 = np.asarray(w, np.float64)
    return _corr(x64, w64), (_corr(np.abs(x64), np.abs(w64)) if absum else None)


def wgrad_f64(dy, x, absum=True):
    d64, x64 = np.asarray(dy, np.float64), np.asarray(x, np.float64)
    return _wcorr(d64, x64), (_wcorr(np.abs(d64), np.abs(x64)) if absum else None)


def bound(absum, n):
    """the error model: |y - value| <= 1.01 n 2^-24 absum"""
    return 1.01 * n * U24 * absum


def bound_f64(abs64, n):
    """against float64 on the unquantised operands, both in the normal f16 range: (2^-10 + 2^-22 + 1.01 n 2^-24) sum |w||x|"""
    return (2.0 ** -10 + 2.0 ** -22 + 1.01 * n * U24) * abs64


# ---- EDSR inside PlanesSR, layer by layer ------------------------------------------------------------------------------------------------
def wide(Cin, Cout):
    """the layers that run the one-limb kernels (csrc/sr_core.h conv_limb16_eligible); the others run what they run under 'f16x2': three bf16
    limbs or exact f32 products forward and backward, two f16 limbs in their weight gradient -- f32-grade, taken as float64 here"""
    return Cin % 32 == 0 and Cout % 128 == 0


def split_blob(blob, Cin, Cout, hid, nblocks, n_up):
    """the natural blob (state-dict order) -> [w [Co,Ci,3,3]] : conv_input, (conv1, conv2) x nblocks, conv_mid, n_up x up-conv, conv_output"""
    shapes = [(hid, Cin)] + [(hid, hid)] * (2 * nblocks + 1) + [(4 * hid, hid)] * n_up + [(Cout, hid)]
    ws, off = [], 0
    for co, ci in shapes:
        ws.append(np.asarray(blob[off: off + 9 * co * ci], np.float32).reshape(co, ci, 3, 3))
        off += 9 * co * ci
    assert off == len(blob)
    return ws


def _shuffle(y):
    C4, H, W = y.shape
    return y.reshape(C4 // 4, 2, 2, H, W).transpose(0, 3, 1, 4, 2).reshape(C4 // 4, 2 * H, 2 * W)


def _unshuffle(g):
    C, H2, W2 = g.shape
    return g.reshape(C, H2 // 2, 2, W2 // 2, 2).transpose(0, 2, 4, 1, 3).reshape(4 * C, H2 // 2, W2 // 2)


def _f32(a):
    return np.asarray(a, np.float32)          # tensors live in f32 memory between the layers


class EdsrChain:
    """EDSR(Cin, Cout, hid, nblocks, 2^n_up) on a LIST of inputs of different sizes (one ragged launch per layer on the device: a gradient
    tensor's scale is taken over all planes, a weight gradient is the sum over them).  quantise=True: the wide layers in the one-limb
    arithmetic; False: everything in float64 (the check of this chain against the project's oracle)."""

    def __init__(self, blob, Cin, Cout, hid, nblocks, n_up, quantise):
        self.ws = split_blob(blob, Cin, Cout, hid, nblocks, n_up)
        self.nblocks, self.n_up, self.q = nblocks, n_up, quantise

    def _conv(self, x, w, pad=0, s=X_SCALE):
        if self.q and wide(w.shape[1], w.shape[0]):
            return conv_f16(x, w, pad, s, absum=False)[0]
        return conv_f64(x, w, pad, absum=False)[0]

    def _dgrad(self, gs, w):
        """data gradients of one layer for all planes"""
        if self.q and wide(w.shape[0], w.shape[1]):          # (the data gradient is a convolution Cout -> Cin)
            s = tensor_scale(*gs)
            return [conv_f16(g, _flip(w), 2, s, absum=False)[0] for g in gs]
        return [conv_f64(g, _flip(w), 2, absum=False)[0] for g in gs]

    def _wgrad(self, gs, xs, w):
        if self.q and wide(w.shape[1], w.shape[0]):
            s = tensor_scale(*gs)
            return sum(wgrad_f16(g, x, s, absum=False)[0] for g, x in zip(gs, xs))
        return sum(wgrad_f64(g, x, absum=False)[0] for g, x in zip(gs, xs))

    def forward(self, xs):
        """-> outputs; keeps the layer inputs for backward()"""
        nb = self.nblocks
        self.inputs = [[] for _ in self.ws]          # inputs[l][plane]
        outs = []
        for x in xs:
            a = _f32(x)
            for l, w in enumerate(self.ws):
                self.inputs[l].append(a)
                y = self._conv(a, w)
                if 1 <= l <= 2 * nb:
                    if l & 1:
                        y = np.maximum(y, 0.0)
                    else:
                        xb = self.inputs[l - 1][-1].astype(np.float64)
                        y = _f32(_f32(y) * np.float32(0.1)).astype(np.float64) + xb[:, 2:-2, 2:-2]
                elif 2 * nb + 1 < l < len(self.ws) - 1:
                    y = _shuffle(y)
                a = _f32(y)
            outs.append(a)
        return outs

    def backward(self, d_outs):
        """-> ([dW per layer, float64], [dx per plane])"""
        nb, n = self.nblocks, len(self.ws)
        gs = [_f32(g) for g in d_outs]
        dws = [None] * n
        l = n - 1
        while l >= 0:
            w = self.ws[l]
            if 2 * nb + 1 < l < n - 1:                                  # up-sampling convolution: undo the shuffle first
                gs = [_f32(_unshuffle(g)) for g in gs]
                dws[l] = self._wgrad(gs, self.inputs[l], w)
                gs = [_f32(g) for g in self._dgrad(gs, w)]
                l -= 1
            elif 1 <= l <= 2 * nb:                                      # block: layers l - 1 (conv1), l (conv2)
                t1s, xbs, w1 = self.inputs[l], self.inputs[l - 1], self.ws[l - 1]
                dws[l] = 0.1 * self._wgrad(gs, t1s, w)
                g1 = [_f32(np.where(t1 > 0, _f32(_f32(d) * np.float32(0.1)), np.float32(0))) for d, t1 in zip(self._dgrad(gs, w), t1s)]
                dws[l - 1] = self._wgrad(g1, xbs, w1)
                gs = [_f32(d + np.pad(g.astype(np.float64), ((0, 0), (2, 2), (2, 2)))) for d, g in zip(self._dgrad(g1, w1), gs)]
                l -= 2
            else:
                dws[l] = self._wgrad(gs, self.inputs[l], w)
                gs = [_f32(g) for g in self._dgrad(gs, w)]
                l -= 1
        return dws, gs


def sr_roi(R0, R1, roi):
    """csrc/sr_core.h sr_roi: roi [ymin, xmin, ymax, xmax] in [-1, 1] -> LR pixel bounds (lo, hi), in f32 like the library"""
    lo, hi = [0, 0], [R0, R1]
    if roi is not None:
        r = np.asarray(roi, np.float32).reshape(-1)
        for a, size in enumerate((R0, R1)):
            mn = np.float32(size) * (np.float32(1) + r[a]) / np.float32(2)
            mx = np.float32(size) * (np.float32(1) + r[2 + a]) / np.float32(2)
            lo[a] = max(int(np.floor(mn)) - 1, 0)
            hi[a] = min(int(np.ceil(mx)) + 1, size)
    return lo, hi


def sr_crop(lr, roi, pad):
    """PlanesSR's network input: the region with `pad` texels of context, replicate-padded at the plane's border -> (crop, row index, column index)"""
    R0, R1 = lr.shape[-2:]
    lo, hi = sr_roi(R0, R1, roi)
    iy = np.clip(np.arange(lo[0] - pad, hi[0] + pad), 0, R0 - 1)
    ix = np.clip(np.arange(lo[1] - pad, hi[1] + pad), 0, R1 - 1)
    return np.ascontiguousarray(lr[:, iy][:, :, ix]), iy, ix


def sr_uncrop(dx, iy, ix, R0, R1):
    """adjoint of sr_crop: the gradient of the crop added back onto the plane"""
    out = np.zeros((dx.shape[0], R0, R1))
    np.add.at(out, (slice(None), iy[:, None], ix[None, :]), dx)
    return out


def rms(a):
    return float(np.sqrt(np.mean(np.square(np.asarray(a, np.float64)))))


# ---- the small end-to-end case of tests/test_conv_f16.py (its CPU half: tests/test_conv_f16_host.py) ---------------------------------------
E2E = dict(R=12, hid=128, nblocks=2, n_up=1, seed=61,
           rois=[[-0.9, -0.35, 0.1, 0.8], [-1.0, -1.0, 0.2, 0.3], [-0.2, -0.6, 0.95, 0.6]])


def e2e_case(models):
    """the network (CPU), its LR planes and output gradients: everything the CPU reference and the GPU run share.  models: the package's module"""
    import torch
    torch.manual_seed(E2E["seed"])
    sr = models.PlanesSR(models.EDSR, 1 << E2E["n_up"], 48, 48, {"model": {"hidden_size": E2E["hid"], "n_blocks": E2E["nblocks"]}}, "bilinear")
    with torch.no_grad():
        for p_ in sr.parameters():
            p_.mul_(3.0)          # (PlanesSR initialises at 1/10 of He scale: x3 keeps the activations of 8 layers O(0.1))
    rng = np.random.default_rng(E2E["seed"] + 1)
    R, sf = E2E["R"], 1 << E2E["n_up"]
    lrs = [(rng.standard_normal((48, R, R)) * 0.5).astype(np.float32) for _ in range(3)]
    d_outs = [rng.standard_normal((48, sf * R, sf * R)).astype(np.float32) for _ in range(3)]
    return sr, lrs, d_outs


def e2e_oracle(oracle, sr, lrs, d_outs, with_crops=True):
    """the project's float64 oracle on the whole PlanesSR -> {out: [per plane, NaN outside its region], d_lr: [per plane], dw: the natural
    blob's gradient summed over the planes, layer_sizes}; with_crops: also what EdsrChain needs -- every region's network input, its place on
    the plane, the gradient of the network's output and the oracle's gradient of the network's input"""
    net = sr.inner_model
    Cin, Cout, hid, nb, n_up = net.geometry
    pad, over, sf = int(net.required_padding), int(sr.HR_overpadding), 1 << n_up
    blob = np.concatenate([w.detach().cpu().numpy().reshape(-1) for w in net.conv_weights()]).astype(np.float32)
    R = lrs[0].shape[-1]
    o = dict(out=[], d_lr=[], dw=np.zeros(blob.shape, np.float64), layer_sizes=[w.numel() for w in net.conv_weights()], blob=blob, regions=[])
    for lr, roi, d_out in zip(lrs, E2E["rois"], d_outs):
        roi_a = np.asarray(roi, np.float32).reshape(2, 2)
        o["out"].append(oracle.planes_sr(lr, blob, hid, nb, n_up, pad, over, roi=roi_a).astype(np.float64))
        gw, glr = oracle.planes_sr_backward(lr, blob, hid, nb, n_up, pad, over, d_out, roi=roi_a)
        o["dw"] += gw
        o["d_lr"].append(glr.astype(np.float64))
        if not with_crops:
            continue
        crop, iy, ix = sr_crop(lr, roi, pad)
        lo, hi = sr_roi(R, R, roi)
        box = (slice(None), slice(sf * lo[0], sf * hi[0]), slice(sf * lo[1], sf * hi[1]))
        inside = np.zeros(o["out"][-1].shape, bool)
        inside[box] = True
        assert np.array_equal(~np.isnan(o["out"][-1]), inside), "sr_roi disagrees with the oracle's region"
        d_diff = np.pad(d_out[box], ((0, 0), (over, over), (over, over)))
        o["regions"].append(dict(crop=crop, box=box, iy=iy, ix=ix, d_diff=d_diff, up=oracle.upsample_bilinear(lr, sf).astype(np.float64)[box],
                                 dx=oracle.edsr_backward(crop, blob, Cout, hid, nb, n_up, d_diff)[1].astype(np.float64)))
    return o


def e2e_reference(sr, o, quantise=True):
    """EdsrChain on the regions' crops of e2e_oracle's result `o`, carried to the planes by the oracle's own (linear) pre- and post-processing:
    out = diff[over:-over] + bilinear(LR), d_lr = oracle d_lr + uncrop(dx - oracle dx).  -> {out, d_lr, dw} like the oracle's"""
    Cin, Cout, hid, nb, n_up = sr.inner_model.geometry
    over = int(sr.HR_overpadding)
    chain = EdsrChain(o["blob"], Cin, Cout, hid, nb, n_up, quantise)
    diffs = chain.forward([g["crop"] for g in o["regions"]])
    dws, dxs = chain.backward([g["d_diff"] for g in o["regions"]])
    r = dict(out=[], d_lr=[], dw=np.concatenate([d.reshape(-1) for d in dws]))
    for g, diff, dx, oout, odlr in zip(o["regions"], diffs, dxs, o["out"], o["d_lr"]):
        out = np.full(oout.shape, np.nan)
        out[g["box"]] = diff[:, over:-over, over:-over].astype(np.float64) + g["up"]
        r["out"].append(out)
        r["d_lr"].append(odlr + sr_uncrop(dx.astype(np.float64) - g["dx"], g["iy"], g["ix"], *odlr.shape[-2:]))
    return r


def e2e_errors(got, orc):
    """rms(got - oracle) / rms(oracle): of the outputs inside their regions (all planes), of the LR-plane gradients, of every layer's weight gradient"""
    inside = [~np.isnan(o) for o in orc["out"]]
    cat = lambda ts, ms=None: np.concatenate([np.asarray(t, np.float64)[m].reshape(-1) if m is not None else np.asarray(t, np.float64).reshape(-1)
                                              for t, m in zip(ts, ms or [None] * len(ts))])
    e = dict(out=rms(cat(got["out"], inside) - cat(orc["out"], inside)) / rms(cat(orc["out"], inside)),
             d_lr=rms(cat(got["d_lr"]) - cat(orc["d_lr"])) / rms(cat(orc["d_lr"])), dw=[])
    off = 0
    for n in orc["layer_sizes"]:
        e["dw"].append(rms(np.asarray(got["dw"], np.float64)[off: off + n] - orc["dw"][off: off + n]) / rms(orc["dw"][off: off + n]))
        off += n
    return e


# e_ref = rms(ref - oracle) / rms(oracle) of e2e_reference(quantise=True) for the case above, computed on the CPU (tests/test_conv_f16_host.py
# recomputes them): what the ARITHMETIC costs on this network, the yardstick of the GPU run (within 2 x each).  The outputs and the LR-plane
# gradients are dominated by PlanesSR's bilinear residual, which no arithmetic touches; conv1 of a block (layers 1, 3) sees the ReLU gates that
# flip where a pre-activation is within an f16 rounding of zero (rms ~ the square root of the flipped fraction).
E2E_EREF = dict(out=1.0192e-05, d_lr=1.1677e-05,
                dw=[4.8535e-04, 1.4708e-02, 6.1395e-04, 1.3653e-02, 5.9305e-04, 4.1573e-04, 4.1446e-04, 4.1328e-04])
