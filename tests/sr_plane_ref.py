"""Float64 restatement of PlanesSR's plane stage -- the five small kernels around the EDSR network (csrc/sr.hip sr_prepare_kernel /
sr_finish_kernel, csrc/sr_bwd.hip sr_finish_backward_kernel / sr_residual_backward_gather_kernel / sr_prepare_backward_kernel, with
bilinear_tap / cubic_tap / sr_roi of csrc/sr_core.h) -- for tests/test_sr_plane_stage_host.py (CPU) and tests/test_sr_plane_stage.py (GPU).
Plain torch on the CPU and numpy, written from the semantics stated in include/nvsr.h and the kernels' comments:

    lo, hi   = roi_bounds(R0, R1, roi)                                  the region in LR texels -- an integer decision made in FLOAT32
    x        = lr[clamp(lo - pad .. hi + pad)]  (optionally (x - mean) / std)                        clamped gather = crop + replicate padding
    diff     = EDSR(x): conv2d, ReLU, 0.1 t + h[2:-2], pixel_shuffle                                  float64
    out      = diff[over:-over] + F.interpolate(lr, scale_factor, mode, align_corners)  inside the region, NaN outside

The gradients are float64 autograd of sum(nan_to_zero(out) * d_out): d_lr and the weight gradients in the natural (state-dict) layout.

The region bounds follow sr_roi operation for operation in float32: shape * (1 + roi) / 2, floor / ceil, lo = max(lo - 1, 0),
hi = min(hi + 1, R).  A float64 restatement differs: for the region [[-0.35, -0.6], [0.2, 0.15]] on 20 rows float32 gives rows 5..13
(1 + 0.2f rounds, 20 * 1.2f / 2 is exactly 12), float64 gives 5..14 (12.00000003 -> ceil 13).

A-priori bounds (nothing here is fitted to a device's output)
-------------------------------------------------------------
u = 2^-24 is the unit roundoff of an f32 operation.  The device forms every sum of products in f32 in some order; for a sum of n terms
|fl(sum) - sum| <= gamma_n sum|terms|, gamma_n <= 1.01 n u, and for a chain of such sums the n add up along the path (Higham, Accuracy and
Stability of Numerical Algorithms, 3.1 / 3.5).  So:

  * network part.  The same chain is run on |lr| and |weights| with the ReLU gates of the float64 run (as 0 / 1 masks), and its autograd
    with |d_out|: that is the abs-sum A of every output element, LR-gradient element and weight-gradient element.  The bound is
    1.01 n u A with n the number of accumulated terms along the longest path:
      forward  n_f = 9 Cin per layer  (9 C + nblocks (18 hid + 2) + 9 hid + n_up 9 hid + 9 hid;  the "+ 2" is the block's 0.1 t and + h)
                     + 2 with normalisation ((x - mean) / std) + 1 for the final diff + residual;
      backward n_b = 9 Cout per layer (9 C + n_up 36 hid + 9 hid + nblocks (18 hid + 2) + 9 hid) + 1 for the division by std;
      weights  n_w = n_f + n_b + the largest number of pixels a layer's weight gradient contracts + its row slabs (<= rows) + 4
                     + the number of planes summed into the blob.
    (0.1 is the f32 constant 0.1f here, as in the device's epilogue: the reference multiplies by float(np.float32(0.1)).)
    A ReLU gate cannot differ between the device and float64 where |pre-activation| >= 2 x its own bound (relu_margins); the case table's
    ReLU seeds are chosen so that this holds for EVERY pre-activation, so the bound applies unchanged.

  * residual part.  The up-sampling is separable, out = My lr Mx^T with tap matrices M[o, i] (tap_matrix; checked against F.interpolate
    by the host test).  The device forms the source position src in f32 (bilinear_tap / cubic_tap):
      align_corners:  src = fl(fl((in - 1) / (out - 1)) o)              two roundings:         |d src| <= 2.01 u |src|
      otherwise:      src = fl(fl(inv (o + 0.5)) - 0.5)                 a multiply, a subtract: |d src| <= 1.01 u (|(o + 0.5) / sf| + |src|)
    (floor and src - floor are exact).  The tap weights are continuous functions of src -- a source position that crosses an integer hands
    its weight to the neighbour tap continuously -- with Lipschitz constant 1 (the bilinear hat) or <= 1.35 < 1.5 (the cubic convolution
    kernel with A = -0.75: |K'| peaks at |x| = 0.6), so every weight moves by at most L |d src|: E[o, i] = L |d src| on every texel under the
    taps of src - d and src + d.  The cubic weights are Horner polynomials in t with intermediates below 16 in about 8 operations: an
    absolute 128 u per tap on top.  The error of src times the largest texel difference under the taps is then bounded by
    ((|My| + Ey) |lr| (|Mx| + Ex)^T - |My| |lr| |Mx|^T) -- per element, with the texels actually under the taps.  The weighted sum's own
    rounding is 1.01 n_r u (|My| + Ey) |lr| (|Mx| + Ex)^T with n_r = 8 (bilinear: 1 - w, product, add, product, add, and the final add)
    or 12 (bicubic: product, three adds, product, four adds, the final add).
    Backward: the transposes, with |d_out|; a term is g wy wx (n_r = 6) and, for the bilinear gather, a row sum and a column sum of 3 sf + 1
    candidates each (n_r = 6 + 2 (3 sf + 1)).

  * accumulation into d_lr.  d_lr is accumulated in place: the prepared input's gradient is scattered by float atomics (every texel
    receives as many terms as gather positions clamp onto it), the residual's share by a gather's one += or by atomics (as many terms as
    HR pixels of the region whose taps include the texel).  Each of these n_acc additions rounds at the magnitude of the running sum,
    at most base + all abs-sums, base = |what the buffer held before|: + 1.01 n_acc u (base + A).

The tight yardstick of the network path (stated, not a-priori)
--------------------------------------------------------------
The abs-sum A of a chain of L random layers grows by sqrt(2 * 9 Cin / pi) per layer while its values do not grow: from x4 upward, and for
the gradients of the ReLU case, the a-priori bound exceeds the values it bounds (an all-zero gradient would pass).  It stays as the
necessary condition; what makes the network-path checks able to fail is a second yardstick that does not grow with depth:

    tight = RW u sqrt(n) Q,     Q = sqrt(the sum of the SQUARED path products) -- the same chain on lr^2, weights^2 (0.1f^2, 1 / std^2,
                                    the float64 run's gates) and its autograd with d_out^2;  n as above;  RW = 8

Reasoning: an f32 sum of n terms t_i whose signs are random (the tables' weights, planes and output gradients are independent centred
Gaussians) has partial sums of size sqrt(k) rms(t); each addition rounds by at most u / 2 of its partial sum, independently, so the sum's
error is a random walk of standard deviation <= u sqrt(sum_k k rms^2 / 3) / 2 < u sqrt(n / 6) sqrt(sum t^2).  Errors made in one layer pass
through the later layers like the values do, in quadrature, and the layers' errors add in quadrature: sigma <= u sqrt(n / 6) Q with n the
terms along the path.  RW = 8 is 8 sqrt(6) = 19.6 sigma of this model -- a factor 4 for what the model leaves out (the order of the sums
on the device, MFMA's internal accumulation, partial sums that are not exactly sqrt(k)) times the 4.9 sigma that 10^6 Gaussian elements
reach once in a few suites.  A float32 run of the same chain on the CPU stays within it (host test).  On top of it: the residual part's
a-priori terms as they are (they are tight: the residual is one short sum), one rounding of the final add (u |out|), and for d_lr the
accumulation term with the running sum's magnitude base + 4 Q + the residual's abs-sum in place of base + A.
The a-priori bounds are tight where the chain is short (the residual alone: measured ratios 0.01 .. 0.65); for the network path the tight
yardstick is the check that can fail, and the host test shows every network-path mutant exceeding it at x2, x8 and in the ReLU case.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
TENTH = float(np.float32(0.1))
CUBIC_LIP = 1.5
CUBIC_W_EPS = 128 * U
RW = 8.0                           # the random-walk yardstick's factor (module docstring)


# ---- the region ---------------------------------------------------------------------------------------------------------------------------
def roi_bounds(R0, R1, roi, dtype=np.float32):
    """csrc/sr_core.h sr_roi: roi = None (full plane) or [ymin, xmin, ymax, xmax] host floats -> (lo, hi) in LR texels.  dtype: the arithmetic
    (float32 is the library's and upstream's; float64 is the mutant of the sensitivity test)"""
    lo, hi = [0, 0], [R0, R1]
    if roi is None:
        return lo, hi
    r = np.asarray(roi, np.float32).reshape(-1)
    f = dtype
    for a, size in enumerate((R0, R1)):
        mn = f(size) * (f(1) + f(r[a])) / f(2)
        mx = f(size) * (f(1) + f(r[2 + a])) / f(2)
        lo[a] = max(int(math.floor(mn)) - 1, 0)
        hi[a] = min(int(math.ceil(mx)) + 1, size)
    return lo, hi


# ---- the network ------------------------------------------------------------------------------------------------------------------------
def layer_shapes(C, hid, nblocks, n_up):
    """(Cout, Cin) in edsr_layers' order: conv_input, (conv1, conv2) x nblocks, conv_mid, up-convs, conv_output"""
    return [(hid, C)] + [(hid, hid)] * (2 * nblocks + 1) + [(4 * hid, hid)] * n_up + [(C, hid)]


def split_blob(blob, C, hid, nblocks, n_up):
    ws, off = [], 0
    blob = torch.as_tensor(np.asarray(blob)).reshape(-1)
    for co, ci in layer_shapes(C, hid, nblocks, n_up):
        ws.append(blob[off: off + 9 * co * ci].reshape(co, ci, 3, 3))
        off += 9 * co * ci
    assert off == blob.numel()
    return ws


def join_blob(ws):
    return np.concatenate([np.asarray(w.detach() if hasattr(w, "detach") else w).reshape(-1) for w in ws])


def pad_over(nblocks, n_up):
    """required_padding / HR_overpadding as models.EDSR / PlanesSR derive them: the valid convolutions eat 2 nblocks + 2 texels a side before the
    up-sampling, one per up-conv (at its scale) and one at the output"""
    sf = 1 << n_up
    eaten = sf * (2 * nblocks + 2) + sum(sf >> u for u in range(n_up)) + 1          # HR pixels a side
    pad = -(-eaten // sf)
    return pad, pad * sf - eaten


def forward_terms(C, hid, nblocks, n_up, normalised):
    return 9 * C + nblocks * (18 * hid + 2) + 9 * hid + n_up * 9 * hid + 9 * hid + (2 if normalised else 0) + 1


def backward_terms(C, hid, nblocks, n_up):
    return 9 * C + n_up * 36 * hid + 9 * hid + nblocks * (18 * hid + 2) + 9 * hid + 1


def _edsr(x, ws, nblocks, n_up, gates=None, rec=None, n0=0, tenth=TENTH):
    """x [1, C, H, W] float64.  gates = None: the value run (ReLU as a 0 / 1 mask of the pre-activation's sign); a list: those masks (the abs
    run).  rec: receives (pre-activation, mask, accumulated terms) per block"""
    hid = ws[0].shape[0]
    h = F.conv2d(x, ws[0])
    n, k = n0 + 9 * ws[0].shape[1], 1
    for b in range(nblocks):
        pre = F.conv2d(h, ws[k])
        gate = (pre > 0).to(pre.dtype) if gates is None else gates[b]
        if rec is not None:
            rec.append((pre.detach(), gate.detach(), n + 9 * hid))
        t = F.conv2d(pre * gate, ws[k + 1])
        h = t * tenth + h[..., 2:-2, 2:-2]
        n, k = n + 18 * hid + 2, k + 2
    h = F.conv2d(h, ws[k])
    k += 1
    for _ in range(n_up):
        h = F.pixel_shuffle(F.conv2d(h, ws[k]), 2)
        k += 1
    return F.conv2d(h, ws[k])


# ---- the residual's taps ----------------------------------------------------------------------------------------------------------------
def tap_matrix(n_in, sf, mode, align):
    """F.interpolate(scale_factor=sf, mode, align_corners=align) along an axis of n_in texels as a matrix M [n_in sf, n_in] (float64), and
    E >= 0: the bound on |the device's f32 tap weights - M| per entry (module docstring)"""
    n_out = n_in * sf
    M, E = np.zeros((n_out, n_in)), np.zeros((n_out, n_in))
    cubic = mode == "bicubic"
    for o in range(n_out):
        if align:
            src = o * ((n_in - 1) / (n_out - 1)) if n_out > 1 else 0.0
            d = 2.01 * U * abs(src)
        else:
            src = (o + 0.5) / sf - 0.5
            d = 1.01 * U * (abs((o + 0.5) / sf) + abs(src))
            if not cubic:
                src = max(src, 0.0)
        if cubic:
            fl = math.floor(src)
            t = src - fl
            A = -0.75
            x = (t + 1.0, t, 1.0 - t, 2.0 - t)
            w = (((A * x[0] - 5 * A) * x[0] + 8 * A) * x[0] - 4 * A, ((A + 2) * x[1] - (A + 3)) * x[1] * x[1] + 1,
                 ((A + 2) * x[2] - (A + 3)) * x[2] * x[2] + 1, ((A * x[3] - 5 * A) * x[3] + 8 * A) * x[3] - 4 * A)
            for k in range(4):
                M[o, min(max(fl - 1 + k, 0), n_in - 1)] += w[k]
            for s in (src - d, src + d):
                for k in range(4):
                    E[o, min(max(math.floor(s) - 1 + k, 0), n_in - 1)] += CUBIC_LIP * d + CUBIC_W_EPS
        else:
            i0 = min(int(src), n_in - 1)
            i1 = min(i0 + 1, n_in - 1)
            w1 = min(max(src - i0, 0.0), 1.0)
            M[o, i0] += 1.0 - w1
            M[o, i1] += w1
            if d > 0:
                for s in (max(src - d, 0.0), src + d):
                    j0 = min(int(s), n_in - 1)
                    for j in (j0, min(j0 + 1, n_in - 1), i0, i1):
                        E[o, j] = d
    return M, E


# ---- the stage --------------------------------------------------------------------------------------------------------------------------
MUTANTS = ("clamp_R_minus_2", "origin_plus_1", "over_off_by_one", "align_flipped", "axes_swapped_in_clamp", "bounds_in_float64",
           "window_without_lo_minus_1", "std_not_in_backward")


def _t64(a):
    if a is None:
        return None
    return torch.tensor(np.asarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a, np.float64))


def _stage(lr, lr_res, ws, nblocks, n_up, pad, over, roi, mean, std, mode, align, mutant=None, gates=None, rec=None, taps=None, tenth=TENTH):
    """out [C, sf R0, sf R1] (NaN outside the region) of lr -> network, lr_res -> residual (the same plane twice, so that the two shares of its
    gradient can be told apart).  taps = (Ay, Ax): the residual as Ay lr Ax^T in place of F.interpolate (the abs run)"""
    Cc, R0, R1 = lr.shape
    sf = 1 << n_up
    lo, hi = roi_bounds(R0, R1, roi, np.float64 if mutant == "bounds_in_float64" else np.float32)
    o = 1 if mutant == "origin_plus_1" else 0
    ys, xs = torch.arange(lo[0] - pad + o, hi[0] + pad + o), torch.arange(lo[1] - pad + o, hi[1] + pad + o)
    c0, c1 = (R1 - 1, R0 - 1) if mutant == "axes_swapped_in_clamp" else (R0 - 2, R1 - 2) if mutant == "clamp_R_minus_2" else (R0 - 1, R1 - 1)
    ys, xs = ys.clamp(0, max(c0, 0)), xs.clamp(0, max(c1, 0))
    flat = (ys[:, None] * R1 + xs[None, :]).clamp(max=R0 * R1 - 1)          # (a no-op unless a mutant's index leaves the plane, as a kernel's would)
    x = lr.reshape(Cc, -1)[:, flat]
    n0 = 0
    if mean is not None:
        xn = (x - mean[:, None, None]) / std[:, None, None]
        x = x - x.detach() + xn.detach() if mutant == "std_not_in_backward" else xn
        n0 = 2
    diff = _edsr(x[None], ws, nblocks, n_up, gates, rec, n0, tenth)[0]
    H, W = (hi[0] - lo[0]) * sf, (hi[1] - lo[1]) * sf
    ov = over - 1 if mutant == "over_off_by_one" else over
    diff = diff[:, ov: ov + H, ov: ov + W]
    if taps is None:
        up = F.interpolate(lr_res[None], scale_factor=sf, mode=mode, align_corners=(not align) if mutant == "align_flipped" else bool(align))[0]
    else:
        up = torch.einsum("oy,cyx,px->cop", taps[0], lr_res, taps[1])
    out = torch.full((Cc, R0 * sf, R1 * sf), float("nan"), dtype=lr.dtype)
    box = (slice(None), slice(lo[0] * sf, hi[0] * sf), slice(lo[1] * sf, hi[1] * sf))
    out[box] = diff + up[box]
    return out, lo, hi


def planes_sr64(lr, weights, nblocks, n_up, pad, over, roi, mean=None, std=None, mode="bilinear", align=True):
    """PlanesSR.forward in float64: lr [C, R0, R1], weights = the [Cout, Cin, 3, 3] tensors in edsr_layers' order -> out [C, sf R0, sf R1] as a
    float64 array, NaN outside the region"""
    lr = _t64(lr)
    return _stage(lr, lr, [_t64(w) for w in weights], nblocks, n_up, pad, over, roi, _t64(mean), _t64(std), mode, align)[0].numpy()


def reference(lr, weights, nblocks, n_up, pad, over, roi, mean=None, std=None, mode="bilinear", align=True, d_out=None, mutant=None,
              bounds=True):
    """The stage, its gradients and their a-priori bounds.  -> dict:
         out, lo, hi;  with d_out [C, sf R0, sf R1] (entries outside the region are ignored): d_lr [C, R0, R1], gw (natural blob)
         bounds: out_bound, d_lr_bound (of a d_lr that held zeros: d_lr_bound() adds what it held), gw_abs and gw_terms (gw_bound combines planes),
                 relu = [(|pre-activation|, its bound)] per block"""
    lr = _t64(lr)
    ws = [_t64(w) for w in weights]
    mean, std = _t64(mean), _t64(std)
    Cc, R0, R1 = lr.shape
    hid, sf = ws[0].shape[0], 1 << n_up
    want_grad = d_out is not None
    a = lr.clone().requires_grad_(want_grad)
    b = lr.clone().requires_grad_(want_grad)
    wl = [w.clone().requires_grad_(want_grad) for w in ws]
    rec = []
    out, lo, hi = _stage(a, b, wl, nblocks, n_up, pad, over, roi, mean, std, mode, align, mutant, None, rec)
    res = dict(out=out.detach().numpy(), lo=lo, hi=hi)
    inside = ~torch.isnan(out.detach())
    if want_grad:
        g = torch.where(inside, _t64(d_out), torch.zeros((), dtype=torch.float64))
        grads = torch.autograd.grad((torch.nan_to_num(out) * g).sum(), [a, b] + wl, allow_unused=True)
        z = lambda t, like: torch.zeros_like(like) if t is None else t
        d_net, d_res = z(grads[0], lr), z(grads[1], lr)
        if mutant == "window_without_lo_minus_1" and lo[0] > 0:
            d_res = d_res.clone()
            d_res[:, lo[0] - 1] = 0.0
        res["d_lr"] = (d_net + d_res).numpy()
        res["gw"] = join_blob([z(t, w) for t, w in zip(grads[2:], ws)])
    if not bounds:
        return res
    # ---- the abs run: |lr|, |weights|, the value run's gates, the perturbed tap matrices
    (My, Ey), (Mx, Ex) = tap_matrix(R0, sf, mode, align), tap_matrix(R1, sf, mode, align)
    Ay, Ax = torch.as_tensor(np.abs(My) + Ey), torch.as_tensor(np.abs(Mx) + Ex)
    a2 = lr.abs().requires_grad_(want_grad)
    b2 = lr.abs().requires_grad_(want_grad)
    wl2 = [w.abs().requires_grad_(want_grad) for w in ws]
    rec2 = []
    zero = torch.zeros_like(lr)
    n_f, n_b = forward_terms(Cc, hid, nblocks, n_up, mean is not None), backward_terms(Cc, hid, nblocks, n_up)
    cubic = mode == "bicubic"
    n_r = 12 if cubic else 8
    # (three abs runs that share nothing but the inputs: the network alone, the residual with the perturbed taps, the residual with |M|)
    net_abs, _, _ = _stage(a2, zero, wl2, nblocks, n_up, pad, over, roi, None if mean is None else -mean.abs(), None if std is None else std.abs(),
                           mode, align, None, [r[1] for r in rec], rec2, (Ay, Ax))
    up_pert = torch.einsum("oy,cyx,px->cop", Ay, b2, Ax)
    up_abs = torch.einsum("oy,cyx,px->cop", torch.as_tensor(np.abs(My)), lr.abs(), torch.as_tensor(np.abs(Mx)))
    net_abs0 = torch.nan_to_num(net_abs)
    ob = 1.01 * U * (n_f * net_abs0 + n_r * up_pert) + (up_pert - up_abs)
    res["out_bound"] = torch.where(inside, ob, torch.zeros((), dtype=torch.float64)).detach().numpy()
    res["relu"] = [(r[0].abs().numpy(), (1.01 * r[2] * U * r2[0]).numpy()) for r, r2 in zip(rec, rec2)]
    if not want_grad:
        return res
    ga = g.abs()
    gr = torch.autograd.grad((net_abs0 * ga).sum(), [a2] + wl2, allow_unused=True)
    G_net = z(gr[0], lr)
    G_res_pert = torch.einsum("oy,cop,px->cyx", Ay, ga, Ax)
    G_res_abs = torch.einsum("oy,cop,px->cyx", torch.as_tensor(np.abs(My)), ga, torch.as_tensor(np.abs(Mx)))
    n_rb = 6 + (0 if cubic else 2 * (3 * sf + 1))
    # additions that land on a texel: clamped gather positions + HR pixels of the region whose taps include it
    ys = np.clip(np.arange(lo[0] - pad, hi[0] + pad), 0, R0 - 1)
    xs = np.clip(np.arange(lo[1] - pad, hi[1] + pad), 0, R1 - 1)
    cnt = np.outer(np.bincount(ys, minlength=R0), np.bincount(xs, minlength=R1)).astype(np.float64)
    cnt += np.outer((Ay.numpy()[lo[0] * sf: hi[0] * sf] > 0).sum(0), (Ax.numpy()[lo[1] * sf: hi[1] * sf] > 0).sum(0))
    total = G_net + G_res_pert
    res["d_lr_bound"] = (1.01 * U * (n_b * G_net + n_rb * G_res_pert) + (G_res_pert - G_res_abs) + 1.01 * U * torch.as_tensor(cnt) * total).numpy()
    res["d_lr_adds"] = cnt
    res["gw_abs"] = join_blob([z(t, w) for t, w in zip(gr[1:], ws)])
    px = (hi[0] - lo[0] + 2 * pad) * sf * (hi[1] - lo[1] + 2 * pad) * sf          # (more than any layer contracts)
    res["gw_terms"] = n_f + n_b + px + (hi[0] - lo[0] + 2 * pad) * sf + 4
    # ---- the quadrature run: lr^2, weights^2, d_out^2 through the same chain -> the sum of the SQUARED path products of every element
    a3 = (lr * lr).requires_grad_(True)
    wl3 = [(w * w).requires_grad_(True) for w in ws]
    net_sq, _, _ = _stage(a3, zero, wl3, nblocks, n_up, pad, over, roi, None if mean is None else -mean * mean, None if std is None else std * std,
                          mode, align, None, [r[1] for r in rec], None, (Ay, Ax), TENTH * TENTH)
    net_sq0 = torch.nan_to_num(net_sq)
    q_out = net_sq0.detach().sqrt()
    ot = RW * U * math.sqrt(n_f) * q_out + 1.01 * U * n_r * up_pert + (up_pert - up_abs) + 1.01 * U * torch.nan_to_num(out.detach()).abs()
    res["out_tight"] = torch.where(inside, ot, torch.zeros((), dtype=torch.float64)).detach().numpy()
    gq = torch.autograd.grad((net_sq0 * ga * ga).sum(), [a3] + wl3, allow_unused=True)
    q_lr = z(gq[0], lr).sqrt()
    res["d_lr_tight"] = (RW * U * math.sqrt(n_b) * q_lr + 1.01 * U * n_rb * G_res_pert + (G_res_pert - G_res_abs)
                         + 1.01 * U * torch.as_tensor(cnt) * (4 * q_lr + G_res_pert)).numpy()
    res["gw_sq"] = join_blob([z(t, w) for t, w in zip(gq[1:], ws)])
    return res


def d_lr_bound(ref, base):
    """the bound of what a backward ADDED to a d_lr that held `base` (scalar or [C, R0, R1]): every addition rounds at base's magnitude too"""
    return ref["d_lr_bound"] + 1.01 * U * ref["d_lr_adds"] * np.abs(np.asarray(base, np.float64))


def d_lr_tight(ref, base):
    """d_lr_bound's tight twin (module docstring: the random-walk yardstick)"""
    return ref["d_lr_tight"] + 1.01 * U * ref["d_lr_adds"] * np.abs(np.asarray(base, np.float64))


def gw_tight(refs):
    """gw_bound's tight twin, of a blob that held zeros: RW u sqrt(n) sqrt(sum of the squared path products over the planes)"""
    n = max(r["gw_terms"] for r in refs) + len(refs)
    return RW * U * math.sqrt(n) * np.sqrt(sum(r["gw_sq"] for r in refs))


def gw_bound(refs, base=0.0):
    """the bound of the weight-gradient blob that the planes `refs` (reference() results) were summed into, on top of |base|"""
    A = sum(r["gw_abs"] for r in refs)
    n = max(r["gw_terms"] for r in refs) + len(refs)
    return 1.01 * U * n * (A + np.abs(base))


def relu_margins(ref):
    """min over all pre-activations of |a| / bound (>= 2: no gate can differ), and their number"""
    worst, count = float("inf"), 0
    for a, bnd in ref["relu"]:
        worst = min(worst, float((a / bnd).min()))
        count += a.size
    return worst, count


def worst_ratio(got, want, bound):
    """max |got - want| / bound over the elements (0 / 0 -> 0: an element that must be exact and is), and where"""
    err = np.abs(np.asarray(got, np.float64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    r = np.where(np.isnan(r), np.inf, r)
    i = int(np.argmax(r))
    return float(r.reshape(-1)[i]), np.unravel_index(i, r.shape) if r.ndim else ()


# ---- the case tables (shared by the host and the GPU tests) ---------------------------------------------------------------------------
C = 5
REGIONS = {
    "none": None,
    "full": [-1.0, -1.0, 1.0, 1.0],
    "beyond": [-1.25, -1.25, 1.25, 1.25],                 # beyond the plane: clamps to the full plane
    "top_left": [-1.0, -1.0, -0.5, -0.25],
    "bottom_right": [0.125, 0.2, 1.0, 1.0],
    "point": [0.0, 0.0, 0.0, 0.0],                        # 2 or 3 texels by the parity of R
    "g09": [-0.35, -0.6, 0.2, 0.15],                      # rows 5..13 of 20 in float32, 5..14 in float64
    "interior": [-0.125, 0.0, 0.125, 0.125],              # lo - 1 > 0 and hi + 1 < R on both axes of the larger planes
}
PLANES = [(7, 11), (11, 7), (20, 20), (2, 2), (1, 5)]
SMALLEST_PLANES = [(2, 2), (1, 5)]

# A. the residual alone: a zero-weight network (hid 4, 0 blocks); n_up 0 and 4 have no gather instantiation (the bilinear scatter)
RESIDUAL = dict(hid=4, nblocks=0, n_ups=(0, 1, 2, 3, 4), modes=("bilinear", "bicubic"), aligns=(1, 0))

# B. a linear network: hid 8, 0 blocks, weights N(0, 1 / (9 Cin)), lr 0.5 N(0, 1)
LINEAR = dict(hid=8, nblocks=0, planes=[(7, 11), (11, 7), (2, 2)],
              cases=[(n_up, mode, 1) for n_up in (1, 2, 3) for mode in ("bilinear", "bicubic")] + [(2, "bilinear", 0), (1, "bicubic", 0)],
              mean=[-0.9, -0.4, 0.1, 0.5, 1.1], std=[0.5, 0.8, 1.1, 1.5, 2.0])
LINEAR_WIDE = dict(n_up=2, extra_pad=1)                   # pad + 1, over + sf: the entry's consistency check accepts it; over = 5

# C. ReLU and the residual epilogue, a ragged batch of three planes with three regions.  Seeds: a CPU search over 0..39 found 13 whose 5760
# pre-activations of the float64 run are ALL at least 2 x their a-priori bound away from zero (1, 3, 4, 10, 19, 21, 25, 26, 27, 28, 35, 36, 38);
# the two recorded here have the widest margins but one (4.69 x and 9.5 x).  The host test certifies them
RELU = dict(hid=8, nblocks=1, n_up=2, pad=6, over=1, plane=(9, 13), regions=("full", "top_left", "bottom_right"), seeds=(19, 25))


def border_situations(R0, R1, roi, pad):
    """what a (plane, region) pair exercises"""
    lo, hi = roi_bounds(R0, R1, roi)
    s = set()
    s.add("full_plane" if lo == [0, 0] and hi == [R0, R1] else "cropped")
    if roi is not None and (min(roi) < -1 or max(roi) > 1):
        s.add("clamped_from_beyond")
    for a, R in enumerate((R0, R1)):
        if lo[a] == 0 and hi[a] < R:
            s.add("touches_low_border_only")
        if lo[a] > 0 and hi[a] == R:
            s.add("touches_high_border_only")
        if hi[a] - lo[a] == 2:
            s.add("two_texels")
        if hi[a] - lo[a] == 3:
            s.add("three_texels")
        if R == 1:
            s.add("axis_of_one_texel")
        if R < pad:
            s.add("plane_narrower_than_padding")
    if all(lo[a] - 1 > 0 and hi[a] + 1 < R for a, R in enumerate((R0, R1))):
        s.add("interior_on_both_axes")
    if R0 != R1:
        s.add("R0_lt_R1" if R0 < R1 else "R0_gt_R1")
    if hi[0] - lo[0] != hi[1] - lo[1]:
        s.add("region_not_square")
    if roi is not None and roi_bounds(R0, R1, roi, np.float64) != (lo, hi):
        s.add("float32_bounds_differ_from_float64")
    return s


ALL_SITUATIONS = {"full_plane", "cropped", "clamped_from_beyond", "touches_low_border_only", "touches_high_border_only", "two_texels", "three_texels",
                  "axis_of_one_texel", "plane_narrower_than_padding", "interior_on_both_axes", "R0_lt_R1", "R0_gt_R1", "region_not_square",
                  "float32_bounds_differ_from_float64"}


def make_case(seed, hid, nblocks, n_up, planes, zero_weights=False):
    """weights, LR planes and output gradients as f32 arrays (what the device gets; the reference reads the same f32 values)"""
    g = torch.Generator().manual_seed(seed)
    ws = [(torch.zeros(co, ci, 3, 3) if zero_weights else torch.randn(co, ci, 3, 3, generator=g, dtype=torch.float64) / math.sqrt(9 * ci)).float().numpy()
          for co, ci in layer_shapes(C, hid, nblocks, n_up)]
    sf = 1 << n_up
    lrs = [(torch.randn(C, R0, R1, generator=g, dtype=torch.float64) * 0.5).float().numpy() for R0, R1 in planes]
    d_outs = [torch.randn(C, R0 * sf, R1 * sf, generator=g, dtype=torch.float64).float().numpy() for R0, R1 in planes]
    return ws, lrs, d_outs
