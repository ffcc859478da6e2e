"""numpy reference of the generic geometries' planes-only TRAINING in 'f16x2' (csrc/generic_fused_bwd_limb.hip) for
tests/test_generic_train_limb_host.py (CPU) and tests/test_generic_train_limb.py (GPU).  A plain helper module like generic_limb_ref.py (not
collected, not a conftest).

Forward: generic_limb_ref's limb layers on the f32 decoder inputs; the gate of a unit is "its activation is > 0" (NaN and 0: closed).
Heads: dH = d_out W_head in float64, rounded to f32 (the kernel: an exact-f32 chain).
A transposed hidden layer, per point p: the gated row dZ[p][.] (f32) is multiplied by s = 2^e, e = ANCHOR + 127 - (biased exponent of the row's
largest |dZ|), which puts that maximum into [2^14, 2^15) -- ANCHOR = 14 is the highest binade whose every number and its rounding to f16 are
finite (65520 and above round to inf), and a scale per layer need not leave room for a chain's growth as the native backward's 2^3 does; a zero
row takes e = 0.  z^ = limbs of s dZ, w^ = limbs of 2^8 W, the products Wh zl + Wh zh + Wl zh exact, their sum in float64 (the kernel: f32
accumulation over 16-row blocks of m), dX = sum 2^(-8 - e) rounded to f32.  A row that holds an inf or a NaN gives a NaN row.  A skip layer's
part and layer 0's part are added into the decoder input's gradient in f32, layers descending.
Tail: the gradients of the decoder inputs (Xd, Xr) are pulled back to the planes by generic_train_ref's float64 autograd through a decoder of
no hidden layers whose heads are identity matrices -- the combination rules, the taps and the scatter in float64 (the kernel: f32).
Also here: the transposed fragment layout of nvsr_pack_generic_decoder_bwd_ext (include/nvsr.h) restated on numpy arrays."""
import numpy as np

import generic_limb_ref as fwd
import generic_train_ref as ref64
from generic_limb_ref import F16_W_SCALE, U24

ANCHOR = 14


def is_skip_layer(layer_num, skip_connect_every):
    return ref64.is_skip_layer(layer_num, skip_connect_every)


def decoder_layers(sd, name, nlayers, prefix=""):
    return [(np.asarray(sd[prefix + "%s.0.%d.weight" % (name, l)], np.float32), np.asarray(sd[prefix + "%s.0.%d.bias" % (name, l)], np.float32))
            for l in range(nlayers)]


def activations(layers, inp, skip_connect_every, layer_fn):
    """[h_0 .. h_{n-1}]: the outputs of the hidden layers on the decoder input inp [P, k0]"""
    h, out = inp, []
    for l, (W, b) in enumerate(layers):
        if is_skip_layer(l - 1, skip_connect_every):
            h = np.concatenate([h, inp], 1)
        h = layer_fn(W, b, h)
        out.append(h)
    return out


def gates(sd, planes, box, x, layer_fn=fwd.layer, dec_density_layers=4, dec_rgb_layers=4, skip_connect_every=None, prefix="", **kw):
    """the gates [P, hidden] (bool) of every hidden layer, density decoder first, and the smallest |activation| margin is NOT here: a gate is
    h > 0.  layer_fn = generic_limb_ref.layer: the limb forward's; generic_limb_ref.layer_f64: float64's on the same f32 inputs."""
    Xd, Xr = fwd.inputs(sd, planes, box, x, prefix=prefix, skip_connect_every=skip_connect_every, **kw)
    acts = activations(decoder_layers(sd, "density_dec", dec_density_layers, prefix), Xd, skip_connect_every, layer_fn) + \
           activations(decoder_layers(sd, "rgb_dec", dec_rgb_layers, prefix), Xr, skip_connect_every, layer_fn)
    return [np.asarray(a) > 0 for a in acts]


def row_scale(dz):
    """dz [P, M] f32 -> (e [P] int, bad [P] bool): the exponent of the row's power of two and whether the row holds an inf or a NaN"""
    bits = np.ascontiguousarray(np.abs(np.asarray(dz, np.float32))).view(np.uint32)
    amax = bits.max(axis=1) if bits.shape[1] else np.zeros(bits.shape[0], np.uint32)
    eb = (amax >> 23).astype(np.int64)
    return np.where(amax == 0, 0, ANCHOR + 127 - eb), eb == 255


def transposed_layer(W, dz, hi_only=False):
    """dz [P, M] f32 (gated), W [M, K] -> dX [P, K] f32 in the two-limb arithmetic under the row scale; also sum_m |w^||z^| 2^(-8 - e) [P, K]"""
    e, bad = row_scale(dz)
    with np.errstate(invalid="ignore", over="ignore"):
        z = np.ldexp(np.asarray(dz, np.float32), e[:, None].astype(np.int32)).astype(np.float32)
        zh = z.astype(np.float16)
        zl = (z - zh.astype(np.float32)).astype(np.float16)
        zh, zl = zh.astype(np.float64), zl.astype(np.float64)
        wh, wl = fwd.limbs(W, F16_W_SCALE)
        acc = zh @ wh if hi_only else zl @ wh + zh @ wh + zh @ wl
        dx = np.ldexp(acc, (-8 - e)[:, None].astype(np.int32)).astype(np.float32)
        absum = np.ldexp(np.abs(zh) @ np.abs(wh), (-8 - e)[:, None].astype(np.int32)) * (1.0 + 2.0 ** -10)
    dx[bad] = np.nan
    return dx, absum


def input_gradients(sd, name, head, nlayers, inp, g_head, skip_connect_every, prefix="", hi_only=False):
    """one decoder: inp [P, k0] f32, g_head [P, 1 | 3] -> (d inp [P, k0] f32, sum of the absolute-sum models of the parts that reach d inp)"""
    layers = decoder_layers(sd, name, nlayers, prefix)
    acts = activations(layers, inp, skip_connect_every, fwd.layer)
    k0 = inp.shape[1]
    Wh = np.asarray(sd[prefix + head + ".0.weight"], np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        dh = (np.asarray(g_head, np.float64) @ Wh).astype(np.float32)
    dx_in, absum_in = np.zeros((inp.shape[0], k0), np.float32), np.zeros((inp.shape[0], k0))
    for l in range(nlayers - 1, -1, -1):
        dz = np.where(acts[l] > 0, dh, np.float32(0)).astype(np.float32)
        dx, absum = transposed_layer(layers[l][0], dz, hi_only)
        K1 = k0 if l == 0 else layers[l][0].shape[0]
        if l == 0:
            dx_in, absum_in = dx_in + dx, absum_in + absum
            break
        if dx.shape[1] > K1:
            dx_in, absum_in = dx_in + dx[:, K1:], absum_in + absum[:, K1:]
        dh = dx[:, :K1]
    return dx_in.astype(np.float32), absum_in


def decoder_input_gradients(sd, planes, box, x, cotangent, dec_density_layers=4, dec_rgb_layers=4, skip_connect_every=None, prefix="", hi_only=False,
                            **kw):
    """-> (dXd [P, Kd], dXr [P, Kr], their absolute-sum models): the gradients of the two decoders' inputs for the cotangent [P, 4]"""
    Xd, Xr = fwd.inputs(sd, planes, box, x, prefix=prefix, skip_connect_every=skip_connect_every, **kw)
    G = np.asarray(cotangent, np.float32)
    dXd, ad = input_gradients(sd, "density_dec", "fc_alpha", dec_density_layers, Xd, G[:, 3:4], skip_connect_every, prefix, hi_only)
    dXr, ar = input_gradients(sd, "rgb_dec", "fc_rgb", dec_rgb_layers, Xr, G[:, 0:3], skip_connect_every, prefix, hi_only)
    return dXd, dXr, ad, ar


def pull_back(sd, planes, box, x, dXd, dXr, prefix="", **kw):
    """[d plane] float64 [1, C, H, W] of the decoder-input gradients: generic_train_ref's autograd through an identity decoder"""
    Kd, Kr = dXd.shape[1], dXr.shape[1]
    probe = {k: v for k, v in sd.items() if "coord_projector" in k}
    probe.update({"fc_alpha.0.weight": np.eye(Kd), "fc_alpha.0.bias": np.zeros(Kd), "fc_rgb.0.weight": np.eye(Kr), "fc_rgb.0.bias": np.zeros(Kr)})
    kw = {k: v for k, v in kw.items() if k not in ("dec_density_layers", "dec_rgb_layers")}
    cot = np.concatenate([np.asarray(dXr, np.float64), np.asarray(dXd, np.float64)], 1)          # (out = [rgb | alpha] = [Xr | Xd])
    return ref64.plane_gradients(probe, planes, box, x, cot, dec_density_layers=0, dec_rgb_layers=0, **kw)[1]


def plane_gradients(sd, planes, box, x, cotangent, **kw):
    """the new backward restated: [d plane] float64 [1, C, H, W]"""
    dXd, dXr, _, _ = decoder_input_gradients(sd, planes, box, x, cotangent, **kw)
    kw = {k: v for k, v in kw.items() if k != "hi_only"}
    return pull_back(sd, planes, box, x, dXd, dXr, **kw)


def layer_parts(sd, hidden, dec_density_layers=4, dec_rgb_layers=4, skip_connect_every=None, prefix="", **_):
    """[(W, K1)] of the hidden layers in state-dict order: the matrix and the width of its first column part (a skip layer has a second one)"""
    out = []
    for name, n in (("density_dec", dec_density_layers), ("rgb_dec", dec_rgb_layers)):
        for l, (W, _) in enumerate(decoder_layers(sd, name, n, prefix)):
            out.append((W, W.shape[1] if l == 0 else hidden))
    return out


def pack_bwd(parts, hidden):
    """[(W [hidden, K], K1)] -> the transposed blob as uint32 words (include/nvsr.h, nvsr_pack_generic_decoder_bwd_ext): per layer the column
    part [0, K1) and, where K > K1, the part [K1, K); per part the fragments [mb][t][limb] of 256 words; word 4 lane + j of lane (k = lane & 31,
    h = lane >> 5) = f16 W~[16 mb + 8 h + 2 j][c0 + 32 t + k] | f16 W~[16 mb + 8 h + 2 j + 1][c0 + 32 t + k] << 16, W~ = 2^8 W with +0 beyond
    the matrix and the part, limb 0 = RN_f16(W~), limb 1 = RN_f16(W~ - limb 0)"""
    MB = (hidden + 15) // 16
    lane = np.arange(64)
    k, h = lane & 31, lane >> 5
    out = []
    for W, K1 in parts:
        W = np.asarray(W, np.float32)
        for c0, cols in ((0, K1), (K1, W.shape[1] - K1)):
            if cols == 0:
                continue
            TT = (cols + 31) // 32
            pad = np.zeros((16 * MB, 32 * TT), np.float32)
            pad[:hidden, :cols] = W[:, c0:c0 + cols] * np.float32(F16_W_SCALE)
            with np.errstate(over="ignore", invalid="ignore"):
                hi = pad.astype(np.float16)
                lo = (pad - hi.astype(np.float32)).astype(np.float16)
            blob = np.zeros((MB, TT, 2, 64, 4), np.uint32)
            for mb in range(MB):
                for t in range(TT):
                    for li, limb in enumerate((hi, lo)):
                        for j in range(4):
                            m = 16 * mb + 8 * h + 2 * j
                            a = limb[m, 32 * t + k].view(np.uint16).astype(np.uint32)
                            b = limb[m + 1, 32 * t + k].view(np.uint16).astype(np.uint32)
                            blob[mb, t, li, :, j] = a | (b << 16)
            out.append(blob.reshape(-1))
    return np.concatenate(out)


def packed_bwd_words(hidden, parts):
    """the size nvsr_generic_packed_bwd_floats_ext must answer, from the layout alone"""
    MB = (hidden + 15) // 16
    return sum(MB * ((cols + 31) // 32) * 512 for W, K1 in parts for cols in (K1, W.shape[1] - K1) if cols)


def bwd_row_floats(Kd, Kr, hidden, layers):
    """the row of the limb backward (include/nvsr.h): Kr + Kd (each up to 4) + hidden (up to 16) + 4 + layers x ceil(hidden / 32), up to 4 x odd"""
    up = lambda v, a: (v + a - 1) // a * a
    ld = up(up(Kr, 4) + up(Kd, 4) + up(hidden, 16) + 4 + layers * ((hidden + 31) // 32), 4)
    return ld + 4 if (ld // 4) % 2 == 0 else ld
