"""numpy reference of the generic geometries' fused evaluation in 'f16x2' (csrc/generic_fused_limb.hip) for tests/test_generic_limb_host.py
(CPU) and tests/test_generic_limb.py (GPU).  A plain helper module like render_f16_ref.py (not collected, not a conftest).

Decoder inputs: oracle.generic_decoder.decode's own geometry logic (positions, projections, taps, combination rules, float64), read out of
it through a decoder of no hidden layers whose heads are identity matrices, and rounded to f32 -- the kernel's stage 0 is f32.
Per hidden layer: w^ = limbs of 2^8 W, x^ = limbs of 2^4 x (hi = RN_f16(v), lo = RN_f16(v - hi), the subtraction exact in f32), the products
Wh xl + Wh xh + Wl xh exact, their sum in float64, / 4096 + b, a ReLU that keeps NaN, rounded to f32 -- what the kernel leaves in LDS up to the
order of its f32 accumulation.  An operand beyond the f16 range has the limbs (inf, -inf): the sum is NaN.  Heads: float64 on the f32
activations, +-inf -> NaN.  hi_only=True drops the two products with a low limb: the arithmetic of a kernel that forgot them.
Also here: the packed fragment layout of nvsr_pack_generic_decoder_ext (include/nvsr.h) restated on numpy arrays."""
import numpy as np

from oracle.generic_decoder import decode, is_skip_layer

F16_W_SCALE, F16_X_SCALE = 256.0, 16.0
U24 = 2.0 ** -24


def limbs(v, scale):
    """f32 values -> (hi, lo) of v * scale as float64; beyond 65504: (+-inf, -+inf); NaN: (NaN, NaN)"""
    with np.errstate(over="ignore", invalid="ignore"):
        s = np.asarray(v, np.float32) * np.float32(scale)
        hi = s.astype(np.float16)
        lo = (s - hi.astype(np.float32)).astype(np.float16)
    return hi.astype(np.float64), lo.astype(np.float64)


def layer(W, b, x, hi_only=False):
    """x [P, K] f32, W [out, K], b [out] -> relu(W x + b) [P, out] f32 in the two-limb arithmetic"""
    wh, wl = limbs(W, F16_W_SCALE)
    xh, xl = limbs(x, F16_X_SCALE)
    with np.errstate(invalid="ignore", over="ignore"):
        acc = xh @ wh.T if hi_only else xl @ wh.T + xh @ wh.T + xh @ wl.T
        y = acc / (F16_W_SCALE * F16_X_SCALE) + np.asarray(b, np.float64)
        return np.where(y < 0, 0.0, y).astype(np.float32)             # (a NaN stays a NaN)


def layer_absum(W, x):
    """sum_k |w^||x^| / 4096 of a layer's outputs [P, out] (high limbs: the low ones add 2^-11 of it), for the accumulation-error model"""
    wh, _ = limbs(W, F16_W_SCALE)
    xh, _ = limbs(x, F16_X_SCALE)
    return (np.abs(xh) @ np.abs(wh).T) / (F16_W_SCALE * F16_X_SCALE) * (1.0 + 2.0 ** -10)


def head(W, b, x):
    with np.errstate(invalid="ignore", over="ignore"):
        y = np.asarray(x, np.float64) @ np.asarray(W, np.float64).T + np.asarray(b, np.float64)
    return np.where(np.isinf(y), np.nan, y)


def inputs(sd, planes, box, x, prefix="", **kw):
    """(Xd [P, Kd], Xr [P, Kr]) as f32: the inputs of the density and the colour decoder"""
    Kd, Kr = sd[prefix + "density_dec.0.0.weight"].shape[1], sd[prefix + "rgb_dec.0.0.weight"].shape[1]
    probe = {k: v for k, v in sd.items() if "coord_projector" in k}
    probe.update({prefix + "fc_alpha.0.weight": np.eye(Kd), prefix + "fc_alpha.0.bias": np.zeros(Kd), prefix + "fc_rgb.0.weight": np.eye(Kr),
                  prefix + "fc_rgb.0.bias": np.zeros(Kr)})
    kw = dict(kw, dec_density_layers=0, dec_rgb_layers=0, prefix=prefix)
    with np.errstate(invalid="ignore", over="ignore"):
        out = decode(probe, planes, box, x, **kw)
    return out[:, Kr:].astype(np.float32), out[:, :Kr].astype(np.float32)


def hidden_layers(sd, dec_density_layers=4, dec_rgb_layers=4, prefix="", **_):
    """[(W, b)] of the hidden layers in state-dict order: the density layers, then the rgb layers"""
    return [(np.asarray(sd[prefix + "%s.0.%d.weight" % (name, l)], np.float32), np.asarray(sd[prefix + "%s.0.%d.bias" % (name, l)], np.float32))
            for name, n in (("density_dec", dec_density_layers), ("rgb_dec", dec_rgb_layers)) for l in range(n)]


def decode_limb(sd, planes, box, x, hi_only=False, layer_fn=None, dec_density_layers=4, dec_rgb_layers=4, skip_connect_every=None, prefix="", **kw):
    """oracle.generic_decoder.decode's signature -> [P, 4] float64 = [rgb, sigma] with the hidden layers in two f16 limbs.
    layer_fn(W, b, h): another arithmetic for the hidden layers (float64, say) on the same f32 inputs."""
    Xd, Xr = inputs(sd, planes, box, x, prefix=prefix, skip_connect_every=skip_connect_every, **kw)
    fn = layer_fn or (lambda W, b, h: layer(W, b, h, hi_only))

    def mlp(inp, name, nlayers, head_name):
        h = inp
        for l in range(nlayers):
            if is_skip_layer(l - 1, skip_connect_every):
                h = np.concatenate([h, inp], 1)
            h = fn(sd[prefix + "%s.0.%d.weight" % (name, l)], sd[prefix + "%s.0.%d.bias" % (name, l)], h)
        return head(sd[prefix + head_name + ".0.weight"], sd[prefix + head_name + ".0.bias"], h), h

    alpha, _ = mlp(Xd, "density_dec", dec_density_layers, "fc_alpha")
    rgb, _ = mlp(Xr, "rgb_dec", dec_rgb_layers, "fc_rgb")
    return np.concatenate([rgb, alpha], 1)


def layer_f64(W, b, h):
    """the float64 layer on the same inputs (activations kept in float64)"""
    return np.maximum(np.asarray(h, np.float64) @ np.asarray(W, np.float64).T + np.asarray(b, np.float64), 0.0)


def pack(layers, hidden):
    """[(W [hidden, K], b)] -> the packed blob as uint32 words (include/nvsr.h, nvsr_pack_generic_decoder_ext): per layer the fragments
    [kb][t][limb] of 256 words; word 4 lane + j of lane (m = lane & 31, h = lane >> 5) = f16 W~[32 t + m][16 kb + 8 h + 2 j] | f16 W~[..][.. + 1]
    << 16, W~ = 2^8 W with +0 beyond the matrix, limb 0 = RN_f16(W~), limb 1 = RN_f16(W~ - limb 0)"""
    TT = (hidden + 31) // 32
    out = []
    lane = np.arange(64)
    m, h = lane & 31, lane >> 5
    for W, _ in layers:
        K = W.shape[1]
        KB = (K + 15) // 16
        pad = np.zeros((32 * TT, 16 * KB), np.float32)
        pad[:hidden, :K] = np.asarray(W, np.float32) * np.float32(F16_W_SCALE)
        with np.errstate(over="ignore", invalid="ignore"):
            hi = pad.astype(np.float16)
            lo = (pad - hi.astype(np.float32)).astype(np.float16)
        blob = np.zeros((KB, TT, 2, 64, 4), np.uint32)
        for kb in range(KB):
            for t in range(TT):
                for li, limb in enumerate((hi, lo)):
                    for j in range(4):
                        col = 16 * kb + 8 * h + 2 * j
                        a = limb[32 * t + m, col].view(np.uint16).astype(np.uint32)
                        b = limb[32 * t + m, col + 1].view(np.uint16).astype(np.uint32)
                        blob[kb, t, li, :, j] = a | (b << 16)
        out.append(blob.reshape(-1))
    return np.concatenate(out)


def seeded_state(pkg, seed, n_pos=3, res=10, **kw):
    """test_generic_fused.random_model's seeded model without a device: (CPU model, state dict, planes [1, C, res, res], kw) -- the same
    seeds, so the same weights and planes as the GPU tests' model of that seed"""
    import torch
    torch.manual_seed(seed)
    np.random.seed(seed)
    m = pkg.models.TwoDimPlanesModel(use_viewdirs=True, align_corners=True, num_planes_or_rot_mats=n_pos, **kw)
    with torch.no_grad():
        for p in m.decoder_parameters():
            p.normal_(0.0, float(np.sqrt(2.0 / p.shape[1]))) if p.dim() == 2 else p.uniform_(-0.1, 0.4)
    sd = {k: v.detach().numpy().copy() for k, v in m.state_dict().items()}
    rng = np.random.default_rng(seed)
    planes = [rng.standard_normal((1, kw.get("num_plane_channels", 48), res, res)).astype(np.float32) for _ in range(n_pos + 1)]
    return m, sd, planes, kw


def exact_state(sd, seed, dec_density_layers=4, dec_rgb_layers=4, prefix="", **_):
    """render_f16_ref.exact_decoder's idea on any geometry: a copy of the state dict sd with one weight +-1 or +-1/2 per row of every hidden
    layer, biases multiples of 1/8 in [-1, 1], heads with two weights +-1/2 per row (one where the layer has one input).  From zero planes every
    activation is a small multiple of a power of two: an f16 number after its scale, and every sum is exact in f32 in any order."""
    rng = np.random.default_rng(seed)
    sd = dict(sd)
    names = [("density_dec.0.%d" % l, 1) for l in range(dec_density_layers)] + [("fc_alpha.0", 2)] + \
            [("rgb_dec.0.%d" % l, 1) for l in range(dec_rgb_layers)] + [("fc_rgb.0", 2)]
    for name, per_row in names:
        out, fan = sd[prefix + name + ".weight"].shape
        W = np.zeros((out, fan), np.float32)
        n = min(per_row, fan)
        for i in range(out):
            W[i, rng.choice(fan, n, replace=False)] = rng.choice([1.0, -1.0, 0.5, -0.5], n)
        sd[prefix + name + ".weight"] = W
        sd[prefix + name + ".bias"] = (rng.integers(-8, 9, out) / 8.0).astype(np.float32)
    return sd
