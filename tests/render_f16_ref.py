"""numpy reference of the render pass's one-limb arithmetic, NVSR_ARITH_F16 / 'f16' (csrc/render3.hip at LIMBS = 1, limb_core.h), for
tests/test_render_f16_host.py (CPU) and tests/test_render_f16.py (GPU).  A plain helper module like triplane_checks.py (not collected, not a
conftest).

Per layer:  w^ = RN_f16(W 2^8),  x^ = RN_f16(x 2^4)  (f16x2's static scales), the products w^ x^ exact, their sum in float64, the scales undone,
the bias added, ReLU, and the activation rounded to f32 -- what the kernel holds in a register, up to the order of its f32 accumulation.  An
operand beyond the f16 range rounds to +-inf: the sum is then +-inf or NaN, and the reference -- like the kernel -- makes +-inf a NaN before the
ReLU, so that no out-of-range operand yields a finite number.  The heads are dot products of the f32 activations in float64 (the kernel: f32 on
the vector unit, in every arithmetic), +-inf -> NaN.

The first layer's features are the kernel's f32 blend restated on triplane_checks' float32 taps with the tap weights scaled by 2^4 (exact):
F = fma(T3, se, fma(T2, sw, fma(T1, ne, T0 nw))), D = ((F0 + F1) + F2) / 3, one f32 rounding per operation.
"""
import numpy as np

import triplane_checks as tc

F16_W_SCALE, F16_X_SCALE = 256.0, 16.0


def rn16(x):
    """round to nearest even f16 of f32 values -> float64 (beyond 65504: +-inf)"""
    with np.errstate(over="ignore"):
        return np.asarray(x, np.float32).astype(np.float16).astype(np.float64)


def inf_to_nan(y):
    return np.where(np.isinf(y), np.nan, y)


def layer(W, b, x):
    """one hidden / feature layer: x [P, K] f32 activations (unscaled), W [out, K], b [out] -> relu(W x + b) as f32 [P, out]"""
    wh, xh = rn16(np.asarray(W, np.float32) * np.float32(F16_W_SCALE)), rn16(np.asarray(x, np.float32) * np.float32(F16_X_SCALE))
    with np.errstate(invalid="ignore", over="ignore"):
        acc = inf_to_nan(xh @ wh.T)                                   # exact products (22 bits), float64 sum; inf x 0 and inf - inf are NaN
        y = acc / (F16_W_SCALE * F16_X_SCALE) + np.asarray(b, np.float64)
        return np.where(y < 0, 0.0, y).astype(np.float32)           # (a NaN stays a NaN)


def head(W, b, x):
    with np.errstate(invalid="ignore", over="ignore"):
        return inf_to_nan(np.asarray(x, np.float64) @ np.asarray(W, np.float64).T + np.asarray(b, np.float64))


def _fma32(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def features32(planes, rays, z, scene):
    """the kernel's f32 features, unscaled: [f0, f1, f2, f_view] [P, 48] f32 and D = ((f0 + f1) + f2) / 3.  The blend runs on weights scaled
    by 2^4 and is divided by it afterwards: exact both ways unless a value underflows, so that 2^4 F is what the kernel's registers hold."""
    N, S = z.shape
    s = np.float32(F16_X_SCALE)
    f = []
    with np.errstate(invalid="ignore", over="ignore"):
        for d in range(4):
            t = tc.position_taps(rays, z, scene, d, np.float32) if d < 3 else tc.view_taps(rays, scene, S, np.float32)
            tex = np.asarray(planes[d], np.float32).reshape(-1, tc.C)
            idx, w = t.idx.reshape(-1, 4), (t.w.reshape(-1, 4).astype(np.float32) * s)
            F = (tex[idx[:, 0]] * w[:, 0:1]).astype(np.float32)
            for k in (1, 2, 3):
                F = _fma32(tex[idx[:, k]], np.broadcast_to(w[:, k:k + 1], F.shape), F)
            f.append(F)
        D = (((f[0] + f[1]).astype(np.float32) + f[2]).astype(np.float32).astype(np.float64) / 3.0).astype(np.float32)
    return [(x / s).astype(np.float32) for x in f], (D / s).astype(np.float32)


def forward(dec, planes, rays, z, scene):
    """-> raw [P, 4] float64 = [rgb logits, sigma] of the one-limb arithmetic; dec: triplane_checks.unpack's layers (torch or numpy)"""
    A = lambda t: np.asarray(t, np.float64)
    f, D = features32(planes, rays, z, scene)
    x = D
    for l in range(4):
        x = layer(A(dec.Wd[l]), A(dec.bd[l]), x)
    sigma = head(A(dec.Wa), A(dec.ba), x)
    x = np.concatenate(f, 1)
    for l in range(4):
        x = layer(A(dec.Wr[l]), A(dec.br[l]), x)
    return np.concatenate([head(A(dec.Wc), A(dec.bc), x), sigma], 1)


# ---- operands that are f16 numbers after their scales: nothing is rounded, every arithmetic gives the float64 result -----------------------

def exact_decoder(seed):
    """natural blob: one weight +-1 or +-1/2 per row of every layer (a row then adds at most one bit below its input's last), biases multiples
    of 1/8 in [-1, 1], heads with two weights +-1/2 per row.  From zero features every activation is a multiple of 2^-6 below 8: at most 9
    significant bits, an f16 number after the scale 2^4, and every head sum is exact in f32."""
    rng = np.random.default_rng(seed)
    nat = np.zeros(tc.NATURAL, np.float32)

    def put(off, out, fan, per_row):
        W = np.zeros((out, fan), np.float32)
        for i in range(out):
            W[i, rng.choice(fan, per_row, replace=False)] = rng.choice([1.0, -1.0, 0.5, -0.5], per_row)
        nat[off:off + out * fan] = W.reshape(-1)
        nat[off + out * fan:off + out * fan + out] = rng.integers(-8, 9, out) / 8.0

    put(tc.N_DEN_W0, tc.HID, tc.C, 1)
    put(tc.N_RGB_W0, tc.HID, 4 * tc.C, 1)
    for l in range(3):
        put(tc.N_DEN_W1 + l * tc.N_HID_STRIDE, tc.HID, tc.HID, 1)
        put(tc.N_RGB_W1 + l * tc.N_HID_STRIDE, tc.HID, tc.HID, 1)
    put(tc.N_ALPHA_W, 1, tc.HID, 2)
    put(tc.N_FCRGB_W, 3, tc.HID, 2)
    return nat


def zero_planes(scene):
    return [np.zeros((h, w, tc.C), np.float32) for h, w in zip(scene.ph, scene.pw)]


def rms(a):
    a = np.asarray(a, np.float64)
    return float(np.sqrt(np.mean(a * a)))
