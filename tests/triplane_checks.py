"""float64 references and error bounds of the tri-plane training kernels -- csrc/decode_core.h, decode_limb.hip, decode_pair.hip (forward),
bwd_core.h, render_bwd.hip, render_bwd_limb.hip (backward) -- for tests/test_triplane_training_edges.py (GPU) and
tests/test_triplane_training_edges_host.py (CPU).  A plain helper module like nerf_baseline_checks.py (not collected, not a conftest).

Inputs with exact taps.  Ray origins are multiples of 2^-5 in [-1, 1], directions multiples of 2^-4 in [-1, 1], depths multiples of 2^-5 in
[2, 6], the box is lo = -4, range = 8 and the projections select axes: ro + rd z is a multiple of 2^-9 below 8, norm_coord gives a multiple
of 2^-11, the pixel coordinate (g + 1)(W - 1) / 2 a multiple of 2^-12 with at most 24 significant bits for W <= 800, and the four bilinear
weights are products of two 12-bit fractions: every intermediate of norm_coord and make_taps_cell is exact in f32, whatever the compiler
contracts.  assert_exact_taps restates both functions in float32 and float64 and compares; the float64 reference then shares the kernel's
weights, cell and clamped neighbours, and needs no tap tolerance on the position planes.

The view plane's coordinates come from atan2f and are not exact: view_tap_error counts the roundings (see there).  The random-coordinate case
counts the roundings of the position taps the same way (pos_tap_error).  Such a tap error e is an absolute error of each of the four weights;
since the hat functions of bilinear interpolation are continuous, a cell that differs between f32 and float64 is covered when the term e |g|
is scattered onto the 4 x 4 texel block around the float64 cell.
"""
from types import SimpleNamespace as NS

import numpy as np
import torch

from nerf_baseline_checks import U, assert_within, bits, gemm_eps

C, HID = 48, 128
NATURAL = 130564
# natural (state-dict) blob offsets, include/nvsr.h nvsr_pack_decoder / csrc/nvsr_common.h
N_DEN_W0, N_DEN_B0, N_DEN_W1, N_HID_STRIDE = 0, 6144, 6272, 16512
N_ALPHA_W, N_ALPHA_B, N_RGB_W0, N_RGB_B0, N_RGB_W1, N_FCRGB_W, N_FCRGB_B = 55808, 55936, 55937, 80513, 80641, 130177, 130561
RECORD_DUMP_ROWS = 32
BL_F16_UP = 3                      # render_bwd_limb.hip: a chain's largest |dL/draw| is scaled into [2^3, 2^4)
ATAN2_ULP = 4.0                    # allowance for atan2f (the device-library documentation on the build machine states no bound)
PAIR_GATE_FLOOR = 2.0 ** -29       # test_pair_forward_matches_the_one_tile_forward: a positive activation below it reads as closed


def gamma(n):
    return n * U / (1 - n * U)


# ---- decoder ----------------------------------------------------------------------------------------------------------------------------

def make_decoder(seed):
    """natural blob: weights N(0, 1) / sqrt(fan-in), biases uniform in +-[0.02, 0.1] (small, non-zero: about half of the gates are open)"""
    rng = np.random.default_rng(seed)
    nat = np.zeros(NATURAL, np.float32)

    def put(off, out, fan):
        nat[off:off + out * fan] = (rng.standard_normal(out * fan) / np.sqrt(fan)).astype(np.float32)
        nat[off + out * fan:off + out * fan + out] = (rng.uniform(0.02, 0.1, out) * np.where(rng.random(out) < 0.5, -1, 1)).astype(np.float32)

    put(N_DEN_W0, HID, C)
    for l in range(3):
        put(N_DEN_W1 + l * N_HID_STRIDE, HID, HID)
    put(N_ALPHA_W, 1, HID)
    put(N_RGB_W0, HID, 4 * C)
    for l in range(3):
        put(N_RGB_W1 + l * N_HID_STRIDE, HID, HID)
    put(N_FCRGB_W, 3, HID)
    return nat


def unpack(nat, device="cpu"):
    """natural blob -> float64 layers: Wd[l] / bd[l], Wr[l] / br[l] (l = 0..3), heads Wa [1, 128] / ba, Wc [3, 128] / bc"""
    t = torch.as_tensor(nat).to(device).double()

    def lin(off, out, fan):
        return t[off:off + out * fan].view(out, fan), t[off + out * fan:off + out * fan + out]

    d = [lin(N_DEN_W0, HID, C)] + [lin(N_DEN_W1 + l * N_HID_STRIDE, HID, HID) for l in range(3)]
    r = [lin(N_RGB_W0, HID, 4 * C)] + [lin(N_RGB_W1 + l * N_HID_STRIDE, HID, HID) for l in range(3)]
    Wa, ba = lin(N_ALPHA_W, 1, HID)
    Wc, bc = lin(N_FCRGB_W, 3, HID)
    return NS(Wd=[w for w, _ in d], bd=[b for _, b in d], Wr=[w for w, _ in r], br=[b for _, b in r], Wa=Wa, ba=ba, Wc=Wc, bc=bc)


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------

PI32 = float(np.float32(np.pi))


def make_scene(sizes):
    """sizes: four (H, W).  box lo = -4, range = 8; view box az in [-pi, pi], el in [-pi/2, pi/2] (f32 values); the position planes look at
    (x, y), (x, z), (y, z)"""
    proj = np.zeros((3, 3, 2), np.float32)
    for d, (a, b) in enumerate(((0, 1), (0, 2), (1, 2))):
        proj[d, a, 0] = 1.0
        proj[d, b, 1] = 1.0
    lo = np.float32([-4, -4, -4, -PI32, -PI32 / 2])
    rng_ = np.float32([8, 8, 8, 2 * PI32, PI32])
    return NS(ph=[int(h) for h, _ in sizes], pw=[int(w) for _, w in sizes], lo=lo, range=rng_, proj=proj.reshape(3, 6))


def make_planes(scene, seed):
    """four channel-last planes [H, W, 48], N(0, 1)"""
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((h, w, C)).astype(np.float32) for h, w in zip(scene.ph, scene.pw)]


def make_rays(N, S, seed, exact=True, sort=True):
    """packed rays [N, 11] and depths [N, S].  exact: the dyadic grid of the module docstring (duplicated depths occur); otherwise ordinary
    random numbers of the same ranges.  Columns 8..10 hold a real unit vector."""
    rng = np.random.default_rng(seed)
    if exact:
        ro = rng.integers(-32, 33, (N, 3)) / 32.0
        rd = rng.integers(-16, 17, (N, 3)) / 16.0
        z = rng.integers(64, 193, (N, S)) / 32.0
    else:
        ro = rng.uniform(-1, 1, (N, 3))
        rd = rng.uniform(-1, 1, (N, 3))
        z = rng.uniform(2, 6, (N, S))
    if sort:
        z = np.sort(z, -1)
    v = rng.standard_normal((N, 3))
    v /= np.linalg.norm(v, axis=-1, keepdims=True)
    rays = np.concatenate([ro, rd, np.tile([2.0, 6.0], (N, 1)), v], -1).astype(np.float32)
    return rays, np.ascontiguousarray(z, dtype=np.float32)


def spread_g_raw(N, S, seed):
    """dL/draw [N, S, 4]: N(0, 1) times 10^U(-4, 4) per point; |dL/dsigma| 2^20 above |dL/drgb| at every third point and the reverse at the
    others that follow them; a few all-zero rows and a few rows with zero rgb and non-zero sigma (pow2_scales' e == 0 branch); the extremes
    on the last sample of the last chunk of the last ray.  Everything stays far inside the f16x2 range (|.| 2^20 1e4 ~ 1e10 scaled per point)."""
    rng = np.random.default_rng(seed)
    P = N * S
    g = rng.standard_normal((P, 4)) * 10.0 ** rng.uniform(-4, 4, (P, 1))
    g[::3, 3] *= 2.0 ** 20
    g[1::3, :3] *= 2.0 ** 20
    if P > 8:
        g[2::7] = 0.0
        g[4::11, :3] = 0.0
    sign = np.where(rng.random(4) < 0.5, -1.0, 1.0)
    g[-1] = sign * [1e-4, 1e-4, 1e-4, 1e4 * 2.0 ** 20]
    if P > 1:
        g[-2] = sign * [1e4, 1e4, 1e4, 1e-4]
    return g.astype(np.float32).reshape(N, S, 4)


# ---- taps: norm_coord + make_taps_cell + view_taps restated (csrc/decode_core.h) --------------------------------------------------------

def _points(rays, z, dt):
    r, zz = rays.astype(dt), z.astype(dt)
    return r[:, None, 0:3] + r[:, None, 3:6] * zz[:, :, None]          # [N, S, 3]: fadd(ro, fmul(rd, z))


def _norm(v, lo, rng_, dt):
    return (dt(2) * (v - dt(lo))) / dt(rng_) - dt(1)


def _cell(gx, gy, H, W, dt):
    """make_taps_cell: -> texel indices [.., 4] (nw, ne, sw, se) and weights [.., 4], pixel coordinates x, y, cell ix, iy"""
    mx, my = dt(W - 1), dt(H - 1)
    hx, hy = mx / dt(2), my / dt(2)
    x = np.minimum(mx, np.maximum((gx + dt(1)) * hx, dt(0)))
    y = np.minimum(my, np.maximum((gy + dt(1)) * hy, dt(0)))
    xw, yn = np.floor(x), np.floor(y)
    w = x - xw
    e = dt(1) - w
    n = y - yn
    s = dt(1) - n
    ix, iy = xw.astype(np.int64), yn.astype(np.int64)
    ix1, iy1 = np.minimum(ix + 1, W - 1), np.minimum(iy + 1, H - 1)
    idx = np.stack([iy * W + ix, iy * W + ix1, iy1 * W + ix, iy1 * W + ix1], -1)
    wt = np.stack([s * e, s * w, n * e, n * w], -1)
    return NS(idx=idx, w=wt, x=x, y=y, ix=ix, iy=iy, fx=w, ex=e, fy=n, ey=s)


def position_taps(rays, z, scene, d, dt=np.float64):
    p = _points(rays, z, dt)
    n = [_norm(p[..., i], scene.lo[i], scene.range[i], dt) for i in range(3)]
    M = scene.proj[d].astype(dt)
    gx = n[0] * M[0] + n[1] * M[2] + n[2] * M[4]
    gy = n[0] * M[1] + n[1] * M[3] + n[2] * M[5]
    t = _cell(gx, gy, scene.ph[d], scene.pw[d], dt)
    t.g = (gx, gy)
    return t


def view_taps(rays, scene, S, dt=np.float64):
    """view_taps on the f32 direction of columns 8..10, broadcast over the S samples of a ray"""
    v = rays[:, 8:11].astype(dt)
    az = np.arctan2(v[:, 1], v[:, 0])
    el = np.arctan2(v[:, 2], np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]))
    t = _cell(_norm(az, scene.lo[3], scene.range[3], dt), _norm(el, scene.lo[4], scene.range[4], dt), scene.ph[3], scene.pw[3], dt)
    for k, a in vars(t).items():
        setattr(t, k, np.repeat(a[:, None], S, 1))
    return t


def assert_exact_taps(rays, z, scene):
    """the f32 restatement of the position taps equals the float64 one: pixel coordinates, fractions, their complements, the four products,
    the cell -> the share of clamped coordinates (on either axis of any plane)"""
    clamped = 0.0
    for d in range(3):
        a, b = position_taps(rays, z, scene, d, np.float32), position_taps(rays, z, scene, d, np.float64)
        for k in ("x", "y", "fx", "ex", "fy", "ey", "w"):
            assert np.array_equal(getattr(a, k).astype(np.float64), getattr(b, k)), "plane %d: %s is not exact in f32" % (d, k)
        assert np.array_equal(a.idx, b.idx)
        for g, m in zip(b.g, (scene.pw[d], scene.ph[d])):
            if m > 1:
                clamped = max(clamped, float((np.abs(g) >= 1).mean()))
    return clamped


def view_tap_error(scene):
    """e_v: the absolute error of one bilinear weight of the view plane against the float64 reference on the same f32 direction, in units of
    u = 2^-24, by counting the roundings of view_taps, norm_coord and make_taps_cell:
        az = atan2f(vy, vx)                  ATAN2_ULP ulp of |az| <= pi: ulp = 2^-22            d_az = 4 ATAN2_ULP u
        r = sqrtf(vx vx + vy vy)             3 roundings under the root (halved) + 1: 2.5 u r
        el = atan2f(vz, r)                   |d el / d r| r = |vz| r / (vz^2 + r^2) <= 1/2, + ATAN2_ULP ulp of |el| <= pi/2 (ulp 2^-23)
                                                                                                  d_el = (1.25 + 2 ATAN2_ULP) u
        g = 2 (a - lo) / range - 1           a - lo rounds once (|.| <= range): 2 u after the scaling; the division (|.| <= 2): 2 u; the
                                             subtraction (|.| <= 1): u                            d_g = 2 d_a / range + 5 u
        x = (g + 1) hx                       g + 1 rounds once (<= 2): 2 u hx; the product (<= W - 1 = 2 hx): 2 u hx
                                                                                                  d_x = hx (d_g + 4 u)
    Clamping is 1-Lipschitz, x - floor(x) is exact; a weight is a product of two hat functions (Lipschitz 1, values <= 1) whose complement
    1 - w and whose product round once each: e_v = d_x + d_y + d_x d_y + 2 u.  A plane of width 1 has hx = 0: no error on that axis."""
    hx, hy = (scene.pw[3] - 1) / 2.0, (scene.ph[3] - 1) / 2.0
    d_az, d_el = 4 * ATAN2_ULP * U, (1.25 + 2 * ATAN2_ULP) * U
    dx = hx * (2 * d_az / float(scene.range[3]) + 9 * U)
    dy = hy * (2 * d_el / float(scene.range[4]) + 9 * U)
    return dx + dy + dx * dy + 2 * U


def pos_tap_error(rays, z, scene, d):
    """the same count for a position plane at ordinary coordinates, per point [N, S]:
        p = ro + rd z                        two roundings: u (|rd z| + |p|)
        g = 2 (p - lo) / range - 1           d_g = 2 (d_p + u |p - lo|) / range + u |g + 1| + u |g|
        (the projection multiplies by 0 and 1 and adds zeros: exact)
        x = (g + 1) hx                       d_x = hx (d_g + u |g + 1|) + u |x|
    e = d_x + d_y + d_x d_y + 2 u, as for the view plane"""
    r, zz = rays.astype(np.float64), z.astype(np.float64)
    p = r[:, None, 0:3] + r[:, None, 3:6] * zz[:, :, None]
    dz = np.abs(r[:, None, 3:6] * zz[:, :, None])
    M = scene.proj[d].reshape(3, 2)
    out = []
    for col, m in ((0, scene.pw[d]), (1, scene.ph[d])):
        i = int(np.argmax(M[:, col]))
        lo, rg, h = float(scene.lo[i]), float(scene.range[i]), (m - 1) / 2.0
        g = 2 * (p[..., i] - lo) / rg - 1
        d_p = U * (dz[..., i] + np.abs(p[..., i]))
        d_g = 2 * (d_p + U * np.abs(p[..., i] - lo)) / rg + U * np.abs(g + 1) + U * np.abs(g)
        out.append(h * (d_g + U * np.abs(g + 1)) + U * np.abs((g + 1) * h))
    return out[0] + out[1] + out[0] * out[1] + 2 * U


def block_indices(t, H, W):
    """the 4 x 4 texel block around the float64 cell: indices [.., 16] and a mask of those inside the plane"""
    dx = np.tile(np.arange(-1, 3), 4)
    dy = np.repeat(np.arange(-1, 3), 4)
    bx, by = t.ix[..., None] + dx, t.iy[..., None] + dy
    ok = (bx >= 0) & (bx < W) & (by >= 0) & (by < H)
    return np.where(ok, by * W + bx, 0), ok


def all_taps(rays, z, scene, exact):
    """per plane: float64 taps (idx, w flattened to [P, 4]), the per-point tap error e [P] (0: exact) and the 4 x 4 block for the planes with e > 0"""
    N, S = z.shape
    out = []
    for d in range(4):
        t = position_taps(rays, z, scene, d) if d < 3 else view_taps(rays, scene, S)
        if d == 3:
            e = np.full((N, S), view_tap_error(scene))
        else:
            e = np.zeros((N, S)) if exact else pos_tap_error(rays, z, scene, d)
        blk, ok = block_indices(t, scene.ph[d], scene.pw[d])
        out.append(NS(idx=t.idx.reshape(-1, 4), w=t.w.reshape(-1, 4), e=e.reshape(-1), blk=blk.reshape(-1, 16), ok=ok.reshape(-1, 16),
                      texels=scene.ph[d] * scene.pw[d]))
    return out


def taps_to(taps, device):
    """numpy taps -> tensors on `device`"""
    T = lambda a: torch.as_tensor(a, device=device)
    return [NS(idx=T(t.idx), w=T(t.w), e=T(t.e), blk=T(t.blk), ok=T(t.ok).double(), texels=t.texels, inexact=bool((t.e > 0).any())) for t in taps]


# ---- the record and the gates (csrc/nvsr_common.h) ---------------------------------------------------------------------------------------

def record_rows(N, S):
    return (N * S + 7) // 8 * 8 + RECORD_DUMP_ROWS


def record_views(rec, N, S):
    """the flat record -> Xd [P, 64], Hd / Gd / Hr / Gr [4, P, 128], Xr [P, 192], g4 [P, 4] (rows < P = N S) and `tail`: the same arrays' rows
    >= P in front of the 32 dump rows, concatenated flat (they must stay unwritten)"""
    P, Pp = N * S, record_rows(N, S)
    o, v, tail = 0, {}, []
    for name, L, cols in (("Xd", 1, 64), ("Hd", 4, HID), ("Gd", 4, HID), ("Xr", 1, 4 * C), ("Hr", 4, HID), ("Gr", 4, HID), ("g4", 1, 4)):
        a = rec[o:o + L * Pp * cols].view(L, Pp, cols)
        o += L * Pp * cols
        v[name] = a[:, :P] if L > 1 else a[0, :P]
        tail.append(a[:, P:Pp - RECORD_DUMP_ROWS].reshape(-1))
    v["tail"] = torch.cat(tail)
    v["floats"] = o
    return NS(**v)


def gate_bit(ib, r):
    return (ib & 1) * 8 + (r >> 1) + 16 * (r & 1)


def gate_words(Hd, Hr):
    """[H > 0] of the eight layers ([4, P, 128] each, density then rgb) -> the gate words [P, 2, 16] (int32) of nvsr_common.h: word
    2 layer + (ib >> 1) of lane half h, bit gate_bit(ib, r) <=> feature 32 ib + (r & 3) + 8 (r >> 2) + 4 h"""
    P = Hd.shape[1]
    H = torch.cat([Hd, Hr], 0) > 0                                      # [8, P, 128]
    words = torch.zeros(P, 2, 16, dtype=torch.int64, device=Hd.device)
    for h in range(2):
        for ib in range(4):
            for r in range(16):
                f = 32 * ib + (r & 3) + 8 * (r >> 2) + 4 * h
                words[:, h, (ib >> 1)::2] |= H[:, :, f].T.long() << gate_bit(ib, r)
    return torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)


def gates_to_masks(gates, P):
    """gate words [P, 2, 16] -> 0 / 1 masks (float64) [8, P, 128]"""
    g = gates.view(P, 2, 16).long() & 0xFFFFFFFF
    m = torch.zeros(8, P, HID, dtype=torch.float64, device=gates.device)
    for h in range(2):
        for ib in range(4):
            for r in range(16):
                f = 32 * ib + (r & 3) + 8 * (r >> 2) + 4 * h
                m[:, :, f] = ((g[:, h, (ib >> 1)::2] >> gate_bit(ib, r)) & 1).T.double()
    return m


# ---- forward ----------------------------------------------------------------------------------------------------------------------------

def blend(planes, taps):
    """float64 bilinear blend of every plane: features [4][P, 48], sum_t |w_t||texel_t| and (inexact planes) sum over the 4 x 4 block of |texel|"""
    f, mag, blk = [], [], []
    for pl, t in zip(planes, taps):
        tex = pl.double().view(-1, C)
        v = tex[t.idx]                                                   # [P, 4, 48]
        f.append((v * t.w[..., None]).sum(1))
        mag.append((v.abs() * t.w[..., None]).sum(1))
        blk.append((tex.abs()[t.blk] * t.ok[..., None]).sum(1) if t.inexact else None)
    return f, mag, blk


def layer_bound(arith, W, x, y):
    """check_forward_layers' bound (nerf_baseline_checks): (e S + floor)(1 + 2^-24) + 2^-24 |y|, S = |x| |W|^T, e = gemm_eps(arith, K);
    f16x2 floor = 2^-29 sum_k |W_k| + 2^-33 sum_k |x_k| (static scales W 2^8 and x 2^4)"""
    prod = gemm_eps(arith, W.shape[1]) * (x.abs() @ W.abs().T)
    if arith == "f16x2":
        prod = prod + 2.0 ** -29 * W.abs().sum(1) + 2.0 ** -33 * x.abs().sum(1, keepdim=True)
    return prod * (1 + U) + U * y.abs()


def check_forward(arith, dec, planes, taps, rec, raw):
    """Every stage of the recording forward from the kernel's own record of its input, in float64 (decode_core.h decode_step, decode_limb.hip
    decode_step_limb):
        Xr = [f0 | f1 | f2 | f_view]       gather24: fma(d, se, fma(c, sw, fma(b, ne, a nw))) -- 4 roundings: gamma_4 sum_t |w_t||texel_t|, and
                                           e sum |texel| over the 4 x 4 block where the weights are inexact (f16x2 puts 2^4 on the weights and
                                           takes it off the recorded row: exact)
        Xd[:, :48] = (f0 + f1 + f2) / 3    from the recorded features: two adds and div3 (correctly rounded): gamma_3 (|f0| + |f1| + |f2|) / 3;
                                           columns 48..63 are zero
        Hd[l], Hr[l]                       relu(W x + b) from the recorded input: layer_bound at K = 48, 128, 192
        raw                                the heads are f32 dot products on the vector unit in every arithmetic (head_dots: 64 fmaf per lane
                                           half, one add of the halves, one add of the bias; f16x2 carries 2^4 on the activations and 2^-4 on
                                           the head weights, exact): gamma_128 sum |w||x| + 2^-24 |y|
    -> {stage: worst err / bound}"""
    rep = {}
    f, mag, blk = blend(planes, taps)
    Xr, Xd = rec.Xr.double(), rec.Xd.double()
    for d in range(4):
        bound = gamma(4) * mag[d]
        if taps[d].inexact:
            bound = bound + taps[d].e[:, None] * blk[d]
            rep["tap share %d" % d] = float((taps[d].e[:, None] * blk[d] / bound.clamp_min(1e-300)).max())
        rep["Xr.%d" % d] = assert_within("Xr plane %d" % d, Xr[:, C * d:C * d + C], f[d], bound)
    fs = [Xr[:, C * d:C * d + C] for d in range(3)]
    rep["Xd"] = assert_within("Xd", Xd[:, :C], (fs[0] + fs[1] + fs[2]) / 3, gamma(3) * (fs[0].abs() + fs[1].abs() + fs[2].abs()) / 3)
    assert bool((bits(rec.Xd[:, C:]) == 0).all()), "Xd columns 48..63 are not zero"
    for name, Ws, bs, X0, H, Wh, bh, out in (("d", dec.Wd, dec.bd, Xd[:, :C], rec.Hd.double(), dec.Wa, dec.ba, raw[:, 3:4].double()),
                                              ("r", dec.Wr, dec.br, Xr, rec.Hr.double(), dec.Wc, dec.bc, raw[:, :3].double())):
        x = X0
        for l in range(4):
            y = x @ Ws[l].T + bs[l]
            rep["H%s%d" % (name, l)] = assert_within("H%s[%d]" % (name, l), H[l], y.clamp_min(0), layer_bound(arith, Ws[l], x, y))
            x = H[l]
        y = x @ Wh.T + bh
        rep["head " + name] = assert_within("head " + name, out, y, gamma(HID) * (x.abs() @ Wh.abs().T) + U * y.abs())
    return rep


# ---- backward ---------------------------------------------------------------------------------------------------------------------------

def pow2_undo(m):
    """render_bwd_limb.hip pow2_scales' undo factor for per-point maxima m (float32) -> float64 2^(eu - 127), eu = (127 for a zero / subnormal
    or non-finite m, else clamp(biased exponent, 1 + UP, 253)) - UP; the chain runs at m / undo in [2^UP, 2^(UP + 1))"""
    e = ((np.ascontiguousarray(m, dtype=np.float32).view(np.uint32) >> 23) & 0xFF).astype(np.int64)
    eu = np.where((e == 0) | (e == 255), 127, np.clip(e, 1 + BL_F16_UP, 253)) - BL_F16_UP
    return np.ldexp(1.0, eu - 127)


def undo_factors(g_raw):
    """-> (un_d, un_r) [P, 1] float64 on g_raw's device; ones outside f16x2"""
    g = g_raw.detach().cpu().numpy().reshape(-1, 4)
    mk = lambda v: torch.as_tensor(pow2_undo(v), device=g_raw.device)[:, None]
    return mk(np.abs(g[:, 3])), mk(np.abs(g[:, :3]).max(1))


def bwd_eps_floor(arith, W, G, un):
    """error of one transposed product y = G W (G [P, K] the gradient of the layer above, W [K, M] = [out, in]) per element:
        gemm_eps(arith, K) |G| |W|
        f16x2 floor: the gradient operand runs at G / un (un: pow2_scales' per-point, per-chain power of two, BL_F16_UP = 3 with its exponent
        clamps); G / un = hi + lo + d with |d| <= 2^-25 where lo is subnormal (2^-22 |G / un| otherwise, inside gemm_eps): 2^-25 un per
        gradient element, times |W|.  The transposed weights are packed UNSCALED: W = hi + lo + d, |d| <= 2^-25 where lo is subnormal
        (|W| < 0.125), times |G|.  The accumulator is unscaled by an exact power of two that rounds only below 2^-126: + 2^-149 un."""
    b = gemm_eps(arith, W.shape[0]) * (G.abs() @ W.abs())
    if arith == "f16x2":
        b = b + 2.0 ** -25 * un * W.abs().sum(0) + 2.0 ** -25 * G.abs().sum(1, keepdim=True) + 2.0 ** -149 * un
    return b


def head_gradients(dec, g, masks, un_d=None, un_r=None):
    """G[3] of both chains in float64 and their bounds: density w_alpha dL/dsigma (one product: 2^-24 |.|), rgb fmaf(w2, g2, fmaf(w1, g1, w0 g0))
    (3 roundings: gamma_3 sum_c |w_c||g_c|); f16x2 multiplies dL/draw by the chain's power of two first and the record row by its inverse:
    exact above 2^-126 (+ 2^-149 un)"""
    Gd3 = masks[3] * (g[:, 3:4] * dec.Wa)
    Gr3 = masks[7] * (g[:, :3] @ dec.Wc)
    Ed3 = masks[3] * (U * Gd3.abs() + (2.0 ** -149 * un_d if un_d is not None else 0.0))
    Er3 = masks[7] * (gamma(3) * (g[:, :3].abs() @ dec.Wc.abs()) + (2.0 ** -149 * un_r if un_r is not None else 0.0))
    return Gd3, Ed3, Gr3, Er3


def check_backward_layers(arith, dec, rec, g_raw, gates):
    """Every transposed layer of the recording backward from the kernel's own record of the gradient above and the gate words it was given
    (bwd_core.h apply_mask; render_bwd.hip, render_bwd_limb.hip):
        g4 = dL/draw                                       bit for bit
        Gd[3] = gate_3 dL/dsigma w_alpha                   head_gradients
        Gd[l] = gate_l (Gd[l + 1] W_{l + 1}), l = 2, 1, 0   bwd_eps_floor at K = 128 with the density chain's un (f16x2); the rgb chain alike
    -> {layer: worst err / bound}"""
    P = g_raw.numel() // 4
    g = g_raw.reshape(P, 4)
    assert torch.equal(bits(rec.g4), bits(g)), "g4 is not dL/draw"
    masks = gates_to_masks(gates, P)
    un_d, un_r = undo_factors(g_raw) if arith == "f16x2" else (None, None)
    Gd3, Ed3, Gr3, Er3 = head_gradients(dec, g.double(), masks, un_d, un_r)
    rep = {}
    for name, G, G3, E3, Ws, m0, un in (("Gd", rec.Gd.double(), Gd3, Ed3, dec.Wd, 0, un_d), ("Gr", rec.Gr.double(), Gr3, Er3, dec.Wr, 4, un_r)):
        rep[name + "3"] = assert_within(name + "[3]", G[3], G3, E3)
        for l in (2, 1, 0):
            y = G[l + 1] @ Ws[l + 1]
            rep["%s%d" % (name, l)] = assert_within("%s[%d]" % (name, l), G[l], masks[m0 + l] * y, bwd_eps_floor(arith, Ws[l + 1], G[l + 1], un))
    return rep


def feature_gradients(arith, dec, Gd0, Gr0, Ed0=None, Er0=None, un_d=None, un_r=None):
    """per-point feature gradients gF[d] [P, 48] in float64 and their bounds from layer 0's gradients (and, E given, their propagated errors):
        gD = (Gd0 W_d0) / 3                                div3 is correctly rounded: + 2^-24 |gD|
        gF_d = gD + Gr0 W_r0[:, 48 d : 48 d + 48]  (d < 3);  gF_3 = Gr0 W_r0[:, 144:192]
    f32 starts the rgb product's accumulator from gD (layer0_T on gF = gD): gD passes through that product's roundings too, e |gD|; the limb
    kernels add it once (fma(P, un_r, gD) or a + d): 2^-24 |gF|.  So E = (2 e + 2 u) A_d + (e + u) A_r + floors, A = |G||W| (A_d with the 1/3),
    and with incoming errors E0: |W|^T E0 enters A and the value."""
    z = lambda G: torch.zeros_like(G)
    Ed0 = z(Gd0) if Ed0 is None else Ed0
    Er0 = z(Gr0) if Er0 is None else Er0
    e = gemm_eps(arith, HID)
    Wd0, Wr0 = dec.Wd[0], dec.Wr[0]
    gD = (Gd0 @ Wd0) / 3
    Pd = (bwd_eps_floor(arith, Wd0, Gd0.abs() + Ed0, un_d) + Ed0 @ Wd0.abs()) / 3
    A_d = ((Gd0.abs() + Ed0) @ Wd0.abs()) / 3
    gF, E = [], []
    for d in range(4):
        Wp = Wr0[:, C * d:C * d + C]
        A_r = (Gr0.abs() + Er0) @ Wp.abs()
        v = Gr0 @ Wp
        Er = bwd_eps_floor(arith, Wp, Gr0.abs() + Er0, un_r) + Er0 @ Wp.abs()
        if d < 3:
            gF.append(gD + v)
            E.append(Pd + Er + (e + 2 * U) * A_d + U * A_r)
        else:
            gF.append(v)
            E.append(Er + U * A_r)
    return gF, E


def chain_from_gates(arith, dec, g_raw, gates):
    """Kernels without a record: the float64 chain from dL/draw and the gate words, with the error bound propagated layer by layer:
    E_below = gate (|W|^T E_above + eps |W|^T (|G| + E_above) + floor)  ->  (Gd0, Ed0, Gr0, Er0, un_d, un_r)"""
    P = g_raw.numel() // 4
    masks = gates_to_masks(gates, P)
    un_d, un_r = undo_factors(g_raw) if arith == "f16x2" else (None, None)
    Gd, Ed, Gr, Er = head_gradients(dec, g_raw.reshape(P, 4).double(), masks, un_d, un_r)
    for l in (2, 1, 0):
        Ed = masks[l] * (Ed @ dec.Wd[l + 1].abs() + bwd_eps_floor(arith, dec.Wd[l + 1], Gd.abs() + Ed, un_d))
        Gd = masks[l] * (Gd @ dec.Wd[l + 1])
        Er = masks[4 + l] * (Er @ dec.Wr[l + 1].abs() + bwd_eps_floor(arith, dec.Wr[l + 1], Gr.abs() + Er, un_r))
        Gr = masks[4 + l] * (Gr @ dec.Wr[l + 1])
    return Gd, Ed, Gr, Er, un_d, un_r


def scatter_reference(initial, tap, gF, E):
    """one plane, per texel and channel, in float64: ref = initial + sum_p w_tap(p) gF(p) and the bound
        gamma_(n + 2) (|initial| + sum |w gF|) + sum w E + (inexact taps) sum over the 4 x 4 block of e |gF| (+ e E)
    over the n contributions to the texel -- each contribution is one rounded product (or an fma into a partial sum) and takes part in at most
    n additions, in any order of atomics and partial sums; a view-plane row summed per ray or per chunk first passes through no more additions
    than its points.  -> ref, bound, touched (texels inside the reference's footprint, the blocks included), the tap term's largest share"""
    T = tap.texels
    init = initial.double().view(T, C)
    dev = init.device
    idx = tap.idx.reshape(-1)
    wg = (tap.w[..., None] * gF[:, None, :]).reshape(-1, C)
    ref = init.clone().index_add_(0, idx, wg)
    mag = init.abs().index_add_(0, idx, wg.abs())
    n = torch.zeros(T, dtype=torch.float64, device=dev).index_add_(0, idx, (tap.w.reshape(-1) != 0).double())
    err = torch.zeros_like(init).index_add_(0, idx, (tap.w[..., None] * E[:, None, :]).reshape(-1, C))
    touched = torch.zeros(T, dtype=torch.bool, device=dev)
    touched[idx[tap.w.reshape(-1) != 0]] = True
    g = gamma(n + 2)[:, None]
    bound = g * mag + err * (1 + g)
    share = 0.0
    if tap.inexact:
        te = (tap.ok[..., None] * (tap.e[:, None] * (gF.abs() + E))[:, None, :]).reshape(-1, C)
        extra = torch.zeros_like(init).index_add_(0, tap.blk.reshape(-1), te)
        nb = torch.zeros(T, dtype=torch.float64, device=dev).index_add_(0, tap.blk.reshape(-1), tap.ok.reshape(-1))
        g = gamma(nb + 2)[:, None]                                    # (a flipped cell may add contributions to a neighbour texel)
        bound = g * mag + err * (1 + g) + extra * (1 + g)
        touched[tap.blk.reshape(-1)[tap.ok.reshape(-1) > 0]] = True
        share = float((extra / bound.clamp_min(1e-300)).max())
    return ref, bound, touched, share



def check_plane(name, got, initial, tap, gF, E):
    """a gradient plane after the call against scatter_reference; texels outside the footprint keep their initial bits -> worst err / bound, tap share"""
    ref, bound, touched, share = scatter_reference(initial, tap, gF, E)
    g = got.view(tap.texels, C)
    same = bits(g[~touched]) == bits(initial.view(tap.texels, C)[~touched])
    assert bool(same.all()), "%s: %d words outside the footprint changed" % (name, int((~same).sum()))
    return assert_within(name, g.double()[touched], ref[touched], bound[touched]), share


# ---- the whole model in float64 (host test: autograd against the manual chain) -----------------------------------------------------------

def forward64(dec, planes, rays, z, scene):
    """float64 forward with grid_sample(align_corners=True, padding_mode='border') on the reference's [C, H, W] planes -> raw [P, 4] and the
    post-ReLU activations (Hd, Hr) [4, P, 128]"""
    import torch.nn.functional as F
    N, S = z.shape
    r, zz = torch.as_tensor(rays).double(), torch.as_tensor(z).double()
    p = (r[:, None, 0:3] + r[:, None, 3:6] * zz[:, :, None]).reshape(-1, 3)
    lo, rg = torch.as_tensor(scene.lo).double(), torch.as_tensor(scene.range).double()
    n = 2 * (p - lo[:3]) / rg[:3] - 1
    v = r[:, 8:11]
    az, el = torch.atan2(v[:, 1], v[:, 0]), torch.atan2(v[:, 2], torch.sqrt(v[:, 0] ** 2 + v[:, 1] ** 2))
    gv = torch.stack([2 * (az - lo[3]) / rg[3] - 1, 2 * (el - lo[4]) / rg[4] - 1], -1).repeat_interleave(S, 0)
    f = []
    for d in range(4):
        g = n @ torch.as_tensor(scene.proj[d].reshape(3, 2)).double() if d < 3 else gv
        img = planes[d].permute(2, 0, 1)[None]
        f.append(F.grid_sample(img, g[None, None], mode="bilinear", padding_mode="border", align_corners=True)[0, :, 0].T)
    Hd, Hr = [], []
    x = (f[0] + f[1] + f[2]) / 3
    for l in range(4):
        x = torch.relu(x @ dec.Wd[l].T + dec.bd[l])
        Hd.append(x)
    sigma = x @ dec.Wa.T + dec.ba
    x = torch.cat(f, 1)
    for l in range(4):
        x = torch.relu(x @ dec.Wr[l].T + dec.br[l])
        Hr.append(x)
    return torch.cat([x @ dec.Wc.T + dec.bc, sigma], 1), torch.stack(Hd), torch.stack(Hr)


# ---- the cases (shared by the GPU tests and the CPU check of their inputs) ---------------------------------------------------------------

SIZES = ([(9, 12), (40, 56), (17, 17), (9, 9)],         # non-square position planes; view planes of at most 9 x 9
         [(1, 7), (12, 9), (56, 40), (2, 3)],           # a plane with a single row
         [(17, 17), (3, 200), (7, 12), (1, 1)])         # a single view texel
RANDOM_SIZES = [(200, 200), (200, 200), (200, 200), (9, 9)]

RECORD_SHAPES = [(1, 1), (1, 31), (1, 32), (33, 1),                                     # below one tile, one tile
                 (1, 33), (3, 33), (5, 37), (7, 65), (3, 64), (9, 97), (2, 96),         # partial last chunk; 2, 6, 10, 21, 6, 36, 6 wave tiles
                 (127, 3), (128, 3), (129, 3), (255, 3), (256, 3), (257, 3),            # f32 ray blocks of 128 and 256
                 (5, 129), (3, 160), (2, 193), (4, 128)]                                # f16x2 without a record: the tile-pair forward
UNSORTED = (5, 37)
# past the grid caps (2048 limb workgroups of 4 wave tiles, 1024 f32 workgroups); without a record
CAP_SHAPES = {"limb": [(8195, 1), (4098, 33)], "f32_gates": [(257, 513)], "f32_recompute": [(129, 513)]}   # (BPTS = 128: 2 x 513 tiles)
RANDOM_SHAPE = (257, 70)


def cases():
    out = []
    for i, (N, S) in enumerate(RECORD_SHAPES):
        out.append(NS(N=N, S=S, sizes=SIZES[i % 3], seed=100 + i, exact=True, sort=(N, S) != UNSORTED, record=True, kind="record", null=i % 4))
    out.append(NS(N=RANDOM_SHAPE[0], S=RANDOM_SHAPE[1], sizes=RANDOM_SIZES, seed=77, exact=False, sort=True, record=True, kind="random", null=1))
    i = 0
    for kind, shapes in CAP_SHAPES.items():
        for N, S in shapes:
            # (the largest planes of SIZES: 10^5 points on a plane of one or seven texels serialise their atomics, in the kernel and in the reference)
            out.append(NS(N=N, S=S, sizes=SIZES[0], seed=200 + i, exact=True, sort=True, record=False, kind=kind, null=None))
            i += 1
    return out


def case_id(c):
    return "%s-%dx%d" % (c.kind, c.N, c.S)


def case_inputs(c):
    """-> scene, planes (numpy, channel-last), rays [N, 11], z [N, S], dL/draw [N, S, 4]; exact cases assert their taps exact"""
    scene = make_scene(c.sizes)
    rays, z = make_rays(c.N, c.S, c.seed, exact=c.exact, sort=c.sort)
    if c.exact:
        assert_exact_taps(rays, z, scene)
    return scene, make_planes(scene, c.seed + 1), rays, z, spread_g_raw(c.N, c.S, c.seed + 2)
