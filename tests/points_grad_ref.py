"""Restatements behind tests/test_points_grad_host.py (CPU) and tests/test_points_grad.py (GPU), no GPU needed:

  points_grad_f32   numpy float32 transcription of nvsr_triplane_points_grad in the order include/nvsr.h states: every numpy operation on float32
                    arrays is one correctly rounded float32 operation, like the kernel's __f*_rn (the library is built with -ffp-contract=off)
  points_grad_f64   the same expressions in float64 FROM THE FLOAT32 PIXEL COORDINATES ON (the point at which the kernel evaluates the slope is the
                    forward's float32 coordinate; w = xc - floor(xc) is exact), and A: the same expressions with every product and every
                    difference of texels replaced by its absolute value -- the kernel-alone bound is K * 2^-24 * A per component
  model64           the whole model call in float64 with autograd (torch grid_sample + linear layers, as
                    test_hip_parity.py::test_model_call_is_differentiable_vs_torch_reference states it in float32)

K, the number of roundings on the longest path of the stated order:
  d_points   1 (e = 1 - w) + 1 (T01 - T00) + 1 (s .) + 1 (+ n .) + 1 (row[c] .) + 3 (four channels of a lane) + 4 (tree over 16 lanes) + 1 (hx .)
             + 1 (M .) + 1 (M Gx + M Gy) + 2 (three planes onto +0: the first addition is exact) + 1 (/ range; 2 . is exact)          = 18
  d_viewdir  the slope as above up to hx . : 13, + 1 (/ range) = 14 for d_az, d_el;  q = vx vx + vy vy carries 2, h = q + vz vz 3, r = sqrt(q) 2:
             a = d_az / q: 17;  b = d_el / h: 18;  c = (b vz) / r: 18 + 1 + 1 + 2 = 22;  vx c: 23;  the final subtraction: 24            = 24"""
import numpy as np
import torch
import torch.nn.functional as F

K_POINTS, K_VIEW = 18, 24
U = 2.0 ** -24
f32 = np.float32


def load_case():
    """g23_points_grad.npz + the decoder it was made with (g11's coarse.* overwritten by g23's entries) -> (g, state dict, planes, rot)"""
    from conftest import load_golden
    g, g11 = load_golden("g23_points_grad.npz"), load_golden("g11_grads.npz")
    vals = [np.asarray(g11[k], dtype=np.float64).reshape(-1) for k in sorted(g11) if k.startswith(("coarse.", "fine."))]
    flat = np.concatenate(vals)
    assert np.array_equal(np.array([flat.sum(), np.square(flat).sum(), flat.size]), g["g11_decoders"]), "g11_grads.npz changed: regenerate g23"
    sd = {k[len("coarse."):]: v for k, v in g11.items() if k.startswith("coarse.")}
    sd.update({k[len("coarse."):]: v for k, v in g.items() if k.startswith("coarse.")})
    planes = [g["plane%d" % d] for d in range(4)]
    eye = np.eye(3, dtype=np.float32)
    rot = [eye[:, 1:], eye[:, [1, 0, 2]][:, 1:], eye[:, [2, 0, 1]][:, 1:]]          # CoordProjector(3): the shipped frames, columns 1..2
    assert all(np.array_equal(sd["coord_projector.rot_mats_NON_LEARNED.%d" % d][:, 1:], rot[d]) for d in range(3))
    return g, sd, planes, rot


def scene_consts(box, rot):
    """lo[5], range[5] (the subtraction in double, then cast: TwoDimPlanesModel.scene_args), proj[3][6] = M[k][c] row-major"""
    box = np.asarray(box, dtype=np.float64)
    return box[0].astype(f32), (box[1] - box[0]).astype(f32), [np.asarray(r, dtype=f32).reshape(6) for r in rot]


def channel_last(plane):
    return np.ascontiguousarray(np.asarray(plane, dtype=f32).reshape(plane.shape[-3:]).transpose(1, 2, 0))


def as_rays(x, direction=None, z=None):
    """points [P,6] as one-sample rays (origin = point, direction 0, depth 0), or origins + directions with depths z [N,S]"""
    P = x.shape[0]
    rays = np.zeros((P, 11), f32)
    rays[:, 0:3], rays[:, 8:11] = x[:, 0:3], x[:, 3:6]
    if direction is not None:
        rays[:, 3:6] = direction
    return rays, (np.zeros((P, 1), f32) if z is None else np.asarray(z, f32))


# ---- the cell ---------------------------------------------------------------------------------------------------------------------------
def _cell(plane, gx, gy):
    """make_taps_cell's cell for float32 grid coordinates: pixel coordinates, fractions and the four texel rows [M,48]"""
    H, W = plane.shape[:2]
    mx, my = f32(W - 1), f32(H - 1)
    hx, hy = mx / f32(2), my / f32(2)
    x, y = (gx + f32(1)) * hx, (gy + f32(1)) * hy
    xc = np.minimum(mx, np.where(np.isnan(x), f32(0), np.maximum(x, f32(0))))       # fmaxf(NaN, 0) = 0
    yc = np.minimum(my, np.where(np.isnan(y), f32(0), np.maximum(y, f32(0))))
    xw, yn = np.floor(xc), np.floor(yc)
    w, n = xc - xw, yc - yn
    ix, iy = xw.astype(np.int64), yn.astype(np.int64)
    ix1, iy1 = np.minimum(ix + 1, W - 1), np.minimum(iy + 1, H - 1)
    return dict(x=x, y=y, mx=mx, my=my, hx=hx, hy=hy, w=w, n=n, T00=plane[iy, ix], T01=plane[iy, ix1], T10=plane[iy1, ix], T11=plane[iy1, ix1])


def _tree16(p):
    """[M,48] products -> [M]: four channels per lane left to right, lanes 12..15 +0, then the balanced tree over neighbouring lanes"""
    a = p.reshape(p.shape[0], 12, 4)
    a = ((a[:, :, 0] + a[:, :, 1]) + a[:, :, 2]) + a[:, :, 3]
    a = np.concatenate([a, np.zeros((a.shape[0], 4), f32)], 1)
    while a.shape[1] > 1:
        a = a[:, 0::2] + a[:, 1::2]
    return a[:, 0]


def slope_f32(plane, gx, gy, row):
    c = _cell(plane, gx, gy)
    w, n = c["w"][:, None], c["n"][:, None]
    e, s = f32(1) - w, f32(1) - n
    dx = s * (c["T01"] - c["T00"]) + n * (c["T11"] - c["T10"])
    dy = e * (c["T10"] - c["T00"]) + w * (c["T11"] - c["T01"])
    Ax, Ay = _tree16(row * dx), _tree16(row * dy)
    Gx = np.where((c["x"] <= 0) | (c["x"] >= c["mx"]), f32(0), c["hx"] * Ax)
    Gy = np.where((c["y"] <= 0) | (c["y"] >= c["my"]), f32(0), c["hy"] * Ay)
    return Gx.astype(f32), Gy.astype(f32)


def slope_f64(plane, gx, gy, row, absolute):
    c = _cell(plane, gx, gy)
    d = np.float64
    w, n = c["w"].astype(d)[:, None], c["n"].astype(d)[:, None]
    T = {k: c[k].astype(d) for k in ("T00", "T01", "T10", "T11")}
    fix = np.abs if absolute else (lambda v: v)
    row = fix(row.astype(d))
    dx = (1 - n) * fix(T["T01"] - T["T00"]) + n * fix(T["T11"] - T["T10"])
    dy = (1 - w) * fix(T["T10"] - T["T00"]) + w * fix(T["T11"] - T["T01"])
    Gx = np.where((c["x"] <= 0) | (c["x"] >= c["mx"]), 0.0, d(c["hx"]) * (row * dx).sum(1))
    Gy = np.where((c["y"] <= 0) | (c["y"] >= c["my"]), 0.0, d(c["hy"]) * (row * dy).sum(1))
    return Gx, Gy


# ---- positions --------------------------------------------------------------------------------------------------------------------------
def _norm_pos(consts, rays, z):
    lo, rng, _ = consts
    N, S = z.shape
    ray = np.repeat(np.arange(N), S)
    zz = z.reshape(-1)
    p = [rays[ray, k] + rays[ray, 3 + k] * zz for k in range(3)]
    return p, [(f32(2) * (p[k] - lo[k])) / rng[k] - f32(1) for k in range(3)]


def _grid_pos(n, P):
    return (n[0] * P[0] + n[1] * P[2]) + n[2] * P[4], (n[0] * P[1] + n[1] * P[3]) + n[2] * P[5]


def points_grad_f32(planes_cl, consts, rays, z, rows, view_rows, az_el=None):
    """-> (d_points [N*S,3] or None when rows is None, d_viewdir [N,3]); rows: three [N*S,48] arrays or None entries; view_rows [N,48] or None.
    az_el: the float32 (az, el) of every ray as the DEVICE's atan2f gives them (default: numpy's arctan2 in float32, which need not agree
    with it in the last bit)"""
    lo, rng, proj = consts
    d_points = None
    if rows is not None:
        p, n = _norm_pos(consts, rays, z)
        dn = [np.zeros(p[0].shape, f32) for _ in range(3)]
        for d in range(3):
            if rows[d] is None:
                continue
            P = proj[d]
            Gx, Gy = slope_f32(planes_cl[d], *_grid_pos(n, P), rows[d])
            for k in range(3):
                dn[k] = dn[k] + (P[2 * k] * Gx + P[2 * k + 1] * Gy)
        d_points = np.stack([(f32(2) * dn[k]) / rng[k] for k in range(3)], 1)
        d_points[np.isnan(p[0]) | np.isnan(p[1]) | np.isnan(p[2])] = np.nan
    vx, vy, vz = rays[:, 8], rays[:, 9], rays[:, 10]
    with np.errstate(all="ignore"):
        q = vx * vx + vy * vy
        r = np.sqrt(q)
        Gx = Gy = np.zeros(vx.shape, f32)
        if view_rows is not None:
            az, el = (np.arctan2(vy, vx).astype(f32), np.arctan2(vz, r).astype(f32)) if az_el is None else az_el
            Gx, Gy = slope_f32(planes_cl[3], (f32(2) * (az - lo[3])) / rng[3] - f32(1), (f32(2) * (el - lo[4])) / rng[4] - f32(1), view_rows)
        d_az, d_el = (f32(2) * Gx) / rng[3], (f32(2) * Gy) / rng[4]
        h = q + vz * vz
        a, b = d_az / q, d_el / h
        c = (b * vz) / r
        d_view = np.stack([(-vy) * a - vx * c, vx * a - vy * c, r * b], 1).astype(f32)
    d_view[np.isnan(vx) | np.isnan(vy) | np.isnan(vz)] = np.nan
    return d_points, d_view


def points_grad_f64(planes_cl, consts, rays, z, rows, view_rows, az_el=None, absolute=False):
    """the float64 value of the same expressions (absolute=False) or the magnitude A of the bound (absolute=True); same arguments and results
    as points_grad_f32.  The float32 pixel coordinates are the kernel's (see the module docstring)."""
    lo, rng, proj = consts
    dd = np.float64
    fix = np.abs if absolute else (lambda v: v)
    d_points = None
    if rows is not None:
        p, n = _norm_pos(consts, rays, z)
        dn = [np.zeros(p[0].shape, dd) for _ in range(3)]
        for d in range(3):
            if rows[d] is None:
                continue
            P = fix(proj[d].astype(dd))
            Gx, Gy = slope_f64(planes_cl[d], *_grid_pos(n, proj[d]), rows[d], absolute)
            for k in range(3):
                dn[k] = dn[k] + (P[2 * k] * Gx + P[2 * k + 1] * Gy)
        d_points = np.stack([2 * dn[k] / dd(rng[k]) for k in range(3)], 1)
        d_points[np.isnan(p[0]) | np.isnan(p[1]) | np.isnan(p[2])] = np.nan
    vx, vy, vz = (rays[:, 8 + k].astype(dd) for k in range(3))
    with np.errstate(all="ignore"):
        q = vx * vx + vy * vy
        r = np.sqrt(q)
        Gx = Gy = np.zeros(vx.shape, dd)
        if view_rows is not None:
            r32 = np.sqrt(rays[:, 8] * rays[:, 8] + rays[:, 9] * rays[:, 9])
            az, el = (np.arctan2(rays[:, 9], rays[:, 8]).astype(f32), np.arctan2(rays[:, 10], r32).astype(f32)) if az_el is None else az_el
            Gx, Gy = slope_f64(planes_cl[3], (f32(2) * (az - lo[3])) / rng[3] - f32(1), (f32(2) * (el - lo[4])) / rng[4] - f32(1), view_rows, absolute)
        d_az, d_el = 2 * Gx / dd(rng[3]), 2 * Gy / dd(rng[4])
        h = q + vz * vz
        a, b = d_az / q, d_el / h
        c = b * fix(vz) / r
        if absolute:
            d_view = np.stack([np.abs(vy) * a + np.abs(vx) * c, np.abs(vx) * a + np.abs(vy) * c, r * b], 1)
        else:
            d_view = np.stack([-vy * a - vx * c, vx * a - vy * c, r * b], 1)
    d_view[np.isnan(vx) | np.isnan(vy) | np.isnan(vz)] = np.nan
    return d_points, d_view


def assert_within_bound(got, planes_cl, consts, rays, z, rows, view_rows, az_el=None):
    """got = (d_points, d_viewdir) float32 against float64: |got - f64| <= K 2^-24 A per component over the finite rows; -> the largest ratio of
    error to bound (points, view)"""
    want = points_grad_f64(planes_cl, consts, rays, z, rows, view_rows, az_el)
    mag = points_grad_f64(planes_cl, consts, rays, z, rows, view_rows, az_el, absolute=True)
    worst = []
    for g, w, A, K, name in zip(got, want, mag, (K_POINTS, K_VIEW), ("d_points", "d_viewdir")):
        if g is None:
            worst.append(0.0)
            continue
        ok = np.isfinite(w).all(1)
        assert np.array_equal(np.isnan(g).all(1), ~ok) and np.isfinite(g[ok]).all(), name
        err, bound = np.abs(g[ok].astype(np.float64) - w[ok]), K * U * A[ok]
        assert (err <= bound).all(), (name, float((err / np.maximum(bound, 1e-300)).max()))
        worst.append(float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0)
    return worst


# ---- the whole model call in float64 ------------------------------------------------------------------------------------------------
DEC_KEYS = ["density_dec.0.%d" % i for i in range(4)] + ["fc_alpha.0"] + ["rgb_dec.0.%d" % i for i in range(4)] + ["fc_rgb.0"]


def model64(sd, planes, box, rot, x, g_out=None):
    """TwoDimPlanesModel.forward (the shipped geometry) on x [P,6] in float64 on the CPU.  -> dict(out [P,4]); with g_out the gradients of
    (out * g_out).sum(): x_grad [P,6], planes (four arrays shaped like `planes`), decoder (the natural blob's order: weight, bias per layer
    of DEC_KEYS), rows (dL/d feature [P,48] of the four planes)"""
    d = torch.float64
    pl = [torch.tensor(np.asarray(p), dtype=d).reshape(1, *p.shape[-3:]).requires_grad_(True) for p in planes]
    w = {k + "." + leaf: torch.tensor(sd[k + "." + leaf], dtype=d).requires_grad_(True) for k in DEC_KEYS for leaf in ("weight", "bias")}
    xt = torch.tensor(np.asarray(x), dtype=d).requires_grad_(True)
    P = xt.shape[0]
    boxt = torch.tensor(np.asarray(box), dtype=d)
    az = torch.atan2(xt[:, 4], xt[:, 3])
    el = torch.atan2(xt[:, 5], torch.sqrt(xt[:, 3] ** 2 + xt[:, 4] ** 2))
    x5 = torch.cat([xt[:, :3], az[:, None], el[:, None]], -1)
    n5 = 2 * (x5 - boxt[0]) / (boxt[1] - boxt[0]) - 1
    feats = []
    for k in range(3):
        grid = (n5[:, :3] @ torch.tensor(np.asarray(rot[k]), dtype=d)).reshape(1, P, 1, 2)
        feats.append(F.grid_sample(pl[k], grid, mode="bilinear", align_corners=True, padding_mode="border")[0, :, :, 0].t())
    feats.append(F.grid_sample(pl[3], n5[:, 3:].reshape(1, P, 1, 2), mode="bilinear", align_corners=True, padding_mode="border")[0, :, :, 0].t())
    for f in feats:
        f.retain_grad()
    hden = torch.stack(feats[:3], 0).mean(0)
    for l in range(4):
        hden = torch.relu(F.linear(hden, w["density_dec.0.%d.weight" % l], w["density_dec.0.%d.bias" % l]))
    sigma = F.linear(hden, w["fc_alpha.0.weight"], w["fc_alpha.0.bias"])
    hrgb = torch.cat(feats, -1)
    for l in range(4):
        hrgb = torch.relu(F.linear(hrgb, w["rgb_dec.0.%d.weight" % l], w["rgb_dec.0.%d.bias" % l]))
    out = torch.cat([F.linear(hrgb, w["fc_rgb.0.weight"], w["fc_rgb.0.bias"]), sigma], -1)
    res = dict(out=out.detach().numpy())
    if g_out is not None:
        (out * torch.tensor(np.asarray(g_out), dtype=d)).sum().backward()
        res.update(x_grad=xt.grad.numpy(), planes=[p.grad.numpy().reshape(np.asarray(q).shape) for p, q in zip(pl, planes)],
                   decoder=np.concatenate([w[k + "." + leaf].grad.numpy().reshape(-1) for k in DEC_KEYS for leaf in ("weight", "bias")]),
                   rows=[f.grad.numpy() for f in feats])
    return res


def rel_l2(got, want):
    """relative L2 error over the rows of `want` that are finite"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    ok = np.isfinite(want).reshape(want.shape[0], -1).all(1)
    return float(np.linalg.norm(got[ok] - want[ok]) / np.linalg.norm(want[ok]))
