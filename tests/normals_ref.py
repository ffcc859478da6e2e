"""Restatements behind tests/test_normals_host.py (CPU) and tests/test_normals.py (GPU), no GPU needed:

  live_ray_points_f32    numpy float32 transcription of nvsr_live_ray_points (include/nvsr.h, "surface normals")
  normals_composite_f32  numpy float32 transcription of nvsr_normals_composite: the slope is points_grad_ref.points_grad_f32 on the one-sample
                         rays (the kernels share their device functions, the transcriptions share this one), then the normalisation and the
                         left fold per ray, one float32 operation each
  normals_composite_f64  the same expressions in float64 from the float32 pixel coordinates on (points_grad_ref.points_grad_f64), and the
                         magnitude A of the bound
  normals_exact64        everything in float64, the pixel coordinates included: what reproduces the golden the upstream code wrote

The bound, per ray and component k, T = the number of live samples of the ray, u = 2^-24:  |got - f64| <= K(T) u A_k,  K(T) = 18 + 4 + 2 T.
  g      points_grad's 18 roundings against ITS magnitude A^g (points_grad_ref: every product and texel difference by absolute value): an
         ABSOLUTE error 18 u A^g_j per component, not relative to g_j (the slope cancels).  Through n = -g / |g| to first order:
         |dn_k| <= (dg_k + |n_k| sum_j |n_j| dg_j) / r, so the magnitude of a normal is G_k = (A^g_k + |n_k| sum_j |n_j| A^g_j) / r >= |n_k|.
  4      the normalisation's own roundings, relative to |n_k| <= G_k: q = (g0 g0 + g1 g1) + g2 g2 is a sum of positive terms, one rounding per
         product and two additions: 3; the square root halves them and adds its own: 2.5; the division: 3.5; rounded up (the half left over
         covers the second-order terms of the first-order step above).
  2 T    per term of the fold one rounding of w n_k and one of the addition, the latter relative to a partial sum that the sum of the
         magnitudes bounds.
  A_k = |normal before the call| + sum over the ray's live samples of |w| G_k;  a sample with q == 0 has n = 0 exactly and adds nothing."""
import numpy as np

import points_grad_ref as R

f32 = np.float32
U = R.U
K_GRAD, K_NORMALISE = R.K_POINTS, 4


def K(T):
    return K_GRAD + K_NORMALISE + 2 * np.asarray(T)


def live_list(weights):
    """nvsr_generic_live_list: ascending flat positions p with not (w[p] == 0); NaN is live"""
    w = np.asarray(weights).reshape(-1)
    return np.nonzero(~(w == 0))[0].astype(np.int32)


def live_ray_points_f32(index, rays, z):
    N, S = z.shape
    index = np.asarray(index, np.int64)
    out = np.zeros((index.size, 11), f32)
    ok = (index >= 0) & (index < N * S)
    p = index[ok]
    ray = p // S
    zc = z.reshape(-1)[p]
    for k in range(3):
        out[ok, k] = rays[ray, k] + rays[ray, 3 + k] * zc
    out[ok, 8:11] = rays[ray, 8:11]
    return out


def _runs(index, N, S):
    """[(ray, first entry, one past the last)] of the rays with a non-empty run in the ascending list"""
    index = np.asarray(index, np.int64)
    lo = np.searchsorted(index, np.arange(N) * S, side="left")
    hi = np.searchsorted(index, (np.arange(N) + 1) * S, side="left")
    return [(r, int(lo[r]), int(hi[r])) for r in range(N) if lo[r] < hi[r]]


def normals_composite_f32(planes_cl, consts, index, live_rays, rows, weights, normal):
    """-> the new normal [N,3] (float32; `normal` is what the call accumulates into and is left unchanged here)"""
    N, S = weights.shape
    out = np.array(normal, f32, copy=True)
    M = len(index)
    if M == 0 or N == 0:
        return out
    with np.errstate(all="ignore"):
        g = R.points_grad_f32(planes_cl, consts, live_rays, np.zeros((M, 1), f32), rows, None)[0]
        q = (g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]
        r = np.sqrt(q)
        n = np.where((q == 0)[:, None], f32(0), -(g / r[:, None])).astype(f32)
        w = weights.reshape(-1)
        for ray, a, b in _runs(index, N, S):
            for i in range(a, b):
                out[ray] = out[ray] + w[index[i]] * n[i]
    return out


def normals_composite_f64(planes_cl, consts, index, live_rays, rows, weights, normal):
    """-> (value [N,3] float64, magnitude A [N,3], T [N] live samples per ray) of the same expressions"""
    N, S = weights.shape
    val = np.array(normal, np.float64, copy=True)
    A = np.abs(val)
    T = np.zeros(N, np.int64)
    M = len(index)
    if M == 0 or N == 0:
        return val, A, T
    z0 = np.zeros((M, 1), f32)
    with np.errstate(all="ignore"):
        g = R.points_grad_f64(planes_cl, consts, live_rays, z0, rows, None)[0]
        Ag = R.points_grad_f64(planes_cl, consts, live_rays, z0, rows, None, absolute=True)[0]
        q = (g * g).sum(1)
        r = np.sqrt(q)[:, None]
        flat = (q == 0)[:, None]
        n = np.where(flat, 0.0, -g / r)
        G = np.where(flat, 0.0, (Ag + np.abs(n) * (np.abs(n) * Ag).sum(1, keepdims=True)) / r)
        w = weights.reshape(-1).astype(np.float64)
        for ray, a, b in _runs(index, N, S):
            wi = w[np.asarray(index[a:b], np.int64)][:, None]
            val[ray] += (wi * n[a:b]).sum(0)
            A[ray] += (np.abs(wi) * G[a:b]).sum(0)
            T[ray] = b - a
    return val, A, T


def assert_within_bound(got, planes_cl, consts, index, live_rays, rows, weights, normal):
    """got [N,3] float32 against float64: |got - f64| <= K(T) 2^-24 A per component over the rays whose float64 value is finite, NaN rows where
    it is not; -> the largest ratio of error to bound"""
    want, A, T = normals_composite_f64(planes_cl, consts, index, live_rays, rows, weights, normal)
    ok = np.isfinite(want).all(1)
    assert np.array_equal(np.isnan(got).any(1), ~ok) and np.isfinite(got[ok]).all()
    err, bound = np.abs(got[ok].astype(np.float64) - want[ok]), (K(T)[ok, None] * U) * A[ok]
    assert (err <= bound).all(), float((err / np.maximum(bound, 1e-300)).max())
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


# ---- everything in float64 ------------------------------------------------------------------------------------------------------------
def slope_exact64(plane, gx, gy, row):
    """points_grad_ref.slope_f64 with the pixel coordinates in float64 too: plane [H,W,48], gx, gy [M], row [M,48] -> (Gx, Gy)"""
    H, W = plane.shape[:2]
    plane = np.asarray(plane, np.float64)
    x, y = (gx + 1) * (W - 1) / 2, (gy + 1) * (H - 1) / 2
    xc, yc = np.clip(x, 0, W - 1), np.clip(y, 0, H - 1)
    ix, iy = np.floor(xc).astype(np.int64), np.floor(yc).astype(np.int64)
    w, n = (xc - ix)[:, None], (yc - iy)[:, None]
    ix1, iy1 = np.minimum(ix + 1, W - 1), np.minimum(iy + 1, H - 1)
    T00, T01, T10, T11 = plane[iy, ix], plane[iy, ix1], plane[iy1, ix], plane[iy1, ix1]
    dx = (1 - n) * (T01 - T00) + n * (T11 - T10)
    dy = (1 - w) * (T10 - T00) + w * (T11 - T01)
    Gx = np.where((x <= 0) | (x >= W - 1), 0.0, (W - 1) / 2 * (row * dx).sum(1))
    Gy = np.where((y <= 0) | (y >= H - 1), 0.0, (H - 1) / 2 * (row * dy).sum(1))
    return Gx, Gy


def normals_exact64(sd, planes, box, rot, rays, z, weights):
    """the route of ops.normals_of_pass in float64: the live list of `weights`, the live points, the rows of g_raw = (0, 0, 0, 1) from the
    float64 model (points_grad_ref.model64), the slope, the normalisation, the fold.  sd: the decoder's state dict; planes [1,48,H,W] x 4;
    rays [N,11], z, weights [N,S].  -> (index, g [M,3], normal [N,3])"""
    rays, z, weights = (np.asarray(a, np.float64) for a in (rays, z, weights))
    N, S = z.shape
    index = live_list(weights)
    ray = index // S
    p = rays[ray, 0:3] + rays[ray, 3:6] * z.reshape(-1)[index][:, None]
    g_sigma = np.zeros((len(index), 4))
    g_sigma[:, 3] = 1
    rows = R.model64(sd, planes, box, rot, np.concatenate([p, rays[ray, 8:11]], 1), g_sigma)["rows"]
    box = np.asarray(box, np.float64)
    nrm = 2 * (p - box[0, :3]) / (box[1, :3] - box[0, :3]) - 1
    dn = np.zeros((len(index), 3))
    for d in range(3):
        P = np.asarray(rot[d], np.float64)                    # [3,2]: column 0 -> gx, column 1 -> gy
        Gx, Gy = slope_exact64(R.channel_last(planes[d]), nrm @ P[:, 0], nrm @ P[:, 1], rows[d])
        dn += P[:, 0][None] * Gx[:, None] + P[:, 1][None] * Gy[:, None]
    g = 2 * dn / (box[1, :3] - box[0, :3])
    q = (g * g).sum(1)
    with np.errstate(all="ignore"):
        n = np.where((q == 0)[:, None], 0.0, -g / np.sqrt(q)[:, None])
    normal = np.zeros((N, 3))
    np.add.at(normal, ray, weights.reshape(-1)[index][:, None] * n)
    return index, g, normal


# ---- seeded inputs of the kernel tests (never a backward's rows) -------------------------------------------------------------------------
def seeded_pass(N, S, seed, dead_rays=(), full_rays=()):
    """rays, depths and compositor-like weights of a pass: about half of the samples dead (exact zeros), some samples outside the box"""
    rng = np.random.default_rng(seed)
    x = np.concatenate([rng.uniform(-2.5, 2.5, (N, 3)), rng.standard_normal((N, 3))], 1).astype(np.float32)
    x[:, 3:] /= np.linalg.norm(x[:, 3:], axis=1, keepdims=True)
    rays, z = R.as_rays(x, rng.standard_normal((N, 3)).astype(np.float32), np.sort(rng.uniform(0.1, 2.5, (N, S)), 1))
    w = (rng.uniform(0.0, 0.4, (N, S)) * (rng.uniform(size=(N, S)) < 0.5)).astype(np.float32)
    for r in dead_rays:
        w[r] = 0
    for r in full_rays:
        w[r] = rng.uniform(0.05, 0.3, S)
    return rays, z, w


def seeded_rows(M, seed):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((M, 48)).astype(np.float32) for _ in range(3)]


def load_case():
    """g28_normals.npz + the decoders it was made with (g11's coarse.* / fine.* overwritten by g28's entries) -> (g, coarse sd, fine sd, planes, rot)"""
    from conftest import load_golden
    g, g11 = load_golden("g28_normals.npz"), load_golden("g11_grads.npz")
    vals = [np.asarray(g11[k], dtype=np.float64).reshape(-1) for k in sorted(g11) if k.startswith(("coarse.", "fine."))]
    flat = np.concatenate(vals)
    assert np.array_equal(np.array([flat.sum(), np.square(flat).sum(), flat.size]), g["g11_decoders"]), "g11_grads.npz changed: regenerate g28"
    sds = []
    for prefix in ("coarse.", "fine."):
        sd = {k[len(prefix):]: v for k, v in g11.items() if k.startswith(prefix)}
        sd.update({k[len(prefix):]: v for k, v in g.items() if k.startswith(prefix)})
        sds.append(sd)
    planes = [g["plane%d" % d] for d in range(4)]
    eye = np.eye(3, dtype=np.float32)
    rot = [eye[:, 1:], eye[:, [1, 0, 2]][:, 1:], eye[:, [2, 0, 1]][:, 1:]]
    assert all(np.array_equal(sds[1]["coord_projector.rot_mats_NON_LEARNED.%d" % d][:, 1:], rot[d]) for d in range(3))
    return g, sds[0], sds[1], planes, rot
