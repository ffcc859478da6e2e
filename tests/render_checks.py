"""float64 references and error bounds of the forward compositors -- composite_sample / composite_weight / composite_colour (csrc/side_work.h: the
two-tile kernels of render2.hip and render3.hip), render_pass_kernel (csrc/render.hip), composite_kernel (csrc/aux.hip) and coarse_depth
(csrc/nvsr_common.h) -- for tests/test_render_forward_edges.py (GPU) and tests/test_render_forward_edges_host.py (CPU).  A plain helper module
like triplane_checks.py (not collected, not a conftest).

composite64 restates one pass of volume_render_radiance_field in float64 exactly as the kernels state it (dist of the last sample 1e10 times
the norm, T *= 1 - alpha + 1e-10, disp = 1 / max(1e-10, depth / acc) with NaN where acc == 0, white background adds 1 - acc).  The one float32
step it reproduces is sn = raw3 + noise: the kernels round it once, and so does the reference, so relu's threshold falls on the same side and no
ray is left out near sigma = 0.  relu is where(sn < 0, 0, sn): a NaN stays a NaN and inf * 0 is NaN.

The bound of every output element is propagated through the same recurrence from float64 quantities alone (never from a kernel's output), with
u = 2^-24 and v~ = v (1 + d) the computed value of v:
    nrm = sqrtf(dx dx + dy dy + dz dz)   three rounded products and two additions of non-negative terms: gamma_3 under the root (halved by it),
                                         then SQRT_ULP ulp
    delta = z[s + 1] - z[s]              one rounding (exactly 0 for equal depths: a dead sample whatever its density); mip: the same
    dist = delta nrm                     one rounding; the last sample's 1e10 is exact in f32
    x = sig dist                         sig is exact (reproduced), one rounding: r_x relative
    E = expf(-x)                         its argument moves E inside [exp(-x (1 + r_x)), exp(-x (1 - r_x))] (an interval: no first-order term
                                         for x = 1e12), expf itself EXP_ULP ulp, results below 2^-126 may be flushed: + TINY
    alpha = 1 - E                        one rounding
    fac = (1 - alpha) + 1e-10            two roundings; an INTERVAL [fac - e, fac + e] clamped at 0: where alpha rounds to 1 the relative error
                                         of fac is of order 1, its absolute error is not
    T_s = prod_{k < s} fac_k             the products of the intervals' ends, times (1 -+ u)^n for n = l + s / 64 + 1 multiplications, l the live
                                         samples before s (a dead one's factor is fl(1 + 1e-10) = 1.0, within 1e-10 and exact to multiply by): a
                                         product of l factors takes l - 1 multiplications in any order (the wave scan of composite_kernel is a tree over
                                         disjoint ranges), + one per 64-lane chunk for the carry and the lane's own
    w = alpha T                          one rounding
    sigmoid = 1 / (1 + expf(-r))         EXP_ULP ulp, one rounding of the sum, DIV_ULP ulp of the division
    sums of S terms (acc, depth, rgb)    every term passes through at most n - 1 inexact additions in any order, n the terms that are not +0.0: gamma_n sum(|term| + e) + sum e; the
                                         products w z and w sigmoid round once (contracted into an fma: not at all)
    white: c + (1 - acc)                 two roundings
    disp = 1 / max(1e-10, depth / acc)   q = depth / acc moves by (e_depth + |q| e_acc) / (acc - e_acc), INFINITE where acc's interval reaches 0
                                         (the kernel's acc may be exactly 0 there and its disp NaN); max is 1-Lipschitz; two divisions
No fitted factor anywhere.  The device-library documentation on the build machine states no ulp bounds for expf, sqrtf and the division, so
they are named allowances (EXP_ULP, SQRT_ULP, DIV_ULP) as ATAN2_ULP is in triplane_checks.py; 1 ulp <= 2 u relative.

An element whose bound is wider than the tolerance include/nvsr.h states for its output (TOLERANCE) counts as "left out": it is still compared
under its bound, but the comparison says less than the header promises.  The host test caps the share of such elements at 1 % per output and case.
"""
from types import SimpleNamespace as NS

import numpy as np

import triplane_checks as tc

U = 2.0 ** -24
EXP_ULP = 2.0                      # expf
SQRT_ULP = 1.0                     # sqrtf
DIV_ULP = 1.0                      # a / b written with the operator (the __fdiv_rn of coarse_depth is correctly rounded: inside it)
TINY = 2.0 ** -126                 # a result below the normal range may be flushed to zero
F_1E10 = float(np.float32(1e10))
F_1EM10 = float(np.float32(1e-10))
OUTPUTS = ("weights", "acc", "depth", "disp", "rgb")
DECODER_TOLERANCE = 2e-5           # include/nvsr.h: "2e-5 on decoder outputs", here relative to the float64 range of the outputs (decoder_range)
# include/nvsr.h's parity tolerances per output: absolute on rgb, acc and weights, times far on depth, relative on disp (the golden test's rtol)
TOLERANCE = {"rgb": 2e-5, "acc": 2e-5, "weights": 2e-5, "depth": 2e-5, "disp": 1e-4}
LEFT_OUT_CAP = 0.01


def gamma(n):
    return n * U / (1 - n * U)


def _rnd(v, e):
    """the error of fl(v~) where v~ is within e of v: one more rounding"""
    return e + U * (np.abs(v) + e)


def _sum(term, e):
    """sum over the last axis of `term` (errors e) in f32, in any order -> value, error.  A term that is exactly 0 in float64 is +0.0 in the
    kernel (a dead sample) and adding it is exact: only the n others count, gamma_n"""
    n = (term != 0).sum(-1)
    return term.sum(-1), e.sum(-1) + gamma(n) * (np.abs(term) + e).sum(-1)


def stages64(raw, z, rd_or_rays, noise, mip=False):
    """the per-sample stages of one pass, each with its error as the header derives it: dist (r_x: the relative error of x), sn, x, E, alpha,
    fac with its interval [lo, hi], n_mul, T, w, zs (every field [N, S]; r_nrm a number, r_delta [N, S] or a number) -- what composite64 sums,
    and what render_backward_checks.backward64 differentiates"""
    raw = np.ascontiguousarray(raw, dtype=np.float32)
    N, S = raw.shape[:2]
    z = np.ascontiguousarray(z, dtype=np.float32).astype(np.float64)
    d = np.ascontiguousarray(rd_or_rays, dtype=np.float32)
    d = (d[:, 3:6] if d.shape[1] == 11 else d).astype(np.float64)
    assert z.shape == (N, S + (1 if mip else 0)) and d.shape == (N, 3)
    with np.errstate(all="ignore"):
        nrm = np.sqrt((d * d).sum(-1))[:, None]
        r_nrm = 0.5 * gamma(3) * (1 + gamma(3)) + 2 * SQRT_ULP * U
        if mip:
            delta, r_delta = z[:, 1:] - z[:, :-1], U
            zs = 0.5 * (z[:, 1:] + z[:, :-1])
            e_zs = U * np.abs(zs)
        else:
            delta = np.concatenate([z[:, 1:] - z[:, :-1], np.full((N, 1), F_1E10)], -1)
            r_delta = np.concatenate([np.full((N, S - 1), U), np.zeros((N, 1))], -1)
            zs, e_zs = z, np.zeros_like(z)
        dist = delta * nrm
        r_x = (1 + r_delta) * (1 + r_nrm) * (1 + U) * (1 + U) - 1
        sn32 = raw[..., 3] if noise is None else raw[..., 3] + np.ascontiguousarray(noise, dtype=np.float32)      # float32: the kernels' one rounding
        sn = sn32.astype(np.float64)
        sig = np.where(sn < 0, 0.0, sn)                                      # NaN stays NaN
        x = sig * dist                                                       # inf * 0 = NaN
        E = np.exp(-x)
        Ea, Eb = np.exp(-x * (1 + r_x)), np.exp(-x * (1 - r_x))
        e_E = np.maximum(np.abs(Ea - E), np.abs(Eb - E)) + 2 * EXP_ULP * U * np.maximum(Ea, Eb) + TINY
        e_E = np.where(x == 0, 0.0, e_E)                                     # expf(-0) is 1: a dead sample's weight is +0.0 exactly
        alpha = 1 - E
        e_alpha = np.where(x == 0, 0.0, _rnd(alpha, e_E))
        fac = (1 - alpha) + F_1EM10
        e_fac = np.where(x == 0, F_1EM10, _rnd(fac, _rnd(1 - alpha, e_alpha)))      # a dead sample: fl(1 + 1e-10) is 1.0
        lo, hi = np.maximum(fac - e_fac, 0.0), fac + e_fac
        one = np.ones((N, 1))
        excl_count = lambda live: np.cumsum(np.concatenate([np.zeros((N, 1), dtype=np.int64), live[:, :-1].astype(np.int64)], -1), -1)
        excl = lambda a: np.cumprod(np.concatenate([one, a[:, :-1]], -1), -1)
        s_ = np.arange(S)[None, :]
        n_mul = excl_count(x != 0) + s_ // 64 + 1                            # (a dead sample's factor is 1.0: that product is exact)
        T = excl(fac)
        e_T = np.maximum(excl(hi) * (1 + U) ** n_mul - T, T - excl(lo) * (1 - U) ** n_mul) + n_mul * TINY
        e_T[:, 0] = np.where(np.isnan(T[:, 0]), np.nan, 0.0)                 # T_0 = 1 exactly
        w = alpha * T
        e_w = np.where(alpha == 0, 0.0 * T, _rnd(w, e_alpha * T + np.abs(alpha) * e_T + e_alpha * e_T))      # (0 x T = +0.0 exactly; NaN T stays NaN)
    return NS(N=N, S=S, raw=raw, nrm=nrm, r_nrm=r_nrm, delta=delta, r_delta=r_delta, dist=dist, r_x=r_x, sn=sn, x=x, E=E, e_E=e_E, alpha=alpha,
              e_alpha=e_alpha, fac=fac, e_fac=e_fac, lo=lo, hi=hi, n_mul=n_mul, T=T, e_T=e_T, w=w, e_w=e_w, zs=zs, e_zs=e_zs)


def sigmoid64(r):
    """1 / (1 + expf(-r)) of float32 logits -> sigmoid, its error, the relative error of the denominator D = 1 + expf(-r) (header: sigmoid)"""
    with np.errstate(all="ignore"):
        r3 = np.asarray(r, dtype=np.float32).astype(np.float64)
        Ec = np.exp(-r3)
        e_Ec = 2 * EXP_ULP * U * Ec + TINY
        D = 1 + Ec
        rel_D = np.where(np.isfinite(D), _rnd(D, e_Ec) / D, 0.5)
        sg = 1 / D
        e_sg = sg * rel_D / (1 - rel_D) + 2 * DIV_ULP * U * sg + TINY
    return sg, e_sg, rel_D


def composite64(raw, z, rd_or_rays, noise, white, mip=False):
    """raw [N, S, 4], z [N, S] (mip: [N, S + 1] interval edges), rd [N, 3] or packed rays [N, 11], noise [N, S] or None (all float32) ->
    weights [N, S], acc, depth, disp [N], rgb [N, 3] in float64, .bound with the same fields, .sn [N, S] and .live [N] (samples with w != 0; a
    NaN weight is live)"""
    st = stages64(raw, z, rd_or_rays, noise, mip)
    raw, sn, w, e_w, zs, e_zs = st.raw, st.sn, st.w, st.e_w, st.zs, st.e_zs
    with np.errstate(all="ignore"):
        acc, e_acc = _sum(w, e_w)
        p = w * zs
        depth, e_depth = _sum(p, _rnd(p, e_w * np.abs(zs) + np.abs(w) * e_zs + e_w * e_zs))
        sg, e_sg, _ = sigmoid64(raw[..., :3])
        q = w[..., None] * sg
        e_q = _rnd(q, e_w[..., None] * sg + np.abs(w)[..., None] * e_sg + e_w[..., None] * e_sg)
        rgb, e_rgb = _sum(np.moveaxis(q, 1, -1), np.moveaxis(e_q, 1, -1))
        if white:
            bg = 1 - acc
            e_bg = _rnd(bg, e_acc)
            rgb = rgb + bg[:, None]
            e_rgb = _rnd(rgb, e_rgb + e_bg[:, None])
        qd = depth / acc                                                     # 0 / 0 = NaN
        a_lo = np.abs(acc) - e_acc
        e_qd = np.where(a_lo > 0, (e_depth + np.abs(qd) * e_acc) / np.where(a_lo > 0, a_lo, 1.0), np.inf)
        e_qd = np.where(np.isnan(qd), np.nan, e_qd + 2 * DIV_ULP * U * (np.abs(qd) + e_qd))
        m = np.where(np.isnan(qd), np.nan, np.maximum(F_1EM10, qd))
        m_lo = m - e_qd
        disp = 1 / m
        e_disp = np.where(m_lo > 0, e_qd / (m * np.where(m_lo > 0, m_lo, 1.0)), np.inf)
        e_disp = np.where(np.isnan(m), np.nan, e_disp + 2 * DIV_ULP * U * (disp + e_disp))
    live = (~(w == 0)).sum(-1)
    return NS(weights=w, acc=acc, depth=depth, disp=disp, rgb=rgb, sn=sn, live=live,
              bound=NS(weights=e_w, acc=e_acc, depth=e_depth, disp=e_disp, rgb=e_rgb))


def coarse_depth64(near, far, s, S, lindisp):
    """coarse_depth (csrc/nvsr_common.h) of f32 near / far [N] at the sample indices s (an int array) of S -> float64 depth [N, len(s)], bound
        t = linspace01(s, S)     step = 1 / (S - 1) (DIV_ULP ulp), t = step s below the middle (one rounding), else 1 - step (S - 1 - s) (two)
        1 - t                    one rounding
        lin:      near (1 - t) + far t                       two products, one addition
        lindisp:  1 / ((1 / near) (1 - t) + (1 / far) t)     __fdiv_rn twice (u each), two products, one addition, __fdiv_rn"""
    nr = np.ascontiguousarray(near, dtype=np.float32).astype(np.float64)[:, None]
    fr = np.ascontiguousarray(far, dtype=np.float32).astype(np.float64)[:, None]
    s = np.asarray(s, dtype=np.int64)[None, :]
    if S == 1:
        t, e_t = np.zeros(s.shape), np.zeros(s.shape)
    else:
        t = s / (S - 1.0)
        first = s < S // 2
        a = np.where(first, t, 1 - t)                                        # the product step * i
        e_a = (2 * DIV_ULP * U + U) * a * (1 + U)
        e_t = np.where(first, e_a, _rnd(t, e_a))
    om = 1 - t
    e_om = _rnd(om, e_t)
    if not lindisp:
        p1, p2 = nr * om, fr * t
        z = p1 + p2
        return z, _rnd(z, _rnd(p1, np.abs(nr) * e_om) + _rnd(p2, np.abs(fr) * e_t))
    i_n, i_f = 1 / nr, 1 / fr
    e_in, e_if = U * np.abs(i_n), U * np.abs(i_f)
    p1, p2 = i_n * om, i_f * t
    e1 = _rnd(p1, np.abs(i_n) * e_om + e_in * om + e_in * e_om)
    e2 = _rnd(p2, np.abs(i_f) * e_t + e_if * t + e_if * e_t)
    dd = p1 + p2
    e_d = _rnd(dd, e1 + e2)
    z = 1 / dd
    lo = np.abs(dd) - e_d
    return z, np.where(lo > 0, e_d / (np.abs(dd) * np.where(lo > 0, lo, 1.0)), np.inf) + U * np.abs(z) * (1 + U)


# ---- the comparison -----------------------------------------------------------------------------------------------------------------------

def compare(tag, name, got, ref, bound):
    """one output of a kernel against composite64's: NaN exactly where the reference is NaN, every other element finite and within its bound;
    an element whose bound is infinite (disp where acc's interval reaches 0) may hold anything -> the worst err / bound of the rest"""
    got = np.asarray(got, dtype=np.float64).reshape(ref.shape)
    want_nan = np.isnan(ref)
    free = ~want_nan & np.isinf(bound)
    assert not (np.isnan(bound) & ~want_nan).any(), "%s %s: the bound is NaN on a finite element" % (tag, name)
    wrong = (np.isnan(got) != want_nan) & ~free
    assert not wrong.any(), "%s %s: %d elements are NaN where the reference is finite or finite where it is NaN, the first at %s (got %r, want %r)" % (
        tag, name, int(wrong.sum()), tuple(np.argwhere(wrong)[0]), got[tuple(np.argwhere(wrong)[0])], ref[tuple(np.argwhere(wrong)[0])])
    chk = ~want_nan & ~free
    if not chk.any():
        return 0.0
    err = np.abs(got[chk] - ref[chk])
    b = bound[chk]
    bad = ~(err <= b)
    if bad.any():
        i = int(np.argmax(np.where(bad, err / np.maximum(b, 1e-300), 0)))
        raise AssertionError("%s %s: %d of %d elements beyond their bound; the worst is element %s: got %.9g, want %.9g, err %.3g, bound %.3g" % (
            tag, name, int(bad.sum()), int(chk.sum()), tuple(np.argwhere(chk)[i]), got[chk][i], ref[chk][i], err[i], b[i]))
    return float((err / np.maximum(b, 1e-300)).max())


def left_out(ref, far=6.0):
    """share of the finite elements of every output whose bound is wider than include/nvsr.h's tolerance for it (far: a number or one per
    ray) -> {output: share}"""
    out = {}
    for name in OUTPUTS:
        v, b = getattr(ref, name), getattr(ref.bound, name)
        ok = ~np.isnan(v)
        tol = TOLERANCE[name] * ((np.zeros(v.shape) + far)[ok] if name == "depth" else np.abs(v[ok]) if name == "disp" else 1.0)
        out[name] = float((b[ok] > tol).mean()) if ok.any() else 0.0
    return out


# ---- the cases (shared by the GPU tests and the CPU check of their inputs) ------------------------------------------------------------------

SIZES = tc.SIZES[0]
DECODER_SEED, PLANES_SEED = 7, 11
SIGMA_SCALE = 512.0                # the density head of make_decoder times 512 (a power of two: exact): sigma dist of order 1 and more on the
                                   # 2^-5 grid -- at sigma dist of 0.01 a ray has dozens of live samples under T = 1, each with expf's absolute error
DEAD, NOISE_STD = -1.0e4, 4.0      # noise of a dictated dead sample; of a natural ray's samples (make_noise)
# fused kernels: (N, S); every N of {1, 33, 293, 2305} and every S of {1, 2, 3, 33, 65} occurs, 4096 + 513 only on the two-phase route
FUSED_SHAPES = [(1, 1), (1, 33), (33, 2), (33, 65), (293, 3), (293, 33), (2305, 1), (2305, 3)]
TWO_PHASE_SHAPE = (4096 + 513, 3)
# composite_kernel: the carry across 64-lane chunks at S = 63, 64, 65, 129, 192; WPB = 4 rays per workgroup
COMPOSITE_SHAPES = [(1, 1), (33, 63), (33, 64), (5, 65), (33, 129), (37, 192)]
GROUP = 128                        # the smallest workgroup of the fused kernels (render.hip: 128 rays; the two-tile kernels: 256)


def case_id(c):
    return "%dx%d" % (c.N, c.S)


def fused_cases():
    return [NS(N=N, S=S, seed=300 + i, grid=5) for i, (N, S) in enumerate(FUSED_SHAPES + [TWO_PHASE_SHAPE])]


def composite_cases():
    return [NS(N=N, S=S, seed=400 + i, grid=7) for i, (N, S) in enumerate(COMPOSITE_SHAPES)]


def ray_class(N):
    """ray i of a case: 0 natural (the decoder's own densities + noise), 1 empty, 2 partial, 3 full -- dictated by the noise of the noise-on launches"""
    return np.arange(N) % 4


def special(N):
    """ray i of the NaN / inf launch: 1 +inf on an interval of positive length, 2 +inf on a zero-length one, 3 -inf, 5 / 6 / 7 NaN on the
    first / a middle / the last sample, 0 and 4 nothing.  A single ray gets the NaN in the middle."""
    return (np.arange(N) + (6 if N == 1 else 0)) % 8


def make_inputs(c):
    """-> scene, rays [N, 11], z [N, S] of a case.  triplane_checks.make_rays(exact=True): every position tap is exact in f32; depths are sorted
    multiples of 2^-grid in [2, 6], so ties -- zero-length intervals, dead whatever their density -- are frequent.  The rays of class 3 (full
    lists) get DISTINCT depths; the rays of special() == 2 get z[1] = z[0]; rays 12, 28, 44, ... (natural, special() == 4) have a zero
    direction (norm 0: every interval is empty and the last one is 1e10 x 0)."""
    scene = tc.make_scene(SIZES)
    rays, z = tc.make_rays(c.N, c.S, c.seed, exact=True)
    rng = np.random.default_rng(c.seed + 50)
    q = 2 ** c.grid
    if c.grid != 5:
        z = np.sort(rng.integers(2 * q, 6 * q + 1, (c.N, c.S)) / float(q), -1).astype(np.float32)
        # (composite_kernel at S up to 192: directions of norm >= sqrt(3) / 2, or a short ray's hundred live samples all sit under T = 1)
        rays[:, 3:6] = rng.integers(8, 17, (c.N, 3)) / 16.0 * np.where(rng.random((c.N, 3)) < 0.5, -1, 1)
    cls, sp = ray_class(c.N), special(c.N)
    for i in np.nonzero(cls == 3)[0]:
        z[i] = np.sort(rng.choice(np.arange(2 * q, 6 * q + 1), c.S, replace=False)) / float(q)
    if c.S >= 2:
        z[sp == 2, 1] = z[sp == 2, 0]
    rays[12::16, 3:6] = 0.0
    if c.grid == 5:
        tc.assert_exact_taps(rays, z, scene)
    return scene, rays, np.ascontiguousarray(z, dtype=np.float32)


def z_rays(rays, seed):
    """the same rays for the kernels that compute their depths in registers: near in [0.5, 3] and far in [4, 9] per ray (multiples of 2^-5),
    every seventh ray near == far"""
    rng = np.random.default_rng(seed + 60)
    r = rays.copy()
    N = r.shape[0]
    r[:, 6] = rng.integers(16, 97, N) / 32.0
    r[:, 7] = rng.integers(128, 289, N) / 32.0
    r[3::7, 7] = r[3::7, 6]
    return r


def make_decoder():
    nat = tc.make_decoder(DECODER_SEED)
    nat[tc.N_ALPHA_W:tc.N_ALPHA_B + 1] *= np.float32(SIGMA_SCALE)
    return nat


def make_planes(scene):
    return tc.make_planes(scene, PLANES_SEED)


def make_raw(c):
    """random raw [N, S, 4] for the compositors that read it: rgb logits N(0, 2) with a few at +-30 and +-100, sigma N(-40, 64): about a quarter of the
    samples are live, so that a sum of S = 192 terms has some fifty inexact additions"""
    rng = np.random.default_rng(c.seed + 70)
    raw = rng.standard_normal((c.N, c.S, 4)) * [2, 2, 2, 64] + [0, 0, 0, -40]
    big = rng.random((c.N, c.S, 3)) < 0.02
    raw[..., :3] = np.where(big, rng.choice([-100.0, -30.0, 30.0, 100.0], (c.N, c.S, 3)), raw[..., :3])
    return raw.astype(np.float32)


def make_noise(c, raw3):
    """the noise of the noise-on launches, from the launch's own raw3 [N, S] (float32): N(0, NOISE_STD) on the natural rays; DEAD on every
    sample of an empty ray and on a random half of a partial ray's (at least one dead, at least one live where S >= 2: a single sample is
    live); a dictated live sample gets U(2, 8) - raw3, so sn is in [2, 8] whatever the decoder said and T stays far above the f32 underflow
    (sum of sigma dist <= 8 x 4 x sqrt(3) = 55).  A full ray has distinct depths (make_inputs), so its S weights are all positive unless its
    direction is zero.  The cases of composite_kernel (grid 7: no live lists) have partial rays in place of the full ones; from S = 128 on
    three quarters of a partial ray are dead and sn grows with S / 64: a sum of 192 live terms has a bound of 192 u on its own."""
    rng = np.random.default_rng(c.seed + 80)
    N, S = raw3.shape
    cls = ray_class(N)[:, None]
    if c.grid != 5:
        cls = np.where(cls == 3, 2, cls)
    nat = NOISE_STD * rng.standard_normal((N, S))
    live = rng.uniform(2.0, 8.0, (N, S)) * max(1, S // 64) - raw3.astype(np.float64)
    dead = rng.random((N, S)) < (0.5 if S < 128 else 0.75)
    if S >= 2:
        dead[:, 0], dead[:, 1] = True, False
        dead = rng.permuted(dead, axis=1)
    else:
        dead[:] = False
    noise = np.where(cls == 0, nat, np.where(cls == 1, DEAD, np.where((cls == 2) & dead, DEAD, live)))
    return noise.astype(np.float32)


KNIFE_ULPS = (0, 1, 3, -1, -3)


def knife_noise(c, raw3, base, mip=False):
    """the knife-edge launch: the noise is float32(-raw3) moved by 0, +1, +3, -1 or -3 ulps -- sn = raw3 + noise is then exactly 0, barely
    positive or barely negative (the difference of two neighbours is exact) -- on the last sample, where dist is 1e10, of the rays with
    i % 8 < 4 (every class; mip, where the last interval is finite too: not the empty rays), and on every other sample (from S = 128 on: every eighth; each carries expf's absolute error) of the full rays (between two solidly live ones: a barely positive sample adds a
    weight near 1e-8 there, not a ray whose acc is 1e-8 and whose disp no bound can hold).  The other samples keep `base`.
    -> noise, mask of the knife samples"""
    N, S = raw3.shape
    i, s = np.arange(N)[:, None], np.arange(S)[None, :]
    cls = ray_class(N)[:, None]
    mask = (((i + s) % (2 if S < 128 else 8) == 0) & (cls == 3)) | ((s == S - 1) & (i % 8 < 4) & ((cls != 1) | (not mip)))
    k = np.asarray(KNIFE_ULPS)[(7 * i + 3 * s) % 5]
    v = (-raw3).astype(np.float32)
    for step in (1, 2, 3):
        up = np.nextafter(v, np.float32(np.inf))
        dn = np.nextafter(v, np.float32(-np.inf))
        v = np.where(k >= step, up, np.where(-k >= step, dn, v)).astype(np.float32)
    return np.where(mask, v, base).astype(np.float32), mask


def special_noise(c, z, base):
    """the NaN / inf launch: `base` with the values of special() -> noise, {kind: [(ray, sample)]}.  +inf on an interval of positive length
    takes the first such interval of the ray (the last sample's 1e10 if there is no other); +inf on a zero-length one takes sample 0 of a ray
    whose z[1] == z[0] (make_inputs; S >= 2)."""
    N, S = base.shape
    sp = special(N)
    noise = base.copy()
    where = {}
    for i in range(N):
        k = sp[i]
        if k == 1:
            pos = np.nonzero(np.diff(z[i]) > 0)[0]
            s = int(pos[0]) if pos.size else S - 1
        elif k == 2:
            if S < 2 or z[i, 1] != z[i, 0]:            # (depths computed in registers have no such tie: the ray gets nothing)
                continue
            s = 0
        elif k == 3:
            s = S // 3
        elif k in (5, 6, 7):
            s = {5: 0, 6: S // 2, 7: S - 1}[k]
        else:
            continue
        noise[i, s] = {1: np.inf, 2: np.inf, 3: -np.inf}.get(k, np.nan)
        where.setdefault(int(k), []).append((i, s))
    return noise, where


def assert_live_mix(tag, live, S, N):
    """every workgroup's rays (GROUP consecutive ones; a group of fewer than 8 rays is exempt) hold an empty, a partial and a full live list"""
    if S < 2 or N < 8:
        return
    for g0 in range(0, N, GROUP):
        n = live[g0:g0 + GROUP]
        if n.size < 8:
            continue
        assert (n == 0).any() and (n == S).any() and ((n > 0) & (n < S)).any(), "%s: group at ray %d lacks a kind of live list" % (tag, g0)
