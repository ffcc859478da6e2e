"""float64 reference and error bound of the backward compositor -- composite_backward_kernel (csrc/render_bwd.hip), reached through
nvsr_composite_backward, _mip, _depth and _rays -- for tests/test_render_backward_edges.py (GPU) and tests/test_render_backward_edges_host.py
(CPU).  A plain helper module like render_checks.py (not collected, not a conftest).

backward64 differentiates the recurrence of render_checks.composite64 (the stages come from render_checks.stages64: the one float32 step is
sn = raw3 + noise, so relu's gate falls on the kernel's side), restated WITHOUT the division the kernel makes:
    gw_s        = sum_c g_c sigmoid(r_sc) + (g_acc - white (g_0 + g_1 + g_2)) + g_dep zs_s          zs: z_s, mip: the interval's mid-point
    B_s         = sum_{k > s} alpha_k gw_k prod_{s < j < k} fac_j
    dL/dalpha_s = T_s (gw_s - B_s)
    g_raw[s, 3] = dL/dalpha_s dist_s exp(-x_s) where sn_s > 0, +0.0 where sn_s <= 0, NaN where sn_s is NaN (relu's subgradient at 0 is 0; its
                  backward passes the incoming gradient through a NaN input)
    g_raw[s, c] = w_s g_c sigmoid (1 - sigmoid)
The kernel computes suffix_s / fac_s with suffix_s = sum_{k > s} w_k gw_k.  Every computed T_k, k > s, holds the computed fac_s as a factor
(T~_k = prod_{j < k} fac~_j times (1 + d)^n_mul), so the quotient is sum_{k > s} alpha~_k gw~_k P~_sk with P_sk = prod_{j < k, j != s} fac_j,
up to relative roundings: the bound does not blow up behind an opaque sample although fac_s's own interval reaches 1e-10 there.

The bound, from float64 quantities alone (u = 2^-24, the library is built with -ffp-contract=off: every operation rounds once):
    sigmoid, D = 1 + expf(-r)   render_checks.sigmoid64; g_c / D~ moves by |g_c| sigmoid rel_D / (1 - rel_D), DIV_ULP ulp, + TINY
    ga = g_acc - (g0 + g1) - g2 three roundings with a white background (two and an exact negation without g_acc), none without
    gw                          ((t0 + t1) + t2) + ga, + fl(g_dep zs): one rounding per operation
    alpha, 1 - alpha, fac       as composite64, with one case more: where E + e_E < 2^-25 the computed alpha is exactly 1, 1 - alpha exactly +0.0
                                and fac exactly fl(1e-10) -- the error of all three is E itself (without it the 1e10 last sample of most rays
                                gets a bound of hundreds: |dL/dalpha dist| times u).  The computed fac is never below fl(1e-10): lo is clamped
                                there.  (The reference takes 1 - alpha as E and fac as E + fl(1e-10): float64's own 1 - (1 - E) is off by 1e-16,
                                1e-6 of an opaque fac.)
    T_s, w_s                    as composite64, from these intervals
    term k of the quotient      a_k = alpha_k gw_k with e_a; P~_sk inside [Tlo_s Qlo_sk, Thi_s Qhi_sk] (products of the intervals' ends, j != s)
                                times (1 -+ u)^M, M = n_mul_k + 2 (w, w gw) + m_s: |a_k| e_P + e_a Phi; the N x S x S pair products are formed
    m_s, the reverse scan       six shfl_down steps per chunk (a tree over the lanes behind s), "- own", "+ carry", one carry addition per
                                later chunk -- and never more inexact additions than there are live terms: min(6 + chunks behind, live - 1) + 2
    the division                DIV_ULP ulp; a product flushed on its way (w, w gw, n_mul of T_k: TINY each) is divided by lo_s
    p1 = T gw, G = p1 - q, G dist, (G dist)(1 - alpha)
                                one rounding each; dist's relative error is x's without the last product; the last factor is the COMPUTED
                                1 - alpha, so it carries that error, not expf's alone.  The final rounding term u (|v| + e) keeps err <= bound
                                where the kernel's value is exactly 0 and the reference's is q E.
    "- own"                     the kernel forms the exclusive suffix as (inclusive - own_s) + carry.  The roundings of the inclusive tree are
                                relative to partial sums that hold own_s = w_s gw_s, which does NOT hold fac_s as a factor: d_s <= gamma_m |own_s|
                                stays in the suffix and is divided by fac_s.  The output multiplies by the computed 1 - alpha, and the computed
                                fac = fl((1 - alpha) + 1e-10) is never below it, so the term reaches g_raw[s, 3] as at most gamma_m |own_s| dist_s
                                (1 + 8 u) -- and as 0 where 1 - alpha is exactly +0.0.  (A sequential restatement has no such term; the kernel has.)
    columns 0..2                ((w g_c) sigmoid)(1 - sigmoid): three products, the rounding of 1 - sigmoid
No fitted factor anywhere; EXP_ULP, SQRT_ULP, DIV_ULP and TINY are render_checks's named allowances.

An element whose bound is wider than the tolerance of the older test (2e-4 |ref| + 2e-6 max |ref| of the launch, the four columns together)
counts as left out: it is still compared under its bound.  The host test caps their number per launch at 1 % of the finite elements or one.
"""
import functools
from types import SimpleNamespace as NS

import numpy as np

import render_checks as rc
from render_checks import DIV_ULP, F_1EM10, TINY, U, _rnd, gamma

EXTRA_SHAPES = [(6, 2), (33, 3), (5, 511), (9, 512)]
# (name, noise, white, g_acc given, g_dep given)
LAUNCHES = [("plain", None, 0, False, False), ("white", None, 1, True, False), ("noise", "on", 0, True, True), ("noise+white", "on", 1, False, True),
            ("knife", "knife", 0, True, True), ("special", "special", 1, True, True)]
LAUNCH_NAMES = [l[0] for l in LAUNCHES]
RTOL, ATOL = 2e-4, 2e-6            # test_hip_parity.py::test_composite_backward_vs_autograd_formula
LEFT_OUT_CAP = 0.01
MIP_TAIL = np.float32(0.25)        # the last interval edge of the mip launches, as test_composite_kernel extends z


def cases():
    return rc.composite_cases() + [NS(N=N, S=S, seed=410 + i, grid=7) for i, (N, S) in enumerate(EXTRA_SHAPES)]


CASES = cases()
IDS = [rc.case_id(c) for c in CASES]


@functools.lru_cache(maxsize=None)
def inputs(i, mip):
    """case i -> NS(c, rays [N, 11], z [N, S (+ 1)], raw, g_rgb, g_acc, g_dep, L: {launch: NS(noise, white, g_acc, g_dep)}, mask: the knife
    samples, where: the special positions); every array float32"""
    c = CASES[i]
    _, rays, z = rc.make_inputs(c)
    if mip:
        z = np.concatenate([z, z[:, -1:] + MIP_TAIL], -1)
    raw = rc.make_raw(c)
    on = rc.make_noise(c, raw[..., 3])
    knife, mask = rc.knife_noise(c, raw[..., 3], on, mip)
    special, where = rc.special_noise(c, z[:, :c.S], on)
    rng = np.random.default_rng(c.seed + 90)
    g_rgb = rng.standard_normal((c.N, 3)).astype(np.float32)
    g_acc = rng.standard_normal(c.N).astype(np.float32)
    g_dep = rng.standard_normal(c.N).astype(np.float32)
    noises = {None: None, "on": on, "knife": knife, "special": special}
    L = {name: NS(noise=noises[n], white=white, g_acc=g_acc if a else None, g_dep=g_dep if d else None) for name, n, white, a, d in LAUNCHES}
    return NS(c=c, mip=bool(mip), rays=rays, z=z, raw=raw, g_rgb=g_rgb, g_acc=g_acc, g_dep=g_dep, L=L, mask=mask, where=where)


@functools.lru_cache(maxsize=None)
def reference(i, mip, launch):
    """backward64 of a launch of case i, computed once and shared (the tests leave it unchanged)"""
    p = inputs(i, mip)
    l = p.L[launch]
    return backward64(p.raw, p.z, p.rays, l.noise, l.white, p.mip, p.g_rgb, l.g_acc, l.g_dep)


def _between(f):
    """f [N, S] -> Q [N, S, S], Q[:, s, k] = prod_{s < j < k} f_j for k > s (anything elsewhere: mask with s < k)"""
    N, S = f.shape
    Q = np.zeros((N, S, S))
    col = np.zeros((N, S))
    for k in range(1, S):
        col = col * f[:, k - 1:k]
        col[:, k - 1] = 1.0
        Q[:, :, k] = col
    return Q


def backward64(raw, z, rd_or_rays, noise, white, mip, g_rgb, g_acc, g_dep, e_acc=0.0, e_dep=0.0):
    """raw [N, S, 4], z [N, S] (mip: [N, S + 1]), rd [N, 3] or packed rays [N, 11], noise [N, S] or None, g_rgb [N, 3], g_acc, g_dep [N] or None
    -> NS(g_raw [N, S, 4] float64, bound of the same shape, sn, sat).  e_acc, e_dep [N]: how far the g_acc / g_dep the kernel is given may be
    from the ones given here (the operator's fold of disp's gradient rounds in float32)"""
    st = rc.stages64(raw, z, rd_or_rays, noise, mip)
    N, S = st.N, st.S
    f64 = lambda a: np.asarray(a, dtype=np.float64)
    g = f64(g_rgb).reshape(N, 3)
    with np.errstate(all="ignore"):
        # ---- dL/dw ----------------------------------------------------------------------------------------------------------------------
        base = np.zeros(N) if g_acc is None else f64(g_acc).reshape(N)
        e_base = np.zeros(N) + (0.0 if g_acc is None else e_acc)
        if white:
            s01 = g[:, 0] + g[:, 1]
            s3 = s01 + g[:, 2]
            e_s3 = _rnd(s3, U * np.abs(s01))
            ga = base - s3
            e_ga = (e_s3 if g_acc is None else _rnd(ga, e_s3 + e_base))              # 0 - s is exact
        else:
            ga, e_ga = base, e_base
        sg, e_sg, rel_D = rc.sigmoid64(st.raw[..., :3])
        t = g[:, None, :] * sg
        e_t = np.abs(t) * rel_D / (1 - rel_D)
        e_t = e_t + 2 * DIV_ULP * U * (np.abs(t) + e_t) + TINY
        gw = t[..., 0] + t[..., 1]
        e_gw = _rnd(gw, e_t[..., 0] + e_t[..., 1])
        gw = gw + t[..., 2]
        e_gw = _rnd(gw, e_gw + e_t[..., 2])
        gw = gw + ga[:, None]
        e_gw = _rnd(gw, e_gw + e_ga[:, None])
        if g_dep is not None:
            gd = f64(g_dep).reshape(N, 1)
            p = gd * st.zs
            e_p = _rnd(p, np.abs(gd) * st.e_zs + (np.zeros((N, 1)) + np.reshape(e_dep, (-1, 1))) * (np.abs(st.zs) + st.e_zs)) + TINY
            gw = gw + p
            e_gw = _rnd(gw, e_gw + e_p)
        # ---- alpha, 1 - alpha, fac with the saturated case; T and w from them ------------------------------------------------------------
        x, E, alpha, n_mul, dist, sn = st.x, st.E, st.alpha, st.n_mul, st.dist, st.sn
        dead = x == 0
        sat = (E + st.e_E) < 2.0 ** -25                                       # (NaN: False)
        e_alpha = np.where(sat, E, st.e_alpha)
        e_oma = np.where(dead, 0.0, np.where(sat, E, _rnd(E, e_alpha)))
        fac = E + F_1EM10
        e_fac = np.where(dead, F_1EM10, np.where(sat, E, _rnd(fac, e_oma)))
        lo, hi = np.maximum(fac - e_fac, F_1EM10), fac + e_fac
        one = np.ones((N, 1))
        excl = lambda a: np.cumprod(np.concatenate([one, a[:, :-1]], -1), -1)
        T, Tlo, Thi = excl(fac), excl(lo), excl(hi)
        e_T = np.maximum(Thi * (1 + U) ** n_mul - T, T - Tlo * (1 - U) ** n_mul) + n_mul * TINY
        e_T[:, 0] = np.where(np.isnan(T[:, 0]), np.nan, 0.0)
        w = alpha * T
        e_w = np.where(alpha == 0, 0.0 * T, _rnd(w, e_alpha * T + np.abs(alpha) * e_T + e_alpha * e_T))
        # ---- the quotient suffix_s / fac_s = T_s B_s -----------------------------------------------------------------------------------------
        s_ = np.arange(S)
        tri = (s_[:, None] < s_[None, :])[None]
        a = alpha * gw
        e_a = e_alpha * np.abs(gw) + np.abs(alpha) * e_gw + e_alpha * e_gw
        live = (alpha != 0).astype(np.int64)
        L = np.cumsum(live[:, ::-1], -1)[:, ::-1]                             # live samples from s on
        behind = (S + 63) // 64 - 1 - s_ // 64
        m = np.minimum(6 + behind[None, :], np.maximum(L - 1, 0)) + 2
        up_k, dn_k = (1 + U) ** (n_mul + 2), (1 - U) ** (n_mul + 2)
        up_s, dn_s = (1 + U) ** m, (1 - U) ** m
        Q, Qlo, Qhi = _between(fac), _between(lo), _between(hi)
        B = np.where(tri, a[:, None, :] * Q, 0.0).sum(-1)
        P = T[:, :, None] * Q
        Phi = (Thi * up_s)[:, :, None] * Qhi * up_k[:, None, :]
        Plo = (Tlo * dn_s)[:, :, None] * Qlo * dn_k[:, None, :]
        e_P = np.maximum(Phi - P, P - Plo)
        tau = TINY * (np.abs(gw) + e_gw + 1) + n_mul * TINY * (np.abs(a) + e_a)
        e_q = np.where(tri, np.abs(a)[:, None, :] * e_P + e_a[:, None, :] * Phi + tau[:, None, :] / lo[:, :, None], 0.0).sum(-1)
        TB = T * B
        e_q = e_q + 2 * DIV_ULP * U * (np.abs(TB) + e_q) + TINY
        p1 = T * gw
        e_p1 = _rnd(p1, e_T * np.abs(gw) + T * e_gw + e_T * e_gw) + TINY
        G = p1 - TB
        e_G = _rnd(G, e_p1 + e_q)
        r_d = (1 + st.r_delta) * (1 + st.r_nrm) * (1 + U) - 1
        e_dist = r_d * dist
        v1 = G * dist
        e_v1 = _rnd(v1, e_G * dist + np.abs(G) * e_dist + e_G * e_dist) + TINY
        g3 = v1 * E
        e_3 = _rnd(g3, e_v1 * E + np.abs(v1) * e_oma + e_v1 * e_oma) + TINY
        own_hi = (np.abs(w) + e_w) * (np.abs(gw) + e_gw) * (1 + U) + TINY
        e_3 = e_3 + np.where(sat | (alpha == 0), 0.0, gamma(m) * own_hi * (dist + e_dist) * (1 + 8 * U))          # "- own"
        g3 = np.where(np.isnan(sn), np.nan, np.where(sn <= 0, 0.0, g3))
        e_3 = np.where(sn <= 0, 0.0, e_3)
        # ---- the colour columns -------------------------------------------------------------------------------------------------------------
        gk = g[:, None, :]
        v = w[..., None] * gk
        e1 = _rnd(v, e_w[..., None] * np.abs(gk)) + TINY
        v2 = v * sg
        e2 = _rnd(v2, e1 * sg + np.abs(v) * e_sg + e1 * e_sg) + TINY
        om = 1 - sg
        e_om = _rnd(om, e_sg)
        v3 = v2 * om
        e3 = _rnd(v3, e2 * om + np.abs(v2) * e_om + e2 * e_om) + TINY
        e3 = np.where((alpha == 0)[..., None], 0.0 * T[..., None], e3)        # (w is +0.0 exactly; a NaN T stays NaN)
    return NS(g_raw=np.concatenate([v3, g3[..., None]], -1), bound=np.concatenate([e3, e_3[..., None]], -1), sn=sn, sat=sat, weights=w)


def compare(tag, got, ref):
    """g_raw of a kernel against backward64's with render_checks.compare's semantics -> the worst err / bound per column, and under
    "general <column>" the worst over the samples in front of a ray's first saturated one (at and behind it the bound states the kernel's value
    -- alpha exactly 1, fac exactly fl(1e-10) -- rather than bounding it, and the ratio is 1 by construction)"""
    got = np.asarray(got, dtype=np.float64).reshape(ref.g_raw.shape)
    rep = {}
    front = np.cumsum(ref.sat, -1) == 0
    for col, name in enumerate(("g_r", "g_g", "g_b", "g_sigma")):
        rep[name] = rc.compare(tag, name, got[..., col], ref.g_raw[..., col], ref.bound[..., col])
        m = front & ~np.isnan(ref.g_raw[..., col]) & (ref.bound[..., col] > 0)
        rep["general " + name] = float((np.abs(got[..., col] - ref.g_raw[..., col])[m] / ref.bound[..., col][m]).max()) if m.any() else 0.0
    print("render_backward_edges ratio | %s | %s" % (tag, " ".join("%s=%.3f" % (k.replace(" ", "_"), v) for k, v in rep.items())))
    return rep


def left_out(ref):
    """-> (the elements whose bound is wider than the older test's tolerance, the finite elements), or None for a launch whose reference is
    all zero (exempt)"""
    v, b = ref.g_raw, ref.bound
    ok = ~np.isnan(v)
    if not ok.any() or float(np.abs(v[ok]).max()) == 0.0:
        return None
    tol = RTOL * np.abs(v[ok]) + ATOL * float(np.abs(v[ok]).max())
    return int((b[ok] > tol).sum()), int(ok.sum())


def check_rule(tag, g_raw, sn, where, base=None):
    """the NaN rule on a g_raw [N, S, 4] of the special launch (the reference's or a kernel's; sn: the reference's; base: the same launch
    without the special values, or None)"""
    N = g_raw.shape[0]
    nan_rays = set()
    for kind in (5, 6, 7, 2):
        for i, s in where.get(kind, []):
            what = "%s ray %d (%s at sample %d)" % (tag, i, "inf x 0" if kind == 2 else "NaN", s)
            nan_rays.add(i)
            assert np.isnan(g_raw[i, s, 3]), what + ": the density gradient of that sample is not NaN"
            on = sn[i, :s] > 0
            assert np.isnan(g_raw[i, :s, 3][on]).all(), what + ": the density gradient of an earlier live sample is not NaN"
            off = g_raw[i, :s, 3][~on]
            assert (off == 0).all() and not np.signbit(off).any(), what + ": a gated-off sample does not keep its +0.0"
            assert np.isnan(g_raw[i, s:, :3]).all(), what + ": a colour gradient from that sample on is not NaN"
    for kind in (1, 3):
        for i, s in where.get(kind, []):
            assert np.isfinite(g_raw[i]).all(), "%s ray %d (%sinf at sample %d): a gradient is not finite" % (tag, i, "+-"[kind == 3], s)
    for i in range(12, N, 16):
        if i not in nan_rays:
            assert np.isfinite(g_raw[i]).all(), "%s ray %d (zero direction): a gradient is not finite" % (tag, i)
    others = np.array([i not in nan_rays for i in range(N)])
    assert np.isfinite(g_raw[others]).all(), tag + ": a ray without a NaN holds one"
    if base is not None:
        same = lambda p, q: np.array_equal(np.asarray(p, dtype=np.float64).view(np.uint64), np.asarray(q, dtype=np.float64).view(np.uint64))
        plain = np.array([i not in nan_rays and not any(i == r for k in (1, 3) for r, _ in where.get(k, [])) for i in range(N)])
        assert same(g_raw[plain], base[plain]), tag + ": a ray without a special value changed"
