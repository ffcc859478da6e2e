"""CPU checks of tests/render_backward_checks.py, the float64 reference behind tests/test_render_backward_edges.py:
  * backward64 (the division-free form) against float64 torch autograd of the reference's formula on the rays where autograd itself is well
    conditioned: the same function, mip and white off and on, g_acc and g_dep given and absent;
  * the left-out cap on every case and launch, on the reference alone;
  * the NaN rule on the reference;
  * a float32 numpy restatement of composite_backward_kernel (kernel32: the kernel's operations in the kernel's order, the six shfl_down steps
    and "(inclusive - own) + carry" included; the product scan sequential) passes every launch under the bound with the reference's NaN
    pattern, and each mutant of it fails its named launches; "exp(-x) in place of 1 - alpha" passes every launch -- with the exclusive suffix
    summed directly: against "(inclusive - own_s)" only the computed 1 - alpha cancels the term the bound calls "- own".  The mutants live here
    only; none is ever run on a GPU."""
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import render_backward_checks as bc
import render_checks as rc

F = np.float32
PAIRS = [(i, mip) for i in range(len(bc.CASES)) for mip in (0, 1)]
PAIR_IDS = ["%s-%s" % (bc.IDS[i], "mip" if mip else "plain") for i, mip in PAIRS]


def kernel32(p, l, mutant=None):
    """composite_backward_kernel in float32 numpy on the launch l of the inputs p -> g_raw [N, S, 4] float32"""
    raw, z, mip = p.raw, p.z, p.mip
    N, S = raw.shape[:2]
    with np.errstate(all="ignore"):
        d = p.rays[:, 3:6]
        nrm = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])[:, None]
        if mip:
            delta = z[:, 1:] - z[:, :-1]
            zs = z[:, :-1] if mutant == "mip_left_edge" else F(0.5) * (z[:, :-1] + z[:, 1:])
        else:
            last = (z[:, -1:] - z[:, -2:-1]) if (mutant == "last_dist_from_z" and S >= 2) else np.full((N, 1), 1e10, F)
            delta = np.concatenate([z[:, 1:] - z[:, :-1], last], -1)
            zs = z
        dist = delta * nrm
        sn = raw[..., 3] if l.noise is None else raw[..., 3] + l.noise
        sig = np.where(sn < 0, F(0), sn)
        E = np.exp(-(sig * dist))
        alpha = F(1) - E
        oma = F(1) - alpha
        fac = oma + F(1e-10)
        g0, g1, g2 = (p.g_rgb[:, k] for k in range(3))
        ga = (l.g_acc if l.g_acc is not None else np.zeros(N, F)) - (((g0 + g1) + g2) if (l.white and mutant != "white_kept") else F(0))
        D = F(1) + np.exp(-raw[..., :3])
        gw = g0[:, None] / D[..., 0] + g1[:, None] / D[..., 1] + g2[:, None] / D[..., 2] + ga[:, None]
        if l.g_dep is not None:
            gw = gw + l.g_dep[:, None] * zs
        T = np.empty((N, S), F)
        carry = np.ones(N, F)
        for b in range(0, S, 64):
            incl = np.cumprod(fac[:, b:b + 64], -1, dtype=F)
            T[:, b:b + 64] = np.concatenate([np.ones((N, 1), F), incl[:, :-1]], -1) * carry[:, None]
            if mutant != "no_Tcarry":
                carry = incl[:, -1] * carry
        w = alpha * T
        own = w * gw
        suffix = np.empty((N, S), F)
        scarry = np.zeros(N, F)
        for b in range(((S + 63) // 64 - 1) * 64, -1, -64):
            o_ = np.zeros((N, 64), F)
            n = min(64, S - b)
            o_[:, :n] = own[:, b:b + n]
            suf = o_.copy()
            step = 1
            while step < 64:
                nxt = suf.copy()
                nxt[:, :64 - step] = suf[:, :64 - step] + suf[:, step:]
                suf, step = nxt, step * 2
            sx = (suf + scarry[:, None]) if mutant == "inclusive" else ((suf - o_) + scarry[:, None])
            suffix[:, b:b + n] = sx[:, :n]
            if mutant != "no_scarry":
                scarry = scarry + suf[:, 0]
        if mutant == "exp":      # a sequential exclusive suffix: "(inclusive - own_s)" leaves gamma_m |own_s| / fac_s, which only the COMPUTED 1 - alpha cancels
            rev = np.cumsum(own[:, ::-1], -1, dtype=F)[:, ::-1]
            suffix = np.concatenate([rev[:, 1:], np.zeros((N, 1), F)], -1)
        g_alpha = T * gw - suffix / fac
        val = g_alpha * dist * (E if mutant == "exp" else oma)
        if mutant == "gate_ge":
            o3 = np.where(sn >= 0, val, F(0))
        elif mutant == "gate_nan":
            o3 = np.where(sn > 0, val, F(0))
        else:
            o3 = np.where(sn <= 0, F(0), val)
        c = F(1) / D
        col = w[..., None] * p.g_rgb[:, None, :] * c * (F(1) - c)
    out = np.concatenate([col, o3[..., None]], -1)
    assert out.dtype == F
    return out


def _vrrf_float64(raw, z, nrm, white, mip):
    """the reference's formula (volume_render_radiance_field) in float64 torch with the kernels' constants; raw[..., 3] is sn"""
    dists = z[..., 1:] - z[..., :-1]
    if not mip:
        dists = torch.cat((dists, torch.full_like(z[..., :1], rc.F_1E10)), -1)
    dists = dists * nrm
    rgb = torch.sigmoid(raw[..., :3])
    alpha = 1.0 - torch.exp(-torch.relu(raw[..., 3]) * dists)
    t = torch.cumprod(1.0 - alpha + rc.F_1EM10, -1)
    t = torch.cat((torch.ones_like(t[..., :1]), t[..., :-1]), -1)
    w = alpha * t
    rgb_map = (w[..., None] * rgb).sum(-2)
    zz = 0.5 * (z[:, :-1] + z[:, 1:]) if mip else z
    depth = (w * zz).sum(-1)
    acc = w.sum(-1)
    if white:
        rgb_map = rgb_map + (1.0 - acc[..., None])
    return rgb_map, acc, depth


@pytest.mark.parametrize("i,mip", PAIRS, ids=PAIR_IDS)
def test_backward64_equals_float64_autograd(i, mip):
    """the division-free form is the same function: every launch without a NaN, on the rays whose sum of x is below 20"""
    p = bc.inputs(i, mip)
    seen = 0
    for name in ("plain", "white", "noise", "noise+white", "knife"):
        l, ref = p.L[name], bc.reference(i, mip, name)
        st = rc.stages64(p.raw, p.z, p.rays, l.noise, p.mip)
        r64 = torch.tensor(np.concatenate([p.raw[..., :3].astype(np.float64), st.sn[..., None]], -1), requires_grad=True)
        rgb, acc, depth = _vrrf_float64(r64, torch.tensor(p.z.astype(np.float64)), torch.tensor(st.nrm), l.white, p.mip)
        loss = (rgb * torch.tensor(p.g_rgb.astype(np.float64))).sum()
        if l.g_acc is not None:
            loss = loss + (acc * torch.tensor(l.g_acc.astype(np.float64))).sum()
        if l.g_dep is not None:
            loss = loss + (depth * torch.tensor(l.g_dep.astype(np.float64))).sum()
        loss.backward()
        want = r64.grad.numpy()
        ok = st.x.sum(-1) < 20
        seen += int(ok.sum())
        if ok.any():
            scale = np.abs(want[ok]).max(axis=(1, 2), keepdims=True)
            err = np.abs(ref.g_raw[ok] - want[ok])
            assert (err <= 1e-9 * np.maximum(np.abs(want[ok]), 1e-3 * scale)).all(), (name, float((err / np.maximum(np.abs(want[ok]), 1e-300)).max()))
    assert seen > 0


@pytest.mark.parametrize("i,mip", PAIRS, ids=PAIR_IDS)
def test_left_out_cap(i, mip):
    for name in bc.LAUNCH_NAMES:
        ref = bc.reference(i, mip, name)
        assert not np.isinf(ref.bound).any(), name
        lo = bc.left_out(ref)
        if lo is None:
            assert bc.CASES[i].S == 1, name
            continue
        n, finite = lo
        print("%s %s: left out %d of %d" % (PAIR_IDS[PAIRS.index((i, mip))], name, n, finite))
        assert n <= max(1, int(bc.LEFT_OUT_CAP * finite)), (name, n, finite)


@pytest.mark.parametrize("i,mip", PAIRS, ids=PAIR_IDS)
def test_nan_rule_on_the_reference(i, mip):
    p = bc.inputs(i, mip)
    c, l = p.c, p.L["special"]
    ref = bc.reference(i, mip, "special")
    base = bc.backward64(p.raw, p.z, p.rays, p.L["noise"].noise, l.white, p.mip, p.g_rgb, l.g_acc, l.g_dep)
    bc.check_rule(PAIR_IDS[PAIRS.index((i, mip))], ref.g_raw, ref.sn, p.where, base.g_raw)
    if c.N >= 8:
        assert all(p.where.get(k) for k in (1, 3, 5, 6, 7)) and (c.S < 2 or p.where.get(2))
    elif c.N == 1:
        assert p.where.get(6)
    k = bc.reference(i, mip, "knife")
    if c.N >= 8:
        sn = k.sn[p.mask]
        assert (sn == 0).any() and (sn > 0).any() and (sn < 0).any()


def _passes(i, mip, name, mutant):
    p = bc.inputs(i, mip)
    try:
        bc.compare("%s %s %s" % (PAIR_IDS[PAIRS.index((i, mip))], name, mutant), kernel32(p, p.L[name], mutant), bc.reference(i, mip, name))
    except AssertionError:
        return False
    return True


@pytest.mark.parametrize("i,mip", PAIRS, ids=PAIR_IDS)
def test_the_restatement_passes_every_launch(i, mip):
    """kernel32 and its "exp(-x) in place of 1 - alpha" variant (closer to the reference) within the bound, NaN exactly where the reference's"""
    p = bc.inputs(i, mip)
    for name in bc.LAUNCH_NAMES:
        for mutant in (None, "exp"):
            bc.compare("%s %s %s" % (PAIR_IDS[PAIRS.index((i, mip))], name, mutant or "kernel32"), kernel32(p, p.L[name], mutant), bc.reference(i, mip, name))
        if name == "special":
            base = kernel32(p, NS(**{**vars(p.L[name]), "noise": p.L["noise"].noise}))
            bc.check_rule("kernel32 " + bc.IDS[i], kernel32(p, p.L[name]).astype(np.float64), bc.reference(i, mip, name).sn, p.where, base.astype(np.float64))


# mutant -> the (case, mip, launch)s it must fail
MUTANTS = {
    "inclusive": [("33x3", 0, "noise"), ("33x64", 1, "white"), ("37x192", 0, "noise")],
    "no_scarry": [("33x129", 0, "plain"), ("37x192", 1, "noise"), ("9x512", 0, "plain")],
    "no_Tcarry": [("33x129", 0, "noise"), ("37x192", 0, "plain"), ("5x511", 1, "special")],
    "gate_ge": [("33x64", 0, "knife"), ("37x192", 1, "knife"), ("1x1", 0, "knife")],
    "gate_nan": [("33x64", 0, "special"), ("37x192", 1, "special"), ("1x1", 0, "special")],
    "last_dist_from_z": [("33x63", 0, "plain"), ("37x192", 0, "noise"), ("33x3", 0, "white")],
    "white_kept": [("33x3", 0, "white"), ("37x192", 1, "noise+white"), ("33x64", 0, "special")],
    "mip_left_edge": [("33x129", 1, "noise"), ("6x2", 1, "knife"), ("37x192", 1, "noise+white")],
}


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_a_mutant_of_the_restatement_fails(mutant):
    for case, mip, name in MUTANTS[mutant]:
        i = bc.IDS.index(case)
        assert _passes(i, mip, name, None)
        assert not _passes(i, mip, name, mutant), "%s passes %s %s" % (mutant, case, name)
        if mutant == "gate_nan":             # the kernel before the fix: only the special launch sees it
            for n in bc.LAUNCH_NAMES:
                if n != "special":
                    assert _passes(i, mip, n, mutant), n
