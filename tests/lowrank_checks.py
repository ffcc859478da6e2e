"""References and bounds for the low-rank plane operators (torch.ops.nvsr.lowrank_planes / lowrank_planes_backward, csrc/lowrank.hip).

A factor tensor is F [1,C,R,2r]; U = F[..., :r], V = F[..., r:]; plane[0,c,y,x] = sum_k U[c,y,k] V[c,x,k] (reference models.py:223-230).

Bounds.  Both kernels compute every output element as ONE chain of f32 fused multiply-adds from +0.0 in a fixed order.  A chain of n fmas has
the classical bound |got - exact| <= gamma(n) sum |a_i b_i| with gamma(n) = n u / (1 - n u), u = 2^-24 (Higham, Accuracy and Stability of
Numerical Algorithms, 3.1: each term passes through at most n roundings).  The tests use gamma(n + 1):
  forward    |plane - ref64| <= gamma(r + 1) sum_k |U||V|
  backward   |dU - ref64|    <= gamma(R + 1) sum_x |G||V|,   |dV - ref64| <= gamma(R + 1) sum_y |G||U|
with ref64 the float64 einsum of the SAME f32 inputs (float64's own error, gamma64(n) ~ n 1.1e-16, is nine orders below and ignored).  An
element whose products are all zero has bound 0 and must be exactly 0."""
import numpy as np
import torch

U32 = 2.0 ** -24


def gamma(n):
    return n * U32 / (1.0 - n * U32)


def make_factors(C, R, r, seed, device=None, std=1.0):
    """F [1,C,R,2r] whose magnitudes span a few binades (normal values times 2^{-3..3}), both signs"""
    g = torch.Generator().manual_seed(seed)
    f = torch.randn(1, C, R, 2 * r, generator=g) * std * torch.exp2(torch.randint(-3, 4, (1, C, R, 2 * r), generator=g).float())
    return f if device is None else f.to(device)


def split64(F, r):
    F = F.detach().double().cpu().reshape(F.shape[-3:])
    return F[..., :r], F[..., r:]


def plane_ref(F, r):
    """-> (float64 plane [C,R,R], sum_k |U||V| [C,R,R])"""
    U, V = split64(F, r)
    return torch.einsum("cyk,cxk->cyx", U, V), torch.einsum("cyk,cxk->cyx", U.abs(), V.abs())


def check_plane(plane, F, r, what=""):
    """plane [1,C,R,R] (any strides) against the forward bound; -> worst err / bound"""
    ref, mag = plane_ref(F, r)
    got = plane.detach().double().cpu().reshape(ref.shape)
    err, bound = (got - ref).abs(), gamma(r + 1) * mag
    bad = err > bound
    worst = float((err / bound.clamp_min(1e-300)).max())
    assert not bool(bad.any()), "%s: %d of %d plane elements outside gamma(r+1) sum|U||V| (worst err / bound %.3g)" % (
        what, int(bad.sum()), bad.numel(), worst)
    return worst


def factor_grad_ref(G, F, r):
    """G [1,C,R,R] (the values the kernel read) -> (float64 dF [C,R,2r], its magnitude sums [C,R,2r])"""
    U, V = split64(F, r)
    G = G.detach().double().cpu().reshape(G.shape[-3:])
    dU, mU = torch.einsum("cyx,cxk->cyk", G, V), torch.einsum("cyx,cxk->cyk", G.abs(), V.abs())
    dV, mV = torch.einsum("cyx,cyk->cxk", G, U), torch.einsum("cyx,cyk->cxk", G.abs(), U.abs())
    return torch.cat([dU, dV], -1), torch.cat([mU, mV], -1)


def check_factor_grad(dF, G, F, r, what=""):
    ref, mag = factor_grad_ref(G, F, r)
    R = F.shape[-2]
    assert tuple(dF.shape) == tuple(F.shape), (dF.shape, F.shape)
    got = dF.detach().double().cpu().reshape(ref.shape)
    err, bound = (got - ref).abs(), gamma(R + 1) * mag
    bad = err > bound
    worst = float((err / bound.clamp_min(1e-300)).max())
    assert not bool(bad.any()), "%s: %d of %d factor-gradient elements outside gamma(R+1) sum|G||.| (worst err / bound %.3g; dU bad %d, dV bad %d)" % (
        what, int(bad.sum()), bad.numel(), worst, int(bad[..., :r].sum()), int(bad[..., r:].sum()))
    return worst


def make_grad(C, R, seed, sparse=False, device=None):
    """dL/d plane [1,C,R,R], NCHW-contiguous; sparse: 80 % of the TEXELS zero (all channels), among them whole rows and columns"""
    g = torch.Generator().manual_seed(seed)
    G = torch.randn(1, C, R, R, generator=g) * torch.exp2(torch.randint(-2, 3, (1, C, R, R), generator=g).float())
    if sparse:
        keep = (torch.rand(R, R, generator=g) < 0.2).float()
        keep[R // 2, :] = 0
        keep[:, R // 3] = 0
        keep[0, :] = 0
        G = G * keep
    return G if device is None else G.to(device)


def rank_dict_ref(resolutions, ratio):
    """the reference's formula (models.py:541): ceil(ratio R) per plane"""
    return [int(np.ceil(ratio * R)) for R in resolutions]


def lowrank_scene(hip, dev, plane_res, ranks, seed, view_res=16):
    """bench.make_synthetic_scene with the three position planes replaced by factor tensors (entries N(0, s^2), s chosen so that the generated
    plane has the synthetic scene's spread 0.7: var = r s^4), plane_rank and one shared generated_planes dict on both models
    -> (coarse, fine, scene id, pose, plane names)"""
    from bench import make_synthetic_scene

    mc, mf, sid, pose = make_synthetic_scene(dev, plane_res=plane_res, view_res=view_res, seed=seed)
    names = [hip.models.get_plane_name(sid, d) for d in range(4)]
    g = torch.Generator().manual_seed(seed + 100)
    planes = {}
    for d, r in enumerate(ranks):
        s = (0.49 / r) ** 0.25
        planes[names[d]] = torch.nn.Parameter((s * torch.randn(1, 48, plane_res, 2 * r, generator=g)).to(dev))
    planes[names[3]] = mc.planes_[names[3]]
    planes = torch.nn.ParameterDict(planes)
    rank, generated = {names[d]: r for d, r in enumerate(ranks)}, {}
    for m in (mc, mf):
        m.planes_, m.plane_rank, m.generated_planes = planes, rank, generated
        m.invalidate()
    return mc, mf, sid, pose, names


def count_launches(monkeypatch, capi, entry="nvsr_lowrank_planes"):
    """count the calls the operators make of one C-ABI entry point (capi.call): -> a list that grows by one per call"""
    calls, inner = [], capi.call

    def counted(name, *a):
        if name == entry:
            calls.append(1)
        return inner(name, *a)

    monkeypatch.setattr(capi, "call", counted)
    return calls


def g26_decoders(g26, g11):
    """the two decoders of fixture g26 as one dict of coarse.* / fine.* arrays: g26 stores only the entries that differ from g11_grads.npz's (two
    full state dicts would take the fixture past the size limit of a committed file), so g26 DEPENDS on g11 -- checked here by the float64 sum,
    sum of squares and element count of g11's decoder arrays that g26 recorded when it was generated (tests/golden/gen_golden_lowrank.py)"""
    base = {k: v for k, v in g11.items() if k.startswith(("coarse.", "fine."))}
    flat = np.concatenate([np.asarray(base[k], dtype=np.float64).reshape(-1) for k in sorted(base)])
    now = np.array([flat.sum(), np.square(flat).sum(), flat.size], dtype=np.float64)
    assert np.array_equal(now, g26["g11_decoders"]), "g11_grads.npz is not the file g26_lowrank.npz was generated from: regenerate g26 (gen_golden_lowrank.py)"
    base.update({k: v for k, v in g26.items() if k.startswith(("coarse.", "fine."))})
    return base
