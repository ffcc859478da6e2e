"""GPU tests of the low-rank feature planes: the two operators against float64 with the bounds of tests/lowrank_checks.py, their bit
identities (run to run, alone vs inside a ragged launch), the registered autograd, and the model wiring (gen_plane, the generated-plane
cache, detach, evaluation, TrainStep / GraphedTrainStep)."""
import pytest
import torch

import lowrank_checks as lc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (R, r): below the MFMA k-step, r == R, r odd (factor rows not 16-byte aligned), R below / one past / one below a multiple of the 16-texel tile
SHAPES = [(5, 1), (5, 5), (12, 3), (17, 4), (33, 5), (70, 7)]
# C: the shipped 48, 24 and 5 (not a multiple of 4), and 50 / 96: a second channel group (of 2 channels: two of the four waves idle; a full one)
CASES = [(48, R, r) for R, r in SHAPES] + [(24, 17, 4), (24, 33, 5), (5, 17, 4), (5, 33, 5), (50, 17, 4), (50, 33, 5), (96, 17, 4)]
IDS = ["C%d-R%d-r%d" % c for c in CASES]


def gen(factors, ranks):
    return torch.ops.nvsr.lowrank_planes(factors, ranks)


def bwd(grads, factors, ranks):
    return torch.ops.nvsr.lowrank_planes_backward(grads, factors, ranks)


@pytest.mark.parametrize("C,R,r", CASES, ids=IDS)
def test_forward_bound_layout_and_repeat(hip, C, R, r):
    F = lc.make_factors(C, R, r, seed=R * 100 + r, device=DEV)
    (p,) = gen([F], [r])
    assert tuple(p.shape) == (1, C, R, R) and p.dtype == torch.float32
    assert p.permute(0, 2, 3, 1).is_contiguous(), "the plane's memory is channel-last [R][R][C]"
    if R > 1 and C > 1:
        assert hip.models.is_native_layout(p)
    worst = lc.check_plane(p, F, r, "C%d R%d r%d" % (C, R, r))
    print("forward C%d R%d r%d: worst err / bound %.3f" % (C, R, r, worst))
    assert torch.equal(p, gen([F], [r])[0])


def test_unaligned_factor_tensor_takes_the_dword_path(hip):
    """r % 4 == 0 lets the generate kernel load 16 bytes per lane -- if the factor tensor is 16-byte aligned.  A tensor at a 4-byte offset gives
    the same bits through the guarded dword loads."""
    C, R, r = 48, 33, 8
    F = lc.make_factors(C, R, r, seed=77, device=DEV)
    buf = torch.empty(F.numel() + 1, device=DEV)
    Fo = buf[1:].view(F.shape)
    Fo.copy_(F)
    assert F.data_ptr() % 16 == 0 and Fo.data_ptr() % 16 == 4 and Fo.is_contiguous()
    p, po = gen([F], [r])[0], gen([Fo], [r])[0]
    lc.check_plane(p, F, r, "aligned")
    assert torch.equal(p, po)
    G = lc.make_grad(C, R, seed=78, device=DEV)
    assert torch.equal(bwd([G], [F], [r])[0], bwd([G], [Fo], [r])[0])


def test_ragged_launch_equals_single_launches(hip):
    shapes = [(12, 3), (33, 5), (17, 17)]
    Fs = [lc.make_factors(48, R, r, seed=7 + i, device=DEV) for i, (R, r) in enumerate(shapes)]
    ranks = [r for _, r in shapes]
    together = gen(Fs, ranks)
    for F, r, p in zip(Fs, ranks, together):
        assert torch.equal(p, gen([F], [r])[0])
        lc.check_plane(p, F, r)
    Gs = [lc.make_grad(48, R, seed=3 + i, device=DEV) for i, (R, _) in enumerate(shapes)]
    d_together = bwd(Gs, Fs, ranks)
    for G, F, r, d in zip(Gs, Fs, ranks, d_together):
        assert torch.equal(d, bwd([G], [F], [r])[0])


def test_fifteen_planes_in_one_launch_and_the_sixteenth_refused(hip):
    shapes = [(5 + 2 * i, 1 + i % 4) for i in range(15)]
    Fs = [lc.make_factors(24, R, r, seed=40 + i, device=DEV) for i, (R, r) in enumerate(shapes)]
    ranks = [r for _, r in shapes]
    for F, r, p in zip(Fs, ranks, gen(Fs, ranks)):
        lc.check_plane(p, F, r)
    Gs = [lc.make_grad(24, R, seed=i, device=DEV) for i, (R, _) in enumerate(shapes)]
    for G, F, r, d in zip(Gs, Fs, ranks, bwd(Gs, Fs, ranks)):
        lc.check_factor_grad(d, G, F, r)
    with pytest.raises(hip.capi.NvsrError, match="NVSR_ERR_SHAPE"):
        gen(Fs + Fs[:1], ranks + ranks[:1])
    with pytest.raises(hip.capi.NvsrError, match="NVSR_ERR_SHAPE"):
        bwd(Gs + Gs[:1], Fs + Fs[:1], ranks + ranks[:1])
    torch.cuda.synchronize()


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
@pytest.mark.parametrize("C,R,r", CASES, ids=IDS)
def test_backward_bound_layouts_and_repeat(hip, C, R, r, sparse):
    F = lc.make_factors(C, R, r, seed=R * 100 + r + 1, device=DEV)
    G = lc.make_grad(C, R, seed=R + r, sparse=sparse, device=DEV)                 # NCHW-contiguous
    G_cl = G.contiguous(memory_format=torch.channels_last) if (R > 1 and C > 1) else G
    (d,) = bwd([G], [F], [r])
    worst = lc.check_factor_grad(d, G, F, r, "C%d R%d r%d %s" % (C, R, r, "sparse" if sparse else "dense"))
    print("backward C%d R%d r%d sparse=%d: worst err / bound %.3f" % (C, R, r, sparse, worst))
    assert torch.equal(d, bwd([G], [F], [r])[0])
    assert torch.equal(d, bwd([G_cl], [F], [r])[0]), "a channels_last gradient (read in place) and an NCHW one (re-laid out) hold the same values"


def test_directional_derivative_matches_the_gradient(hip):
    """<G, plane(F + eD) - plane(F - eD)> / 2e against <dF, D>, both sides accumulated in float64: the plane is bilinear in (U, V), so the central
    difference is exact up to the rounding of the two f32 planes: |diff| <= 2 gamma(r+1) sum|G| sum_k|U||V| / 2e (+ the backward's own bound)"""
    C, R, r, eps = 48, 17, 4, 2.0 ** -6
    F = lc.make_factors(C, R, r, seed=5, device=DEV)
    D = lc.make_factors(C, R, r, seed=6, device=DEV)
    G = lc.make_grad(C, R, seed=8, device=DEV)
    Fp, Fm = F + eps * D, F - eps * D                                            # (exactly representable steps are not needed: both sides use Fp, Fm)
    pp, pm = gen([Fp], [r])[0].double(), gen([Fm], [r])[0].double()
    lhs = float((G.double() * (pp - pm)).sum()) / (2 * eps)
    # the exact derivative of the bilinear map at the midpoint F0 = (Fp + Fm) / 2 in direction (Fp - Fm) / 2e
    F0, Dd = (Fp.double() + Fm.double()) / 2, (Fp.double() - Fm.double()) / (2 * eps)
    (dF,) = bwd([G], [F0.float()], [r])
    rhs = float((dF.double() * Dd).sum())
    _, mag_p = lc.plane_ref(Fp, r)
    _, mag_m = lc.plane_ref(Fm, r)
    Gc = G.double().cpu()[0].abs()
    tol = float((Gc * (mag_p + mag_m)).sum()) * lc.gamma(r + 1) / (2 * eps)
    # F0.float() rounds the midpoint (relative 2^-24 per element) and dF carries gamma(R+1): both inside the second term
    _, gmag = lc.factor_grad_ref(G, F0.float(), r)
    tol += float((gmag * Dd.cpu()[0].abs()).sum()) * (lc.gamma(R + 1) + 2.0 ** -23)
    print("directional derivative: %.9g vs %.9g, |diff| %.3g, tolerance %.3g" % (lhs, rhs, abs(lhs - rhs), tol))
    assert abs(lhs - rhs) <= tol
    assert abs(lhs) > 100 * tol, "the test is vacuous if the derivative itself is inside the tolerance"


def test_registered_autograd_is_the_backward_operator(hip):
    shapes = [(12, 3), (17, 4)]
    Fs = [lc.make_factors(48, R, r, seed=20 + i, device=DEV).requires_grad_() for i, (R, r) in enumerate(shapes)]
    ranks = [r for _, r in shapes]
    planes = gen(Fs, ranks)
    G0 = lc.make_grad(48, 12, seed=1, device=DEV)
    (planes[0] * G0).sum().backward()                                           # plane 1 gets no gradient at all
    assert torch.equal(Fs[0].grad, bwd([G0], [Fs[0].detach()], [3])[0])
    assert Fs[1].grad is None or not bool(Fs[1].grad.any())
    torch.library.opcheck(torch.ops.nvsr.lowrank_planes, ([f.detach() for f in Fs], ranks),
                          test_utils=("test_schema", "test_faketensor", "test_autograd_registration"))
    torch.library.opcheck(torch.ops.nvsr.lowrank_planes_backward, ([G0], [Fs[0].detach()], [3]), test_utils=("test_schema", "test_faketensor"))


# ---------------------------------------------------------------------------------------------------------------------------------
# end to end against the reference (g26) and the model wiring
# ---------------------------------------------------------------------------------------------------------------------------------
def _g26_models(hip):
    from conftest import load_golden
    from test_hip_parity import _grad_models

    g, g11 = load_golden("g26_lowrank.npz"), load_golden("g11_grads.npz")
    dec = lc.g26_decoders(g, g11)                  # (g26 stores what differs from g11's decoders, and checks that g11 is the file it was made from)
    dec["box"] = g["box"]
    sid = "lego_DS8_PlRes12_6"
    mc, mf = _grad_models(hip, dec, [g["plane%d" % d] for d in range(4)], sid)
    names = [hip.models.get_plane_name(sid, d) for d in range(4)]
    rank, generated = {names[d]: int(g["ranks"][d]) for d in range(3)}, {}
    for m in (mc, mf):
        m.plane_rank, m.generated_planes = rank, generated
    return g, mc, mf, sid, names


def test_train_iteration_vs_reference(hip, monkeypatch):
    """run_one_iter_of_nerf(mode='train') + backward on the reference's low-rank scene (g26): generated planes against the fixture's factors
    (forward bound) and the reference's planes, rgb / loss / gradients by the rule of test_plane_gradients_golden (the fine depths are regenerated
    by each side: a few importance samples move, so gradients compare in aggregate); one generation launch serves both passes"""
    from test_hip_parity import N_, T, make_options
    import numpy as np

    g, mc, mf, sid, names = _g26_models(hip)
    nc, nf = (int(v) for v in g["samples"])
    opts, scfg = make_options(nc, nf)
    launches = lc.count_launches(monkeypatch, hip.capi)
    out = hip.train_utils.run_one_iter_of_nerf(8, 8, float(g["hwf"][2]), mc, mf, T(g["rays"]), opts, sid, mode="train", scene_config=scfg, randoms={})
    assert len(launches) == 1, "coarse and fine share one generation of all three planes"
    for d in range(3):
        p = mc.generated_planes[names[d]]
        assert mf.gen_plane(names[d]) is p and hip.models.is_native_layout(p)
        lc.check_plane(p, T(g["plane%d" % d]), int(g["ranks"][d]), "g26 plane %d" % d)
        # the reference's own CPU matmul meets the same bound, so the two are within twice the bound of each other
        _, mag = lc.plane_ref(T(g["plane%d" % d]), int(g["ranks"][d]))
        assert bool(((p.detach().cpu().double()[0] - torch.from_numpy(g["generated%d" % d]).double()[0]).abs() <= 2 * lc.gamma(int(g["ranks"][d]) + 1) * mag).all())
    target = T(g["target"])
    np.testing.assert_allclose(N_(out[0]), g["rgb_coarse"], rtol=0, atol=2e-5)
    loss = torch.nn.functional.mse_loss(out[0], target) + torch.nn.functional.mse_loss(out[3], target)
    assert abs(float(loss.detach()) - float(g["loss"])) < 2e-4
    loss.backward()
    for d in range(4):
        got, ref = N_(mc.planes_[names[d]].grad), g["grad_plane%d" % d]
        assert got.shape == ref.shape
        rel = np.linalg.norm(got - ref) / np.linalg.norm(ref)
        print("g26 plane %d: factor-gradient relative L2 %.2e, max err / max %.2e" % (d, rel, np.abs(got - ref).max() / np.abs(ref).max()))
        assert rel < 1e-2, "plane %d: relative L2 error %.2e" % (d, rel)
        assert np.abs(got - ref).max() <= 3e-2 * np.abs(ref).max()


def test_generated_plane_cache_follows_the_factors(hip, monkeypatch):
    """one generation per factor version: an optimizer step, a `.data` write + invalidate(), generated_planes.clear() and clear_plane_cache()
    each regenerate; a stale entry is never served; detach cuts the gradient"""
    from test_hip_parity import T, make_options

    g, mc, mf, sid, names = _g26_models(hip)
    opts, scfg = make_options(8, 8)
    launches = lc.count_launches(monkeypatch, hip.capi)
    rays = T(g["rays"])

    def iteration():
        out = hip.train_utils.run_one_iter_of_nerf(8, 8, float(g["hwf"][2]), mc, mf, rays, opts, sid, mode="train", scene_config=scfg, randoms={})
        (out[0].sum() + out[3].sum()).backward()

    opt = torch.optim.SGD(list(mc.planes_.values()), lr=1e-2)
    iteration()
    assert len(launches) == 1 and all(float(mc.planes_[n].grad.abs().sum()) > 0 for n in names)
    first = mc.generated_planes[names[0]]
    opt.step()
    iteration()
    assert len(launches) == 2 and mc.generated_planes[names[0]] is not first
    lc.check_plane(mc.generated_planes[names[0]], mc.planes_[names[0]], 3, "after the optimizer step")
    # evaluation: built once per factor version, bit for bit a fresh generation; served to both models
    for m in (mc, mf):
        m.eval()
    with torch.no_grad():
        a = mc.gen_plane(names[1])
        n0 = len(launches)
        assert mf.gen_plane(names[1]) is a and mc.gen_plane(names[1]) is a and len(launches) == n0
        assert torch.equal(a, torch.ops.nvsr.lowrank_planes([mc.planes_[names[1]].detach()], [5])[0])
        n0 = len(launches)
        mc.planes_[names[1]].data.mul_(2.0)                  # a write that bumps no version counter ...
        mc.invalidate()                                       # ... needs invalidate(), like every derived copy
        b = mc.gen_plane(names[1])
        assert len(launches) == n0 + 1 and torch.equal(b, 4 * a)          # (U and V both doubled; powers of two are exact)
        stale = mc.generated_planes[names[2]]
        mc.planes_[names[2]].mul_(0.5)                        # an in-place write through autograd's counter: the entry is stale at once
        c = mc.gen_plane(names[2])
        assert c is not stale
        lc.check_plane(c, mc.planes_[names[2]], 12, "after the in-place write")
        n0 = len(launches)
        mc.generated_planes.clear()
        mc.gen_plane(names[0])
        assert len(launches) == n0 + 1
        hip.models.clear_plane_cache()
        mc.gen_plane(names[0])
        assert len(launches) == n0 + 2
    # detach
    for m in (mc, mf):
        m.train()
    assert mc.gen_plane(names[0]).requires_grad and not mc.gen_plane(names[0], detach=True).requires_grad
    assert not mc.raw_plane(names[0], detach=True).requires_grad
    assert mc.gen_plane(names[3]) is mc.planes_[names[3]], "the view-direction plane is never low-rank"


def test_evaluation_render_equals_the_dense_planes_render(hip):
    """an evaluation render of a low-rank scene (ranks 3, 5, 12) is bit for bit the render of the dense planes lowrank_planes returns, assigned
    as ordinary planes_ (the generated planes are sampled in place: same memory layout, same values)"""
    mc, mf, sid, pose, names = lc.lowrank_scene(hip, DEV, 24, (3, 5, 12), seed=6, view_res=8)
    from bench import render_options
    import numpy as np

    H = W = 12
    focal = 0.5 * W / np.tan(0.5 * 0.6911112)
    ro, rd = hip.nerf_helpers.get_ray_bundle(H, W, focal, pose)
    opts, scfg = render_options(16, 16)
    for m in (mc, mf):
        m.eval()
    with torch.no_grad():
        low = hip.train_utils.eval_nerf(H, W, focal, mc, mf, ro, rd, opts, scene_id=sid, scene_config=scfg)
        dense = torch.ops.nvsr.lowrank_planes([mc.planes_[n].detach() for n in names[:3]], [3, 5, 12])
        planes = torch.nn.ParameterDict({n: torch.nn.Parameter(p) for n, p in zip(names[:3], dense)})
        planes[names[3]] = mc.planes_[names[3]]
        for m in (mc, mf):
            m.planes_, m.plane_rank = planes, None
            m.invalidate()
        ref = hip.train_utils.eval_nerf(H, W, focal, mc, mf, ro, rd, opts, scene_id=sid, scene_config=scfg)
    assert torch.equal(low[0], ref[0]) and torch.equal(low[3], ref[3])
    assert float(low[3].std()) > 1e-3


def test_graphed_planes_only_step_with_low_rank_planes(hip):
    """GraphedTrainStep on a planes-only step whose position planes are low-rank: the factors after 3 replays against 3 eager iterations from the
    same state and random inputs, to the tolerance test_graph_replay_equals_the_eager_iteration uses for what it compares (relative L2 1e-5: the
    plane scatter's float atomics order differently run to run, and runs of several iterations drift apart by that noise whatever launches them;
    SGD, as there, keeps it from being amplified).  The replays must have moved every factor by at least 100 times that tolerance, so a graph
    that left the generation or its backward out cannot pass.  Measured on an MI355X: |difference| / |factors| <= 1.5e-8 with an update of 2.6e-3 ..
    3.0e-3 of the factors' norm, i.e. 4e-6 .. 5e-6 of the three steps' update (printed)."""
    import numpy as np
    from bench import render_options

    H = W = 48
    focal = 0.5 * W / np.tan(0.5 * 0.6911112)
    N, Nc, Nf = 512, 16, 16
    gen_ = torch.Generator(device=DEV).manual_seed(5)
    img = torch.rand(H, W, 3, device=DEV, generator=gen_)

    def setup():
        mc, mf, sid, pose, names = lc.lowrank_scene(hip, DEV, 32, (3, 5, 12), seed=11)
        for m in (mc, mf):
            for n, p in m.named_parameters():
                p.requires_grad_("planes_" in n)
            m.train()
        opts, scfg = render_options(Nc, Nf, perturb=True, noise=0.2)
        planes = list(mc.planes_.values())
        popt = torch.optim.SGD(planes, lr=10.0)          # (MSE gradients of a 512-ray batch are small: three steps move a factor by ~4e-3 of its norm)
        sampler = hip.training.DevicePixelSampler(seed=77)
        step = hip.training.TrainStep(mc, mf, opts, {"LR_planes"}, planes_optimizer=popt, pixel_sampler=sampler)
        return dict(mc=mc, sid=sid, pose=pose, scfg=scfg, planes=planes, sampler=sampler, step=step)

    a, b = setup(), setup()
    rnd = dict(t_rand=torch.rand(N, Nc, device=DEV, generator=gen_), u=torch.rand(N, Nf, device=DEV, generator=gen_),
               noise_coarse=0.2 * torch.randn(N, Nc, device=DEV, generator=gen_), noise_fine=0.2 * torch.randn(N, Nc + Nf, device=DEV, generator=gen_))
    graphed = hip.training.GraphedTrainStep(b["step"], img, b["pose"], H, W, focal, 1, b["sid"], b["scfg"], N, randoms_fn=rnd, warmup=2)
    with torch.no_grad():
        for pa, pb in zip(a["planes"], b["planes"]):
            pa.copy_(pb)
    a["sampler"].calls = b["sampler"].calls
    start = [p.detach().clone() for p in b["planes"]]
    for k in range(3):
        a["step"](k, img, a["pose"], H, W, focal, 1, a["sid"], a["scfg"], N, randoms=rnd)
        graphed()
    torch.cuda.synchronize()
    for i, (pa, pb, p0) in enumerate(zip(a["planes"], b["planes"], start)):
        moved, size = float((pb.detach() - p0).norm()), float(pa.detach().norm())
        rel = float((pa.detach() - pb.detach()).norm()) / size
        print("graphed vs eager, plane %d: |difference| / |factors| %.2e, |update| / |factors| %.2e, |difference| / |update| %.2e" % (
            i, rel, moved / size, rel * size / moved))
        assert moved / size >= (1e-3 if i < 3 else 1e-6), "plane %d hardly trained in the replays (%.2e of its norm)" % (i, moved / size)      # (3: the dense view plane)
        assert rel <= 1e-5, (i, rel)
        if i < 3:
            # each of the three gradients is within 1e-5 of its twin (the existing test's tolerance), so the sum of the three steps is within
            # 3e-5 of the update when the steps point the same way; a backward error inside the graph shows here, not against the factors' norm
            assert rel * size / moved <= 3e-5, (i, rel * size / moved)
    # an eager use between replays sees the factors as the replays left them
    with torch.no_grad():
        lc.check_plane(b["mc"].gen_plane(hip.models.get_plane_name(b["sid"], 0)), b["planes"][0], 3, "after the replays")


def test_sr_refinement_trains_the_factors_of_low_rank_lr_planes(hip):
    """The image-consistency iteration of tests/test_hip_round4.py (the smallest SR geometry a GPU test trains: 20^2 LR planes, x4 EDSR with 16
    channels and 2 blocks, 320 HR rays) with the LR planes low-rank and 'LR_planes' trained: assign_LR_planes hands the GENERATED planes to the SR
    model, so one TrainStep leaves gradients on the factors.  They equal the gradients of the same step on a twin whose planes_ are the generated
    dense planes as leaves, contracted with the factors in float64 -- to 1e-5 relative (that test's tolerance; the plane scatter's float atomics
    order differently run to run)."""
    import copy

    import numpy as np
    from conftest import load_golden
    from test_hip_parity import T, _grad_models, make_options

    tr = hip.training
    g = load_golden("g11_grads.npz")
    sid, R, ranks, ds = "lego_DS8_PlRes20_8", 20, (3, 5, 20), 4
    H = W = 10
    focal = 0.5 * W / np.tan(0.5 * 0.6911112)
    pose = T(load_golden("g08_render.npz")["pose"])
    opts, scfg = make_options(16, 16)
    gen_ = torch.Generator().manual_seed(31)
    factors = [((0.25 / r) ** 0.25 * torch.randn(1, 48, R, 2 * r, generator=gen_)).numpy() for r in ranks]
    view = (0.5 * torch.randn(1, 48, 8, 8, generator=gen_)).numpy()
    names = [hip.models.get_plane_name(sid, d) for d in range(4)]
    img = torch.rand(H, W, 3, generator=torch.Generator().manual_seed(5)).to(DEV)
    torch.manual_seed(9)
    sr0 = hip.models.PlanesSR(hip.models.EDSR, ds, 48, 48, {"model": {"hidden_size": 16, "n_blocks": 2}}, "bilinear").to(DEV)
    with torch.no_grad():
        for p_ in sr0.parameters():
            p_.mul_(10.0)

    def one_step(planes, rank):
        mc, mf = _grad_models(hip, g, planes, sid, what=("planes",))
        generated = {}
        for m in (mc, mf):
            m.plane_rank, m.generated_planes = rank, generated
        sr = copy.deepcopy(sr0)
        mf.assign_SR_model(sr, SR_viewdir=False)
        mf.assign_LR_planes()
        sr.train()
        opt = torch.optim.SGD(sr.parameters(), lr=1e-3)
        step = tr.TrainStep(mc, mf, opts, {"SR", "LR_planes"}, SR_optimizer=opt, SR_model=sr, sr_loss="fine", im_inconsistency_loss_w=1.0, ds_factor=ds)
        np.random.seed(11)
        r = step(0, img, pose, H, W, focal, ds, sid, scfg, 320, sr_iter=True, im_consistency_iter=True)
        return mc, r

    mc_low, r_low = one_step(factors + [view], {names[d]: ranks[d] for d in range(3)})
    with torch.no_grad():
        dense = torch.ops.nvsr.lowrank_planes([T(f) for f in factors], list(ranks))
    mc_dense, r_dense = one_step([p.contiguous().cpu().numpy() for p in dense] + [view], None)
    assert abs(r_low["loss"] - r_dense["loss"]) <= 1e-5 * max(1.0, abs(r_dense["loss"])), (r_low["loss"], r_dense["loss"])
    for d in range(3):
        got = mc_low.planes_[names[d]].grad
        assert got is not None and float(got.abs().sum()) > 0, "factor %d received no gradient through the SR network" % d
        G = mc_dense.planes_[names[d]].grad
        ref, _ = lc.factor_grad_ref(G, T(factors[d]), ranks[d])
        rel = float((got.double().cpu()[0] - ref).norm() / ref.norm())
        print("SR refinement, factor %d: relative L2 %.2e against the dense twin" % (d, rel))
        assert rel <= 1e-5, (d, rel)
    gv, gv_ref = mc_low.planes_[names[3]].grad, mc_dense.planes_[names[3]].grad
    assert float((gv - gv_ref).norm() / gv_ref.norm()) <= 1e-5
