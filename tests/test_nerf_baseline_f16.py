"""GPU tests of the f16x2 arithmetic of the two FlexibleNeRFModel baselines (csrc/nerf_mlp.h: Mip-NeRF, mip.hip, and positional-encoding
NeRF, pe.hip), against the g23 / g24 fixtures and the bf16x3 path.

  range ................. a weight |W| >= 255 or an activation |x| >= 4094 gives NaN (never a finite wrong number) and raises bit 1 of the range
                          flag; bf16x3 is finite there and leaves the flag alone
  accuracy .............. the bounds of the bf16x3 tests (tests/test_mip_nerf.py, tests/test_pe_nerf.py): f16x2's worst case per product,
                          2^-21 |W||x|, is no looser than bf16x3's
  backward .............. one power of two per point: the gradients of loss 2^k are 2^k times those of the loss, bit for bit
  evaluation ............ an out-of-range frame is rendered again in bf16x3 (warned once), later frames of the same parameters go there directly
  training .............. TrainStep / GraphedTrainStep run the baselines; an out-of-range iteration raises when its metrics are read
"""
import copy
import sys
import warnings

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden
from nerf_baseline_checks import DEV, N_, T, chain_abs_sum, check_grads, check_render, cpu_eval, scene
import nerf_baseline_checks as checks

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import mip_params  # noqa: E402
import pe_params  # noqa: E402

pytestmark = pytest.mark.gpu
MODELS = ["mip", "pe"]

SPEC = {
    "mip": dict(npz="g23_mip_nerf.npz", params=mip_params, kwargs=dict(include_input_xyz=False), encode="mip", enc=36, extra=1,
                fwd_tags=(("a.", "raw"),), train_seed=23, chunk=400, adam_seed=29),
    "pe": dict(npz="g24_pe_nerf.npz", params=pe_params, kwargs={}, encode="positional_encoding", enc=39, extra=0,
               fwd_tags=(("a.", "raw"), ("a.ndc.", "ndc.raw")), train_seed=24, chunk=100, adam_seed=31),
}
_G = {}


def gold(model):
    if model not in _G:
        _G[model] = load_golden(SPEC[model]["npz"])
    return _G[model]


def scene_id(model, g):
    return "lego_DS8" if model == "mip" else str(g["scene_id"])


def models_from(hip, model, arith):
    s = SPEC[model]
    return checks.models_from(hip, gold(model), arith, s["params"], **s["kwargs"])


def opts(model, **kw):
    return checks.opts(SPEC[model]["encode"], **kw)


def run(hip, model, mc, mf, o, mode, ndc=False, randoms=None):
    g = gold(model)
    H, W, focal = g["c.hwf"]
    rays = torch.stack((T(g["c.ro"]).reshape(-1, 3), T(g["c.rd"]).reshape(-1, 3)))
    return hip.train_utils.run_one_iter_of_nerf(int(H), int(W), float(focal), mc, mf, rays, o, scene_id(model, g), mode=mode,
                                                scene_config=scene(ndc), randoms=randoms)


def forward(model, m, tag):
    """the fused model call on the fixture's tag -> raw [P, 4] (numpy)"""
    g = gold(model)
    with torch.no_grad():
        if model == "mip":
            raw = m.mip_forward(T(g[tag + "rays"]), T(g[tag + "edges"]), float(g["radius"]))
        else:
            raw = m.pe_forward(T(g[tag + "rays"]), T(g[tag + "z"]))
    return N_(raw).reshape(-1, 4)


def encoded(model, tag):
    g = gold(model)
    return np.concatenate([g[tag + "ipe"] if model == "mip" else g[tag + "enc"], g[tag + "dirs"]], -1)


def flag_word(hip):
    torch.cuda.synchronize()
    return int(N_(hip.capi.range_flag(torch.device(DEV)).word)[0])


def reset_flag(hip):
    hip.capi.range_flag(torch.device(DEV)).reset()


# ---- the range contract ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("model", MODELS)
def test_out_of_range_weight_gives_nan_and_raises_the_flag(hip, model):
    for arith in ("f16x2", "bf16x3"):
        m = models_from(hip, model, arith)[0]
        with torch.no_grad():
            m.layers_xyz[1].weight[5, 7] = 300.0
        reset_flag(hip)
        raw = forward(model, m, "a.")
        word = flag_word(hip)
        if arith == "f16x2":
            # (h3[5] is NaN for every point, and every later layer reads all of h3)
            assert np.isnan(raw).all(), "%d finite raw values" % int(np.isfinite(raw).sum())
            assert word & 1, word
        else:
            assert np.isfinite(raw).all() and word == 0


def _layer_inputs_max(sd, x, enc):
    """float64 per point: the largest |value| that enters a layer's products (encoding, h1 .. h4, feat and directions, hd)"""
    Wr = lambda k: sd[k + ".weight"].astype(np.float64)
    b = lambda k: sd[k + ".bias"].astype(np.float64)
    relu = lambda v: np.maximum(v, 0)
    xyz, view = x[:, :enc].astype(np.float64), x[:, enc:].astype(np.float64)
    mx = np.abs(x).max(1)
    h = xyz @ Wr("layer1").T + b("layer1")
    for j in range(3):
        mx = np.maximum(mx, np.abs(h).max(1))
        h = relu(h @ Wr("layers_xyz.%d" % j).T + b("layers_xyz.%d" % j))
    mx = np.maximum(mx, np.abs(h).max(1))
    feat = relu(h @ Wr("fc_feat").T + b("fc_feat"))
    mx = np.maximum(mx, np.abs(feat).max(1))
    hd = relu(np.concatenate([feat, view], -1) @ Wr("layers_dir.0").T + b("layers_dir.0"))
    return np.maximum(mx, np.abs(hd).max(1))


@pytest.mark.parametrize("model", MODELS)
def test_out_of_range_activation_gives_nan_and_raises_the_flag(hip, model):
    s = SPEC[model]
    sd = s["params"].state_dict(s["params"].SEEDS[0])
    # layer1 scaled to |W| = 250 and layers_xyz.0 by 4: every |W| < 255 ...
    k = 250.0 / float(np.abs(sd["layer1.weight"]).max())
    sd = dict(sd)
    sd["layer1.weight"], sd["layer1.bias"] = sd["layer1.weight"] * k, sd["layer1.bias"] * k
    sd["layers_xyz.0.weight"] = sd["layers_xyz.0.weight"] * 4.0
    assert max(float(np.abs(v).max()) for n, v in sd.items() if n.endswith("weight")) < 255
    mx = _layer_inputs_max(sd, encoded(model, "a."), s["enc"])
    over, under = mx >= 4094 * 1.001, mx < 4094 * 0.999
    assert over.any() and under.any(), "the scaled model keeps every activation in range"       # ... and some activations beyond 4094
    for arith in ("f16x2", "bf16x3"):
        m = models_from(hip, model, arith)[0]
        with torch.no_grad():
            m.layer1.weight.mul_(k)
            m.layer1.bias.mul_(k)
            m.layers_xyz[0].weight.mul_(4.0)
        reset_flag(hip)
        raw = forward(model, m, "a.")
        word = flag_word(hip)
        if arith == "f16x2":
            assert np.isnan(raw[over]).any(-1).all(), "%d of %d points beyond the range came out finite" % (int(np.isfinite(raw[over]).all(-1).sum()), int(over.sum()))
            assert np.isfinite(raw[under]).all()
            assert word & 1, word
        else:
            assert np.isfinite(raw).all() and word == 0


@pytest.mark.parametrize("model", MODELS)
def test_no_finite_wrong_number(hip, model):
    """all weights x 2^j, j = 0..9: every raw element is NaN or within the accuracy bound of the bf16x3 result"""
    s = SPEC[model]
    x = encoded(model, "a.")
    nan_seen = False
    for j in range(10):
        out = {}
        for arith in ("f16x2", "bf16x3"):
            m = models_from(hip, model, arith)[0]
            with torch.no_grad():
                for l in m._layers():
                    l.weight.mul_(2.0 ** j)
            out[arith] = forward(model, m, "a.")
        sd = {k: v.astype(np.float64) * (2.0 ** j if k.endswith("weight") else 1.0) for k, v in s["params"].state_dict(s["params"].SEEDS[0]).items()}
        tol = 1e-5 + 2e-6 * chain_abs_sum(sd, x, s["enc"])
        f, b = out["f16x2"], out["bf16x3"]
        ok = np.isnan(f) | (np.abs(f - b) <= tol)
        assert ok.all(), "j=%d: %d finite values off by up to %.3e (bound %.3e)" % (j, int((~ok).sum()), float(np.nanmax(np.abs(f - b)[~ok])), tol)
        nan_seen |= bool(np.isnan(f).any())
    assert nan_seen           # (the largest scales do leave the range)


def _fixture_op(hip, model):
    """(forward op, backward op, the fixture's encoder inputs of tag a.)"""
    g, nv = gold(model), torch.ops.nvsr
    if model == "mip":
        return nv.mip_nerf, nv.mip_nerf_backward, (T(g["a.rays"]), T(g["a.edges"]), float(g["radius"]))
    return nv.pe_nerf, nv.pe_nerf_backward, (T(g["a.rays"]), T(g["a.z"]))


@pytest.mark.parametrize("model", MODELS)
def test_backward_overflow_raises_the_flag(hip, model):
    """the data backward alone, on a finite record: layers_xyz.1 and .2 at |W| = 250 (in range) make the gradient chain grow past f16 in
    their transposed products -> f16x2 writes non-finite gradients and raises the flag; bf16x3 is finite and leaves it alone"""
    A = hip.capi.ARITHMETIC
    m = models_from(hip, model, "bf16x3")[0]
    with torch.no_grad():
        for l in (m.layers_xyz[1], m.layers_xyz[2]):
            l.weight.mul_(250.0 / float(l.weight.abs().max()))
    nat = m.natural_blob()
    fwd, bwd, inputs = _fixture_op(hip, model)
    raw, rec = fwd(*inputs, nat, True, A["bf16x3"])
    assert torch.isfinite(rec).all() and torch.isfinite(raw).all()
    g_raw = torch.ones_like(raw)
    for arith in ("f16x2", "bf16x3"):
        reset_flag(hip)
        grec = bwd(nat, rec, g_raw, A[arith])
        word = flag_word(hip)
        if arith == "f16x2":
            assert not torch.isfinite(grec).all() and word & 1, word
        else:
            assert torch.isfinite(grec).all() and word == 0


@pytest.mark.parametrize("model", MODELS)
def test_f16x2_backward_with_dl_dalpha_far_above_dl_drgb(hip, model):
    """behind a surface dL/dalpha of a sample can exceed its dL/drgb by many binades: the rgb chain keeps a scale of its own, so the gradients
    of fc_rgb, layers_dir and fc_feat stay as accurate as with balanced dL/draw (one scale per point would run that chain in subnormal f16)"""
    s = SPEC[model]
    torch.manual_seed(6)
    m = hip.models.FlexibleNeRFModel(**s["kwargs"]).to(DEV)
    m.arithmetic = "f16x2"
    N, S = 1024, 32
    rays = hip.train_utils.pack_rays(torch.randn(N, 3, device=DEV), torch.randn(N, 3, device=DEV), 2.0, 6.0)
    if model == "mip":
        d = torch.sort(2.0 + 4.0 * torch.rand(N, S + 1, device=DEV), -1)[0]
        radius = hip.train_utils.mip_radius("lego_DS8")
        raw = m.mip_forward(rays, d, radius)
        x = torch.ops.nvsr.mip_encode(rays, d, radius).cpu().double()
    else:
        d = torch.sort(2.0 + 4.0 * torch.rand(N, S, device=DEV), -1)[0]
        raw = m.pe_forward(rays, d)
        x = torch.ops.nvsr.pe_encode(rays, d).cpu().double()
    g_raw = torch.randn_like(raw)
    g_raw[..., 3] *= 2.0 ** 24
    (raw * g_raw).sum().backward()
    gr = g_raw.reshape(-1, 4).cpu().double()
    _, g64 = cpu_eval(m, x, gr, s["enc"], torch.float64)
    _, g32 = cpu_eval(m, x, gr, s["enc"], torch.float32)
    report = []
    for k, p in m.named_parameters():
        rel = float((p.grad.cpu().double() - g64[k]).norm() / g64[k].norm().clamp_min(1e-30))
        rel32 = float((g32[k] - g64[k]).norm() / g64[k].norm().clamp_min(1e-30))
        report.append("%s %.2e (torch f32 %.2e)" % (k, rel, rel32))
        assert rel <= 4 * rel32 + 2e-3, report


# ---- accuracy: the bounds of the bf16x3 tests ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("model", MODELS)
def test_f16x2_forward_matches_upstream_model(hip, model):
    s, g = SPEC[model], gold(model)
    reset_flag(hip)
    for tag, key in s["fwd_tags"]:
        for i, m in enumerate(models_from(hip, model, "f16x2")):
            raw = forward(model, m, tag)
            tol = 1e-5 + 1e-6 * chain_abs_sum(s["params"].state_dict(s["params"].SEEDS[i]), encoded(model, tag), s["enc"])
            err = np.abs(raw - g["b.m%d.%s" % (i, key)]).max()
            assert err <= tol, "%s model %d: max|err| %.2e > %.2e" % (tag, i, err, tol)
    assert flag_word(hip) == 0


@pytest.mark.parametrize("model", MODELS)
def test_f16x2_validation_render_matches_upstream(hip, model):
    for tag, ndc in (("c.", False), ("c.ndc.", True)):
        mc, mf = models_from(hip, model, "f16x2")
        reset_flag(hip)
        with torch.no_grad(), warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            out = run(hip, model, mc, mf, opts(model), "validation", ndc=ndc)
        check_render(out, gold(model), tag)
        # the NDC scene of the fixture projects rays that graze the near plane to |x| ~ 8000: PE's encoding keeps x itself (include_input),
        # beyond f16x2's 4094 -- that frame is the bf16x3 fallback's, warned; Mip's integrated encoding is damped sin / cos, in range
        fell_back = model == "pe" and ndc
        assert sum("NVSR_ARITH_F16X2" in str(x.message) for x in w) == int(fell_back), tag
        assert flag_word(hip) == 0


@pytest.mark.parametrize("model", MODELS)
def test_f16x2_train_step_outputs_and_gradients_match_upstream(hip, model):
    s, g = SPEC[model], gold(model)
    mc, mf = models_from(hip, model, "f16x2")
    torch.manual_seed(s["train_seed"])
    out = run(hip, model, mc, mf, opts(model, perturb=True, noise=0.2, chunk=s["chunk"]), "train")
    target = T(g["d.target"])
    loss = torch.nn.functional.mse_loss(out[0], target) + torch.nn.functional.mse_loss(out[3], target)
    loss.backward()
    check_render(out, g, "d.")
    check_grads((mc, mf), g, "d")


@pytest.mark.parametrize("model", MODELS)
def test_f16x2_three_adam_steps_match_upstream(hip, model):
    s, g = SPEC[model], gold(model)
    mc, mf = models_from(hip, model, "f16x2")
    target = T(g["d.target"])
    opt = torch.optim.Adam(list(mc.parameters()) + list(mf.parameters()), lr=1e-3)
    torch.manual_seed(s["adam_seed"])
    losses = []
    for _ in range(3):
        opt.zero_grad()
        out = run(hip, model, mc, mf, opts(model, perturb=True, noise=0.2, chunk=s["chunk"]), "train")
        loss = torch.nn.functional.mse_loss(out[0], target) + torch.nn.functional.mse_loss(out[3], target)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    np.testing.assert_allclose(losses, g["e.losses"], rtol=1e-5)
    check_grads((mc, mf), g, "")


@pytest.mark.parametrize("model", MODELS)
def test_f16x2_at_size_against_float64(hip, model):
    """4096 rays x 128 depths: forward and every parameter gradient against float64 on the kernel's own encoder output"""
    s = SPEC[model]
    torch.manual_seed(5)
    m = hip.models.FlexibleNeRFModel(**s["kwargs"]).to(DEV)
    m.arithmetic = "f16x2"
    N, S = 4096, 128
    rays = hip.train_utils.pack_rays(torch.randn(N, 3, device=DEV), torch.randn(N, 3, device=DEV), 2.0, 6.0)
    if model == "mip":
        d = torch.sort(2.0 + 4.0 * torch.rand(N, S + 1, device=DEV), -1)[0]
        radius = hip.train_utils.mip_radius("lego_DS8")
        raw = m.mip_forward(rays, d, radius)
        x = torch.ops.nvsr.mip_encode(rays, d, radius).cpu().double()
    else:
        d = torch.sort(2.0 + 4.0 * torch.rand(N, S, device=DEV), -1)[0]
        raw = m.pe_forward(rays, d)
        x = torch.ops.nvsr.pe_encode(rays, d).cpu().double()
    g_raw = torch.randn_like(raw)
    (raw * g_raw).sum().backward()
    gr = g_raw.reshape(-1, 4).cpu().double()
    out64, g64 = cpu_eval(m, x, gr, s["enc"], torch.float64)
    _, g32 = cpu_eval(m, x, gr, s["enc"], torch.float32)
    e_fwd = float((raw.detach().reshape(-1, 4).cpu().double() - out64).abs().max())
    report = ["forward max|err| %.2e" % e_fwd]
    assert e_fwd <= 1e-4, report
    for k, p in m.named_parameters():
        rel = float((p.grad.cpu().double() - g64[k]).norm() / g64[k].norm().clamp_min(1e-30))
        rel32 = float((g32[k] - g64[k]).norm() / g64[k].norm().clamp_min(1e-30))
        report.append("%s %.2e (torch f32 %.2e)" % (k, rel, rel32))
        assert rel <= 4 * rel32 + 2e-3, report
    print("%s at size (f16x2): " % model + ", ".join(report))


# ---- the backward's per-point scale, determinism, the process default, opcheck --------------------------------------------------------------

def _grads(hip, model, scale):
    s = SPEC[model]
    mc, mf = models_from(hip, model, "f16x2")
    torch.manual_seed(s["train_seed"])
    out = run(hip, model, mc, mf, opts(model, perturb=True, noise=0.2, chunk=s["chunk"]), "train")
    target = T(gold(model)["d.target"])
    loss = torch.nn.functional.mse_loss(out[0], target) + torch.nn.functional.mse_loss(out[3], target)
    (loss * scale).backward()
    return [p.grad.clone() for m in (mc, mf) for p in m.parameters()]


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("k", [-40, 30])
def test_f16x2_gradients_are_scale_invariant(hip, model, k):
    base = _grads(hip, model, 1.0)
    scaled = _grads(hip, model, 2.0 ** k)
    for i, (a, b) in enumerate(zip(base, scaled)):
        want = a.double() * 2.0 ** k
        rel = float((b.double() - want).norm() / want.norm().clamp_min(1e-300))
        assert rel <= 1e-6, (i, rel)
        assert int((b == 0).sum()) <= int((a == 0).sum()), i
        assert torch.isfinite(b).all()


@pytest.mark.parametrize("model", MODELS)
def test_f16x2_backward_is_deterministic(hip, model):
    a, b = _grads(hip, model, 1.0), _grads(hip, model, 1.0)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.parametrize("model", MODELS)
def test_inherited_f16x2_default_runs_bf16x3(hip, model):
    capi = hip.capi
    before = capi.get_decoder_arithmetic()
    try:
        capi.set_decoder_arithmetic("f16x2")
        assert capi.resolve_nerf_arithmetic(None) == capi.ARITHMETIC["bf16x3"]
        assert capi.resolve_nerf_arithmetic("f16x2") == capi.ARITHMETIC["f16x2"]
        ref = models_from(hip, model, "bf16x3")[0]
        inh = models_from(hip, model, None)[0]
        np.testing.assert_array_equal(forward(model, inh, "a."), forward(model, ref, "a."))
        f16 = models_from(hip, model, "f16x2")[0]
        assert not np.array_equal(forward(model, f16, "a."), forward(model, ref, "a."))       # (an explicit f16x2 is honoured)
    finally:
        capi.set_decoder_arithmetic(before)


@pytest.mark.parametrize("model", MODELS)
def test_opcheck_with_f16x2(hip, model):
    g = gold(model)
    nv = torch.ops.nvsr
    m = models_from(hip, model, "f32")[0]
    nat = m.natural_blob()
    chk = lambda op, args: torch.library.opcheck(op, args, test_utils=("test_schema", "test_faketensor"))
    f16 = hip.capi.ARITHMETIC["f16x2"]
    if model == "mip":
        fwd, bwd, inputs = nv.mip_nerf, nv.mip_nerf_backward, (T(g["a.rays"][:4]), T(g["a.edges"][:4]), float(g["radius"]))
    else:
        fwd, bwd, inputs = nv.pe_nerf, nv.pe_nerf_backward, (T(g["a.rays"][:4]), T(g["a.z"][:4]))
    chk(fwd, inputs + (nat, True, f16))
    raw, rec = fwd(*inputs, nat, True, f16)
    chk(bwd, (nat, rec, torch.ones_like(raw), f16))
    torch.library.opcheck(fwd, inputs + (nat.clone().requires_grad_(True), True, f16),
                          test_utils=("test_schema", "test_autograd_registration", "test_faketensor"))


# ---- evaluation heals itself ------------------------------------------------------------------------------------------------------------

def _frame(hip, model, mc, mf):
    with torch.no_grad(), warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        out = run(hip, model, mc, mf, opts(model), "validation")
    ours = [x for x in w if "NVSR_ARITH_F16X2" in str(x.message)]
    return [N_(t) for t in (out[0], out[1], out[2], out[3], out[4], out[5])], len(ours)


@pytest.mark.parametrize("model", MODELS)
def test_evaluation_falls_back_to_bf16x3(hip, model):
    def broken(arith):
        mc, mf = models_from(hip, model, arith)
        with torch.no_grad():
            mc.layers_xyz[1].weight[5, 7] = 300.0
        return mc, mf

    ref, n = _frame(hip, model, *broken("bf16x3"))
    assert n == 0 and all(np.isfinite(ref[i]).all() for i in (0, 2, 3, 5))          # (rgb and acc of both passes)
    mc, mf = broken("f16x2")
    got, n = _frame(hip, model, mc, mf)
    assert n == 1
    for a, b in zip(got, ref):
        np.testing.assert_array_equal(a, b)
    got, n = _frame(hip, model, mc, mf)                  # the same parameters: straight to bf16x3, no warning
    assert n == 0
    for a, b in zip(got, ref):
        np.testing.assert_array_equal(a, b)
    # an in-place update moves the version: f16x2 is tried again -- here the update repairs the model, so the frame is the f16x2 frame
    with torch.no_grad():
        mc.layers_xyz[1].weight[5, 7] = float(SPEC[model]["params"].state_dict(SPEC[model]["params"].SEEDS[0])["layers_xyz.1.weight"][5, 7])
    want, n = _frame(hip, model, *models_from(hip, model, "f16x2"))
    assert n == 0
    got, n = _frame(hip, model, mc, mf)
    assert n == 0
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b)
    assert flag_word(hip) == 0


@pytest.mark.parametrize("model", MODELS)
def test_in_range_f16x2_frame_leaves_the_flag_down(hip, model):
    mc, mf = models_from(hip, model, "f16x2")
    reset_flag(hip)
    with torch.no_grad():
        out = run(hip, model, mc, mf, opts(model), "validation")
    check_render(out, gold(model), "c.")
    assert flag_word(hip) == 0


# ---- training -------------------------------------------------------------------------------------------------------------------------

H_LR = 8
POSE = [[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 4.0], [0.0, 0.0, 0.0, 1.0]]


def _train_step(hip, model, arith, sampler=None, optimizer="adam"):
    mc, mf = models_from(hip, model, arith)
    params = list(mc.parameters()) + list(mf.parameters())
    opt = torch.optim.Adam(params, lr=1e-3) if optimizer == "adam" else torch.optim.SGD(params, lr=1e-2)
    o = opts(model, perturb=True, noise=0.2, chunk=SPEC[model]["chunk"], nc=16, nf=16)
    step = hip.training.TrainStep(mc, mf, o, {"decoder"}, optimizer=opt, ds_factor=2, im_inconsistency_loss_w=1.0,
                                  **({} if sampler is None else dict(pixel_sampler=sampler)))
    return mc, mf, opt, step


def _run_steps(hip, model, arith, break_it=False, iters=2):
    mc, mf, _, step = _train_step(hip, model, arith)
    if break_it:
        with torch.no_grad():
            mc.layers_xyz[1].weight[5, 7] = 300.0
    g = torch.Generator().manual_seed(3)
    img = torch.rand(2 * H_LR, 2 * H_LR, 3, generator=g).to(DEV)
    img_lr = torch.rand(H_LR, H_LR, 3, generator=g).to(DEV)
    pose = torch.tensor(POSE, device=DEV)
    sid = scene_id(model, gold(model))
    scfg = scene(False)
    ms = []
    for it, cons in enumerate((False, True)[:iters]):
        np.random.seed(7 + it)
        torch.manual_seed(11 + it)
        if cons:       # the image-consistency iteration renders ds x ds patches in HR against an LR target
            ms.append(step(it, img_lr, pose, H_LR, H_LR, 20.0, 2, sid, scfg, 64, im_consistency_iter=True))
        else:
            ms.append(step(it, img, pose, 2 * H_LR, 2 * H_LR, 40.0, 1, sid, scfg, 64))
    return ms, (mc, mf)


@pytest.mark.parametrize("model", MODELS)
def test_train_step_runs_the_baseline_in_f16x2(hip, model):
    f16, _ = _run_steps(hip, model, "f16x2")
    b16, _ = _run_steps(hip, model, "bf16x3")
    for a, b in zip(f16, b16):
        for key in ("loss", "coarse_loss", "fine_loss"):
            assert a[key] is not None and np.isfinite(a[key])
            assert abs(a[key] - b[key]) <= 1e-4 * abs(b[key]) + 1e-7, (key, a[key], b[key])


@pytest.mark.parametrize("model", MODELS)
def test_train_step_out_of_range_raises(hip, model):
    # (one iteration: the next call would find this one's metrics finished and raise from inside the step)
    ms, _ = _run_steps(hip, model, "f16x2", break_it=True, iters=1)
    with pytest.raises(hip.capi.NvsrError, match="bf16x3"):
        ms[0]["loss"]


@pytest.mark.parametrize("model", MODELS)
def test_graphed_train_step_equals_the_eager_iterations(hip, model):
    s = SPEC[model]
    N, Nc, Nf, x = 64, 16, 16, s["extra"]
    g = torch.Generator(device=DEV).manual_seed(9)
    img = torch.rand(2 * H_LR, 2 * H_LR, 3, device=DEV, generator=g)
    pose = torch.tensor(POSE, device=DEV)
    sid, scfg = scene_id(model, gold(model)), scene(False)
    rnd = dict(t_rand=torch.rand(N, Nc + x, device=DEV, generator=g), u=torch.rand(N, Nf + x, device=DEV, generator=g),
               noise_coarse=0.2 * torch.randn(N, Nc, device=DEV, generator=g), noise_fine=0.2 * torch.randn(N, Nc + Nf + x, device=DEV, generator=g))
    a_mc, a_mf, a_opt, a_step = _train_step(hip, model, "f16x2", hip.training.DevicePixelSampler(seed=5), optimizer="sgd")
    b_mc, b_mf, b_opt, b_step = _train_step(hip, model, "f16x2", hip.training.DevicePixelSampler(seed=5), optimizer="sgd")
    graphed = hip.training.GraphedTrainStep(b_step, img, pose, 2 * H_LR, 2 * H_LR, 40.0, 1, sid, scfg, N, randoms_fn=rnd, warmup=2)
    a_par = list(a_mc.parameters()) + list(a_mf.parameters())
    b_par = list(b_mc.parameters()) + list(b_mf.parameters())
    for k in range(3):
        with torch.no_grad():
            for pa, pb in zip(a_par, b_par):
                pa.copy_(pb)
        a_opt.load_state_dict(copy.deepcopy(b_opt.state_dict()))
        a_step.pixel_sampler.calls = b_step.pixel_sampler.calls
        before = [p.detach().clone() for p in b_par]
        m_a = a_step(k, img, pose, 2 * H_LR, 2 * H_LR, 40.0, 1, sid, scfg, N, randoms=rnd)
        graphed()
        m_b = graphed.metrics()
        for key in ("loss", "coarse_loss", "fine_loss"):
            assert abs(m_a[key] - m_b[key]) <= 1e-6 * abs(m_a[key]) + 1e-9, (k, key, m_a[key], m_b[key])
        moved = False
        for pa, pb, p0 in zip(a_par, b_par, before):
            assert torch.allclose(pa, pb, rtol=1e-6, atol=1e-7), (k, float((pa - pb).abs().max()))
            moved |= not torch.equal(pb, p0)
        assert moved, k
