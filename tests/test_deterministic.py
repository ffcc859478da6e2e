"""GPU tests of the deterministic route of the tri-plane training step: the ordered scatter against its numpy restatement
bit for bit, the rows backward + taps + scatter against the atomic route, repeatability, accumulation, the ordered decoder weight gradient,
a whole TrainStep and the refusals."""
import functools

import numpy as np
import pytest
import torch

from deterministic_ref import rows_scatter_ref, scatter_case
from test_hip_round3 import _backward_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ARITH = {"bf16x3": 3, "f16x2": 2}
CASES = [("dense", 96, 16), ("sparse", 40, 200), ("unsorted", 70, 48), ("dense", 33, 200)]      # tests/test_hip_round3.py's, N = 257


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. rows_scatter alone against the numpy float32 reference, bit for bit
# ---------------------------------------------------------------------------------------------------------------------------------
SCATTER = [(kind, M, H, W) for kind in ("random",) for M in (1, 257, 4099) for (H, W) in ((5, 7), (16, 16))] + [
    ("one_texel", 4099, 16, 16),        # a segment of 16 396 entries: linear cost, or this test takes minutes
    ("zero_weights", 257, 5, 7), ("nan_row", 257, 16, 16), ("random", 257, 1, 1), ("nan_row", 4099, 5, 7)]


@functools.lru_cache(maxsize=None)
def _scatter_reference(kind, M, H, W):
    rows, texel, weight, g = scatter_case(M, H, W, 7 + M + H, kind)
    return rows, texel, weight, g, rows_scatter_ref(rows, texel, weight, g)


@pytest.mark.parametrize("kind,M,H,W", SCATTER)
def test_rows_scatter_equals_the_numpy_reference_bit_for_bit(hip, kind, M, H, W):
    rows, texel, weight, g, want = _scatter_reference(kind, M, H, W)
    if kind == "random" and H * W > 4 * M:
        assert (want.view(np.uint32) == g.view(np.uint32)).all(-1).any()          # the case has texels no entry names
    r, t, w = (torch.from_numpy(a).to(DEV) for a in (rows, texel, weight))
    nbytes = hip.capi.lib().nvsr_rows_scatter_workspace_bytes(M)
    got = []
    for fill in (0xFF, 0x00):       # 0xFFFFFFFF words are NaNs / huge keys: a read of workspace nobody wrote changes the bits
        ws = torch.full((nbytes,), fill, dtype=torch.uint8, device=DEV)
        out = torch.from_numpy(g).to(DEV)
        torch.ops.nvsr.rows_scatter(r, t, w, out, ws)
        got.append(out.cpu().numpy())
    out = torch.from_numpy(g).to(DEV)
    torch.ops.nvsr.rows_scatter(r, t, w, out, None)                                # (the operator's own workspace)
    got.append(out.cpu().numpy())
    for o in got:
        assert (o.view(np.uint32) == want.view(np.uint32)).all(), (kind, M, H, W, int((o.view(np.uint32) != want.view(np.uint32)).sum()))
    if kind == "nan_row":
        hit = np.zeros(H * W, bool)
        hit[texel[M // 2]] = True
        assert np.isnan(got[0].reshape(-1, 48)[hit]).all() and np.isfinite(got[0].reshape(-1, 48)[~hit]).all()


def test_rows_scatter_traces_and_refuses_bad_tensors(hip):
    rows, texel, weight, g, _ = _scatter_reference("random", 257, 5, 7)
    r, t, w, out = (torch.from_numpy(a).to(DEV) for a in (rows, texel, weight, g))
    torch.library.opcheck(torch.ops.nvsr.rows_scatter, (r, t, w, out, None), test_utils=("test_schema", "test_faketensor"))
    with pytest.raises(ValueError):
        torch.ops.nvsr.rows_scatter(r, t.long(), w, out, None)
    with pytest.raises(ValueError):
        torch.ops.nvsr.rows_scatter(r[:, :40], t, w, out, None)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2.-4. rows backward + taps + scatter: against the atomic route, repeated, accumulated
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pass_inputs(z_kind, S, plane_res, arith):
    """one backward pass of N = 257 rays: inputs, the forward's gates in `arith`, and the ordered route's four planes (computed once)"""
    import nvsr_amd as hip
    nv = torch.ops.nvsr
    N = 257
    mf, rays, z = _backward_inputs(hip, N, S, plane_res, 11, z_kind)
    planes, consts = mf.scene_args()
    g_raw = torch.randn(N, S, 4, device=DEV, generator=torch.Generator(device=DEV).manual_seed(S)) * 1e-2
    packed, packed_bwd = mf.packed_decoder(), mf.packed_decoder_bwd()
    _, gates, _ = nv.decode_rays(planes, consts, packed, rays, z, True, False, arith)
    args = (planes, consts, packed, packed_bwd, rays, z, g_raw, gates, None)
    det = nv.decode_rays_backward_det(*args, [True] * 4, arith)
    return mf, args, det


@pytest.mark.parametrize("arith", list(ARITH))
@pytest.mark.parametrize("z_kind,S,plane_res", CASES)
def test_ordered_route_matches_the_atomic_route(hip, z_kind, S, plane_res, arith):
    """same kernel above emit_plane, same arithmetic, the SAME gates, the same taps: the two routes differ in the order of the sums alone --
    1e-5 of the plane's largest gradient, the project's figure for summation order (test_deduplicated_scatter_matches_per_point_scatter)"""
    nv = torch.ops.nvsr
    mf, args, det = _pass_inputs(z_kind, S, plane_res, ARITH[arith])
    atomic = nv.decode_rays_backward(*args, [True] * 4, ARITH[arith])
    for d in range(4):
        scale = float(atomic[d].abs().max())
        err = float((atomic[d] - det[d]).abs().max())
        print("%s S=%d res=%d %s plane %d: max |atomic - ordered| = %.3g of the largest gradient %.3g" % (z_kind, S, plane_res, arith, d, err / scale, scale))
        assert scale > 0 and torch.isfinite(det[d]).all()
        assert err <= 1e-5 * scale + 1e-12, (d, err, scale)
    # one plane frozen: no row buffer, no scatter for it; the others keep their bits
    need = [True, False, True, True]
    part = nv.decode_rays_backward_det(*args, need, ARITH[arith])
    assert part[1].numel() == 0
    for d in (0, 2, 3):
        assert same_bits(part[d], det[d]), d
    only_view = nv.decode_rays_backward_det(*args, [False, False, False, True], ARITH[arith])
    assert same_bits(only_view[3], det[3]) and all(only_view[d].numel() == 0 for d in range(3))


@pytest.mark.parametrize("arith", list(ARITH))
def test_ordered_route_repeats_its_bits(hip, arith):
    nv = torch.ops.nvsr
    mf, args, det = _pass_inputs("unsorted", 70, 48, ARITH[arith])
    for _ in range(3):
        again = nv.decode_rays_backward_det(*args, [True] * 4, ARITH[arith])
        for d in range(4):
            assert torch.equal(again[d], det[d]) and same_bits(again[d], det[d]), d


def test_second_pass_accumulates_exactly(hip):
    """pass 2 accumulated onto pass 1's planes == a + b of the two functional results, bit for bit: a functional result from zero is the
    texel's sum s itself (0 + s), and the accumulating form adds that same s to what is there"""
    nv = torch.ops.nvsr
    mf, args, a = _pass_inputs("unsorted", 70, 48, 3)
    planes, consts, packed, packed_bwd, rays, z, g_raw, gates, _ = args
    z2 = (z * 0.9 + 0.3).contiguous()
    g2 = torch.randn(z.shape + (4,), device=DEV, generator=torch.Generator(device=DEV).manual_seed(2)) * 1e-2
    _, gates2, _ = nv.decode_rays(planes, consts, packed, rays, z2, True, False, 3)
    args2 = (planes, consts, packed, packed_bwd, rays, z2, g2, gates2, None)
    need = [True] * 4
    b = nv.decode_rays_backward_det(*args2, need, 3)
    acc = [t.clone() for t in a]
    nv.decode_rays_backward_det_(*args2, need, 3, acc)
    for d in range(4):
        assert float(b[d].abs().max()) > 0
        assert torch.equal(acc[d], a[d] + b[d]), d
    with pytest.raises(ValueError):
        nv.decode_rays_backward_det_(*args2, need, 3, [acc[0], acc[1], acc[2], acc[3][:1]])


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. the ordered decoder weight gradient
# ---------------------------------------------------------------------------------------------------------------------------------
def test_ordered_decoder_weight_gradient(hip):
    """nvsr::decoder_weight_grad_det against today's operator on one synthetic record (N = 130, S = 33: 4 290 rows = 17 slabs of 256 rows, the
    last one partial; 5 head slabs), held to what tests/test_hip_parity.py::test_decoder_weight_grad_contraction holds the limb kernel to
    (relative L2 < 1e-5, every element within 2e-4 sqrt(P)); the allocation padding holds NaN; three repeats under two workspace fills: same bits"""
    nv, capi = torch.ops.nvsr, hip.capi
    N, S = 130, 33
    P = N * S
    n = capi.lib().nvsr_decoder_record_floats(N, S)
    Pp = (P + 7) // 8 * 8 + 32
    assert n == Pp * 2308
    rec = torch.randn(n, generator=torch.Generator().manual_seed(5), dtype=torch.float32)
    r, o = rec.numpy(), 0
    for cols, k in ((64, 1), (128, 4), (128, 4), (192, 1), (128, 4), (128, 4), (4, 1)):
        r[o:o + k * cols * Pp].reshape(k, Pp, cols)[:, P:] = np.nan            # rows >= P are allocation padding: never read
        o += k * cols * Pp
    rec = rec.to(DEV)
    want = nv.decoder_weight_grad(rec, N, S, 3)
    nfl = capi.lib().nvsr_decoder_weight_grad_det_workspace_floats(N, S)
    got = []
    for fill in (float("nan"), 0.0):
        for _ in range(3):
            ws = torch.full((nfl,), fill, dtype=torch.float32, device=DEV)
            got.append(nv.decoder_weight_grad_det(rec, N, S, 3, ws))
    got.append(nv.decoder_weight_grad_det(rec, N, S, 3, None))
    got.append(nv.decoder_weight_grad_det(rec, N, S, 2, None))                     # (f16x2 contracts on 3 bf16 limbs as well)
    assert torch.isfinite(got[0]).all() and torch.isfinite(want).all()
    for g in got[1:]:
        assert same_bits(g, got[0])
    diff = (got[0].double() - want.double())
    rel = float(diff.norm() / want.double().norm())
    print("ordered vs atomic weight gradient: relative L2 %.3g, max |diff| %.3g (bound %.3g)" % (rel, float(diff.abs().max()), 2e-4 * np.sqrt(P)))
    assert rel < 1e-5
    assert float(diff.abs().max()) <= 2e-4 * np.sqrt(P)
    with pytest.raises(ValueError):
        nv.decoder_weight_grad_det(rec, N, S, 3, torch.empty(nfl - 1, device=DEV))


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. a whole step
# ---------------------------------------------------------------------------------------------------------------------------------
ORDERED = ("nvsr_render_pass_backward_rows_arith", "nvsr_rows_scatter", "nvsr_internal_plane_taps", "nvsr_view_rows_reduce", "nvsr_decoder_weight_grad_det_arith")
ATOMIC = ("nvsr_render_pass_backward_gates_arith", "nvsr_render_pass_backward_gates", "nvsr_render_pass_backward_ex", "nvsr_render_pass_backward",
          "nvsr_decoder_weight_grad_arith", "nvsr_decoder_weight_grad")


def _train_three_iterations(hip, monkeypatch, deterministic):
    from bench import make_synthetic_scene, render_options
    calls = {}
    real = hip.capi.call

    def counting(name, *a):
        calls[name] = calls.get(name, 0) + 1
        return real(name, *a)

    monkeypatch.setattr(hip.capi, "call", counting)
    mc, mf, sid, pose = make_synthetic_scene(DEV, plane_res=32, view_res=16, seed=21)
    for m in (mc, mf):
        for n, p in m.named_parameters():
            p.requires_grad_("rot_mats" not in n)
        m.train()
    opts, scfg = render_options(16, 16, perturb=True, noise=0.2)
    planes = list(mc.planes_.values())
    dec = list({id(p): p for m in (mc, mf) for p in m.decoder_parameters()}.values())
    step = hip.training.TrainStep(mc, mf, opts, {"LR_planes", "decoder"}, optimizer=torch.optim.Adam(dec, lr=5e-3),
                                  planes_optimizer=torch.optim.Adam(planes, lr=5e-2), pixel_sampler=hip.training.DevicePixelSampler(seed=5),
                                  deterministic=deterministic)
    assert step.deterministic is bool(deterministic)
    H = W = 48
    focal = 0.5 * W / np.tan(0.5 * 0.6911112)
    g = torch.Generator(device=DEV).manual_seed(3)
    img = torch.rand(H, W, 3, device=DEV, generator=g)
    N, Nc, Nf = 512, 16, 16
    rnd = dict(t_rand=torch.rand(N, Nc, device=DEV, generator=g), u=torch.rand(N, Nf, device=DEV, generator=g),
               noise_coarse=0.2 * torch.randn(N, Nc, device=DEV, generator=g), noise_fine=0.2 * torch.randn(N, Nc + Nf, device=DEV, generator=g))
    before = [p.detach().clone() for p in planes + dec]
    for it in range(3):
        step(it, img, pose, H, W, focal, 1, sid, scfg, N, randoms=rnd)
    torch.cuda.synchronize()
    monkeypatch.setattr(hip.capi, "call", real)
    moved = sum(float((p.detach() - b).abs().max()) > 0 for p, b in zip(planes + dec, before))
    return [p.detach().clone() for p in planes], [p.detach().clone() for p in dec], calls, moved


def test_two_deterministic_train_steps_end_with_the_same_bits(hip, monkeypatch):
    """two TrainStep(deterministic=True) from the same seed, planes + decoder, 512 rays, 16 + 16 samples, 32^2 planes, three iterations: every
    plane and decoder parameter equal -- and the counted launches show that the ordered route produced them and no atomic entry ran (an idle GPU
    repeats atomic bits often enough to pass by luck)"""
    monkeypatch.delenv("NVSR_DETERMINISTIC", raising=False)
    monkeypatch.setenv("NVSR_OPS_DISPATCH", "0")
    a_planes, a_dec, calls, moved = _train_three_iterations(hip, monkeypatch, True)
    b_planes, b_dec, calls_b, _ = _train_three_iterations(hip, monkeypatch, True)
    assert moved == len(a_planes) + len(a_dec)                        # every plane and decoder tensor trained
    for name in ATOMIC:
        assert calls.get(name, 0) == 0 and calls_b.get(name, 0) == 0, (name, calls)
    # per iteration: a coarse and a fine pass, each one rows backward, 4 taps + 4 scatters, 1 view reduce, 1 ordered contraction
    assert calls["nvsr_render_pass_backward_rows_arith"] == 6 and calls["nvsr_decoder_weight_grad_det_arith"] == 6, calls
    assert calls["nvsr_rows_scatter"] == 24 and calls["nvsr_internal_plane_taps"] == 24 and calls["nvsr_view_rows_reduce"] == 6, calls
    assert all(calls[name] == calls_b[name] for name in ORDERED), (calls, calls_b)
    for x, y in zip(a_planes + a_dec, b_planes + b_dec):
        assert torch.equal(x, y) and same_bits(x, y)
    # and a step that is NOT in the mode still takes the atomic route (nothing changes unless the mode is asked for)
    _, _, calls_c, _ = _train_three_iterations(hip, monkeypatch, False)
    assert all(calls_c.get(name, 0) == 0 for name in ORDERED), calls_c
    assert calls_c["nvsr_render_pass_backward_gates_arith"] == 6 and calls_c["nvsr_decoder_weight_grad_arith"] == 6, calls_c


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. refusals: a RuntimeError that names the mode, before any launch; never a silent atomic fallback
# ---------------------------------------------------------------------------------------------------------------------------------
def _no_launch(hip, monkeypatch):
    calls = []
    real = hip.capi.call
    monkeypatch.setattr(hip.capi, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    return calls


def test_refusals_name_the_deterministic_mode(hip, monkeypatch):
    from bench import make_synthetic_scene, render_options
    from conftest import load_golden
    from test_oracle import g18_variant
    monkeypatch.delenv("NVSR_DETERMINISTIC", raising=False)
    nv, capi, T = torch.ops.nvsr, hip.capi, hip.training
    mf, args, _ = _pass_inputs("unsorted", 70, 48, 3)
    planes, consts, packed, packed_bwd, rays, z, g_raw, gates, _ = args
    calls = _no_launch(hip, monkeypatch)
    # the f32 arithmetic: the operators themselves ...
    with pytest.raises(RuntimeError, match="deterministic mode"):
        nv.decode_rays_backward_det(*args, [True] * 4, 0)
    with pytest.raises(RuntimeError, match="deterministic mode"):
        nv.decode_rays_backward_det_(*args, [True] * 4, 0, [torch.zeros_like(p) for p in planes])
    with pytest.raises(RuntimeError, match="deterministic mode"):
        nv.decoder_weight_grad_det(torch.zeros(capi.lib().nvsr_decoder_record_floats(4, 4), device=DEV), 4, 4, 0, None)
    # ... decode_rays_backward_recompute, the path for passes without gates
    with capi.deterministic_scope(True):
        with pytest.raises(RuntimeError, match="deterministic mode"):
            nv.decode_rays_backward_recompute(planes, consts, packed, packed_bwd, rays, z, g_raw, [True] * 4, False, 3)
    assert calls == []
    # ... a training step in f32, and one whose pass is too large for a forward record (it would recompute)
    mc, mf2, sid, pose = make_synthetic_scene(DEV, plane_res=32, view_res=16, seed=21)
    for m in (mc, mf2):
        for n, p in m.named_parameters():
            p.requires_grad_("rot_mats" not in n)
        m.train()
    opts, scfg = render_options(16, 16)
    H = W = 32
    focal = 0.5 * W / np.tan(0.5 * 0.6911112)
    img = torch.rand(H, W, 3, device=DEV)
    step = T.TrainStep(mc, mf2, opts, {"LR_planes", "decoder"}, deterministic=True, pixel_sampler=T.DevicePixelSampler(seed=5))
    backward_entries = ("backward", "weight_grad", "rows_scatter", "plane_taps", "decode_rays")
    for m in (mc, mf2):
        m.arithmetic = "f32"
    calls.clear()
    with pytest.raises(RuntimeError, match="deterministic mode"):
        step(0, img, pose, H, W, focal, 1, sid, scfg, 64)
    assert not [c for c in calls if any(k in c for k in backward_entries)], calls
    for m in (mc, mf2):
        m.arithmetic = "bf16x3"
    monkeypatch.setattr(hip.train_utils, "RECORD_FORWARD_MAX_POINTS", 64 * 16 - 1)
    calls.clear()
    with pytest.raises(RuntimeError, match="deterministic mode"):
        step(0, img, pose, H, W, focal, 1, sid, scfg, 64)
    assert not [c for c in calls if any(k in c for k in backward_entries)], calls
    monkeypatch.undo()
    monkeypatch.delenv("NVSR_DETERMINISTIC", raising=False)
    # ... 'SR' in what, GraphedTrainStep
    with pytest.raises(RuntimeError, match="deterministic mode"):
        T.TrainStep(mc, mf2, opts, {"SR"}, deterministic=True)
    with pytest.raises(RuntimeError, match="deterministic mode"):
        T.GraphedTrainStep(step, img, pose, H, W, focal, 1, sid, scfg, 64)
    # ... generic geometries (generic.hip)
    g = load_golden("g18_decoder_variants.npz")
    name = next(iter(__import__("test_oracle").G18_VARIANTS))
    kw, sd_, gplanes = g18_variant(g, name)
    m = hip.models.TwoDimPlanesModel(use_viewdirs=True, align_corners=True, **kw)
    m.load_state_dict({k: torch.as_tensor(v) for k, v in sd_.items()}, strict=True)
    m = m.to(DEV).train()
    gsid = "lego_DS8_PlRes10_6"
    m.planes_ = torch.nn.ParameterDict({hip.models.get_plane_name(gsid, d): torch.nn.Parameter(torch.as_tensor(gplanes[d], dtype=torch.float32, device=DEV))
                                        for d in range(4)})
    m.box_coords = {gsid: torch.as_tensor(g["box"], dtype=torch.float64)}
    m.set_cur_scene_id(gsid)
    assert not m.is_native_geometry()
    x = torch.as_tensor(g[name + ".x"][:64], dtype=torch.float32, device=DEV)
    with capi.deterministic_scope(True):
        with pytest.raises(RuntimeError, match="deterministic mode"):
            m(x)
    assert m(x).requires_grad                       # outside the mode the generic training forward runs as before
