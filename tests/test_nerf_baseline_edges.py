"""GPU tests of the layer engine of the two FlexibleNeRFModel baselines -- csrc/nerf_mlp.h with the encoders of csrc/mip.hip and csrc/pe.hip --
at ragged point counts, through the C ABI (every test owns its buffers), against float64.

The engine tiles the P = N S points of a call by 32 (one wave per tile) and the weight gradient by slabs of 8 192 points (a quarter per wave).
The shapes leave a tile, a wave or a slab partly empty: P < 32, one tile, a full tile plus a partial one, tile counts 1, 2 and 3 (mod 4 and
mod 8), 8 192 k + r for r in {1, 2 047, 2 048, 2 049, 6 145} (each wave of the last slab full, partial or empty), one image row of an
LLFF-sized Mip fine pass (504 x 129); many short rays (S = 1 included) and a few long ones (S > 2 000: tiles straddle ray boundaries at
varied offsets).  Every case runs for both encoders and the three arithmetics.

  encoding ........ nvsr_*_encode equals the record's encoding and direction columns bit for bit
  forward ......... every layer from the kernel's own recorded input, every point (the last of a partial tile included), against float64
                    (nerf_baseline_checks.check_forward_layers: gemm_eps at the layer's width, plus the bias add)
  backward ........ every transposed layer from the kernel's own gradient of the layer above and its recorded gates (check_backward_layers;
                    the f16x2 floor follows the per-point scales), on dL/draw spread over 8 decades, |dL/dalpha| >> |dL/drgb| at every
                    third point, the extremes on the last point
  weight gradient . exact f32 in every arithmetic: a synthetic record against float64 G^T X and sum G
  bounds .......... raw, record, grad_record, the workspace and grad_natural are followed by padding words that hold a NaN sentinel; every
                    call leaves it bit for bit.  P = 0 writes nothing but grad_natural's zeros
  determinism ..... a second call on the same inputs gives the same bits
  f16x2 range ..... in range the flag stays down; an out-of-range PE coordinate or a non-finite dL/draw at the last live point of a partial
                    tile raises it, makes that point's row NaN / non-finite and leaves every other row bit for bit
  host path ....... run_one_iter_of_nerf at 7 x 11 rays and 33 + 17 samples (no pass a multiple of 32 points) against g25_nerf_ragged.npz
                    (the upstream code on the CPU, tests/golden/gen_golden_nerf_ragged.py), with the tolerances of tests/test_mip_nerf.py
"""
import sys
import warnings
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden
from nerf_baseline_checks import (DEV, GREC, G_A, G_L1, MW_SLAB, T, U, assert_within, bits, check_backward_layers, check_forward_layers,
                                  check_grads, check_render, natural_blob, record_columns, scene, wgrad_reference, wgrad_roundings)
import nerf_baseline_checks as checks

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import mip_params  # noqa: E402
import pe_params  # noqa: E402

pytestmark = pytest.mark.gpu

ENC = {"mip": 36, "pe": 39}
ARITHS = ["f32", "bf16x3", "f16x2"]
SENTINEL = 0x7FC0FFEE           # a quiet-NaN bit pattern no kernel computes
PAD = 256                       # sentinel words behind every buffer (64 rows of raw)

SHAPES = [(1, 1), (31, 1), (1, 31),                                   # P < 32
          (1, 32), (4, 8),                                            # one tile
          (33, 1), (3, 11), (5, 37), (7, 65),                         # full tiles and a partial one (2, 2, 6, 15 tiles)
          (6, 25), (7, 29), (9, 29), (12, 25), (337, 1),              # 5, 7, 9, 10, 11 tiles: 1, 3, 1, 2, 3 (mod 4); 5, 7, 1, 2, 3 (mod 8)
          (1, 8191), (64, 128), (3, 2731),                            # 8 191, 8 192, 8 193 points
          (5, 3277), (3, 3413), (80, 128), (10241, 1), (3, 4779),     # 2 x 8 192 + 1; 8 192 + 2 047, 2 048, 2 049, 6 145
          (504, 129)]                                                 # an image row of the LLFF Mip fine pass (P = 16 mod 32)


class Engine:
    """the C entry points of one baseline (nvsr_mip_* / nvsr_pe_*) on caller-owned buffers, with the model of the fixtures' first seed"""

    def __init__(self, hip, model):
        self.capi, self.model, self.enc = hip.capi, model, ENC[model]
        self.extra = (hip.train_utils.mip_radius("lego_DS8"),) if model == "mip" else ()     # (Mip's entry points take the radius after the depths)
        self.rec = record_columns(self.enc).width
        params = mip_params if model == "mip" else pe_params
        self.sd = params.state_dict(params.SEEDS[0])
        self.nat = T(natural_blob(self.sd))

    def _call(self, name, *args):
        self.capi.call("nvsr_%s_%s" % (self.model, name), *args, self.capi.stream())

    def encode(self, N, S, rays, d, out):
        p = self.capi.ptr
        self._call("encode", N, S, p(rays), p(d), *self.extra, p(out))

    def forward(self, N, S, rays, d, raw, rec, arith):
        p = self.capi.ptr
        self._call("nerf_forward_arith", N, S, p(rays), p(d), *self.extra, p(self.nat), p(raw), p(rec), self.capi.ARITHMETIC[arith])

    def backward(self, P, rec, g_raw, grec, arith):
        p = self.capi.ptr
        self._call("nerf_backward_arith", P, p(self.nat), p(rec), p(g_raw), p(grec), self.capi.ARITHMETIC[arith])

    def workspace_floats(self, P):
        return int(getattr(self.capi.lib(), "nvsr_%s_nerf_wgrad_workspace_floats" % self.model)(P))

    def weight_grad(self, P, rec, grec, ws, out):
        p = self.capi.ptr
        self._call("nerf_weight_grad", P, p(rec), p(grec), p(ws), p(out))


def padded(n):
    """n float32 words for a kernel, then PAD words of the sentinel (a float32 view of one int32 allocation)"""
    return torch.full((n + PAD,), SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)


def pad_intact(buf, n):
    return bool((buf.view(torch.int32)[n:] == SENTINEL).all())


def inputs(model, N, S, seed):
    """packed rays [N, 11] (origins and directions N(0, 1), near 2, far 6, unit view directions) and the encoder's depths, sorted in [2, 6]:
    Mip's S + 1 interval edges, PE's S sample depths"""
    rng = np.random.default_rng(seed)
    ro, rd = rng.standard_normal((2, N, 3)).astype(np.float32)
    vd = rd / np.linalg.norm(rd, axis=-1, keepdims=True)
    rays = np.concatenate([ro, rd, np.tile(np.float32([2.0, 6.0]), (N, 1)), vd], -1).astype(np.float32)
    d = np.sort(2.0 + 4.0 * rng.random((N, S + (model == "mip"))), -1).astype(np.float32)
    return T(rays), T(d)


def spread_g_raw(P, seed):
    """dL/draw [P, 4]: N(0, 1) times a per-point magnitude 10^U(-4, 4) (8 decades); dL/dalpha x 2^20 at every third point (far above its
    dL/drgb); the last point -- the last live point of the partial tile, where there is one -- carries the extremes, |dL/drgb| = 1e-4 and
    |dL/dalpha| = 1e4 2^20, and the point before it the other way round"""
    rng = np.random.default_rng(seed)
    g = rng.standard_normal((P, 4)) * 10.0 ** rng.uniform(-4, 4, (P, 1))
    g[::3, 3] *= 2.0 ** 20
    sign = np.where(rng.random(4) < 0.5, -1.0, 1.0)
    g[-1] = sign * [1e-4, 1e-4, 1e-4, 1e4 * 2.0 ** 20]
    if P > 1:
        g[-2] = sign * [1e4, 1e4, 1e4, 1e-4]
    return g.astype(np.float32)


def run(eng, N, S, rays, d, g_raw, arith):
    """encode, recording forward, backward, weight gradient, each into a fresh sentinel-padded buffer -> {name: (buffer, words the call owns)}"""
    P = N * S
    sizes = {"enc": P * (eng.enc + 27), "raw": P * 4, "rec": P * eng.rec, "grec": P * GREC, "ws": eng.workspace_floats(P), "grad": eng.nat.numel()}
    b = {k: (padded(n), n) for k, n in sizes.items()}
    eng.encode(N, S, rays, d, b["enc"][0])
    eng.forward(N, S, rays, d, b["raw"][0], b["rec"][0], arith)
    eng.backward(P, b["rec"][0], g_raw, b["grec"][0], arith)
    eng.weight_grad(P, b["rec"][0], b["grec"][0], b["ws"][0], b["grad"][0])
    torch.cuda.synchronize()
    return b


@pytest.fixture(scope="module", params=[(m, a, s) for m in ENC for a in ARITHS for s in SHAPES],
                ids=lambda c: "%s-%s-%dx%d" % (c[0], c[1], c[2][0], c[2][1]))
def case(request, hip):
    """one (encoder, arithmetic, N x S): the whole chain twice on the same inputs, the range flag reset before and read after"""
    model, arith, (N, S) = request.param
    eng = Engine(hip, model)
    P = N * S
    rays, d = inputs(model, N, S, seed=N * 8209 + S)
    g_raw = T(spread_g_raw(P, seed=P))
    flag = hip.capi.range_flag(torch.device(DEV))
    flag.reset()
    runs = [run(eng, N, S, rays, d, g_raw, arith) for _ in range(2)]
    view = lambda name, cols: runs[0][name][0][:P * cols].view(P, cols)
    return NS(model=model, arith=arith, N=N, S=S, P=P, enc=eng.enc, sd=eng.sd, g_raw=g_raw, runs=runs, flag=int(flag.word[0]),
              rows=view("enc", eng.enc + 27), raw=view("raw", 4), rec=view("rec", eng.rec), grec=view("grec", GREC))


def _tag(c):
    return "%s %s %dx%d" % (c.model, c.arith, c.N, c.S)


def test_encoding_is_the_records_bit_for_bit(case):
    c = case
    same = bits(c.rows) == bits(c.rec[:, :c.enc + 27])
    assert same.all(), "%s: %d encoded values differ from the record, the first at point %d" % (_tag(c), int((~same).sum()),
                                                                                                int((~same).nonzero()[0, 0]))
    if c.model == "mip":
        # every Mip column is a damped sin / cos (the IPE) or a view-direction column (a unit vector's component, sin, cos): |column| <= 1
        # up to rounding, far inside f16x2's activation range (|x| < 4094) -- no Mip input can take the forward out of range, so the
        # out-of-range forward case is PE's alone (test_pe_f16x2_out_of_range_coordinate_at_the_last_live_point)
        assert float(c.rows.abs().max()) <= 1.0 + 1e-6


def test_forward_layer_by_layer(case):
    c = case
    rep = check_forward_layers(c.arith, c.sd, c.rec, c.raw, c.enc)
    print("%s forward, worst err / bound: %s" % (_tag(c), ", ".join("%s %.3f" % kv for kv in rep.items())))


def test_backward_layer_by_layer(case):
    c = case
    rep = check_backward_layers(c.arith, c.sd, c.rec, c.grec, c.g_raw, c.enc)
    print("%s backward, worst err / bound: %s" % (_tag(c), ", ".join("%s %.3f" % kv for kv in rep.items())))


def test_nothing_is_written_beyond_P(case):
    for i, r in enumerate(case.runs):
        for name, (buf, n) in r.items():
            assert pad_intact(buf, n), "%s: call %d wrote into the padding behind %s" % (_tag(case), i, name)


def test_a_second_call_gives_the_same_bits(case):
    a, b = case.runs
    for name in ("enc", "raw", "rec", "grec", "grad"):
        n = a[name][1]
        assert torch.equal(bits(a[name][0][:n]), bits(b[name][0][:n])), "%s: %s" % (_tag(case), name)


def test_in_range_calls_leave_the_range_flag_down(case):
    assert case.flag == 0, "%s: flag %d" % (_tag(case), case.flag)


@pytest.mark.parametrize("model", list(ENC))
def test_zero_points_write_nothing_but_the_zero_gradient(hip, model):
    eng = Engine(hip, model)
    rays, d = inputs(model, 1, 4, seed=0)
    NAT = eng.nat.numel()
    raw, rec, grec, g_raw, ws = padded(0), padded(0), padded(0), padded(0), padded(0)
    grad = padded(NAT)
    grad[:NAT] = 1.0
    assert eng.workspace_floats(0) == 0
    for arith in ARITHS:
        eng.forward(0, 4, rays, d, raw, rec, arith)
        eng.backward(0, rec, g_raw, grec, arith)
    eng.weight_grad(0, rec, grec, ws, grad)
    torch.cuda.synchronize()
    for name, buf in (("raw", raw), ("record", rec), ("grad_record", grec), ("workspace", ws)):
        assert pad_intact(buf, 0), name
    assert (bits(grad[:NAT]) == 0).all() and pad_intact(grad, NAT)         # (+0.0, every word)


# ---- the weight gradient ----------------------------------------------------------------------------------------------------------------

WGRAD_P = [1, 31, 33, 455, 2047, 2048, 2049, 8191, 8192, 8193, 10239, 10240, 10241, 14337, 16385, 65016]


@pytest.mark.parametrize("P", WGRAD_P)
@pytest.mark.parametrize("model", list(ENC))
def test_weight_gradient_against_float64(hip, model, P):
    """nvsr_*_nerf_weight_grad alone, on a synthetic record and grad_record (N(0, 1)), against float64 G^T X and sum_p G of every layer.  The
    G rows of the last wave that holds points (the last partial wave of the last slab) are scaled by 2^10: a dropped or double-counted tail
    point is then a gross error, not noise.
    Per element: |got - ref| <= gamma_n sum_p |G||X| (sum_p |G| for a bias), gamma_n = n 2^-24 / (1 - n 2^-24), n = wgrad_roundings(P): one
    per point of a wave (up to 2 048; the f32 MFMA's products may be rounded, nerf_baseline_checks.gemm_eps), 3 adds of the waves' partial
    sums, slabs - 1 adds of the slabs -- every partial sum is bounded by sum |G||X|.  Relative L2 < 1e-5 (as test_decoder_weight_grad_contraction: round-to-nearest
    errors of the n adds grow like sqrt(n), far below the worst case).  The workspace is exactly nvsr_*_nerf_wgrad_workspace_floats(P) long;
    it, the inputs and grad_natural are followed by sentinel padding."""
    eng = Engine(hip, model)
    R, NAT = eng.rec, eng.nat.numel()
    g = torch.Generator(device=DEV).manual_seed(P)
    rec, grec = padded(P * R), padded(P * GREC)
    rec[:P * R] = torch.randn(P * R, generator=g, device=DEV)
    G = torch.randn(P, GREC, generator=g, device=DEV)
    tail = (P - 1) // (MW_SLAB // 4) * (MW_SLAB // 4)
    G[tail:] *= 2.0 ** 10
    grec[:P * GREC] = G.reshape(-1)
    n_ws = eng.workspace_floats(P)
    assert n_ws == -(-P // MW_SLAB) * NAT
    ws, grad = padded(n_ws), padded(NAT)
    eng.weight_grad(P, rec, grec, ws, grad)
    torch.cuda.synchronize()
    for name, buf, n in (("record", rec, P * R), ("grad_record", grec, P * GREC), ("workspace", ws, n_ws), ("grad_natural", grad, NAT)):
        assert pad_intact(buf, n), name
    ref, mag = wgrad_reference(rec[:P * R].view(P, R), G, eng.enc)
    n = wgrad_roundings(P)
    got = grad[:NAT].double()
    worst = assert_within("dW", got[:, None], ref[:, None], (n * U / (1 - n * U)) * mag[:, None])
    rel = float((got - ref).norm() / ref.norm())
    assert rel < 1e-5, rel
    print("%s P=%d weight gradient: worst err / bound %.3g, relative L2 %.2e" % (model, P, worst, rel))


# ---- the f16x2 range flag at a ragged tail ----------------------------------------------------------------------------------------------

FLAG_SHAPES = [(1, 31), (5, 37), (7, 65), (10241, 1), (504, 129)]        # the last point is the last live point of a partial tile


@pytest.mark.parametrize("shape", FLAG_SHAPES, ids=lambda s: "%dx%d" % s)
def test_pe_f16x2_out_of_range_coordinate_at_the_last_live_point(hip, shape):
    """PE keeps the point itself among its encoding columns: a coordinate >= 4094 at the last live point of a partial tile makes that point's
    raw row NaN and raises the flag; every other point's raw and record rows are the clean run's, bit for bit (a point is a column of every
    product).  (Mip has no such input: test_encoding_is_the_records_bit_for_bit asserts its encoder columns within [-1, 1].)"""
    N, S = shape
    P = N * S
    assert P % 32
    eng = Engine(hip, "pe")
    rays, z = inputs("pe", N, S, seed=P)
    r = rays[N - 1].cpu().numpy()
    j = int(np.abs(r[3:6]).argmax())
    zb = np.float32((5000.0 + abs(float(r[j]))) / abs(float(r[3 + j])))
    assert abs(np.float32(r[j] + np.float32(r[3 + j] * zb))) >= 4094          # (ro + rd z in the kernel's two f32 roundings)
    z_bad = z.clone()
    z_bad[N - 1, S - 1] = float(zb)                                         # (the largest depth of the last ray: still sorted)
    flag = hip.capi.range_flag(torch.device(DEV))
    out = {}
    for tag, zz in (("clean", z), ("bad", z_bad)):
        raw, rec = padded(P * 4), padded(P * eng.rec)
        flag.reset()
        eng.forward(N, S, rays, zz, raw, rec, "f16x2")
        torch.cuda.synchronize()
        assert pad_intact(raw, P * 4) and pad_intact(rec, P * eng.rec), tag
        out[tag] = (raw[:P * 4].view(P, 4), rec[:P * eng.rec].view(P, eng.rec), int(flag.word[0]))
    (raw_c, rec_c, word_c), (raw_b, rec_b, word_b) = out["clean"], out["bad"]
    assert word_c == 0 and word_b & 1, (word_c, word_b)
    assert torch.isnan(raw_b[P - 1]).all(), raw_b[P - 1]
    assert torch.equal(bits(raw_b[:P - 1]), bits(raw_c[:P - 1]))
    assert torch.equal(bits(rec_b[:P - 1]), bits(rec_c[:P - 1]))


@pytest.mark.parametrize("shape", FLAG_SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("model", list(ENC))
def test_f16x2_non_finite_gradient_at_the_last_live_point(hip, model, shape):
    """dL/dalpha = inf at the last live point of a partial tile (its scale stays 1, nerf_pow2_scale): the flag rises, that point's
    grad_record row is non-finite down to layer1's gradient, every other row is the clean run's, bit for bit"""
    N, S = shape
    P = N * S
    eng = Engine(hip, model)
    rays, d = inputs(model, N, S, seed=P)
    raw, rec = padded(P * 4), padded(P * eng.rec)
    eng.forward(N, S, rays, d, raw, rec, "f16x2")
    g = spread_g_raw(P, seed=P)
    g_bad = g.copy()
    g_bad[P - 1, 3] = np.inf
    flag = hip.capi.range_flag(torch.device(DEV))
    out = {}
    for tag, gg in (("clean", g), ("bad", g_bad)):
        grec = padded(P * GREC)
        flag.reset()
        eng.backward(P, rec, T(gg), grec, "f16x2")
        torch.cuda.synchronize()
        assert pad_intact(grec, P * GREC), tag
        out[tag] = (grec[:P * GREC].view(P, GREC), int(flag.word[0]))
    (gc, word_c), (gb, word_b) = out["clean"], out["bad"]
    assert word_c == 0 and word_b & 1, (word_c, word_b)
    assert torch.isinf(gb[P - 1, G_A]) and not torch.isfinite(gb[P - 1, G_L1:G_L1 + 128]).all()
    assert torch.equal(bits(gb[:P - 1]), bits(gc[:P - 1]))


# ---- the host path at ragged sample counts, against the upstream code (g25) -------------------------------------------------------------

SPEC25 = {"mip": dict(params=mip_params, kwargs=dict(include_input_xyz=False), encode="mip", sid="lego_DS8", seed=25),
          "pe": dict(params=pe_params, kwargs={}, encode="positional_encoding", sid="lego", seed=26)}


@pytest.fixture(scope="module")
def g25():
    return load_golden("g25_nerf_ragged.npz")


def _g25(g, model):
    """one baseline's part of the fixture, keys without the "mip." / "pe." prefix"""
    return {k[len(model) + 1:]: v for k, v in g.items() if k.startswith(model + ".")}


def _run25(hip, g, model, mc, mf, mode, ndc=False, **kw):
    s = SPEC25[model]
    H, W, focal = g["c.hwf"]
    o = checks.opts(s["encode"], chunk=int(g["chunksize"]), nc=int(g["num_coarse"]), nf=int(g["num_fine"]), **kw)
    rays = torch.stack((T(g["c.ro"]).reshape(-1, 3), T(g["c.rd"]).reshape(-1, 3)))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # (an out-of-range f16x2 frame is rendered again in bf16x3, warned: test_nerf_baseline_f16.py)
        return hip.train_utils.run_one_iter_of_nerf(int(H), int(W), float(focal), mc, mf, rays, o, s["sid"], mode=mode, scene_config=scene(ndc))


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("model", list(ENC))
def test_ragged_validation_render_matches_upstream(hip, g25, model, arith):
    s, g = SPEC25[model], _g25(g25, model)
    mc, mf = checks.models_from(hip, g, arith, s["params"], **s["kwargs"])
    for tag, ndc in (("c.", False), ("c.ndc.", True)):
        with torch.no_grad():
            out = _run25(hip, g, model, mc, mf, "validation", ndc=ndc)
        assert out[0].shape == g[tag + "rgb_coarse"].shape and out[3].shape == g[tag + "rgb_fine"].shape
        check_render(out, g, tag)


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("model", list(ENC))
def test_ragged_train_step_matches_upstream(hip, g25, model, arith):
    s, g = SPEC25[model], _g25(g25, model)
    mc, mf = checks.models_from(hip, g, arith, s["params"], **s["kwargs"])
    torch.manual_seed(s["seed"])
    out = _run25(hip, g, model, mc, mf, "train", perturb=True, noise=0.2)
    target = T(g["d.target"])
    loss = torch.nn.functional.mse_loss(out[0], target) + torch.nn.functional.mse_loss(out[3], target)
    loss.backward()
    check_render(out, g, "d.")
    check_grads((mc, mf), g, "d")
