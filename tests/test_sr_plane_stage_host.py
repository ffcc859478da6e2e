"""CPU half of tests/test_sr_plane_stage.py: the float64 reference of PlanesSR's plane stage (tests/sr_plane_ref.py) against the committed
goldens, its region bounds against float32 arithmetic in upstream's order, the conditions the case tables promise, and the sensitivity of
the yardsticks: every one-line mutant of the reference exceeds the a-priori bounds somewhere, and -- where those are slack (x8, the ReLU
case) -- the network-path mutants, all-zero gradients and a dropped network output exceed the tight random-walk yardstick, which a float32 run
of the chain on the CPU stays within.  So the GPU assertions can fail."""
import numpy as np
import pytest
import torch

import sr_plane_ref as ref
from conftest import load_golden


def _weights(g):
    return [g[k] for k in g if k.startswith("sd.inner_model.")]


def _cfg(g):
    """-> nblocks, n_up, pad, over of a golden's network"""
    Cc, hid, nblocks, sf, R, pad, over = [int(v) for v in g["cfg"]]
    n_up = sf.bit_length() - 1
    assert sf == 1 << n_up and (pad, over) == ref.pad_over(nblocks, n_up)
    return nblocks, n_up, pad, over


def _forward_matches(out, golden):
    assert np.array_equal(np.isnan(out), np.isnan(golden))
    m = ~np.isnan(golden)
    assert m.any()
    np.testing.assert_allclose(out[m], golden[m], rtol=0, atol=1e-5)


def _gradient_matches(got, golden):
    golden = golden.astype(np.float64)
    assert np.linalg.norm(got - golden) / np.linalg.norm(golden) < 2e-5
    np.testing.assert_allclose(got, golden, rtol=0, atol=2e-5 * np.abs(golden).max())


# ---- 1. the reference against the committed goldens: where they disagree, the reference is wrong --------------------------------------
def test_reference_reproduces_g09_and_g20_forwards():
    g = load_golden("g09_edsr.npz")
    nb, n_up, pad, over = _cfg(g)
    _forward_matches(ref.planes_sr64(g["lr"][0], _weights(g), nb, n_up, pad, over, None), g["sr_full"][0])
    assert np.isnan(g["sr_roi"]).any()
    _forward_matches(ref.planes_sr64(g["lr"][0], _weights(g), nb, n_up, pad, over, g["roi"].reshape(-1)), g["sr_roi"][0])
    g = load_golden("g20_sr_options.npz")
    nb, n_up, pad, over = _cfg(g)
    for key, roi in (("sr_full", None), ("sr_roi", g["roi"].reshape(-1))):
        _forward_matches(ref.planes_sr64(g["lr"][0], _weights(g), nb, n_up, pad, over, roi, g["mean"], g["std"]), g[key][0])
    plain = ref.planes_sr64(g["lr"][0], _weights(g), nb, n_up, pad, over, None)
    assert np.abs(plain - g["sr_full"][0]).max() > 1e-3               # the normalisation matters on this fixture


def test_reference_reproduces_g14_gradients():
    g9, g = load_golden("g09_edsr.npz"), load_golden("g14_sr_grads.npz")
    nb, n_up, pad, over = _cfg(g9)
    for tag, roi in (("roi", g["roi"].reshape(-1)), ("full", None)):
        r = ref.reference(g9["lr"][0], _weights(g9), nb, n_up, pad, over, roi, d_out=np.nan_to_num(g["sr_%s_gout" % tag][0]), bounds=False)
        _gradient_matches(r["gw"], g["sr_%s_gw" % tag])
        _gradient_matches(r["d_lr"], g["sr_%s_glr" % tag][0])


# (g22 holds the full plane's training output and gradients for align_corners=False only)
@pytest.mark.parametrize("name,mode,align,tags", [("sr_align_false", "bilinear", 0, ("roi", "full")), ("sr_bicubic", "bicubic", 1, ("roi",)),
                                                  ("sr_bicubic_noalign", "bicubic", 0, ("roi",))])
def test_reference_reproduces_g22_residual_options(name, mode, align, tags):
    g9, g = load_golden("g09_edsr.npz"), load_golden("g22_model_options.npz")
    nb, n_up, pad, over = _cfg(g9)
    lr, ws = g9["lr"][0], _weights(g9)
    _forward_matches(ref.planes_sr64(lr, ws, nb, n_up, pad, over, None, mode=mode, align=align), g[name + ".full"][0])
    for tag in tags:
        roi = g[name + ".roi"].reshape(-1) if tag == "roi" else None
        r = ref.reference(lr, ws, nb, n_up, pad, over, roi, mode=mode, align=align, d_out=np.nan_to_num(g[name + ".%s_gout" % tag][0]), bounds=False)
        _forward_matches(r["out"], g[name + ".%s_out" % tag][0])
        _gradient_matches(r["gw"], g[name + ".%s_gw" % tag])
        _gradient_matches(r["d_lr"], g[name + ".%s_glr" % tag][0])


def test_tap_matrices_are_f_interpolate():
    """the matrices the residual's bounds are built from are the operation the reference calls"""
    import torch.nn.functional as F
    gen = torch.Generator().manual_seed(2)
    for mode in ("bilinear", "bicubic"):
        for align in (True, False):
            for n in (1, 2, 5, 7):
                for sf in (1, 2, 4, 8, 16):
                    M, E = ref.tap_matrix(n, sf, mode, align)
                    x = torch.randn(1, 1, n, 3, generator=gen, dtype=torch.float64)
                    y = F.interpolate(x, scale_factor=(sf, 1), mode=mode, align_corners=align)[0, 0]
                    assert float((torch.as_tensor(M) @ x[0, 0] - y).abs().max()) < 1e-13, (mode, align, n, sf)
                    assert (E >= 0).all() and E.max() < 1e-3


# ---- 2. the region bounds -----------------------------------------------------------------------------------------------------------------
def _valid_box(t):
    v = ~np.isnan(t[0])
    rows, cols = np.where(v.any(1))[0], np.where(v.any(0))[0]
    assert v[rows[0]: rows[-1] + 1, cols[0]: cols[-1] + 1].all()
    return [int(rows[0]), int(cols[0])], [int(rows[-1]) + 1, int(cols[-1]) + 1]


def test_roi_bounds_equal_the_goldens_valid_boxes():
    g9, g20, g22 = load_golden("g09_edsr.npz"), load_golden("g20_sr_options.npz"), load_golden("g22_model_options.npz")
    cases = [(g9["roi"], g9["sr_roi"][0]), (g20["roi"], g20["sr_roi"][0])]
    cases += [(g22[n + ".roi"], g22[n + ".roi_out"][0]) for n in ("sr_align_false", "sr_bicubic", "sr_bicubic_noalign")]
    for roi, out in cases:
        lo, hi = ref.roi_bounds(20, 20, roi.reshape(-1))
        blo, bhi = _valid_box(out)
        assert [4 * v for v in lo] == blo and [4 * v for v in hi] == bhi
    # g09's region on 20 rows: 1 + 0.2f rounds and 20 * 1.2f / 2 is exactly 12 in float32 -> rows 5..13; float64 keeps 12.00000003 -> 5..14
    assert ref.roi_bounds(20, 20, g9["roi"].reshape(-1))[1][0] == 13
    assert ref.roi_bounds(20, 20, g9["roi"].reshape(-1), np.float64)[1][0] == 14


def test_roi_bounds_equal_float32_arithmetic_in_upstreams_order():
    values = [k / 8 for k in range(-10, 11)] + [0.2, 0.15, -0.35, -0.6]
    for R0 in (1, 2, 7, 11, 20):
        for R1 in (1, 2, 7, 11, 20):
            shape = torch.tensor([R0, R1])
            for a in values:
                for b in values:
                    roi = torch.tensor([[a, b], [b, a]], dtype=torch.float32)
                    box = shape * (1 + roi) / 2                          # (an int64 tensor times a float32 one: float32)
                    assert box.dtype == torch.float32
                    box = torch.stack([torch.floor(box[0]), torch.ceil(box[1])], 0).numpy().astype(np.int32)
                    lo, hi = np.maximum(0, box[0] - 1), np.minimum(np.array([R0, R1]), box[1] + 1)
                    got = ref.roi_bounds(R0, R1, [a, b, b, a])
                    assert got == (lo.tolist(), hi.tolist()), (R0, R1, a, b)


# ---- 3. what the case tables promise ----------------------------------------------------------------------------------------------------
def test_every_border_situation_occurs():
    seen = set()
    for R0, R1 in ref.PLANES:
        for roi in ref.REGIONS.values():
            seen |= ref.border_situations(R0, R1, roi, 4)
    assert seen == ref.ALL_SITUATIONS, ref.ALL_SITUATIONS - seen
    # the larger planes' interior box leaves a texel between its window lo - 1 .. hi + 1 and the border, on both axes
    for R0, R1 in [(7, 11), (11, 7), (20, 20)]:
        assert "interior_on_both_axes" in ref.border_situations(R0, R1, ref.REGIONS["interior"], 4)
    # the point region is 2 or 3 texels by the parity of R
    assert ref.roi_bounds(7, 20, ref.REGIONS["point"]) == ([2, 9], [5, 11])
    # pad and over of the tables' networks
    assert [ref.pad_over(0, n) for n in range(5)] == [(3, 0), (4, 1), (4, 1), (4, 1), (4, 1)]
    assert ref.pad_over(ref.RELU["nblocks"], ref.RELU["n_up"]) == (ref.RELU["pad"], ref.RELU["over"])


def relu_case(seed):
    c = ref.RELU
    ws, lrs, d_outs = ref.make_case(seed, c["hid"], c["nblocks"], c["n_up"], [c["plane"]] * 3)
    return [ref.reference(lr, ws, c["nblocks"], c["n_up"], c["pad"], c["over"], ref.REGIONS[r], d_out=d)
            for lr, d, r in zip(lrs, d_outs, c["regions"])]


@pytest.mark.parametrize("seed", ref.RELU["seeds"])
def test_no_relu_gate_of_the_relu_case_can_flip(seed):
    """every pre-activation of the float64 run is at least 2 x its layer's a-priori bound away from zero: the device's gates are float64's"""
    n = 0
    for r in relu_case(seed):
        worst, count = ref.relu_margins(r)
        assert worst >= 2.0, worst
        n += count
    assert n > 5000


# ---- 4. sensitivity: the bounds notice every one-line mutant ---------------------------------------------------------------------------
def _sensitivity_cases():
    lin = ref.LINEAR
    zero = ref.make_case(11, ref.RESIDUAL["hid"], 0, 2, [(20, 20), (7, 11)], zero_weights=True)
    one = ref.make_case(12, lin["hid"], 0, 1, [(7, 11), (11, 7)])
    ms = (np.array(lin["mean"]), np.array(lin["std"]))
    yield dict(ws=zero[0], lr=zero[1][0], d_out=zero[2][0], n_up=2, roi=ref.REGIONS["g09"], mode="bilinear", align=1, ms=(None, None))
    yield dict(ws=zero[0], lr=zero[1][1], d_out=zero[2][1], n_up=2, roi=ref.REGIONS["interior"], mode="bilinear", align=0, ms=(None, None))
    yield dict(ws=one[0], lr=one[1][0], d_out=one[2][0], n_up=1, roi=ref.REGIONS["bottom_right"], mode="bilinear", align=1, ms=ms)
    yield dict(ws=one[0], lr=one[1][1], d_out=one[2][1], n_up=1, roi=ref.REGIONS["full"], mode="bicubic", align=1, ms=ms)


def _deep_cases():
    """where the a-priori bound of the network path exceeds its values: a x8 linear network (normalised, non-square plane, region on the high
    border) and the ReLU case's three planes"""
    lin, c = ref.LINEAR, ref.RELU
    ws, lrs, d_outs = ref.make_case(230 + 1, lin["hid"], 0, 3, lin["planes"])
    pad, over = ref.pad_over(0, 3)
    yield "x8", (lrs[0], ws, 0, 3, pad, over, ref.REGIONS["bottom_right"], np.array(lin["mean"]), np.array(lin["std"]), "bilinear", 1), d_outs[0]
    ws, lrs, d_outs = ref.make_case(c["seeds"][0], c["hid"], c["nblocks"], c["n_up"], [c["plane"]] * 3)
    for lr, d, rn in zip(lrs, d_outs, c["regions"]):
        yield "relu_" + rn, (lr, ws, c["nblocks"], c["n_up"], c["pad"], c["over"], ref.REGIONS[rn], None, None, "bilinear", 1), d


@pytest.fixture(scope="module")
def deep_refs():
    return [(name, args, d_out, ref.reference(*args, d_out=d_out)) for name, args, d_out in _deep_cases()]


@pytest.fixture(scope="module")
def sensitivity_refs():
    out = []
    for c in _sensitivity_cases():
        pad, over = ref.pad_over(0, c["n_up"])
        args = (c["lr"], c["ws"], 0, c["n_up"], pad, over, c["roi"], c["ms"][0], c["ms"][1], c["mode"], c["align"])
        out.append((args, c["d_out"], ref.reference(*args, d_out=c["d_out"])))
    return out


def _exceeds(r, m):
    if not np.array_equal(np.isnan(r["out"]), np.isnan(m["out"])):
        return True                                                    # (the GPU test asserts the NaN mask exactly)
    ins = ~np.isnan(r["out"])
    return bool((np.abs(m["out"] - r["out"])[ins] > r["out_bound"][ins]).any() or (np.abs(m["d_lr"] - r["d_lr"]) > r["d_lr_bound"]).any())


@pytest.mark.parametrize("mutant", ref.MUTANTS)
def test_every_mutant_exceeds_the_bound_somewhere(sensitivity_refs, mutant):
    hits = [_exceeds(r, ref.reference(*args, d_out=d_out, mutant=mutant, bounds=False)) for args, d_out, r in sensitivity_refs]
    assert any(hits), mutant


NETWORK_MUTANTS = ("clamp_R_minus_2", "origin_plus_1", "over_off_by_one", "axes_swapped_in_clamp", "std_not_in_backward")


@pytest.mark.parametrize("mutant", NETWORK_MUTANTS)
def test_network_path_mutants_exceed_the_tight_yardstick_where_the_a_priori_bound_is_slack(deep_refs, mutant):
    """on the x8 linear case and on the ReLU case the a-priori bounds of d_lr and of the weight gradient exceed the values themselves; the
    tight yardstick notices every mutant of the network path there, in d_lr AND in the weight-gradient blob (std_not_in_backward: d_lr only --
    the weights' gradient does not pass through the division; it needs the normalised case; clamp_R_minus_2 needs a region on the high border).
    The other mutants change the residual or the region, where the a-priori bounds are tight and the NaN mask is asserted exactly."""
    tripped = {"d_lr": set(), "gw": set()}
    for name, args, d_out, r in deep_refs:
        m = ref.reference(*args, d_out=d_out, mutant=mutant, bounds=False)
        if (np.abs(m["d_lr"] - r["d_lr"]) > ref.d_lr_tight(r, 0.0)).any():
            tripped["d_lr"].add(name)
        if (np.abs(m["gw"] - r["gw"]) > ref.gw_tight([r])).any():
            tripped["gw"].add(name)
    if mutant == "std_not_in_backward":
        assert tripped["d_lr"] == {"x8"}
    else:
        assert "x8" in tripped["d_lr"] and "x8" in tripped["gw"], tripped
        assert any(n.startswith("relu") for n in tripped["d_lr"]) and any(n.startswith("relu") for n in tripped["gw"]), tripped


def test_wrong_answers_the_a_priori_bound_admits_fail_the_tight_yardstick(deep_refs):
    """all-zero gradients and a dropped network output: within the a-priori bound on most elements of these cases, outside the tight one"""
    for name, args, d_out, r in deep_refs:
        ins = ~np.isnan(r["out"])
        reached = r["d_lr"] != 0                                        # (texels that the region's gradient reaches at all)
        assert reached.mean() > 0.5 and (np.abs(r["d_lr"]) > ref.d_lr_tight(r, 0.0))[reached].mean() > 0.95, name
        assert (np.abs(r["gw"]) > ref.gw_tight([r])).mean() > 0.95, name
        residual_only = ref.reference(args[0], [0 * w for w in args[1]], *args[2:], bounds=False)["out"]
        assert (np.abs(residual_only - r["out"])[ins] > r["out_tight"][ins]).mean() > 0.95, name
        # ... and the tight yardstick is below the a-priori bound, the necessary condition
        assert (r["out_tight"][ins] <= r["out_bound"][ins] * 1.0000001 + 1.01 * ref.U * np.abs(r["out"][ins])).all()


def _float32_run(lr, ws, nblocks, n_up, pad, over, roi, mean, std, mode, align, d_out):
    """the reference's own chain in float32 on the CPU: an f32 accumulation in another order than the device's"""
    t = lambda a: None if a is None else torch.tensor(np.asarray(a, np.float32))
    a, b, wl = t(lr).requires_grad_(True), t(lr).requires_grad_(True), [t(w).requires_grad_(True) for w in ws]
    out, _, _ = ref._stage(a, b, wl, nblocks, n_up, pad, over, roi, t(mean), t(std), mode, align, tenth=float(np.float32(0.1)))
    g = torch.where(torch.isnan(out.detach()), torch.zeros(()), t(d_out))
    gr = torch.autograd.grad((torch.nan_to_num(out) * g).sum(), [a, b] + wl)
    return out.detach().numpy(), (gr[0] + gr[1]).numpy(), ref.join_blob(gr[2:])


def test_a_float32_run_of_the_chain_is_within_the_tight_yardstick(deep_refs):
    """the random-walk model against an f32 arithmetic that is not the device's: worst |error| / yardstick stays near 4.9 / 19.6 sigma"""
    for name, args, d_out, r in deep_refs:
        out, d_lr, gw = _float32_run(*args, d_out)
        for got, want, bound in ((np.nan_to_num(out), np.nan_to_num(r["out"]), r["out_tight"]), (d_lr, r["d_lr"], ref.d_lr_tight(r, 0.0)),
                                 (gw, r["gw"], ref.gw_tight([r]))):
            assert ref.worst_ratio(got, want, bound)[0] <= 0.5, name


def test_the_unmutated_reference_is_within_its_own_bounds(sensitivity_refs):
    for args, d_out, r in sensitivity_refs:
        assert not _exceeds(r, ref.reference(*args, d_out=d_out, bounds=False))
        assert (r["out_bound"][~np.isnan(r["out"])] > 0).all() and (r["d_lr_bound"] >= 0).all()
