"""CPU tests of the SR convolutions' one-limb arithmetic 'f16' (NVSR_ARITH_F16 = 1): the numpy reference's own properties, and the paths that
accept or refuse the value without a GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

import conv_f16_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pkg():
    import nvsr_amd

    nvsr_amd.capi.lib()
    return nvsr_amd


def test_quantisation_is_idempotent_and_follows_the_hardware_conversion():
    rng = np.random.default_rng(1)
    x = (rng.standard_normal(4096) * np.exp2(rng.uniform(-32, 14, 4096))).astype(np.float32)
    q = R.q16(x, 16.0)
    assert np.isinf(q).any() and (q == 0).any() and np.array_equal(R.q16(q.astype(np.float32)), q)
    # round to nearest EVEN at a tie, subnormals kept, overflow to inf (65520 is the first f32 that rounds up to 2^16)
    assert R.q16(np.float32(2049.0)) == 2048.0 and R.q16(np.float32(2051.0)) == 2052.0
    assert R.q16(np.float32(2.0 ** -24)) == 2.0 ** -24 and R.q16(np.float32(2.0 ** -26)) == 0.0 and R.q16(np.float32(1.5 * 2.0 ** -24)) == 2.0 ** -23
    assert R.q16(np.float32(65519.0)) == 65504.0 and np.isinf(R.q16(np.float32(65520.0))) and np.isinf(R.q16(np.float32(4095.0), 16.0))
    assert np.isfinite(R.q16(np.float32(4094.0), 16.0)) and np.isinf(R.q16(np.float32(255.95), 256.0)) and np.isfinite(R.q16(np.float32(255.9), 256.0))


def test_gradient_scale_puts_the_maximum_into_2_12_2_13():
    for v in (1.0, 0.9999, 3e-7, 7e5, 2.0 ** -100, 4095.9):
        s = R.gradient_scale(v)
        assert 2.0 ** 12 <= np.float32(v) * s < 2.0 ** 13 and np.log2(s) == int(np.log2(s)), v
    assert R.gradient_scale(0.0) == 1.0 and R.gradient_scale(np.inf) == 1.0 and R.gradient_scale(np.nan) == 1.0
    assert R.gradient_scale(2.0 ** -120) == 2.0 ** 127           # the exponent field clamped to 254


def test_representable_operand_builders_pass_their_own_check():
    rng = np.random.default_rng(2)
    w, x, g = R.representable_weights(rng, (128, 32, 3, 3)), R.representable_activations(rng, (32, 8, 40)), R.representable_gradient(rng, (128, 6, 38))
    assert R.is_representable(w, R.W_SCALE) and R.is_representable(x, R.X_SCALE) and R.is_representable(g, R.tensor_scale(g))
    for e in (-30, 0, 11):
        R.representable_gradient(rng, (16, 5, 7), exponent=e)
    # ... and the check refuses what is not: a 12-bit integer, a value below the subnormal spacing, one beyond the range
    assert not R.is_representable(np.float32([4097.0 * 2.0 ** -16]), R.W_SCALE)
    assert not R.is_representable(np.float32([2.0 ** -30]), R.X_SCALE) and not R.is_representable(np.float32([5000.0]), R.X_SCALE)
    # on such operands the reference equals float64 on the unquantised ones
    v, _, _ = R.conv_f16(x, w)
    assert np.array_equal(v, R.conv_f64(x, w)[0])
    v, _, _ = R.wgrad_f16(g, x)
    assert np.array_equal(v, R.wgrad_f64(g, x)[0])


def test_reference_is_within_the_stated_distance_of_float64():
    """random operands over several binades inside the normal f16 range of both scales: |reference - float64| <= (2^-10 + 2^-22) sum |w||x|
    (the reference adds no accumulation error, so the bound's n-term is not needed), for all three operations"""
    rng = np.random.default_rng(3)
    spread = lambda shape, lo, hi: (rng.choice([-1.0, 1.0], shape) * np.exp2(rng.uniform(lo, hi, shape))).astype(np.float32)
    Cin, Cout = 32, 128
    w, x = spread((Cout, Cin, 3, 3), -9, -2), spread((Cin, 8, 40), -5, 3)
    dy = spread((Cout, 6, 38), -20, -14)
    assert np.abs(w).min() * R.W_SCALE >= 2.0 ** -14 and np.abs(x).min() * R.X_SCALE >= 2.0 ** -14 and np.abs(dy).min() * R.tensor_scale(dy) >= 2.0 ** -14
    eps = 2.0 ** -10 + 2.0 ** -22
    v, _, _ = R.conv_f16(x, w)
    v64, a64 = R.conv_f64(x, w)
    assert (np.abs(v - v64) <= eps * a64).all() and (np.abs(v - v64) > 2.0 ** -16 * a64).any()
    v, _, _ = R.dgrad_f16(dy, w)
    v64, a64 = R.conv_f64(dy, R._flip(w), pad=2)
    assert (np.abs(v - v64) <= eps * a64).all()
    v, _, _ = R.wgrad_f16(dy, x)
    v64, a64 = R.wgrad_f64(dy, x)
    assert (np.abs(v - v64) <= eps * a64).all()


def test_binding_knows_the_mode_for_convolutions_only(pkg):
    capi = pkg.capi
    assert capi.ARITHMETIC == {"f32": 0, "f16x2": 2, "bf16x3": 3}
    assert capi.CONV_ARITHMETIC == {"f32": 0, "f16": 1, "f16x2": 2, "bf16x3": 3}
    lib = capi.lib()
    before = lib.nvsr_get_conv_arithmetic()
    try:
        assert lib.nvsr_set_conv_arithmetic(1) == 0 and capi.get_conv_arithmetic() == "f16" and capi.resolve_conv_arithmetic(None) == 1
        assert capi.resolve_conv_arithmetic("f16") == 1
        capi.set_conv_arithmetic("f16x2")
        capi.set_conv_arithmetic("f16")
        assert capi.get_conv_arithmetic() == "f16"
    finally:
        assert lib.nvsr_set_conv_arithmetic(before) == 0
    dec = lib.nvsr_get_decoder_arithmetic()
    assert lib.nvsr_set_decoder_arithmetic(1) == 1 and lib.nvsr_get_decoder_arithmetic() == dec          # NVSR_ERR_SHAPE, nothing changed
    with pytest.raises(KeyError):
        capi.set_decoder_arithmetic("f16")
    # packing "for F16" needs no region of its own: the packed sizes are what they were
    assert lib.nvsr_conv3x3_packed_floats(256, 256) == 256 // 4 * 8 * 1152 + (256 // 16) * 8 * 6912 + (256 // 32) * 16 * 6912 + (256 // 32) * 16 * 4608


def _load(env, tail=""):
    code = "import sys; sys.path.insert(0, %r); import nvsr_amd; nvsr_amd.capi.lib()%s" % (ROOT, tail)
    return subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)


def test_environment_selects_the_mode_for_convolutions_only():
    p = _load({"NVSR_CONV_ARITHMETIC": "f16"}, "; print(nvsr_amd.capi.get_conv_arithmetic(), nvsr_amd.capi.get_decoder_arithmetic())")
    assert p.returncode == 0 and p.stdout.split() == ["f16", "f16x2"], p.stderr[-500:]
    p = _load({"NVSR_DECODER_ARITHMETIC": "f16"})
    assert p.returncode != 0 and "NVSR_DECODER_ARITHMETIC" in p.stderr and "f16x2" in p.stderr, p.stderr[-500:]
    p = _load({"NVSR_CONV_ARITHMETIC": "f16x1"})
    assert p.returncode != 0 and "f16x2 | f16" in p.stderr, p.stderr[-500:]


def test_end_to_end_reference_and_its_recorded_errors(pkg):
    """the chain of the small PlanesSR(EDSR) case in float64 IS the project's oracle (to the f32 storage between the oracle's layers), and in the
    one-limb arithmetic it is as far from the oracle as recorded in conv_f16_ref.E2E_EREF -- the yardstick of the GPU test"""
    from oracle.oracle import Oracle
    orc = Oracle()
    sr, lrs, d_outs = R.e2e_case(pkg.models)
    o = R.e2e_oracle(orc, sr, lrs, d_outs)
    assert len({tuple(int(v) for v in ((~np.isnan(t)).any((0, 2)).sum(), (~np.isnan(t)).any((0, 1)).sum())) for t in o["out"]}) == 3      # ragged
    e = R.e2e_errors(R.e2e_reference(sr, o, quantise=False), o)
    assert e["out"] < 1e-6 and e["d_lr"] < 1e-6 and max(e["dw"]) < 1e-6, e
    e = R.e2e_errors(R.e2e_reference(sr, o, quantise=True), o)
    print("e_ref: out %.4e d_lr %.4e dw %s" % (e["out"], e["d_lr"], ", ".join("%.4e" % v for v in e["dw"])))
    rec = R.E2E_EREF
    assert abs(e["out"] / rec["out"] - 1) < 1e-3 and abs(e["d_lr"] / rec["d_lr"] - 1) < 1e-3
    assert len(e["dw"]) == len(rec["dw"]) == 8 and all(abs(x / y - 1) < 1e-3 for x, y in zip(e["dw"], rec["dw"])), e["dw"]
