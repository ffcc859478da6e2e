"""CPU tests of the render pass's one-limb arithmetic 'f16' (NVSR_ARITH_F16 = 1 given to the evaluation renders): the numpy reference's own
properties (tests/render_f16_ref.py), and the paths that accept or refuse the value without a GPU."""
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import render_f16_ref as R
import triplane_checks as tc

SIZES = [(64, 64)] * 4


@pytest.fixture(scope="module")
def pkg():
    import nvsr_amd

    nvsr_amd.capi.lib()
    return nvsr_amd


def _forward64(dec, planes, rays, z, scene):
    return tc.forward64(dec, [torch.as_tensor(p).double() for p in planes], rays, z, scene)[0].numpy()


def test_reference_equals_float64_where_nothing_is_rounded_and_only_there():
    scene = tc.make_scene(SIZES)
    rays, z = tc.make_rays(37, 5, 3)
    dec = tc.unpack(R.exact_decoder(11))
    planes = R.zero_planes(scene)
    got, want = R.forward(dec, planes, rays, z, scene), _forward64(dec, planes, rays, z, scene)
    assert np.isfinite(want).all() and np.abs(want).max() > 0.25 and len(np.unique(want[0])) > 1
    assert np.array_equal(got, want)                       # zero planes, +-2^-k weights, short biases: every operand an f16 number
    # ordinary operands are rounded: 11 bits of every weight, feature and activation
    dec = tc.unpack(tc.make_decoder(5))
    planes = tc.make_planes(scene, 6)
    got, want = R.forward(dec, planes, rays, z, scene), _forward64(dec, planes, rays, z, scene)
    err = np.abs(got - want).max() / np.abs(want).max()
    assert 2.0 ** -14 < err < 2.0 ** -5, err


def test_reference_never_turns_an_operand_beyond_the_range_into_a_number():
    x = np.float32([[1.0, 2.0, 3.0, 4.0]])
    b = np.zeros(2)
    assert np.isnan(R.layer(np.float32([[300.0, 1, 1, 1], [1, 1, 1, 1]]), b, x)[0, 0])                 # a weight of 300: inf, then NaN
    y = R.layer(np.float32([[-1.0, -1, -1, -1], [1, 1, 1, 1]]), b, np.float32([[5000.0, 1, 1, 1]]))
    assert np.isnan(y).all()                                                                          # -inf is not relu's 0, +inf is not carried on
    assert np.isnan(R.layer(np.float32([[0.0, 1, 1, 1], [1, 1, 1, 1]]), b, np.float32([[5000.0, 1, 1, 1]]))[0, 0])   # inf x 0
    assert np.isnan(R.head(np.float32([[1.0, 1, 0, 0]]), np.zeros(1), np.float32([[np.inf, 1, 1, 1]]))).all()
    assert np.array_equal(R.layer(np.float32([[1.0, 0, 0, 0], [-1, 0, 0, 0]]), np.float32([0.5, 0.5]), x), np.float32([[1.5, 0.0]]))
    assert R.rn16(np.float32(65519.0)) == 65504.0 and np.isinf(R.rn16(np.float32(65520.0))) and R.rn16(np.float32(2049.0)) == 2048.0


def test_tables_of_the_arithmetics(pkg):
    capi = pkg.capi
    assert capi.RENDER_ARITHMETIC == {"f32": 0, "f16": 1, "f16x2": 2, "bf16x3": 3}
    assert capi.ARITHMETIC == {"f32": 0, "f16x2": 2, "bf16x3": 3}               # (tests index it for the calls that refuse 'f16')
    assert capi.render_arith_code("f16") == 1 and capi.render_arith_code(None) == capi.ARITH_INHERIT and capi.render_arith_code(3) == 3
    assert capi.resolve_render_arithmetic("f16") == 1 and capi.resolve_render_arithmetic("bf16x3") == 3
    assert capi.resolve_render_arithmetic(None) == capi.lib().nvsr_get_decoder_arithmetic() != 1
    with pytest.raises(KeyError):
        capi.arith_code("f16")
    with pytest.raises(KeyError):
        capi.resolve_decoder_arithmetic("f16")


def test_f16_is_never_a_process_default_of_the_decoder(pkg):
    capi = pkg.capi
    lib = capi.lib()
    before = lib.nvsr_get_decoder_arithmetic()
    assert lib.nvsr_set_decoder_arithmetic(1) == 1 and lib.nvsr_get_decoder_arithmetic() == before          # NVSR_ERR_SHAPE, nothing changed
    with pytest.raises(KeyError):
        capi.set_decoder_arithmetic("f16")
    assert lib.nvsr_get_decoder_arithmetic() == before


def test_training_is_refused_by_name_before_any_launch(pkg):
    capi = pkg.capi
    ok = NS(arithmetic="f16x2")
    capi.refuse_f16_training(ok, NS(arithmetic=None), NS(arithmetic=2), NS(), None)
    for bad in (NS(arithmetic="f16"), NS(arithmetic=1)):
        with pytest.raises(capi.NvsrError, match="'f16'"):
            capi.refuse_f16_training(ok, bad)
    # the frame driver and the training step ask it first: no tensor of these stand-ins is ever touched
    mc, mf = pkg.models.TwoDimPlanesModel.__new__(pkg.models.TwoDimPlanesModel), NS(arithmetic="f16")
    with pytest.raises(capi.NvsrError, match="'f16'"):
        pkg.train_utils.run_one_iter_of_nerf(8, 8, 1.0, mc, mf, None, NS(nerf=NS(use_viewdirs=True)), "s", mode="train")
    step = pkg.training.TrainStep.__new__(pkg.training.TrainStep)
    step.mc, step.mf = NS(arithmetic="f16"), None
    with pytest.raises(capi.NvsrError, match="'f16'"):
        step.run(0, None, None, 8, 8, 1.0, 1, "s", {}, 16)
