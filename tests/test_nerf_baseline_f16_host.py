"""CPU checks of the f16x2 arithmetic of the two FlexibleNeRFModel baselines: which arithmetic a call runs (capi.resolve_nerf_arithmetic against
the library's nerf_arith), the argument checks of the entry points in NVSR_ARITH_F16X2, and the model's default."""
import pytest


@pytest.fixture(scope="module")
def pkg():
    import nvsr_amd
    return nvsr_amd


def test_resolve_nerf_arithmetic_reads_an_inherited_f16x2_as_bf16x3(pkg):
    capi = pkg.capi
    A = capi.ARITHMETIC
    before = capi.get_decoder_arithmetic()
    try:
        for default, inherited in (("f16x2", "bf16x3"), ("bf16x3", "bf16x3"), ("f32", "f32")):
            capi.set_decoder_arithmetic(default)
            assert capi.resolve_nerf_arithmetic(None) == A[inherited], default
            assert capi.resolve_nerf_arithmetic(capi.ARITH_INHERIT) == A[inherited], default
            for mode in ("f32", "bf16x3", "f16x2"):          # an explicit request is what runs
                assert capi.resolve_nerf_arithmetic(mode) == A[mode]
        # (the decoder's own resolution is unchanged: an inherited f16x2 is f16x2 there)
        capi.set_decoder_arithmetic("f16x2")
        assert capi.resolve_decoder_arithmetic(None) == A["f16x2"]
    finally:
        capi.set_decoder_arithmetic(before)


@pytest.mark.parametrize("prefix", ["mip", "pe"])
def test_f16x2_entry_points_check_their_arguments_before_any_launch(pkg, prefix):
    lib = pkg.capi.lib()
    f16 = pkg.capi.ARITHMETIC["f16x2"]
    fwd = getattr(lib, "nvsr_%s_nerf_forward_arith" % prefix)
    bwd = getattr(lib, "nvsr_%s_nerf_backward_arith" % prefix)
    radius = (0.0,) if prefix == "mip" else ()
    assert fwd(-1, 4, None, None, *radius, None, None, None, f16, None) == 1            # NVSR_ERR_SHAPE
    assert fwd(1, 0, None, None, *radius, None, None, None, f16, None) == 1
    assert fwd(0, 4, None, None, *radius, None, None, None, f16, None) == 0             # nothing to do
    assert fwd(1, 4, None, None, *radius, None, None, None, f16, None) == 3             # NVSR_ERR_NULL
    assert bwd(-1, None, None, None, None, f16, None) == 1
    assert bwd(0, None, None, None, None, f16, None) == 0
    assert bwd(1, None, None, None, None, f16, None) == 3
    assert bwd(1, None, None, None, None, 7, None) == 1


def test_flexible_nerf_default_arithmetic_stays_bf16x3(pkg):
    assert pkg.models.FlexibleNeRFModel.arithmetic == "bf16x3"
    assert pkg.models.FlexibleNeRFModel(include_input_xyz=False).arithmetic == "bf16x3"
