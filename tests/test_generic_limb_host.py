"""CPU tests of the generic geometries' 'f16x2' evaluation (csrc/generic_fused_limb.hip): the numpy reference of the arithmetic
(tests/generic_limb_ref.py) against float64 under the project's bound for these kernels, its power to tell a dropped product, and the entry
points that answer without a device."""
import ctypes as C

import numpy as np
import pytest

import generic_limb_ref as ref
from test_generic_fused import SHAPES, points, within_bound
from test_oracle import G22_BOX

ERR_SHAPE, ERR_NULL = 1, 3          # nvsr_status (include/nvsr.h)


@pytest.fixture(scope="module")
def pkg():
    import nvsr_amd

    nvsr_amd.build_extension()
    return nvsr_amd


@pytest.mark.parametrize("case", list(SHAPES))
def test_two_limbs_meet_the_bound_and_the_high_limbs_alone_do_not(pkg, case):
    """on every shape of test_generic_fused.SHAPES (seed 7, 77 points: the GPU tests' model): the two-limb reference within
    2e-5 max(1, max|ref|) of the float64 restatement; the hi-limb-only variant beyond it -- these inputs can tell a dropped product"""
    from oracle.generic_decoder import decode
    n_pos, kw = SHAPES[case]
    _, sd, planes, kw = ref.seeded_state(pkg, 7, n_pos=n_pos, **kw)
    x = points(77, seed=11)
    f64 = decode(sd, planes, G22_BOX, x, **kw)
    two = ref.decode_limb(sd, planes, G22_BOX, x, **kw)
    bound = 2e-5 * max(1.0, float(np.abs(f64).max()))
    err2 = float(np.abs(two - f64).max())
    err1 = float(np.abs(ref.decode_limb(sd, planes, G22_BOX, x, hi_only=True, **kw) - f64).max())
    print("%s: two limbs %.3g, high limbs only %.3g, bound %.3g" % (case, err2, err1, bound))
    within_bound(two, f64, case)
    assert err1 > bound, (case, err1, bound)


def test_reference_layer_is_the_float64_layer_on_f16_operands(pkg):
    """operands that are f16 numbers after their scales have zero low limbs: the limb layer is the float64 layer"""
    rng = np.random.default_rng(0)
    W = (rng.integers(-512, 513, (33, 50)) / 256.0).astype(np.float32)
    x = (rng.integers(-512, 513, (77, 50)) / 16.0).astype(np.float32)
    b = rng.standard_normal(33).astype(np.float32)
    assert np.array_equal(ref.layer(W, b, x), ref.layer_f64(W, b, x).astype(np.float32))
    assert np.array_equal(ref.layer(W, b, x), ref.layer(W, b, x, hi_only=True))
    # beyond the ranges: NaN, never a number
    W[3, 7] = 300.0
    assert np.isnan(ref.layer(W, b, x)[:, 3]).all() and np.isfinite(ref.layer(W, b, x)[:, 4]).all()
    x[5, 2] = 5000.0
    assert np.isnan(ref.layer(W, b, x)[5]).all()


def geometry(pkg, **kw):
    g = dict(plane_channels=48, viewdir_channels=48, hidden=64, density_layers=4, rgb_layers=4, skip_connect_every=0, proj_combination=1,
             viewdir_combination=4)
    g.update(kw)
    return pkg.capi.DecoderGeometry(*[g[k] for k in ("plane_channels", "viewdir_channels", "hidden", "density_layers", "rgb_layers",
                                                      "skip_connect_every", "proj_combination", "viewdir_combination")])


def test_supported_and_size_entries_answer_without_a_device(pkg):
    lib, A = pkg.capi.lib(), pkg.capi.ARITHMETIC
    F16, INHERIT = pkg.capi.RENDER_ARITHMETIC["f16"], -1
    g = geometry(pkg)
    for arith, want in ((A["f32"], 1), (A["f16x2"], 1), (F16, 0), (A["bf16x3"], 0), (INHERIT, 0), (7, 0)):
        assert lib.nvsr_generic_fused_supported_arith(C.byref(g), 3, arith) == want, arith
    assert lib.nvsr_generic_fused_supported_arith(C.byref(g), 3, A["f32"]) == lib.nvsr_generic_fused_supported(C.byref(g), 3)
    # the packed size: per hidden layer ceil(K / 16) ceil(hidden / 32) 2 fragments of 256 words
    sizes = lambda Ks, hidden: sum(-(-K // 16) * -(-hidden // 32) * 512 for K in Ks)
    assert lib.nvsr_generic_packed_floats_ext(C.byref(g), 3) == sizes([48, 64, 64, 64, 192, 64, 64, 64], 64)
    g33 = geometry(pkg, hidden=33, skip_connect_every=1)             # layers 2, 3 read [hidden | input]
    assert lib.nvsr_generic_packed_floats_ext(C.byref(g33), 3) == sizes([48, 33, 33 + 48, 33 + 48, 192, 33, 33 + 192, 33 + 192], 33)
    assert lib.nvsr_generic_packed_floats_ext(C.byref(geometry(pkg, hidden=1, density_layers=1, rgb_layers=1)), 3) == sizes([48, 192], 1)
    # beyond the capacity: 0, with a size all the same (packing does not depend on the kernel)
    wide = geometry(pkg, hidden=4096, density_layers=1, rgb_layers=1)
    assert lib.nvsr_generic_fused_supported_arith(C.byref(wide), 3, A["f16x2"]) == 0
    assert lib.nvsr_generic_packed_floats_ext(C.byref(wide), 3) == sizes([48, 192], 4096)
    deep_rows = geometry(pkg, plane_channels=40, viewdir_channels=40, hidden=256, proj_combination=2, viewdir_combination=4)
    assert lib.nvsr_generic_fused_supported_arith(C.byref(deep_rows), 15, A["f16x2"]) == 0       # Kr = 640 > 512
    # inconsistent geometries and bad plane counts: the negated status, for every arithmetic
    bad = geometry(pkg, proj_combination=0, viewdir_combination=3)                                 # 'concat' view on summed position features
    for arith in (A["f32"], A["f16x2"], F16):
        assert lib.nvsr_generic_fused_supported_arith(C.byref(bad), 3, arith) == -ERR_SHAPE
        assert lib.nvsr_generic_fused_supported_arith(C.byref(g), 0, arith) == -ERR_SHAPE
        assert lib.nvsr_generic_fused_supported_arith(None, 3, arith) == -ERR_NULL
    assert lib.nvsr_generic_packed_floats_ext(C.byref(bad), 3) == -ERR_SHAPE
    assert lib.nvsr_generic_packed_floats_ext(C.byref(g), 16) == -ERR_SHAPE
    assert lib.nvsr_generic_packed_floats_ext(None, 3) == -ERR_NULL
    assert lib.nvsr_generic_decoder_natural_floats_ext(C.byref(bad), 3) < 0


def test_generic_arithmetic_is_by_name_only(pkg, monkeypatch):
    """the decision touches no GPU: None, the process default and any other name keep 'f32'; 'f16x2' needs the handle or a measured width"""
    import torch
    m, *_ = ref.seeded_state(pkg, 1, dec_channels=64, proj_combination="avg", viewdir_proj_combination="concat_pos")
    m.eval()
    span = m.GENERIC_LIMB_DEFAULT_HIDDEN
    monkeypatch.setenv("NVSR_GENERIC_FUSED", "1")
    with torch.no_grad():
        for name in (None, "f32", "bf16x3", "f16", 2):
            m.arithmetic = name
            assert m.generic_arithmetic() == "f32", name
        m.arithmetic = "f16x2"
        assert m.generic_arithmetic() == "f16x2"
        monkeypatch.setenv("NVSR_GENERIC_FUSED", "0")
        assert m.generic_arithmetic() == "f32"
        monkeypatch.delenv("NVSR_GENERIC_FUSED")
        assert m.generic_arithmetic() == ("f16x2" if span is not None and span[0] <= 64 <= span[1] else "f32")
        monkeypatch.setenv("NVSR_GENERIC_FUSED", "1")
    assert m.generic_arithmetic() == "f32" and m.generic_route() == "layered"       # gradients on, parameters that take them
    assert m.arithmetic == "f16x2"
