"""CPU tests of planes-only training of the generic decoder geometries in 'f16x2' (csrc/generic_fused_bwd_limb.hip): the transposed packing
restated (tests/generic_train_limb_ref.py), the capacity and size entries without a device, the numpy reference's own properties, and the
predicate TwoDimPlanesModel.generic_train_arithmetic() over its inputs.  None touches a GPU."""
import ctypes as C
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from test_generic_fused_host import geometry_of
from test_generic_train_fused_host import supported as f32_supported
from test_oracle import G18_VARIANTS, G22_BOX, G22_KW

import generic_limb_ref as fwd
import generic_train_limb_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F16X2 = 0, 2
HANDLE = "NVSR_GENERIC_TRAIN_FUSED"
SHIPPED = dict(proj_combination="avg", viewdir_proj_combination="concat_pos")


@pytest.fixture(scope="module")
def pkg():
    import nvsr_amd

    nvsr_amd.build_extension()
    return nvsr_amd


def supported(pkg, geometry, arith, n_pos=3):
    geo = pkg.capi.DecoderGeometry(*geometry)
    return pkg.capi.lib().nvsr_generic_backward_fused_supported_arith(C.byref(geo), n_pos, arith)


def test_arithmetic_codes(pkg):
    assert pkg.capi.ARITHMETIC["f32"] == F32 and pkg.capi.ARITHMETIC["f16x2"] == F16X2


def test_capacity_by_arithmetic(pkg):
    """fails without the feature (the entry does not exist).  F32 answers nvsr_generic_backward_fused_supported, F16X2 the limb row of
    include/nvsr.h -- Kr + Kd (each up to 4) + hidden (up to 16) + 4 + layers x ceil(hidden / 32), up to 4 x an odd number, at most 1280 -- and
    every other arithmetic 0"""
    for name, kw in G18_VARIANTS.items():
        geo = geometry_of(dict(dict(skip_connect_every=3), **kw))
        assert supported(pkg, geo, F32) == f32_supported(pkg, geo) == 1 and supported(pkg, geo, F16X2) == 1, name
        for other in (1, 3, 4, 5, -1, 77):
            assert supported(pkg, geo, other) == 0, (name, other)
    assert ref.bwd_row_floats(192, 48, 256, 8) == 564 and supported(pkg, geometry_of(dict(SHIPPED, dec_channels=256)), F16X2) == 1
    assert supported(pkg, geometry_of(dict(SHIPPED, dec_channels=257)), F16X2) == 0
    assert supported(pkg, geometry_of(dict(SHIPPED, dec_channels=4096)), F16X2) == 0
    assert supported(pkg, geometry_of(dict(SHIPPED, dec_channels=31)), F16X2) == 1 and supported(pkg, geometry_of(dict(SHIPPED, dec_channels=33)), F16X2) == 1
    # 512 + 512 + 128 + 4 + 32 = 1188 <= 1280; with hidden 256: 512 + 512 + 256 + 4 + 64 = 1348 > 1280
    assert ref.bwd_row_floats(512, 512, 128, 8) == 1188 and supported(pkg, geometry_of(dict(proj_combination="sum", num_plane_channels=512)), F16X2) == 1
    assert ref.bwd_row_floats(512, 512, 256, 8) > 1280
    assert supported(pkg, geometry_of(dict(proj_combination="sum", num_plane_channels=512, dec_channels=256)), F16X2) == 0
    assert supported(pkg, geometry_of(dict(proj_combination="sum", num_plane_channels=513)), F16X2) == 0
    assert supported(pkg, [48, 48, 128, 4, 4, 0, 0, 3], F16X2) < 0 and supported(pkg, [48, 48, 128, 4, 4, 0, 0, 3], F32) < 0
    assert supported(pkg, geometry_of(SHIPPED), F16X2, 0) < 0 and supported(pkg, geometry_of(SHIPPED), F16X2, 16) < 0
    assert pkg.capi.lib().nvsr_generic_backward_fused_supported_arith(None, 3, F16X2) < 0
    assert torch.cuda.is_available() or not torch.cuda.is_initialized()


def test_limb_capacity_is_never_wider_than_the_forward_limb_kernels(pkg):
    rng = np.random.default_rng(6)
    seen = set()
    for _ in range(400):
        proj = int(rng.integers(0, 3))
        view = int(rng.choice([3, 4] if proj == 2 else [0, 1, 2, 4]))
        c = int(rng.choice([1, 24, 48, 96, 170, 256, 512]))
        geo = [c, c, int(rng.choice([1, 31, 64, 128, 200, 256, 257])), int(rng.integers(1, 65)), int(rng.integers(1, 65)), int(rng.integers(0, 4)), proj, view]
        n_pos = int(rng.integers(1, 16))
        g = pkg.capi.DecoderGeometry(*geo)
        f = pkg.capi.lib().nvsr_generic_fused_supported_arith(C.byref(g), n_pos, F16X2)
        b = supported(pkg, geo, F16X2, n_pos)
        assert f >= 0 and b in (0, 1) and not (b == 1 and f != 1), (geo, n_pos, f, b)
        seen.add((f, b))
    assert seen == {(0, 0), (1, 0), (1, 1)}


CASES = {
    "skip-hidden33": dict(dec_channels=33, dec_density_layers=5, dec_rgb_layers=3, skip_connect_every=1, proj_combination="avg", viewdir_proj_combination="concat_pos"),
    "skip-hidden31": dict(dec_channels=31, dec_density_layers=5, dec_rgb_layers=3, skip_connect_every=2, proj_combination="sum", viewdir_proj_combination="sum"),
    "concat-128": dict(dec_channels=128, proj_combination="concat", viewdir_proj_combination="concat"),
}


@pytest.mark.parametrize("case", list(CASES))
def test_transposed_blob_size_and_layout(pkg, case):
    """nvsr_generic_packed_bwd_floats_ext against the layout's own count; the restated packing unpacks to 2^8 W: the two limbs of every word sum
    to the f32 weight times 256 up to one f32 ulp (2^-23 |W~|) and half a step of the f16 subnormals (2^-25: a low limb below 2^-14), every word beyond the matrix is +0, and a lane's 4 words are 8 consecutive m of one column"""
    kw = CASES[case]
    m, sd, _, _ = fwd.seeded_state(pkg, 5, **kw)
    hidden = kw["dec_channels"]
    opts = dict(dec_density_layers=m.dec_density_layers, dec_rgb_layers=m.dec_rgb_layers, skip_connect_every=kw.get("skip_connect_every"))
    parts = ref.layer_parts(sd, hidden, **opts)
    geo = pkg.capi.DecoderGeometry(*[int(v) for v in m.generic_geometry()])
    words = pkg.capi.lib().nvsr_generic_packed_bwd_floats_ext(C.byref(geo), 3)
    assert words == ref.packed_bwd_words(hidden, parts)
    blob = ref.pack_bwd(parts, hidden)
    assert blob.dtype == np.uint32 and blob.size == words
    MB, at = (hidden + 15) // 16, 0
    for W, K1 in parts:
        for c0, cols in ((0, K1), (K1, W.shape[1] - K1)):
            if not cols:
                continue
            TT = (cols + 31) // 32
            frag = blob[at:at + MB * TT * 512].reshape(MB, TT, 2, 64, 4)
            at += MB * TT * 512
            halves = np.stack([frag & 0xffff, frag >> 16], -1).astype(np.uint16).view(np.float16).astype(np.float64)      # [mb][t][limb][lane][j][e]
            full = np.zeros((16 * MB, 32 * TT))
            for lane in range(64):
                k, h = lane & 31, lane >> 5
                for j in range(4):
                    for e in range(2):
                        mm = 16 * np.arange(MB)[:, None] + 8 * h + 2 * j + e
                        full[mm, 32 * np.arange(TT)[None, :] + k] = halves[:, :, 0, lane, j, e] + halves[:, :, 1, lane, j, e]
            want = np.zeros_like(full)
            want[:hidden, :cols] = W[:, c0:c0 + cols].astype(np.float64) * 256
            assert np.all(np.abs(full - want) <= np.abs(want) * 2.0 ** -23 + 2.0 ** -25), case
            assert not full[hidden:].any() and not full[:, cols:].any()
    assert at == blob.size


def test_row_scale_and_scale_invariance_of_the_reference():
    """the row's maximum lands in [2^14, 2^15); a zero row takes e = 0 and gives zeros; a row with an inf gives NaN; multiplying a row by 2^k
    multiplies the result by 2^k bit for bit"""
    rng = np.random.default_rng(3)
    W = rng.standard_normal((40, 70)).astype(np.float32)
    dz = (rng.standard_normal((6, 40)) * np.array([1e-30, 1e-8, 1.0, 77.0, 1e20, 1e30])[:, None]).astype(np.float32)
    dz[:, ::3] = 0
    e, bad = ref.row_scale(dz)
    top = np.abs(dz).max(1).astype(np.float64) * 2.0 ** e
    assert np.all(top >= 2.0 ** 14) and np.all(top < 2.0 ** 15) and not bad.any()
    dx, _ = ref.transposed_layer(W, dz)
    exact = dz.astype(np.float64) @ W.astype(np.float64)
    assert np.all(np.abs(dx - exact) <= 2.0 ** -20 * (np.abs(dz).astype(np.float64) @ np.abs(W).astype(np.float64)))
    k = np.array([40, 13, 0, -40, -7, 2])                      # (no row leaves the normal f32 numbers)
    dx_k, _ = ref.transposed_layer(W, np.ldexp(dz, k[:, None]).astype(np.float32))
    assert np.array_equal(dx_k, np.ldexp(dx, k[:, None]).astype(np.float32))
    zero, _ = ref.transposed_layer(W, np.zeros((2, 40), np.float32))
    assert not zero.any() and not np.signbit(zero).any()
    dz[1, 4] = np.inf
    dz[2, 5] = np.nan
    nan, _ = ref.transposed_layer(W, dz)
    assert np.isnan(nan[1]).all() and np.isnan(nan[2]).all() and np.isfinite(nan[[0, 3, 4, 5]]).all()
    W2 = W.copy()
    W2[7, 9] = 300.0                                        # beyond the range: limbs (inf, -inf) meet a finite or zero dZ
    assert np.isnan(ref.transposed_layer(W2, dz[[0, 3]])[0][:, 9]).all()


def test_reference_backward_against_float64_autograd(pkg):
    """the whole restated backward on a small skip geometry, against torch.autograd in float64 (generic_train_ref): relative L2 below 2e-5
    wherever the limb forward and float64 agree on every gate -- asserted, for this seed"""
    import generic_train_ref as ref64
    kw = dict(dec_channels=33, dec_density_layers=3, dec_rgb_layers=2, skip_connect_every=1, proj_combination="avg", viewdir_proj_combination="mult")
    _, sd, planes, _ = fwd.seeded_state(pkg, 12, **kw)
    opts = {k: v for k, v in kw.items() if k != "dec_channels"}
    rng = np.random.default_rng(4)
    x = np.concatenate([rng.uniform(-4.3, 4.3, (60, 3)), rng.standard_normal((60, 3))], 1).astype(np.float32)
    G = rng.standard_normal((60, 4)).astype(np.float32)
    a, b = ref.gates(sd, planes, G22_BOX, x, fwd.layer, **opts), ref.gates(sd, planes, G22_BOX, x, fwd.layer_f64, **opts)
    assert all(np.array_equal(u, v) for u, v in zip(a, b))
    got = ref.plane_gradients(sd, planes, G22_BOX, x, G, **opts)
    hi = ref.plane_gradients(sd, planes, G22_BOX, x, G, hi_only=True, **opts)
    _, want = ref64.plane_gradients(sd, planes, G22_BOX, x, G, **opts)
    for d in range(4):
        err, err_hi = ref64.rel_l2(got[d], want[d]), ref64.rel_l2(hi[d], want[d])
        print("plane %d: two limbs %.3g, high limbs alone %.3g" % (d, err, err_hi))
        assert err < 2e-5 and err_hi > 2e-5, (d, err, err_hi)          # (a kernel that forgot the low limbs would be caught at this bound)


# ---- the predicate ----------------------------------------------------------------------------------------------------------------------------
SID = "lego_DS8_PlRes10_6"


def _model(pkg, **kw):
    m = pkg.models.TwoDimPlanesModel(use_viewdirs=True, align_corners=True, **kw)
    c = kw.get("num_plane_channels", 48)
    m.planes_ = torch.nn.ParameterDict({pkg.models.get_plane_name(SID, d): torch.nn.Parameter(torch.zeros(1, c, 4, 4)) for d in range(4)})
    m.set_cur_scene_id(SID)
    for p in m.decoder_parameters():
        p.requires_grad_(False)
    return m.train()


def test_predicate_flips_with_exactly_one_condition(pkg, monkeypatch):
    """fails without the feature.  From the one state in which every condition holds -- train_arithmetic 'f16x2' by name, a graph, a frozen
    decoder, the deterministic mode off, the handle at 1, a geometry both limb kernels hold -- each single change answers 'f32'"""
    for h in (HANDLE, "NVSR_GENERIC_FUSED", "NVSR_DETERMINISTIC", "NVSR_DECODER_ARITHMETIC"):
        monkeypatch.delenv(h, raising=False)
    m = _model(pkg, skip_connect_every=3, **G18_VARIANTS["avg_mult"])
    assert m.train_arithmetic is None and m.generic_train_arithmetic() == "f32"
    monkeypatch.setenv(HANDLE, "1")
    assert m.generic_train_arithmetic() == "f32"                          # the handle alone never selects it
    m.train_arithmetic = "f16x2"
    assert m.generic_train_arithmetic() == "f16x2"
    assert m.generic_train_route() == "fused" and m.generic_route() == "layered" and m.generic_arithmetic() == "f32"      # (the others: as ever)
    # train_arithmetic: by name only
    for other in (None, "f32", "bf16x3", "f16", 2, "F16X2"):
        m.train_arithmetic = other
        assert m.generic_train_arithmetic() == "f32", other
    m.train_arithmetic = None
    m.arithmetic = "f16x2"                                                # model.arithmetic, the process default, the environment: never
    assert m.generic_train_arithmetic() == "f32"
    saved = pkg.capi.get_decoder_arithmetic()
    pkg.capi.set_decoder_arithmetic("f16x2")
    monkeypatch.setenv("NVSR_DECODER_ARITHMETIC", "f16x2")
    try:
        assert m.generic_train_arithmetic() == "f32"
    finally:
        pkg.capi.set_decoder_arithmetic(saved)
    monkeypatch.delenv("NVSR_DECODER_ARITHMETIC")
    m.arithmetic = None
    m.train_arithmetic = "f16x2"
    assert m.generic_train_arithmetic() == "f16x2"
    # the handle
    monkeypatch.setenv(HANDLE, "0")
    assert m.generic_train_arithmetic() == "f32"
    monkeypatch.delenv(HANDLE)
    span = m.GENERIC_TRAIN_LIMB_DEFAULT_HIDDEN                            # unset: the measured widths (None: nowhere)
    assert m.generic_train_arithmetic() == ("f16x2" if span is not None and span[0] <= m.dec_channels <= span[1] else "f32")
    monkeypatch.setattr(type(m), "GENERIC_TRAIN_LIMB_DEFAULT_HIDDEN", (m.dec_channels, m.dec_channels))
    assert m.generic_train_arithmetic() == "f16x2"
    monkeypatch.setattr(type(m), "GENERIC_TRAIN_LIMB_DEFAULT_HIDDEN", (m.dec_channels + 1, 4096))       # the width
    assert m.generic_train_arithmetic() == "f32"
    monkeypatch.setattr(type(m), "GENERIC_TRAIN_LIMB_DEFAULT_HIDDEN", None)
    assert m.generic_train_arithmetic() == "f32"
    monkeypatch.setenv(HANDLE, "1")
    assert m.generic_train_arithmetic() == "f16x2"
    # gradients
    with torch.no_grad():
        assert m.generic_train_arithmetic() == "f32"
    for p in m.planes_.values():
        p.requires_grad_(False)
    assert m.generic_train_arithmetic() == "f32"                          # nothing requires a gradient: no graph
    for p in m.planes_.values():
        p.requires_grad_(True)
    assert m.generic_train_arithmetic() == "f16x2"
    # the decoder
    first = next(iter(m.decoder_parameters()))
    first.requires_grad_(True)
    assert m.generic_train_arithmetic() == "f32" and m.generic_train_route() == "layered"       # decoder gradients: exact f32, layered
    first.requires_grad_(False)
    assert m.generic_train_arithmetic() == "f16x2"
    # the deterministic mode
    with pkg.capi.deterministic_scope(True):
        assert m.generic_train_arithmetic() == "f32"
    assert m.generic_train_arithmetic() == "f16x2"
    # the capacity: each of the two entries alone
    lib = pkg.capi.lib()
    real = m._generic_held
    for missing in ("f16x2", "backward_f16x2"):
        monkeypatch.setattr(m, "_generic_held", lambda *kinds, _missing=missing: missing not in kinds and real(*kinds))
        assert m.generic_train_arithmetic() == "f32", missing
    monkeypatch.setattr(m, "_generic_held", real)
    assert m.generic_train_arithmetic() == "f16x2"
    big = _model(pkg, dec_channels=4096, dec_density_layers=1, dec_rgb_layers=1, proj_combination="sum")
    big.train_arithmetic = "f16x2"
    assert big.generic_train_arithmetic() == "f32" and big.generic_train_route() == "layered"
    # forward capacity without the backward's: 512 + 512 + 256 + 4 + 64 floats
    wide = _model(pkg, dec_channels=256, num_plane_channels=512, proj_combination="sum")
    wide.train_arithmetic = "f16x2"
    geo = C.byref(pkg.capi.DecoderGeometry(*[int(v) for v in wide.generic_geometry()]))
    assert lib.nvsr_generic_fused_supported_arith(geo, 3, F16X2) == 1 and lib.nvsr_generic_backward_fused_supported_arith(geo, 3, F16X2) == 0
    assert wide.generic_train_arithmetic() == "f32"
    assert torch.cuda.is_available() or not torch.cuda.is_initialized()


@pytest.mark.parametrize("train_arithmetic", [None, "f16x2"])
def test_the_four_existing_predicates_answer_the_recorded_table(pkg, monkeypatch, train_arithmetic):
    """tests/generic_route_table.json, row by row, with the new attribute at None and at 'f16x2': no existing predicate reads it"""
    monkeypatch.delenv("NVSR_DETERMINISTIC", raising=False)
    spec = importlib.util.spec_from_file_location("generic_route_table", os.path.join(ROOT, "tools", "generic_route_table.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    make = tool._model

    def model(pkg_, torch_, dec_channels):
        m = make(pkg_, torch_, dec_channels)
        assert m.train_arithmetic is None
        m.train_arithmetic = train_arithmetic
        return m

    monkeypatch.setattr(tool, "_model", model)
    with open(os.path.join(ROOT, "tests", "generic_route_table.json")) as fh:
        want = json.load(fh)
    got = tool.table(pkg)
    assert len(got["rows"]) == len(want["rows"])
    wrong = [i for i, (a, b) in enumerate(zip(got["rows"], want["rows"])) if a != b]
    assert not wrong, "%d rows differ; the first: %s" % (len(wrong), tool.describe(wrong[0]))
