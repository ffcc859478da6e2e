"""CPU tests of the generic geometries' frame in two phases: the numpy statements the GPU tests compare against
(tests/generic_two_phase_ref.py), the new entry points in include/nvsr.h and capi.py, the answers that need no device, the routing decision
TwoDimPlanesModel.generic_frame_route() and the operators' fake implementations."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import generic_two_phase_ref as ref
from test_oracle import G18_VARIANTS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("nvsr_generic_decode_fused_density_arith_ext", "nvsr_generic_decode_fused_colour_arith_ext", "nvsr_generic_live_list",
           "nvsr_generic_live_list_workspace_bytes")
OPS = ("triplane_density_generic_fused_arith", "triplane_colour_generic_fused_arith", "generic_live_list")
ERR_SHAPE = 1


@pytest.fixture(scope="module")
def pkg():
    import nvsr_amd

    nvsr_amd.build_extension()
    return nvsr_amd


def test_reference_live_list_and_assembly_are_self_consistent():
    sub = np.float32(1e-42)
    assert sub != 0 and sub < np.finfo(np.float32).tiny
    w = np.array([0.0, -0.0, np.nan, sub, 2.5, 0.0, -sub, np.inf, -0.0], np.float32)
    idx = ref.live_list(w)
    assert idx.dtype == np.int32 and idx.tolist() == [2, 3, 4, 6, 7]
    assert ref.live_list(w.reshape(3, 3)).tolist() == idx.tolist()                     # flat positions of any shape
    assert ref.live_list(np.zeros(0, np.float32)).size == 0 and ref.live_share(w) == 5 / 9
    rng = np.random.default_rng(0)
    one = rng.standard_normal((9, 4)).astype(np.float32)
    d = ref.density_raw(one)
    assert np.array_equal(d[:, 3], one[:, 3]) and not d[:, :3].any() and not np.signbit(d[:, :3]).any()      # +0.0, not -0.0
    two = ref.two_phase_raw(one, w)
    assert np.array_equal(two[idx], one[idx]) and np.array_equal(two[:, 3], one[:, 3])
    dead = np.setdiff1d(np.arange(9), idx)
    assert not two[dead, :3].any()
    # a colour phase on a part of the list, in any order, moves those rows' colours and nothing else
    before = np.full((9, 4), -7.25, np.float32)
    part = ref.colour_raw(before, one, [7, 2])
    assert np.array_equal(part[[2, 7], :3], one[[2, 7], :3]) and (part[:, 3] == -7.25).all() and (np.delete(part, [2, 7], 0) == -7.25).all()
    assert np.array_equal(ref.colour_raw(ref.colour_raw(d, one, idx[:2]), one, idx[2:]), two)
    # what a compositor makes of a dead sample: weight 0 times any finite colour is the +0 it adds for logits of +0
    colour = 1 / (1 + np.exp(-one[:, :3].astype(np.float64)))
    assert np.array_equal((np.where(w == 0, 0.0, 1.0)[:, None] * colour)[dead], np.zeros((dead.size, 3)))


def test_bias_shift_gives_the_wanted_share():
    sigma = np.random.default_rng(1).standard_normal(1000) * 3 + 2
    for share in (0.1, 1 / 3, 0.5):
        s = ref.bias_shift_for_share(sigma, share)
        assert abs((sigma + s > 0).mean() - share) <= 1e-3


def test_symbols_are_declared_in_the_header_and_bound(pkg):
    header = open(os.path.join(ROOT, "include", "nvsr.h")).read()
    for name in SYMBOLS:
        assert re.search(r"^(int|int64_t) %s\(" % name, header, re.M), name
        assert name in pkg.capi.exported_symbols(), name
        fn = getattr(pkg.capi.lib(), name)
        assert fn.argtypes is not None and fn.restype is not None, name
    # the header says what the capacity answer covers
    assert "answers for both phases" in header
    for op in OPS:
        assert op in pkg.ops.FORWARD_OPS and hasattr(torch.ops.nvsr, op), op


def test_entries_that_answer_without_a_device(pkg):
    lib = pkg.capi.lib()
    assert lib.nvsr_generic_live_list_workspace_bytes(0) == 4
    assert lib.nvsr_generic_live_list_workspace_bytes(1) == 4
    assert lib.nvsr_generic_live_list_workspace_bytes(2048) == 4 and lib.nvsr_generic_live_list_workspace_bytes(2049) == 8
    assert lib.nvsr_generic_live_list_workspace_bytes(70000) == 4 * 35
    assert 0 < lib.nvsr_generic_live_list_workspace_bytes(2 ** 31 - 1) <= 4 * 4096             # the span grows, the counts do not
    assert lib.nvsr_generic_live_list_workspace_bytes(-1) == -ERR_SHAPE and lib.nvsr_generic_live_list_workspace_bytes(2 ** 31) == -ERR_SHAPE
    assert lib.nvsr_generic_live_list(2 ** 31, None, None, None, None, None) == ERR_SHAPE     # refused before anything is touched
    # arithmetics and geometries are refused before a scene is read: no device needed
    geo = pkg.capi.DecoderGeometry(48, 48, 4096, 1, 1, 0, 0, 0)
    sc = pkg.capi.SceneExt()
    sc.num_position_planes = 3
    one = C.c_void_p(16)
    for arith in (1, 3, -1, 7):
        ok = pkg.capi.DecoderGeometry(48, 48, 64, 4, 4, 0, 1, 4)
        assert lib.nvsr_generic_decode_fused_density_arith_ext(C.byref(sc), C.byref(ok), one, one, 8, one, None, one, arith, None) == ERR_SHAPE
        assert lib.nvsr_generic_decode_fused_colour_arith_ext(C.byref(sc), C.byref(ok), one, one, 8, one, None, one, one, 8, one, arith, None) == ERR_SHAPE
    for arith in (0, 2):
        assert lib.nvsr_generic_fused_supported_arith(C.byref(geo), 3, arith) == 0
        assert lib.nvsr_generic_decode_fused_density_arith_ext(C.byref(sc), C.byref(geo), one, one, 8, one, None, one, arith, None) == ERR_SHAPE
        assert lib.nvsr_generic_decode_fused_colour_arith_ext(C.byref(sc), C.byref(geo), one, one, 8, one, None, one, one, 8, one, arith, None) == ERR_SHAPE


def test_generic_frame_route_follows_the_switch_the_route_and_the_gradient_mode(pkg, monkeypatch):
    monkeypatch.delenv("NVSR_GENERIC_FUSED", raising=False)
    monkeypatch.delenv("NVSR_GENERIC_TWO_PHASE", raising=False)
    m = pkg.models.TwoDimPlanesModel(use_viewdirs=True, align_corners=True, skip_connect_every=3, **G18_VARIANTS["avg_mult"])
    table = m.GENERIC_TWO_PHASE_DEFAULT_HIDDEN
    assert set(table) == {"f32", "f16x2"} and table["f16x2"] is None

    def default(model, arith):
        span = table[arith]
        return "two_phase" if span is not None and span[0] <= model.dec_channels <= span[1] else "one_phase"

    with torch.no_grad():
        assert m.generic_route() == "fused" and m.generic_frame_route() == default(m, "f32")
        monkeypatch.setenv("NVSR_GENERIC_TWO_PHASE", "1")
        assert m.generic_frame_route() == "two_phase"
        m.arithmetic = "f16x2"
        assert m.generic_arithmetic() == "f16x2" and m.generic_frame_route() == "two_phase"
        monkeypatch.delenv("NVSR_GENERIC_TWO_PHASE")
        assert m.generic_frame_route() == "one_phase"                                   # 'f16x2': on request only
        m.arithmetic = None
        monkeypatch.setenv("NVSR_GENERIC_TWO_PHASE", "0")
        assert m.generic_frame_route() == "one_phase"                                   # read at every call
        monkeypatch.setenv("NVSR_GENERIC_TWO_PHASE", "1")
        monkeypatch.setenv("NVSR_GENERIC_FUSED", "0")
        assert m.generic_route() == "layered" and m.generic_frame_route() == "one_phase"       # the layered route has no phases
        monkeypatch.delenv("NVSR_GENERIC_FUSED")
        assert m.generic_route() == "fused"                                             # generic_route keeps its two values
    assert m.generic_route() == "layered" and m.generic_frame_route() == "one_phase"   # gradients on, parameters that take them
    with torch.no_grad():
        wide = pkg.models.TwoDimPlanesModel(use_viewdirs=True, align_corners=True, skip_connect_every=3, **G18_VARIANTS["wide256"])
        assert wide.generic_frame_route() == "one_phase"                                # 256 wide: 'layered' unless NVSR_GENERIC_FUSED=1
        monkeypatch.setenv("NVSR_GENERIC_FUSED", "1")
        assert wide.generic_frame_route() == "two_phase"
        big = pkg.models.TwoDimPlanesModel(use_viewdirs=True, align_corners=True, dec_channels=4096, dec_density_layers=1, dec_rgb_layers=1,
                                           proj_combination="sum")
        assert big.generic_frame_route() == "one_phase"                                 # beyond the capacity: no switch changes that
        shipped = pkg.models.TwoDimPlanesModel(use_viewdirs=True, align_corners=True, proj_combination="avg", viewdir_proj_combination="concat_pos")
        assert shipped.is_native_geometry() and shipped.generic_frame_route() == "one_phase"
    assert torch.cuda.is_available() or not torch.cuda.is_initialized()


def test_fake_implementations_give_the_shapes(pkg):
    nv = torch.ops.nvsr
    meta = lambda *s, dtype=torch.float32: torch.empty(s, dtype=dtype, device="meta")
    planes = [meta(10, 10, 48) for _ in range(4)]
    consts = [0.0] * 28
    geometry = [48, 48, 64, 4, 4, 0, 1, 4]
    x = meta(77, 6)
    raw = nv.triplane_density_generic_fused_arith(planes, consts, meta(100), meta(0), geometry, x, True, None, False, 0)
    assert tuple(raw.shape) == (77, 4) and raw.dtype == torch.float32
    index, count = nv.generic_live_list(meta(7, 11))
    assert tuple(index.shape) == (77,) and index.dtype == torch.int32 and tuple(count.shape) == (1,) and count.dtype == torch.int32
    assert nv.triplane_colour_generic_fused_arith(raw, planes, consts, meta(100), meta(0), geometry, x, index, count, True, None, False, 0) is None
    schema = str(nv.triplane_colour_generic_fused_arith.default._schema)
    assert "Tensor(a0!) raw" in schema or "Tensor(a!) raw" in schema, schema        # declared as written in place
