"""CPU tests of the deterministic route's host side: the new C entries exist with their signatures and answer NULL pointers
and bad shapes with the library's error codes before anything is launched, the workspace queries are monotone, capi.deterministic resolves
in its documented order, and the numpy float32 restatement of nvsr_rows_scatter's contract agrees with a float64 sum."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from deterministic_ref import rows_scatter_f64, rows_scatter_ref, scatter_case

OK, ERR_SHAPE, ERR_LAUNCH, ERR_NULL, ERR_ALIGN = 0, 1, 2, 3, 4
NEW = {   # name -> number of C arguments
    "nvsr_render_pass_backward_rows_arith": 14, "nvsr_view_rows_reduce": 5, "nvsr_internal_plane_taps": 9, "nvsr_rows_scatter_workspace_bytes": 1,
    "nvsr_rows_scatter": 10, "nvsr_decoder_weight_grad_det_workspace_floats": 2, "nvsr_decoder_weight_grad_det_arith": 7,
}


@pytest.fixture(scope="module")
def pkg():
    import nvsr_amd

    nvsr_amd.build_extension()
    return nvsr_amd


def test_new_entries_exist_with_their_signatures(pkg):
    lib = pkg.capi.lib()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nvsr.h")).read(), flags=re.S)
    for name, nargs in NEW.items():
        assert hasattr(lib, name), name
        args, res = pkg.capi._PROTOS_OPTIONAL[name]
        assert len(args) == nargs, name
        assert res is (C.c_int64 if "workspace" in name else C.c_int), name
        m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, header)
        assert m and len(m.group(1).split(",")) == nargs, name          # the header declares the same number of parameters
    for op in ("rows_scatter", "decode_rays_backward_det", "decode_rays_backward_det_", "decoder_weight_grad_det"):
        assert hasattr(torch.ops.nvsr, op), op
    import inspect
    assert "deterministic" in inspect.signature(pkg.training.TrainStep.__init__).parameters
    # the existing operators keep their signatures (tests call them positionally)
    assert list(inspect.signature(pkg.ops.decode_rays_backward._init_fn).parameters) == [
        "planes", "consts", "packed", "packed_bwd", "rays", "z", "g_raw", "gates", "record", "need", "arithmetic"]
    assert list(inspect.signature(pkg.ops.decoder_weight_grad._init_fn).parameters) == ["record", "N", "S", "arithmetic"]


def test_bad_arguments_are_answered_before_any_launch(pkg):
    """no GPU here: a call that reached a launch would come back as NVSR_ERR_LAUNCH; every answer below is another code"""
    lib = pkg.capi.lib()
    p, odd = C.c_void_p(0x10000), C.c_void_p(0x10004)         # never dereferenced: the checks return first
    # nvsr_rows_scatter(M, rows, texel, weight, H, W, g, workspace, workspace_bytes, stream)
    big = 1 << 40
    assert lib.nvsr_rows_scatter(4, None, p, p, 5, 7, p, p, big, None) == ERR_NULL
    assert lib.nvsr_rows_scatter(4, p, p, p, 5, 7, None, p, big, None) == ERR_NULL
    assert lib.nvsr_rows_scatter(4, p, p, p, 5, 7, p, None, big, None) == ERR_NULL
    assert lib.nvsr_rows_scatter(4, odd, p, p, 5, 7, p, p, big, None) == ERR_ALIGN
    assert lib.nvsr_rows_scatter(4, p, p, p, 5, 7, p, odd, big, None) == ERR_ALIGN
    assert lib.nvsr_rows_scatter(-1, p, p, p, 5, 7, p, p, big, None) == ERR_SHAPE
    assert lib.nvsr_rows_scatter(1 << 29, p, p, p, 5, 7, p, p, big, None) == ERR_SHAPE              # 4 M would not fit 31 bits
    assert lib.nvsr_rows_scatter(4, p, p, p, 0, 7, p, p, big, None) == ERR_SHAPE
    assert lib.nvsr_rows_scatter(4, p, p, p, 8192, 8192, p, p, big, None) == ERR_SHAPE              # H * W * 48 >= 2^31
    assert lib.nvsr_rows_scatter(4, p, p, p, 5, 7, p, p, lib.nvsr_rows_scatter_workspace_bytes(4) - 1, None) == ERR_SHAPE
    assert lib.nvsr_rows_scatter(0, p, p, p, 5, 7, p, p, big, None) == OK                            # nothing to do, nothing launched
    # nvsr_internal_plane_taps(scene, d, N, S, rays, z, texel, weight, stream)
    sc = pkg.capi.Scene()
    for d in range(4):
        sc.planes[d], sc.ph[d], sc.pw[d] = 0x10000, 4, 4
    assert lib.nvsr_internal_plane_taps(None, 0, 4, 4, p, p, p, p, None) == ERR_NULL
    assert lib.nvsr_internal_plane_taps(C.byref(sc), 0, 4, 4, p, None, p, p, None) == ERR_NULL     # a position plane needs the depths
    assert lib.nvsr_internal_plane_taps(C.byref(sc), 4, 4, 4, p, p, p, p, None) == ERR_SHAPE
    assert lib.nvsr_internal_plane_taps(C.byref(sc), -1, 4, 4, p, p, p, p, None) == ERR_SHAPE
    assert lib.nvsr_internal_plane_taps(C.byref(sc), 1, 4, 0, p, p, p, p, None) == ERR_SHAPE
    assert lib.nvsr_internal_plane_taps(C.byref(sc), 1, 4, 4, p, p, odd, p, None) == ERR_ALIGN
    assert lib.nvsr_internal_plane_taps(C.byref(sc), 3, 0, 4, p, None, p, p, None) == OK
    # nvsr_render_pass_backward_rows_arith(scene, packed, packed_bwd, N, S, rays, z, g_raw, gates, rows, view_ws, record, arithmetic, stream)
    rows = (C.c_void_p * 3)(0x10000, None, 0x10000)
    bf16x3, f32 = pkg.capi.ARITHMETIC["bf16x3"], pkg.capi.ARITHMETIC["f32"]
    f = lib.nvsr_render_pass_backward_rows_arith
    assert f(None, p, p, 4, 4, p, p, p, p, rows, p, None, bf16x3, None) == ERR_NULL
    assert f(C.byref(sc), p, p, 4, 4, p, p, p, None, rows, p, None, bf16x3, None) == ERR_NULL       # no gates
    assert f(C.byref(sc), p, p, 4, 4, p, p, p, p, None, None, None, bf16x3, None) == ERR_NULL       # nothing to produce
    assert f(C.byref(sc), p, p, 4, 4, p, p, p, p, rows, p, None, f32, None) == ERR_SHAPE            # the limb arithmetics only
    assert f(C.byref(sc), p, p, 4, 4, p, p, p, p, rows, p, None, 7, None) == ERR_SHAPE
    assert f(C.byref(sc), p, p, 4, 0, p, p, p, p, rows, p, None, bf16x3, None) == ERR_SHAPE
    assert f(C.byref(sc), p, p, 4, 4, p, p, p, p, (C.c_void_p * 3)(0x10004, None, None), p, None, bf16x3, None) == ERR_ALIGN
    assert f(C.byref(sc), p, p, 0, 4, p, p, p, p, rows, p, None, bf16x3, None) == OK
    # nvsr_view_rows_reduce(N, S, view_ws, view_rows, stream)
    assert lib.nvsr_view_rows_reduce(4, 4, None, p, None) == ERR_NULL and lib.nvsr_view_rows_reduce(4, 4, p, None, None) == ERR_NULL
    assert lib.nvsr_view_rows_reduce(4, 0, p, p, None) == ERR_SHAPE and lib.nvsr_view_rows_reduce(0, 4, p, p, None) == OK
    # nvsr_decoder_weight_grad_det_arith(N, S, record, grad_natural, workspace, arithmetic, stream)
    f = lib.nvsr_decoder_weight_grad_det_arith
    assert f(4, 4, None, p, p, bf16x3, None) == ERR_NULL and f(4, 4, p, None, p, bf16x3, None) == ERR_NULL
    assert f(4, 4, p, p, None, bf16x3, None) == ERR_NULL
    assert f(4, 4, odd, p, p, bf16x3, None) == ERR_ALIGN and f(4, 4, p, p, odd, bf16x3, None) == ERR_ALIGN
    assert f(4, 4, p, p, p, f32, None) == ERR_SHAPE and f(4, 0, p, p, p, bf16x3, None) == ERR_SHAPE and f(-1, 4, p, p, p, bf16x3, None) == ERR_SHAPE
    assert f(0, 4, p, p, p, bf16x3, None) == OK


def test_workspace_queries_are_monotone(pkg):
    lib = pkg.capi.lib()
    sizes = [lib.nvsr_rows_scatter_workspace_bytes(M) for M in (0, 1, 2, 257, 4099, 4100, 1 << 16, 1 << 20, (1 << 29) - 1)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[1] > 0 and sizes[-1] > 16 * ((1 << 29) - 1)
    assert lib.nvsr_rows_scatter_workspace_bytes(-1) == 0 and lib.nvsr_rows_scatter_workspace_bytes(1 << 29) == 0
    q = lib.nvsr_decoder_weight_grad_det_workspace_floats
    prev = 0
    for P in (1, 2, 255, 256, 257, 4290, 7168, 7169, 65536, 262144, 262145, 786432, 1 << 21):
        cur = q(P, 1)
        assert cur >= prev and cur >= pkg.capi.DECODER_NATURAL_FLOATS, P
        assert cur == q(1, P) if P <= 4096 else True                  # a function of N * S alone
        prev = cur
    assert q(130, 33) == q(33, 130) == q(4290, 1)
    assert q(130, 33) > 16 * pkg.capi.DECODER_NATURAL_FLOATS          # 17 slabs of 256 rows at the GPU test's size
    assert q(0, 4) == 0 and q(-1, 4) == 0 and q(4, 0) == 0


def test_mode_resolves_argument_then_environment_then_torch(pkg, monkeypatch):
    det = pkg.capi.deterministic
    monkeypatch.delenv("NVSR_DETERMINISTIC", raising=False)
    assert not torch.are_deterministic_algorithms_enabled()           # nothing in the repository sets torch's switch
    assert det() is False and det(True) is True and det(False) is False
    try:
        torch.use_deterministic_algorithms(True)
        assert det() is True and det(False) is False                  # 3. torch's switch, under 1. the argument
        monkeypatch.setenv("NVSR_DETERMINISTIC", "0")
        assert det() is True                                          # only "1" switches the mode on; anything else leaves it to torch
    finally:
        torch.use_deterministic_algorithms(False)
    assert det() is False
    monkeypatch.setenv("NVSR_DETERMINISTIC", "1")                     # 2. the environment, read at every call
    assert det() is True and det(False) is False
    with pkg.capi.deterministic_scope(False):                         # what TrainStep(deterministic=False) hands down: an explicit argument
        assert det() is False and det(True) is True
    monkeypatch.delenv("NVSR_DETERMINISTIC")
    assert det() is False
    with pkg.capi.deterministic_scope(True):
        assert det() is True
        with pkg.capi.deterministic_scope(None):                      # TrainStep(deterministic=None): no opinion
            assert det() is False
    step = pkg.training.TrainStep(None, None, None, {"LR_planes"}, deterministic=True)
    assert step.deterministic is True
    assert pkg.training.TrainStep(None, None, None, {"LR_planes"}).deterministic is False
    monkeypatch.setenv("NVSR_DETERMINISTIC", "1")
    assert pkg.training.TrainStep(None, None, None, {"LR_planes"}).deterministic is True
    assert pkg.training.TrainStep(None, None, None, {"LR_planes"}, deterministic=False).deterministic is False


def test_host_side_refusals_name_the_mode(pkg, monkeypatch):
    monkeypatch.delenv("NVSR_DETERMINISTIC", raising=False)
    T = pkg.training
    with pytest.raises(RuntimeError, match="deterministic mode"):
        T.TrainStep(None, None, None, {"SR", "LR_planes"}, deterministic=True)
    T.TrainStep(None, None, None, {"SR", "LR_planes"})                # not in the mode: as before
    step = T.TrainStep(None, None, None, {"LR_planes"}, deterministic=True, pixel_sampler=T.DevicePixelSampler(seed=1))
    with pytest.raises(RuntimeError, match="deterministic mode"):
        T.GraphedTrainStep(step, torch.zeros(4, 4, 3), torch.eye(4), 4, 4, 1.0, 1, "s", None, 8)


def test_the_host_decisions_of_a_training_pass_over_the_product_of_their_inputs():
    """train_utils._pass_facts + _refuse_untrainable + ops.gate_route -- the one place that decides, per pass of a training render, what the
    forward publishes, which backward follows and what is refused -- over (N, S, decoder gradient, rays need a gradient, deterministic,
    arithmetic, RECORD_FORWARD_MAX_POINTS) with N S = limit - 1, limit, limit + 1, against the rules as the route had them scattered before:
      forward (`flags`):   record = decoder gradient and N S <= limit;  gates = record or no decoder gradient
      backward:            gate-driven where gates were published -- ordered with points when the rays need a gradient, else ordered in
                           deterministic mode, else atomic -- and recomputing where not
      refusals, in order:  rays that need a gradient with a recomputing pass (NotImplementedError); deterministic mode in 'f32';
                           deterministic mode with a recomputing pass.
    (Rays never need a gradient in 'f32': predict_and_render_radiance warns and drops the request before it decides anything.)
    No GPU, no library call."""
    import itertools
    import nvsr_amd
    tu, ops, capi = nvsr_amd.train_utils, nvsr_amd.ops, nvsr_amd.capi
    f32 = capi.ARITHMETIC["f32"]
    seen = set()
    for (N, S), off, dec, rays, det, arith in itertools.product([(1, 5), (3, 4), (7, 1)], (1, 0, -1), (False, True), (False, True), (False, True),
                                                                [capi.ARITHMETIC[a] for a in ("f32", "bf16x3", "f16x2")]):
        if rays and arith == f32:
            continue
        limit = N * S + off
        too_large = dec and N * S > limit
        if rays and too_large:
            want = (NotImplementedError, "at most %d rays" % (limit // S))
        elif det and arith == f32:
            want = (capi.DeterministicModeError, "a training step in the 'f32' arithmetic")
        elif det and too_large:
            want = (capi.DeterministicModeError, "a pass of more than RECORD_FORWARD_MAX_POINTS points with decoder gradients")
        else:
            record = dec and N * S <= limit
            gates = record or not dec
            want = (gates, record, "recompute" if not gates else "ordered with points" if rays else "ordered" if det else "atomic")
        p = tu._pass_facts(N, S, arith, None, dec, limit)
        try:
            tu._refuse_untrainable((), N, [p], rays, det, limit)
            gates = p.records or not p.dec_grad            # (as _RenderRaysFn.forward asks decode_rays for them)
            got = (gates, p.records, ops.gate_route(det, rays) if gates else "recompute")
        except (NotImplementedError, RuntimeError) as e:
            got = (type(e), want[1] if isinstance(want[1], str) and want[1] in str(e) else str(e))
        assert got == want, ((N, S, limit, dec, rays, det, arith), got, want)
        seen.add(want if isinstance(want[0], bool) else want[0])
    routes = ("atomic", "ordered", "ordered with points")          # every outcome occurred: both refusal types, recompute, each route with / without a record
    assert seen == {NotImplementedError, capi.DeterministicModeError, (False, False, "recompute")} | {(True, r, k) for r in (False, True) for k in routes}


@pytest.mark.parametrize("kind,M,H,W", [("random", 257, 5, 7), ("random", 4099, 16, 16), ("one_texel", 513, 5, 7), ("zero_weights", 257, 16, 16)])
def test_float32_reference_against_a_float64_sum(kind, M, H, W):
    """the reference the GPU test demands bit equality with is itself right: every element within n * 2^-24 * sum |terms| of the float64
    sum (n additions + n products + the final add, each rounded once: (2 n + 1) half-ulps of a partial sum bounded by sum |terms|), and a
    texel no entry names keeps its bits"""
    rows, texel, weight, g = scatter_case(M, H, W, 3, kind)
    got = rows_scatter_ref(rows, texel, weight, g)
    want, mag, count = rows_scatter_f64(rows, texel, weight, g)
    bound = (2 * count[..., None] + 1) * 2.0 ** -24 * mag
    assert (np.abs(got.astype(np.float64) - want) <= bound).all()
    untouched = count == 0
    assert (got[untouched].view(np.uint32) == g[untouched].view(np.uint32)).all()


def test_float32_reference_sends_a_nan_row_to_its_four_texels_only():
    rows, texel, weight, g = scatter_case(257, 16, 16, 5, "nan_row")
    got = rows_scatter_ref(rows, texel, weight, g).reshape(-1, 48)
    hit = np.zeros(256, bool)
    hit[texel[257 // 2]] = True
    assert np.isnan(got[hit]).all() and np.isfinite(got[~hit]).all()
