"""CPU tests of training the generic decoder geometries WITH decoder gradients on the fused launches (csrc/generic_fused_bwd.hip,
nvsr_generic_decode_backward_fused_record_ext, TwoDimPlanesModel.generic_decoder_train_route()): the predicate over the product of what it
reads against tests/generic_decoder_train_route_table.json, the five older predicates under the new handle, the workspace function and the
status codes of the entry in front of a launch.  None touches a GPU."""
import ctypes as C
import importlib.util
import json
import os

import pytest
import torch

from test_generic_entry_status_host import (ERR_NULL, ERR_SHAPE, GEO_288, GEO_FWD_ONLY, GEO_INCONSISTENT, GEO_OK, OK, ONE, _scene,
                                            call as entry_call)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HANDLE = "NVSR_GENERIC_TRAIN_DECODER_FUSED"


@pytest.fixture(scope="module")
def pkg():
    import nvsr_amd

    nvsr_amd.build_extension()
    return nvsr_amd


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_every_row_of_the_predicates_table(pkg, monkeypatch):
    """handle unset / 0 / 1 x dec_channels 64 / 128 / 4096 (beyond the capacity) x the default span / a span that holds 128 alone x gradients
    enabled x decoder frozen x planes requiring gradients x the deterministic mode"""
    monkeypatch.delenv("NVSR_DETERMINISTIC", raising=False)
    tool = _tool("generic_decoder_train_route_table")
    with open(os.path.join(ROOT, "tests", "generic_decoder_train_route_table.json")) as fh:
        want = json.load(fh)
    got = tool.table(pkg)
    assert json.loads(json.dumps(got["axes"])) == want["axes"], "the axes of the tool and of the recorded table differ"
    assert len(got["rows"]) == len(want["rows"]) == 3 * 3 * 2 * 2 ** 4
    wrong = [i for i, (a, b) in enumerate(zip(got["rows"], want["rows"])) if a != b]
    assert not wrong, "%d rows differ; the first: %s: this tree %s, recorded %s" % (
        len(wrong), tool.describe(wrong[0]), got["rows"][wrong[0]], want["rows"][wrong[0]])
    assert set(want["rows"]) == {"F", "L"}
    assert torch.cuda.is_available() or not torch.cuda.is_initialized()


def test_the_recorded_table_follows_the_stated_rule():
    """the table is no mere recording: every row is what the rule of the predicate's docstring gives -- 'fused' exactly when gradients are
    enabled, a decoder parameter requires one (which also records a graph), the mode is off, the geometry is held (dec_channels <= 256 here) and
    the handle is 1, or unset with dec_channels inside the span (the default span is None: nowhere)"""
    import itertools

    with open(os.path.join(ROOT, "tests", "generic_decoder_train_route_table.json")) as fh:
        t = json.load(fh)
    names = [a[0] for a in t["axes"]]
    assert names == [HANDLE, "dec_channels", "span", "grad_enabled", "decoder_frozen", "planes_require_grad", "deterministic"]
    for row, (handle, dec, span, grad, frozen, _planes, det) in zip(t["rows"], itertools.product(*[a[1] for a in t["axes"]])):
        inside = span != "default" and span[0] <= dec <= span[1]
        fused = grad and not frozen and not det and dec <= 256 and handle != "0" and (handle == "1" or inside)
        assert row == ("F" if fused else "L"), (handle, dec, span, grad, frozen, det)


def test_the_default_constant_is_none_or_a_span(pkg):
    span = pkg.models.TwoDimPlanesModel.GENERIC_TRAIN_DECODER_FUSED_DEFAULT_HIDDEN
    assert span is None or (len(span) == 2 and span[0] <= span[1])


@pytest.mark.parametrize("value", [None, "0", "1"])
def test_older_predicates_do_not_read_the_new_handle(pkg, value, monkeypatch):
    """generic_route, generic_train_route, generic_arithmetic, generic_frame_route and train_utils._generic_occupancy answer the recorded table
    of tools/generic_route_table.py with NVSR_GENERIC_TRAIN_DECODER_FUSED unset, 0 and 1; generic_train_arithmetic, which that table does not
    hold, answers the same over its own inputs under every value of the handle"""
    monkeypatch.delenv("NVSR_DETERMINISTIC", raising=False)
    monkeypatch.delenv(HANDLE, raising=False) if value is None else monkeypatch.setenv(HANDLE, value)
    tool = _tool("generic_route_table")
    with open(os.path.join(ROOT, "tests", "generic_route_table.json")) as fh:
        want = json.load(fh)
    got = tool.table(pkg)
    assert got["rows"] == want["rows"]
    m = tool._model(pkg, torch, 64)
    answers = []
    for handle in (None, "0", "1"):
        monkeypatch.delenv(HANDLE, raising=False) if handle is None else monkeypatch.setenv(HANDLE, handle)
        row = []
        for train_handle in (None, "0", "1"):
            monkeypatch.delenv("NVSR_GENERIC_TRAIN_FUSED", raising=False) if train_handle is None else monkeypatch.setenv("NVSR_GENERIC_TRAIN_FUSED", train_handle)
            for name in (None, "f16x2"):
                for frozen in (False, True):
                    for grad in (False, True):
                        for det in (False, True):
                            m.train_arithmetic = name
                            for p in m.decoder_parameters():
                                p.requires_grad_(not frozen)
                            with torch.set_grad_enabled(grad), pkg.capi.deterministic_scope(det):
                                row.append(m.generic_train_arithmetic())
        answers.append(row)
    assert answers[0] == answers[1] == answers[2] and set(answers[0]) == {"f32", "f16x2"}


def test_float64_helper_against_the_references_autograd():
    """tests/generic_train_decoder_ref.py against g19 -- the reference's own float32 autograd -- on the five geometries that carry a
    cotangent: the relative L2 distance of d_natural (the decoder's gradients in natural_blob order) and of the four plane gradients.
    Measured here: d_natural 1.3e-7 .. 3.9e-7, planes 3.7e-7 .. 4.9e-7 (the float32 rounding of the reference; the helper is float64);
    asserted at test_generic_train_fused_host's bound for the planes' helper, 1e-6."""
    import sys

    import numpy as np

    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import generic_train_decoder_ref as ref64
    from conftest import load_golden
    from test_oracle import G18_VARIANTS, g18_variant

    g, gg = load_golden("g18_decoder_variants.npz"), load_golden("g19_decoder_variant_grads.npz")
    names = [n for n in G18_VARIANTS if n + ".gout" in gg]
    assert len(names) == 5
    for name in names:
        kw, sd, planes = g18_variant(g, name)
        out, gnat, grads = ref64.gradients(sd, planes, g["box"], g[name + ".x"], gg[name + ".gout"], **kw)
        np.testing.assert_allclose(out, g[name + ".out"], rtol=0, atol=2e-5 * max(1.0, float(np.abs(g[name + ".out"]).max())), err_msg=name)
        assert gnat.shape == gg[name + ".gnat"].shape
        errs = [ref64.rel_l2(gg[name + ".gnat"], gnat)] + [ref64.rel_l2(gg[name + ".gplane%d" % d], grads[d]) for d in range(4)]
        print(name, ["%.3g" % e for e in errs])
        assert max(errs) < 1e-6, (name, errs)


def _record_floats(pkg, geo, n_pos, P):
    return pkg.capi.lib().nvsr_generic_backward_fused_record_workspace_floats_ext(C.byref(pkg.capi.DecoderGeometry(*geo)), n_pos, P)


def test_workspace_function(pkg):
    """(Kd + Kr + 2 (nd + nr) hidden) x min(P, chunk) floats of record + the 16 floats of alignment room include/nvsr.h documents; monotone in P"""
    chunk = pkg.capi.generic_backward_chunk()
    assert chunk == pkg.capi.lib().nvsr_generic_backward_chunk() and chunk > 0 and chunk % 2048 == 0          # whole slabs of the contraction
    # geometry = [C, Cv, hidden, nd, nr, skip, proj, view]: (Kd, Kr) by include/nvsr.h's rules
    cases = [(GEO_OK, 3, 48, 3 * 48 + 48), ([48, 48, 33, 5, 3, 1, 1, 4], 3, 48, 192), ([24, 24, 96, 4, 4, 0, 2, 3], 3, 72, 96),
             ([48, 48, 31, 5, 3, 2, 0, 0], 3, 48, 48), ([48, 48, 256, 4, 4, 3, 2, 3], 4, 192, 240)]
    for geo, n_pos, Kd, Kr in cases:
        per_point = Kd + Kr + 2 * (geo[3] + geo[4]) * geo[2]
        last = -1
        for P in (0, 1, 31, 32, 33, 2049, chunk - 1, chunk, chunk + 33, 1 << 22):
            got = _record_floats(pkg, geo, n_pos, P)
            assert got == per_point * min(P, chunk) + 16, (geo, P, got)
            assert got >= last
            last = got
    assert _record_floats(pkg, GEO_OK, 3, -1) == -1 and _record_floats(pkg, GEO_INCONSISTENT, 3, 8) == -1 and _record_floats(pkg, GEO_OK, 0, 8) == -1
    assert pkg.capi.lib().nvsr_generic_backward_fused_record_workspace_floats_ext(None, 3, 8) == -1


def record_call(capi, scene="ok", geo=GEO_OK, natural=ONE, P=8, x=ONE, d_out=ONE, d_natural=ONE, d_planes="all", workspace=ONE):
    """one call of the recording entry with everything valid except what the keywords change (test_generic_entry_status_host.call's scheme)"""
    sc = _scene(capi) if isinstance(scene, str) else scene
    g = None if geo is None else capi.DecoderGeometry(*geo)
    n = min(sc.num_position_planes if sc is not None else 3, capi.MAX_POSITION_PLANES) + 1
    arr = None if d_planes is None else (C.c_void_p * 16)(*([ONE] * n if d_planes == "all" else [None] * n))
    return capi.lib().nvsr_generic_decode_backward_fused_record_ext(None if sc is None else C.byref(sc), None if g is None else C.byref(g), natural, P, x,
                                                                    None, d_out, d_natural, arr, workspace, None)


def test_entry_status_codes_in_front_of_a_launch(pkg):
    """No case reaches a launch and nothing dereferences the dummy pointers.  The order is gf_check_entry's: scene, geometry, capacity, the
    caller's pointers (the workspace among them once d_natural is set), the scene's planes, P < 0, then P == 0 / nothing wanted."""
    capi = pkg.capi
    assert record_call(capi, scene=None) == ERR_NULL
    assert record_call(capi, scene=_scene(capi, 0)) == ERR_SHAPE and record_call(capi, scene=_scene(capi, 16)) == ERR_SHAPE
    assert record_call(capi, geo=None) == ERR_NULL and record_call(capi, geo=GEO_INCONSISTENT) == ERR_SHAPE
    assert record_call(capi, geo=GEO_288) == ERR_SHAPE and record_call(capi, geo=GEO_288, natural=None) == ERR_SHAPE        # the capacity is asked first
    assert record_call(capi, geo=GEO_FWD_ONLY) == ERR_SHAPE and record_call(capi, geo=GEO_FWD_ONLY, P=0) == ERR_SHAPE       # the existing backward plan
    for missing in ("natural", "x", "d_out", "workspace"):
        assert record_call(capi, **{missing: None}) == ERR_NULL, missing
        assert record_call(capi, P=-1, **{missing: None}) == ERR_NULL, missing                     # pointers before P
        assert record_call(capi, P=0, **{missing: None}) == ERR_NULL, missing
    assert record_call(capi, scene=_scene(capi, planes=False)) == ERR_NULL
    assert record_call(capi, P=-1) == ERR_SHAPE
    assert record_call(capi, P=0) == OK
    assert record_call(capi, P=0, d_planes=None) == OK
    # nothing wanted: NVSR_OK without a launch; the workspace is not asked for without d_natural
    assert record_call(capi, d_natural=None, d_planes="none") == OK and record_call(capi, d_natural=None, d_planes=None, workspace=None) == OK
    assert record_call(capi, d_natural=None, d_planes="none", P=-1) == ERR_SHAPE


def test_without_d_natural_the_entry_answers_as_the_plane_gradient_entry(pkg):
    """d_natural == NULL: nvsr_generic_decode_backward_fused_ext's status in every case of test_generic_entry_status_host that stops in front of a
    launch (the workspace may be NULL)"""
    capi = pkg.capi
    cases = [dict(scene=None), dict(scene=_scene(capi, 0)), dict(scene=_scene(capi, 16)), dict(geo=None), dict(geo=GEO_INCONSISTENT), dict(geo=GEO_288),
             dict(geo=GEO_288, natural=None), dict(natural=None), dict(geo=GEO_FWD_ONLY, P=0), dict(x=None), dict(x=None, P=-1),
             dict(scene=_scene(capi, planes=False)), dict(scene=_scene(capi, planes=False), P=-1), dict(P=-1), dict(P=0), dict(P=0, x=None),
             dict(d_planes="none"), dict(d_planes=None), dict(d_planes="none", P=-1), dict(geo=GEO_FWD_ONLY, d_planes="none")]
    for kw in cases:
        want = entry_call(capi, "backward", **kw)
        assert record_call(capi, d_natural=None, workspace=None, **kw) == want, kw
    assert record_call(capi, d_natural=None, workspace=None, d_out=None) == entry_call(capi, "backward", out=None) == ERR_NULL
    assert torch.cuda.is_available() or not torch.cuda.is_initialized()
