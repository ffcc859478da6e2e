"""CPU test of what the entry points of the fused generic kernels answer BEFORE a launch (csrc/generic_fused*.hip, the capacity part of
nvsr_generic_occupancy_build_ext): one shared preamble (gf_check_entry, csrc/generic_fused_core.h) fixes the order of the checks and with
it the status codes.  EXPECTED was recorded from the library of the commit before the preamble was folded (`python
tests/test_generic_entry_status_host.py` prints the table of the library in use); the library must keep answering it.  Every call returns
in front of a launch and nothing dereferences the dummy pointers: no GPU is touched."""
import ctypes as C

import pytest
import torch

OK, ERR_SHAPE, ERR_LAUNCH, ERR_NULL, ERR_ALIGN = 0, 1, 2, 3, 4
F32, F16X2 = 0, 2
ONE = 16                                                    # a dummy, 16-byte aligned, non-null pointer
GEO_OK = [48, 48, 64, 4, 4, 0, 1, 4]
GEO_INCONSISTENT = [48, 48, 128, 4, 4, 0, 0, 3]             # 'concat' view features on summed position features
GEO_288 = [48, 48, 288, 4, 4, 0, 1, 4]                      # beyond every fused kernel's capacity
GEO_FWD_ONLY = [512, 512, 256, 4, 4, 0, 0, 0]               # inside the f32 forward's capacity, beyond the backward's (1348-float rows)

FORWARD = ("fused", "arith", "density", "colour", "density_list")
LISTED = ("colour", "density_list")


def _scene(capi, n_pos=3, planes=True):
    sc = capi.SceneExt()
    sc.num_position_planes = n_pos
    if planes:
        for d in range(min(max(n_pos, 0), capi.MAX_POSITION_PLANES) + 1):
            sc.planes[d], sc.ph[d], sc.pw[d] = ONE, 4, 4
    return sc


def call(capi, entry, scene="ok", geo=GEO_OK, natural=ONE, packed=ONE, P=8, x=ONE, out=ONE, index=ONE, count=ONE, max_count=4, arith=F32,
         d_planes="all", G=8, K=1, dilate=0, grid=ONE, workspace=ONE):
    """one call of `entry` with everything valid except what the keywords change; scene: 'ok', None, or a SceneExt"""
    lib = capi.lib()
    sc = _scene(capi) if isinstance(scene, str) else scene
    scp = None if sc is None else C.byref(sc)
    g = None if geo is None else capi.DecoderGeometry(*geo)
    gp = None if g is None else C.byref(g)
    if entry == "fused":
        return lib.nvsr_generic_decode_fused_ext(scp, gp, natural, P, x, None, out, None)
    if entry == "arith":
        return lib.nvsr_generic_decode_fused_arith_ext(scp, gp, natural, packed, P, x, None, out, arith, None)
    if entry == "density":
        return lib.nvsr_generic_decode_fused_density_arith_ext(scp, gp, natural, packed, P, x, None, out, arith, None)
    if entry == "colour":
        return lib.nvsr_generic_decode_fused_colour_arith_ext(scp, gp, natural, packed, P, x, None, index, count, max_count, out, arith, None)
    if entry == "density_list":
        return lib.nvsr_generic_decode_fused_density_list_arith_ext(scp, gp, natural, packed, P, x, None, index, count, max_count, out, arith, None)
    if entry == "backward":
        n = min(sc.num_position_planes if sc is not None else 3, capi.MAX_POSITION_PLANES) + 1
        arr = None if d_planes is None else (C.c_void_p * 16)(*([ONE] * n if d_planes == "all" else [None] * n))
        return lib.nvsr_generic_decode_backward_fused_ext(scp, gp, natural, P, x, None, out, arr, None)
    if entry == "occupancy":
        return lib.nvsr_generic_occupancy_build_ext(scp, gp, natural, packed, G, K, 0.0, dilate, arith, grid, workspace, None)
    raise KeyError(entry)


def observed(capi):
    """{case: status} of the library in use.  No case reaches a launch: each changes something a check in front of it refuses, or has
    nothing to do (P = 0, an empty list, no wanted gradient)."""
    lib = capi.lib()
    t = {}
    arith_entries = FORWARD[1:]
    for e in FORWARD + ("backward", "occupancy"):
        occ = e == "occupancy"
        t[e + ":null_scene"] = call(capi, e, scene=None)
        t[e + ":planes_0"] = call(capi, e, scene=_scene(capi, 0))
        t[e + ":planes_16"] = call(capi, e, scene=_scene(capi, 16))
        t[e + ":null_geometry"] = call(capi, e, geo=None)
        t[e + ":inconsistent"] = call(capi, e, geo=GEO_INCONSISTENT)
        t[e + ":hidden_288"] = call(capi, e, geo=GEO_288)
        t[e + ":hidden_288,null_natural"] = call(capi, e, geo=GEO_288, natural=None)             # the capacity is asked first
        t[e + ":null_natural"] = call(capi, e, natural=None)
        if occ:
            continue
        t[e + ":fwd_only_geometry,P=0"] = call(capi, e, geo=GEO_FWD_ONLY, P=0)
        t[e + ":null_x"] = call(capi, e, x=None)
        t[e + ":null_out"] = call(capi, e, out=None)
        t[e + ":null_x,P=-1"] = call(capi, e, x=None, P=-1)                                       # pointers before P
        t[e + ":scene_without_planes"] = call(capi, e, scene=_scene(capi, planes=False))
        t[e + ":scene_without_planes,P=-1"] = call(capi, e, scene=_scene(capi, planes=False), P=-1)
        t[e + ":P=-1"] = call(capi, e, P=-1)
        t[e + ":P=0"] = call(capi, e, P=0)
        t[e + ":P=0,null_x"] = call(capi, e, P=0, x=None)
    for e in arith_entries + ("occupancy",):
        for a in (1, 3, -1, 7):
            t["%s:arith=%d" % (e, a)] = call(capi, e, arith=a)
        t[e + ":arith=1,null_scene"] = call(capi, e, arith=1, scene=None)
        t[e + ":f16x2,null_packed"] = call(capi, e, arith=F16X2, packed=None)
        t[e + ":f16x2,hidden_288"] = call(capi, e, arith=F16X2, geo=GEO_288)
    for e in arith_entries:
        t[e + ":f32,null_packed,P=0"] = call(capi, e, packed=None, P=0)                           # not read in f32: allowed
        t[e + ":f16x2,null_packed,P=0"] = call(capi, e, arith=F16X2, packed=None, P=0)
        t[e + ":f16x2,P=0"] = call(capi, e, arith=F16X2, P=0)
        t[e + ":f16x2,P=-1"] = call(capi, e, arith=F16X2, P=-1)
        t[e + ":f16x2,fwd_only_geometry,P=0"] = call(capi, e, arith=F16X2, geo=GEO_FWD_ONLY, P=0)
    for e in LISTED:
        for a, tag in ((F32, "f32"), (F16X2, "f16x2")):
            t["%s:%s,null_index" % (e, tag)] = call(capi, e, arith=a, index=None)
            t["%s:%s,null_count" % (e, tag)] = call(capi, e, arith=a, count=None)
            t["%s:%s,max_count=-1" % (e, tag)] = call(capi, e, arith=a, max_count=-1)
            t["%s:%s,max_count=P+1" % (e, tag)] = call(capi, e, arith=a, max_count=9)
            t["%s:%s,max_count=0" % (e, tag)] = call(capi, e, arith=a, max_count=0)
            t["%s:%s,P=0,max_count=0" % (e, tag)] = call(capi, e, arith=a, P=0, max_count=0)
            t["%s:%s,P=0,max_count=1" % (e, tag)] = call(capi, e, arith=a, P=0, max_count=1)
        t[e + ":null_index,P=-1"] = call(capi, e, index=None, P=-1)
        t[e + ":null_index,scene_without_planes"] = call(capi, e, index=None, scene=_scene(capi, planes=False))
        t[e + ":P=2^31,max_count=0"] = call(capi, e, P=1 << 31, max_count=0)                      # int32 indices
    t["backward:no_wanted_plane"] = call(capi, "backward", d_planes="none")
    t["backward:null_d_planes"] = call(capi, "backward", d_planes=None)
    t["backward:no_wanted_plane,P=-1"] = call(capi, "backward", d_planes="none", P=-1)
    t["backward:fwd_only_geometry,no_wanted_plane"] = call(capi, "backward", geo=GEO_FWD_ONLY, d_planes="none")
    t["occupancy:G=0"] = call(capi, "occupancy", G=0)
    t["occupancy:K=0"] = call(capi, "occupancy", K=0)
    t["occupancy:dilate=-1"] = call(capi, "occupancy", dilate=-1)
    t["occupancy:G=0,null_scene"] = call(capi, "occupancy", G=0, scene=None)
    t["occupancy:null_grid"] = call(capi, "occupancy", grid=None)
    t["occupancy:null_workspace"] = call(capi, "occupancy", workspace=None)
    t["occupancy:f32,null_packed,misaligned_workspace"] = call(capi, "occupancy", packed=None, workspace=8)      # packed is not read in f32
    t["occupancy:fwd_only_geometry,null_grid"] = call(capi, "occupancy", geo=GEO_FWD_ONLY, grid=None)
    t["occupancy:f16x2,fwd_only_geometry,null_grid"] = call(capi, "occupancy", arith=F16X2, geo=GEO_FWD_ONLY, grid=None)
    # the three *_supported entries: 1 / 0 / -status
    for tag, geo, n_pos in (("ok", GEO_OK, 3), ("null_geometry", None, 3), ("planes_0", GEO_OK, 0), ("planes_16", GEO_OK, 16),
                            ("inconsistent", GEO_INCONSISTENT, 3), ("hidden_288", GEO_288, 3), ("fwd_only_geometry", GEO_FWD_ONLY, 3)):
        gp = None if geo is None else C.byref(capi.DecoderGeometry(*geo))
        t["supported:" + tag] = lib.nvsr_generic_fused_supported(gp, n_pos)
        t["backward_supported:" + tag] = lib.nvsr_generic_backward_fused_supported(gp, n_pos)
        for a in (F32, F16X2, 1, 3, -1):
            t["supported_arith=%d:%s" % (a, tag)] = lib.nvsr_generic_fused_supported_arith(gp, n_pos, a)
    return t


# recorded from the library of the parent commit
EXPECTED = {
    'fused:null_scene': 3,
    'fused:planes_0': 1,
    'fused:planes_16': 1,
    'fused:null_geometry': 3,
    'fused:inconsistent': 1,
    'fused:hidden_288': 1,
    'fused:hidden_288,null_natural': 1,
    'fused:null_natural': 3,
    'fused:fwd_only_geometry,P=0': 0,
    'fused:null_x': 3,
    'fused:null_out': 3,
    'fused:null_x,P=-1': 3,
    'fused:scene_without_planes': 3,
    'fused:scene_without_planes,P=-1': 3,
    'fused:P=-1': 1,
    'fused:P=0': 0,
    'fused:P=0,null_x': 3,
    'arith:null_scene': 3,
    'arith:planes_0': 1,
    'arith:planes_16': 1,
    'arith:null_geometry': 3,
    'arith:inconsistent': 1,
    'arith:hidden_288': 1,
    'arith:hidden_288,null_natural': 1,
    'arith:null_natural': 3,
    'arith:fwd_only_geometry,P=0': 0,
    'arith:null_x': 3,
    'arith:null_out': 3,
    'arith:null_x,P=-1': 3,
    'arith:scene_without_planes': 3,
    'arith:scene_without_planes,P=-1': 3,
    'arith:P=-1': 1,
    'arith:P=0': 0,
    'arith:P=0,null_x': 3,
    'density:null_scene': 3,
    'density:planes_0': 1,
    'density:planes_16': 1,
    'density:null_geometry': 3,
    'density:inconsistent': 1,
    'density:hidden_288': 1,
    'density:hidden_288,null_natural': 1,
    'density:null_natural': 3,
    'density:fwd_only_geometry,P=0': 0,
    'density:null_x': 3,
    'density:null_out': 3,
    'density:null_x,P=-1': 3,
    'density:scene_without_planes': 3,
    'density:scene_without_planes,P=-1': 3,
    'density:P=-1': 1,
    'density:P=0': 0,
    'density:P=0,null_x': 3,
    'colour:null_scene': 3,
    'colour:planes_0': 1,
    'colour:planes_16': 1,
    'colour:null_geometry': 3,
    'colour:inconsistent': 1,
    'colour:hidden_288': 1,
    'colour:hidden_288,null_natural': 1,
    'colour:null_natural': 3,
    'colour:fwd_only_geometry,P=0': 1,
    'colour:null_x': 3,
    'colour:null_out': 3,
    'colour:null_x,P=-1': 3,
    'colour:scene_without_planes': 3,
    'colour:scene_without_planes,P=-1': 3,
    'colour:P=-1': 1,
    'colour:P=0': 1,
    'colour:P=0,null_x': 3,
    'density_list:null_scene': 3,
    'density_list:planes_0': 1,
    'density_list:planes_16': 1,
    'density_list:null_geometry': 3,
    'density_list:inconsistent': 1,
    'density_list:hidden_288': 1,
    'density_list:hidden_288,null_natural': 1,
    'density_list:null_natural': 3,
    'density_list:fwd_only_geometry,P=0': 1,
    'density_list:null_x': 3,
    'density_list:null_out': 3,
    'density_list:null_x,P=-1': 3,
    'density_list:scene_without_planes': 3,
    'density_list:scene_without_planes,P=-1': 3,
    'density_list:P=-1': 1,
    'density_list:P=0': 1,
    'density_list:P=0,null_x': 3,
    'backward:null_scene': 3,
    'backward:planes_0': 1,
    'backward:planes_16': 1,
    'backward:null_geometry': 3,
    'backward:inconsistent': 1,
    'backward:hidden_288': 1,
    'backward:hidden_288,null_natural': 1,
    'backward:null_natural': 3,
    'backward:fwd_only_geometry,P=0': 1,
    'backward:null_x': 3,
    'backward:null_out': 3,
    'backward:null_x,P=-1': 3,
    'backward:scene_without_planes': 3,
    'backward:scene_without_planes,P=-1': 3,
    'backward:P=-1': 1,
    'backward:P=0': 0,
    'backward:P=0,null_x': 3,
    'occupancy:null_scene': 3,
    'occupancy:planes_0': 1,
    'occupancy:planes_16': 1,
    'occupancy:null_geometry': 3,
    'occupancy:inconsistent': 1,
    'occupancy:hidden_288': 1,
    'occupancy:hidden_288,null_natural': 1,
    'occupancy:null_natural': 3,
    'arith:arith=1': 1,
    'arith:arith=3': 1,
    'arith:arith=-1': 1,
    'arith:arith=7': 1,
    'arith:arith=1,null_scene': 1,
    'arith:f16x2,null_packed': 3,
    'arith:f16x2,hidden_288': 1,
    'density:arith=1': 1,
    'density:arith=3': 1,
    'density:arith=-1': 1,
    'density:arith=7': 1,
    'density:arith=1,null_scene': 1,
    'density:f16x2,null_packed': 3,
    'density:f16x2,hidden_288': 1,
    'colour:arith=1': 1,
    'colour:arith=3': 1,
    'colour:arith=-1': 1,
    'colour:arith=7': 1,
    'colour:arith=1,null_scene': 1,
    'colour:f16x2,null_packed': 3,
    'colour:f16x2,hidden_288': 1,
    'density_list:arith=1': 1,
    'density_list:arith=3': 1,
    'density_list:arith=-1': 1,
    'density_list:arith=7': 1,
    'density_list:arith=1,null_scene': 1,
    'density_list:f16x2,null_packed': 3,
    'density_list:f16x2,hidden_288': 1,
    'occupancy:arith=1': 1,
    'occupancy:arith=3': 1,
    'occupancy:arith=-1': 1,
    'occupancy:arith=7': 1,
    'occupancy:arith=1,null_scene': 3,
    'occupancy:f16x2,null_packed': 3,
    'occupancy:f16x2,hidden_288': 1,
    'arith:f32,null_packed,P=0': 0,
    'arith:f16x2,null_packed,P=0': 3,
    'arith:f16x2,P=0': 0,
    'arith:f16x2,P=-1': 1,
    'arith:f16x2,fwd_only_geometry,P=0': 0,
    'density:f32,null_packed,P=0': 0,
    'density:f16x2,null_packed,P=0': 3,
    'density:f16x2,P=0': 0,
    'density:f16x2,P=-1': 1,
    'density:f16x2,fwd_only_geometry,P=0': 0,
    'colour:f32,null_packed,P=0': 1,
    'colour:f16x2,null_packed,P=0': 3,
    'colour:f16x2,P=0': 1,
    'colour:f16x2,P=-1': 1,
    'colour:f16x2,fwd_only_geometry,P=0': 1,
    'density_list:f32,null_packed,P=0': 1,
    'density_list:f16x2,null_packed,P=0': 3,
    'density_list:f16x2,P=0': 1,
    'density_list:f16x2,P=-1': 1,
    'density_list:f16x2,fwd_only_geometry,P=0': 1,
    'colour:f32,null_index': 3,
    'colour:f32,null_count': 3,
    'colour:f32,max_count=-1': 1,
    'colour:f32,max_count=P+1': 1,
    'colour:f32,max_count=0': 0,
    'colour:f32,P=0,max_count=0': 0,
    'colour:f32,P=0,max_count=1': 1,
    'colour:f16x2,null_index': 3,
    'colour:f16x2,null_count': 3,
    'colour:f16x2,max_count=-1': 1,
    'colour:f16x2,max_count=P+1': 1,
    'colour:f16x2,max_count=0': 0,
    'colour:f16x2,P=0,max_count=0': 0,
    'colour:f16x2,P=0,max_count=1': 1,
    'colour:null_index,P=-1': 3,
    'colour:null_index,scene_without_planes': 3,
    'colour:P=2^31,max_count=0': 1,
    'density_list:f32,null_index': 3,
    'density_list:f32,null_count': 3,
    'density_list:f32,max_count=-1': 1,
    'density_list:f32,max_count=P+1': 1,
    'density_list:f32,max_count=0': 0,
    'density_list:f32,P=0,max_count=0': 0,
    'density_list:f32,P=0,max_count=1': 1,
    'density_list:f16x2,null_index': 3,
    'density_list:f16x2,null_count': 3,
    'density_list:f16x2,max_count=-1': 1,
    'density_list:f16x2,max_count=P+1': 1,
    'density_list:f16x2,max_count=0': 0,
    'density_list:f16x2,P=0,max_count=0': 0,
    'density_list:f16x2,P=0,max_count=1': 1,
    'density_list:null_index,P=-1': 3,
    'density_list:null_index,scene_without_planes': 3,
    'density_list:P=2^31,max_count=0': 1,
    'backward:no_wanted_plane': 0,
    'backward:null_d_planes': 0,
    'backward:no_wanted_plane,P=-1': 1,
    'backward:fwd_only_geometry,no_wanted_plane': 1,
    'occupancy:G=0': 1,
    'occupancy:K=0': 1,
    'occupancy:dilate=-1': 1,
    'occupancy:G=0,null_scene': 1,
    'occupancy:null_grid': 3,
    'occupancy:null_workspace': 3,
    'occupancy:f32,null_packed,misaligned_workspace': 4,
    'occupancy:fwd_only_geometry,null_grid': 3,
    'occupancy:f16x2,fwd_only_geometry,null_grid': 3,
    'supported:ok': 1,
    'backward_supported:ok': 1,
    'supported_arith=0:ok': 1,
    'supported_arith=2:ok': 1,
    'supported_arith=1:ok': 0,
    'supported_arith=3:ok': 0,
    'supported_arith=-1:ok': 0,
    'supported:null_geometry': -3,
    'backward_supported:null_geometry': -3,
    'supported_arith=0:null_geometry': -3,
    'supported_arith=2:null_geometry': -3,
    'supported_arith=1:null_geometry': -3,
    'supported_arith=3:null_geometry': -3,
    'supported_arith=-1:null_geometry': -3,
    'supported:planes_0': -1,
    'backward_supported:planes_0': -1,
    'supported_arith=0:planes_0': -1,
    'supported_arith=2:planes_0': -1,
    'supported_arith=1:planes_0': -1,
    'supported_arith=3:planes_0': -1,
    'supported_arith=-1:planes_0': -1,
    'supported:planes_16': -1,
    'backward_supported:planes_16': -1,
    'supported_arith=0:planes_16': -1,
    'supported_arith=2:planes_16': -1,
    'supported_arith=1:planes_16': -1,
    'supported_arith=3:planes_16': -1,
    'supported_arith=-1:planes_16': -1,
    'supported:inconsistent': -1,
    'backward_supported:inconsistent': -1,
    'supported_arith=0:inconsistent': -1,
    'supported_arith=2:inconsistent': -1,
    'supported_arith=1:inconsistent': -1,
    'supported_arith=3:inconsistent': -1,
    'supported_arith=-1:inconsistent': -1,
    'supported:hidden_288': 0,
    'backward_supported:hidden_288': 0,
    'supported_arith=0:hidden_288': 0,
    'supported_arith=2:hidden_288': 0,
    'supported_arith=1:hidden_288': 0,
    'supported_arith=3:hidden_288': 0,
    'supported_arith=-1:hidden_288': 0,
    'supported:fwd_only_geometry': 1,
    'backward_supported:fwd_only_geometry': 0,
    'supported_arith=0:fwd_only_geometry': 1,
    'supported_arith=2:fwd_only_geometry': 1,
    'supported_arith=1:fwd_only_geometry': 0,
    'supported_arith=3:fwd_only_geometry': 0,
    'supported_arith=-1:fwd_only_geometry': 0,
}


@pytest.fixture(scope="module")
def pkg():
    import nvsr_amd

    nvsr_amd.build_extension()
    return nvsr_amd


def test_every_entry_answers_the_recorded_status(pkg):
    got = observed(pkg.capi)
    assert list(got) == list(EXPECTED), "the cases of observed() and of EXPECTED differ"
    wrong = {k: (got[k], EXPECTED[k]) for k in got if got[k] != EXPECTED[k]}
    assert not wrong, "case: (this library, recorded) %r" % wrong
    assert torch.cuda.is_available() or not torch.cuda.is_initialized()


def test_the_table_covers_every_status_and_every_entry():
    """the recording is not vacuous: each entry is refused for a shape, for a null pointer, and answers NVSR_OK where there is nothing to do"""
    for e in FORWARD + ("backward",):
        seen = {v for k, v in EXPECTED.items() if k.startswith(e + ":")}
        assert {OK, ERR_SHAPE, ERR_NULL} <= seen, (e, seen)
    assert {ERR_SHAPE, ERR_NULL, ERR_ALIGN} <= {v for k, v in EXPECTED.items() if k.startswith("occupancy:")}
    assert ERR_LAUNCH not in EXPECTED.values()                  # no case reaches a launch
    assert EXPECTED["supported:ok"] == 1 and EXPECTED["supported:hidden_288"] == 0 and EXPECTED["supported:null_geometry"] == -ERR_NULL
    assert EXPECTED["supported:fwd_only_geometry"] == 1 and EXPECTED["backward_supported:fwd_only_geometry"] == 0


if __name__ == "__main__":
    import os
    import sys

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import nvsr_amd

    print("EXPECTED = {")
    for k, v in observed(nvsr_amd.capi).items():
        print("    %r: %d," % (k, v))
    print("}")
