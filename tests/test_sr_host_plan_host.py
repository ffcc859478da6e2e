"""CPU tests of the SR stage's host side ("Host side of the SR route"): the sizing functions and the status codes of every SR entry
point equal a table recorded from the library before the host code was folded into one conv route, one forward walk, one backward walk and one
region setup (sr_host_plan_table.json beside this file; `record_table` below regenerates it from whichever library NVSR_HIP_LIB names), and
the packed regions conv_kinds_for reports are exactly the region the route reads.  Pure host calls through ctypes: nothing is launched."""
import ctypes as C
import itertools
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
TABLE = os.path.join(HERE, "sr_host_plan_table.json")
OK, ERR_SHAPE, ERR_LAUNCH, ERR_NULL, ERR_ALIGN = 0, 1, 2, 3, 4
F32, F16, F16X2, BF16X3, INHERIT, PACK_ALL = 0, 1, 2, 3, -1, -3

HIDS, NBLOCKS, NUPS, CHANNELS = (16, 64, 128, 256), (0, 1, 2, 16), (0, 1, 2), (3, 48, 300)
GEOMETRIES = list(itertools.product(HIDS, NBLOCKS, NUPS)) + [(64, 291, 1), (64, 1, 9)]          # ... and the refused nblocks / n_up
ROIS = (None, (-0.6, -0.5, 0.1, 0.3), (-0.2, 0.1, 0.7, 0.9), (-1.0, -0.3, 0.2, 1.0))            # full plane, three ROIs (the last touches two borders)


@pytest.fixture(scope="module")
def pkg():
    import nvsr_amd

    nvsr_amd.build_extension()
    return nvsr_amd


def bind(capi):
    """the library NVSR_HIP_LIB names (or the tree's), with the prototypes capi declares for the symbols it has -- a library from before this
    test's route hook loads too"""
    lib = C.CDLL(capi.LIB_PATH)
    for name, (args, res) in {**capi._PROTOS, **capi._PROTOS_OPTIONAL, **capi._PROTOS_LAUNCH}.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.argtypes, fn.restype = args, res
    return lib


def out_dim(h, nblocks, n_up):
    h = h - 2 - 4 * nblocks - 2
    for _ in range(n_up):
        h = (h - 2) * 2
    return h - 2


def edsr_sizes(nblocks, n_up):
    """(H, W) from one below the smallest legal size up to 200"""
    hmin = next(h for h in range(3, 4000) if out_dim(h, nblocks, n_up) >= 1)
    if hmin > 200:
        return [(hmin - 1, hmin - 1), (hmin, hmin), (hmin, hmin + 3)]
    mid = (hmin + 200) // 2 | 1
    return [(hmin - 1, hmin - 1), (hmin, hmin), (hmin + 1, hmin + 1), (mid, mid), (200, 200), (hmin, 200), (200, hmin + 1), (hmin - 1, 200)]


def roi_arg(rois):
    flat = [v for r in rois for v in r]
    return (C.c_float * len(flat))(*flat)


def sizing_rows(lib):
    """every sizing call of the grid, in a fixed order -> {function: [values]}"""
    t = {}

    def put(name, v):
        t.setdefault(name, []).append(int(v))

    for hid, nb, nup in GEOMETRIES:
        for cin, cout in itertools.product(CHANNELS, CHANNELS):
            put("nvsr_edsr_natural_floats", lib.nvsr_edsr_natural_floats(cin, cout, hid, nb, nup))
            put("nvsr_edsr_packed_floats", lib.nvsr_edsr_packed_floats(cin, cout, hid, nb, nup))
            put("nvsr_edsr_packed_dgrad_floats", lib.nvsr_edsr_packed_dgrad_floats(cin, cout, hid, nb, nup))
        for H, W in edsr_sizes(nb, nup):
            ho, wo = C.c_int(-7), C.c_int(-7)
            put("nvsr_edsr_out_size", lib.nvsr_edsr_out_size(H, W, nb, nup, C.byref(ho), C.byref(wo)))
            put("nvsr_edsr_out_size", ho.value)
            put("nvsr_edsr_out_size", wo.value)
            put("nvsr_edsr_workspace_floats", lib.nvsr_edsr_workspace_floats(hid, nb, nup, H, W))
            for cin, cout in ((3, 3), (48, 48), (300, 300), (3, 300), (300, 48)):
                put("nvsr_edsr_acts_floats", lib.nvsr_edsr_acts_floats(cin, cout, hid, nb, nup, H, W))
                put("nvsr_edsr_backward_workspace_floats", lib.nvsr_edsr_backward_workspace_floats(cin, cout, hid, nb, nup, H, W))
        natural_pad = 2 * nb + 3 + 2 * nup
        for cc, (r0, r1), pad, roi in itertools.product(CHANNELS, ((5, 7), (24, 24), (63, 200), (200, 200)), (natural_pad, 0), ROIS):
            r = roi_arg([roi]) if roi else None
            for name in ("nvsr_planes_sr_workspace_floats", "nvsr_planes_sr_keep_floats", "nvsr_planes_sr_backward_workspace_floats"):
                put(name, getattr(lib, name)(cc, r0, r1, hid, nb, nup, pad, r))
        for cc, (r0, r1), B, ragged in itertools.product((3, 48), ((24, 24), (63, 200)), (1, 3, 4, 0, 5), (False, True)):
            r = roi_arg([ROIS[1 + b % 3] for b in range(max(B, 1))]) if ragged else None
            for name in ("nvsr_planes_sr_batch_keep_floats", "nvsr_planes_sr_batch_workspace_floats", "nvsr_planes_sr_batch_backward_workspace_floats"):
                put(name, getattr(lib, name)(B, cc, r0, r1, hid, nb, nup, natural_pad, r))
    return t


def status_cases():
    """(entry point, arguments) of calls that are wrong in one argument, or in two (the order of the checks).  Pointers are never dereferenced:
    every call is answered before its first launch.  Geometry: hid 16, one block, one up-conv, pad 6, over 1 on a 24^2 plane of 3 channels."""
    p, odd = C.c_void_p(0x10000), C.c_void_p(0x10004)
    cases = []

    def vary(name, good, *mutations):
        for m in mutations:
            args = list(good)
            for i, v in m.items():
                args[i] = v
            cases.append((name, tuple(args)))

    def ptrs(*v):
        return (C.c_void_p * len(v))(*v)

    for name, tr in (("nvsr_pack_conv3x3", 0), ("nvsr_pack_conv3x3_dgrad", 1)):
        vary(name, (p, 16, 64, p, None), {0: None}, {3: None}, {1: 0}, {2: -1}, {3: odd}, {0: None, 1: 0}, {1: 0, 3: odd})
    vary("nvsr_conv3x3", (p, 16, 9, 9, p, 64, 0, None, p, None), {0: None}, {8: None}, {6: 4}, {6: 2}, {6: 3, 5: 66}, {4: odd}, {0: None, 6: 7}, {6: 9, 4: odd})
    vary("nvsr_conv3x3_arith", (p, 16, 9, 9, p, 64, 0, None, p, BF16X3, 0, None), {4: None}, {6: -1}, {4: odd}, {9: F16}, {4: odd, 9: F16}, {6: 2, 4: odd},
         {9: 7}, {10: 5}, {10: 17}, {9: F32, 10: 8}, {2: 2}, {9: 7, 10: 5})
    vary("nvsr_conv3x3_dgrad", (p, 16, 9, 9, p, 64, p, None), {0: None}, {6: None}, {4: odd}, {2: 2}, {4: odd, 3: 1}, {4: None, 2: 2})
    vary("nvsr_conv3x3_dgrad_arith", (p, 16, 9, 9, p, 64, p, BF16X3, 0, None), {0: None}, {4: odd}, {3: 2}, {7: F16}, {7: 9}, {8: 21}, {4: odd, 3: 2}, {7: F16, 3: 2})
    vary("nvsr_conv3x3_wgrad", (p, p, 16, 9, 9, 64, C.c_float(1.0), p, p, None), {0: None}, {1: None}, {7: None}, {8: None}, {2: 0}, {4: 2}, {0: None, 2: 0})
    vary("nvsr_conv3x3_wgrad_arith", (p, p, 16, 9, 9, 64, C.c_float(1.0), p, p, BF16X3, None), {8: None}, {5: 0}, {9: F16}, {9: 11}, {8: None, 9: 11}, {3: 2, 9: F16})
    for name in ("nvsr_pack_edsr", "nvsr_pack_edsr_dgrad"):
        vary(name, (p, 3, 3, 16, 1, 1, p, None), {0: None}, {6: None}, {4: 291}, {4: -1}, {5: 9}, {6: odd}, {4: 291, 6: odd}, {0: None, 5: 9})
    for name in ("nvsr_pack_edsr_arith", "nvsr_pack_edsr_dgrad_arith"):
        vary(name, (p, 3, 3, 16, 1, 1, p, BF16X3, None), {6: None}, {5: 9}, {6: odd}, {7: 5}, {6: odd, 7: 5}, {5: 9, 6: odd})
    vary("nvsr_edsr_forward", (p, 3, 36, 36, p, 3, 16, 1, 1, p, p, None), {0: None}, {4: None}, {9: None}, {10: None}, {2: 11}, {3: 2}, {0: None, 2: 11})
    vary("nvsr_edsr_forward_batch", (p, 2, 3, 36, 36, p, 3, 16, 1, 1, p, p, None), {0: None}, {11: None}, {1: 0}, {3: 11}, {1: 0, 10: None}, {1: 0, 3: 11})
    vary("nvsr_edsr_forward_batch_arith", (p, 2, 3, 36, 36, p, 3, 16, 1, 1, p, p, BF16X3, None), {5: None}, {1: -1}, {4: 11}, {5: None, 1: -1})
    vary("nvsr_edsr_forward_train", (p, 3, 36, 36, p, 3, 16, 1, 1, p, p, None), {0: None}, {10: None}, {4: odd}, {2: 11}, {7: 291}, {8: 9}, {6: 0}, {4: odd, 2: 11},
         {10: None, 4: odd})
    vary("nvsr_edsr_forward_train_arith", (p, 3, 36, 36, p, 3, 16, 1, 1, p, p, BF16X3, None), {9: None}, {4: odd}, {3: 11}, {4: odd, 8: 9}, {9: None, 3: 11})
    vary("nvsr_edsr_backward", (p, 3, 36, 36, p, p, 3, 16, 1, 1, p, p, p, p, None), {0: None}, {4: None}, {5: None}, {10: None}, {11: None}, {13: None}, {5: odd}, {13: odd},
         {2: 11}, {8: 291}, {5: odd, 2: 11}, {10: None, 13: odd})
    vary("nvsr_edsr_backward_arith", (p, 3, 36, 36, p, p, 3, 16, 1, 1, p, p, None, p, BF16X3, None), {13: None}, {13: odd}, {3: 11}, {9: 9}, {13: odd, 9: 9}, {0: None, 13: odd})
    # PlanesSR: (.., Cc, R0, R1, packed, hid, nblocks, n_up, pad, over, roi, ..)
    roi = roi_arg([ROIS[1]])
    vary("nvsr_planes_sr", (p, 3, 24, 24, p, 16, 1, 1, 6, 1, None, None, None, p, p, None), {0: None}, {4: None}, {13: None}, {14: None}, {11: p}, {12: p}, {9: 0}, {8: 0},
         {8: 5}, {10: roi, 8: 5}, {13: None, 9: 0}, {11: p, 9: 0})
    vary("nvsr_planes_sr_arith", (p, 3, 24, 24, p, 16, 1, 1, 6, 1, None, None, None, p, p, BF16X3, None), {14: None}, {12: p}, {9: 2}, {2: 2, 8: 0}, {12: p, 9: 2}, {0: None, 9: 2})
    lrs, outs, holes = ptrs(0x10000, 0x20000, 0x30000), ptrs(0x40000, 0x50000, 0x60000), ptrs(0x10000, None, 0x30000)
    vary("nvsr_planes_sr_batch", (lrs, 3, 3, 24, 24, p, 16, 1, 1, 6, 1, None, None, None, outs, p, None), {0: None}, {5: None}, {14: None}, {15: None}, {12: p}, {1: 0}, {1: 65},
         {0: holes}, {14: holes}, {10: 0}, {1: 0, 12: p}, {1: 0, 0: holes}, {0: holes, 10: 0})
    vary("nvsr_planes_sr_batch_arith", (lrs, 3, 3, 24, 24, p, 16, 1, 1, 6, 1, None, None, None, outs, p, BF16X3, None), {15: None}, {1: 65}, {10: 3}, {14: holes, 10: 3}, {1: 65, 15: None})
    vary("nvsr_planes_sr_batch_ex", (lrs, 3, 3, 24, 24, p, 16, 1, 1, 6, 1, None, None, None, outs, p, BF16X3, 1, 0, None), {0: None}, {18: 2}, {18: -1}, {13: p}, {1: 0}, {10: 0},
         {18: 2, 13: p}, {0: None, 18: 2}, {13: p, 1: 0}, {1: 0, 14: holes})
    vary("nvsr_planes_sr_train", (p, 3, 24, 24, p, 16, 1, 1, 6, 1, None, None, None, p, p, p, None), {15: None}, {0: None}, {14: None}, {11: p}, {9: 0}, {15: None, 9: 0}, {11: p, 9: 0})
    vary("nvsr_planes_sr_train_arith", (p, 3, 24, 24, p, 16, 1, 1, 6, 1, None, None, None, p, p, p, BF16X3, None), {15: None}, {4: None}, {9: 5}, {6: 291}, {15: None, 9: 5}, {13: None, 6: 291})
    vary("nvsr_planes_sr_backward", (3, 24, 24, p, p, 16, 1, 1, 6, 1, None, None, p, p, None, p, None), {3: None}, {4: None}, {12: None}, {13: None}, {15: None}, {9: 0}, {8: 0},
         {7: 9}, {6: 291}, {3: None, 9: 0}, {15: None, 8: 0})
    vary("nvsr_planes_sr_backward_arith", (3, 24, 24, p, p, 16, 1, 1, 6, 1, None, None, p, p, p, p, BF16X3, None), {13: None}, {9: 4}, {0: 0}, {13: None, 9: 4}, {12: None, 0: 0})
    rois = roi_arg([ROIS[1], ROIS[2], ROIS[3]])
    good = (lrs, 3, 3, 24, 24, p, 16, 1, 1, 6, 1, rois, None, None, outs, p, p, BF16X3, 1, 0, None)
    vary("nvsr_planes_sr_train_batch_arith", good, {0: None}, {5: None}, {14: None}, {15: None}, {16: None}, {12: p}, {19: 3}, {5: odd}, {15: odd}, {16: odd}, {1: 0}, {1: 5},
         {0: holes}, {14: holes}, {10: 0}, {9: 0}, {7: 291}, {8: 9}, {12: p, 19: 3}, {19: 3, 5: odd}, {16: odd, 1: 5}, {1: 5, 0: holes}, {14: holes, 10: 0}, {16: None, 19: 3})
    douts, dlrs = ptrs(0x40000, 0x50000, 0x60000), ptrs(0x70000, None, 0x80000)
    good = (3, 3, 24, 24, p, p, 16, 1, 1, 6, 1, rois, None, douts, p, dlrs, p, BF16X3, 1, 0, None)
    vary("nvsr_planes_sr_backward_batch_arith", good, {4: None}, {5: None}, {13: None}, {14: None}, {16: None}, {0: 0}, {0: 5}, {19: 7}, {5: odd}, {16: odd}, {4: odd}, {13: holes},
         {10: 0}, {9: 1}, {8: 9}, {0: 5, 19: 7}, {0: 0, 16: odd}, {19: 7, 4: odd}, {5: odd, 13: holes}, {13: holes, 10: 0}, {16: None, 0: 5})
    layers, events = (C.c_int32 * 2)(0, 3), ptrs(0x90000, 0xa0000)
    good = (3, 3, 24, 24, p, p, 16, 1, 1, 6, 1, rois, None, douts, p, dlrs, p, BF16X3, 1, 0, 2, layers, events, None)
    vary("nvsr_planes_sr_backward_batch_marks", good, {14: None}, {20: -1}, {21: None}, {22: None}, {0: 5}, {16: odd}, {10: 4}, {21: None, 0: 5}, {20: -1, 16: odd}, {22: None, 10: 4},
         {21: (C.c_int32 * 2)(-1, 3), 19: 2})
    return cases


def status_rows(lib):
    return [int(getattr(lib, name)(*args)) for name, args in status_cases()]


def record_table(path=TABLE):
    """python -c "import sys; sys.path.insert(0, 'tests'); import test_sr_host_plan_host as t; t.record_table()" with NVSR_HIP_LIB=<the build to
    record from>: writes the table the tests below compare against"""
    import nvsr_amd

    lib = bind(nvsr_amd.capi)
    with open(path, "w") as f:
        json.dump({"sizing": sizing_rows(lib), "status": status_rows(lib)}, f, separators=(",", ":"))
        f.write("\n")


@pytest.fixture(scope="module")
def table():
    with open(TABLE) as f:
        return json.load(f)


def test_sizing_functions_return_the_recorded_values(pkg, table):
    got = sizing_rows(bind(pkg.capi))
    assert sorted(got) == sorted(table["sizing"])
    for name, want in table["sizing"].items():
        assert len(got[name]) == len(want), name
        bad = [i for i, (a, b) in enumerate(zip(got[name], want)) if a != b]
        assert not bad, "%s: %d of %d calls differ, first at call %d: %d, recorded %d" % (name, len(bad), len(want), bad[0], got[name][bad[0]], want[bad[0]])
    # the grid has what it is for: refusals (-1) and answers in every function, and the Cout > hid case changes the backward workspace
    for name, want in table["sizing"].items():
        if name not in ("nvsr_edsr_natural_floats", "nvsr_edsr_out_size", "nvsr_edsr_workspace_floats"):
            assert -1 in want and max(want) > 0, name


def test_status_codes_equal_the_recorded_ones_and_come_before_any_launch(pkg, table):
    """no GPU here: a call that reached a launch would come back as NVSR_ERR_LAUNCH"""
    cases, got = status_cases(), status_rows(bind(pkg.capi))
    assert len(got) == len(table["status"])
    for (name, args), g, want in zip(cases, got, table["status"]):
        assert g == want, "%s%r: %d, recorded %d" % (name, args, g, want)
        assert g in (ERR_SHAPE, ERR_NULL, ERR_ALIGN), (name, args, g)
    assert {ERR_SHAPE, ERR_NULL, ERR_ALIGN} <= set(got)


def kinds_before(cin, cout, arith):
    """the packer's predicate as it stood beside the launcher's branches (sr_core.h before the route): bit k = region k"""
    if arith == PACK_ALL:
        return 15
    if arith == F32:
        return 1
    ncb = (cout + 63) // 64 * 2
    wl, w16 = cin % 16 == 0 and (ncb % 8 == 0 or ncb == 2), cin % 32 == 0 and cout % 128 == 0
    if wl and ncb == 2:
        return 2
    if w16:
        return 8 if arith in (F16, F16X2) else 4
    return 2 if wl else 1


def test_route_and_packed_regions_agree(pkg):
    lib = pkg.capi.lib()
    chans = (3, 16, 48, 64, 128, 256, 512)
    fam, reg, kinds = C.c_int(), C.c_int(), C.c_uint()
    families = set()
    for cin, cout, arith in itertools.product(chans, chans, (F32, BF16X3, F16X2, F16, PACK_ALL)):
        assert lib.nvsr_internal_conv_route(cin, cout, 40, 40, arith, 0, C.byref(fam), C.byref(reg), C.byref(kinds)) == OK
        assert kinds.value == kinds_before(cin, cout, arith), (cin, cout, arith)
        if arith == PACK_ALL:
            assert (fam.value, reg.value) == (-1, -1)
            continue
        assert kinds.value == 1 << reg.value, (cin, cout, arith, fam.value)          # the packer writes exactly the region the launch reads
        families.add(fam.value)
    assert families == {0, 1, 3, 4, 5}          # narrow limb, 16x16x32, wide limb, exact-f32 wide and narrow (the 8-row wide kernel is opt-in)
    # the opt-in kernels and the refusals of rows_per_tile
    route = lambda cin, cout, arith, rows: (lib.nvsr_internal_conv_route(cin, cout, 40, 40, arith, rows, C.byref(fam), C.byref(reg), C.byref(kinds)), fam.value, reg.value)
    assert route(256, 256, BF16X3, 8) == (OK, 2, 1) and route(256, 256, BF16X3, 3) == (OK, 3, 1) and route(256, 256, BF16X3, 19) == (OK, 1, 2)
    assert route(256, 256, F16X2, 22) == (OK, 1, 3) and route(256, 256, BF16X3, 22)[0] == ERR_SHAPE
    assert route(48, 128, BF16X3, 16)[0] == ERR_SHAPE and route(128, 128, BF16X3, 8)[0] == ERR_SHAPE and route(256, 256, F32, 8)[0] == ERR_SHAPE
    assert route(256, 256, BF16X3, 5)[0] == ERR_SHAPE and route(256, 256, 7, 0)[0] == ERR_SHAPE and route(256, 256, F32, 2) == (OK, 4, 0)
    assert lib.nvsr_internal_conv_route(16, 16, 2, 40, BF16X3, 0, C.byref(fam), C.byref(reg), C.byref(kinds)) == ERR_SHAPE
    assert lib.nvsr_internal_conv_route(16, 16, 40, 40, BF16X3, 0, None, C.byref(reg), C.byref(kinds)) == ERR_NULL
