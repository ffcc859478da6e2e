"""The answers of the route predicates of the generic decoder geometries over the product of everything they read, as one table:
TwoDimPlanesModel.generic_route / generic_train_route / generic_arithmetic / generic_frame_route and train_utils._generic_occupancy.

    python tools/generic_route_table.py            # writes tests/generic_route_table.json from THIS tree

tests/test_generic_routes_host.py replays table() and compares it with the committed file, row by row.  The file is regenerated only by a
change that means to move a route (a new measured default, a new handle); a refactor of the predicates must leave it as it is.
No GPU is touched: the predicates ask the library's *_supported entries, which are host code."""
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "generic_route_table.json")
SID = "lego_DS8_PlRes10_6"
HANDLES = ("NVSR_GENERIC_FUSED", "NVSR_GENERIC_TRAIN_FUSED", "NVSR_GENERIC_TWO_PHASE")
# the axes in the order of the rows (itertools.product: the last one runs fastest)
AXES = [("NVSR_GENERIC_FUSED", [None, "0", "1"]), ("NVSR_GENERIC_TRAIN_FUSED", [None, "0", "1"]), ("NVSR_GENERIC_TWO_PHASE", [None, "0", "1"]),
        ("dec_channels", [32, 64, 128, 256, 288]), ("arithmetic", [None, "f16x2"]), ("grad_enabled", [False, True]),
        ("decoder_frozen", [False, True]), ("planes_require_grad", [False, True]), ("jitter", [0.0, 0.5]), ("deterministic", [False, True]),
        ("grid_built", [False, True])]
# a row is five letters: generic_route, generic_train_route, generic_arithmetic, generic_frame_route, _generic_occupancy
LETTERS = ({"fused": "F", "layered": "L"}, {"fused": "F", "layered": "L"}, {"f16x2": "h", "f32": "s"}, {"two_phase": "T", "one_phase": "O"})


def _model(pkg, torch, dec_channels):
    m = pkg.models.TwoDimPlanesModel(use_viewdirs=True, align_corners=True, dec_channels=dec_channels, proj_combination="avg",
                                     viewdir_proj_combination="mult", skip_connect_every=3)
    m.planes_ = torch.nn.ParameterDict({pkg.models.get_plane_name(SID, d): torch.nn.Parameter(torch.zeros(1, 48, 4, 4)) for d in range(4)})
    m.set_cur_scene_id(SID)
    m.train()                                        # (the jitter is drawn in training mode only)
    assert not m.is_native_geometry()
    m.__dict__["occupancy_entry"] = lambda scene_id: ("grid", 16)      # a grid that is never stale: the key needs the planes on a device
    return m


def table(pkg):
    """the rows, in the order of itertools.product over AXES"""
    import torch

    saved = {h: os.environ.get(h) for h in HANDLES}
    models = {}
    rows = []
    try:
        for combo in itertools.product(*[values for _, values in AXES]):
            f, tf, tp, dec, arithmetic, grad, frozen, planes_grad, jitter, det, grid = combo
            for h, v in zip(HANDLES, (f, tf, tp)):
                os.environ.pop(h, None) if v is None else os.environ.__setitem__(h, v)
            m = models.get(dec) or models.setdefault(dec, _model(pkg, torch, dec))
            m.arithmetic = arithmetic
            m.point_coords_noise = jitter
            for p in m.decoder_parameters():
                p.requires_grad_(not frozen)
            for p in m.planes_.values():
                p.requires_grad_(planes_grad)
            if grid:
                m.__dict__["_occupancy"] = {SID: (None, "grid", 16)}
            else:
                m.__dict__.pop("_occupancy", None)
            with torch.set_grad_enabled(grad), pkg.capi.deterministic_scope(det):
                answers = (m.generic_route(), m.generic_train_route(), m.generic_arithmetic(), m.generic_frame_route())
                occ = pkg.train_utils._generic_occupancy(m, None, None)
            rows.append("".join(t[a] for t, a in zip(LETTERS, answers)) + ("N" if occ is None else "G"))
    finally:
        for h, v in saved.items():
            os.environ.pop(h, None) if v is None else os.environ.__setitem__(h, v)
    return {"axes": [[name, values] for name, values in AXES], "rows": rows}


def describe(index):
    """the inputs of row `index`, for a message"""
    combo = list(itertools.product(*[values for _, values in AXES]))[index]
    return ", ".join("%s=%r" % (name, v) for (name, _), v in zip(AXES, combo))


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    import nvsr_amd

    nvsr_amd.build_extension()
    t = table(nvsr_amd)
    with open(OUT, "w") as fh:
        json.dump(t, fh, separators=(",", ":"))
        fh.write("\n")
    print("%d rows -> %s; distinct: %s" % (len(t["rows"]), OUT, sorted(set(t["rows"]))))
