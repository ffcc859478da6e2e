"""The answers of TwoDimPlanesModel.generic_decoder_train_route() -- the route of a generic geometry's training WITH decoder gradients -- over the
product of everything it reads, as one table.

    python tools/generic_decoder_train_route_table.py      # writes tests/generic_decoder_train_route_table.json from THIS tree

tests/test_generic_train_decoder_fused_host.py replays table() and compares it with the committed file, row by row.  The file is regenerated
only by a change that means to move the route (a measured default width, a new condition).  The five older predicates keep their own table
(tools/generic_route_table.py).  No GPU is touched: the predicate asks the library's *_supported entries, which are host code."""
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "generic_decoder_train_route_table.json")
SID = "lego_DS8_PlRes10_6"
HANDLE = "NVSR_GENERIC_TRAIN_DECODER_FUSED"
# the axes in the order of the rows (itertools.product: the last one runs fastest).  dec_channels 4096 is beyond the fused kernels' capacity
# ("held" is false there); span: "default" = GENERIC_TRAIN_DECODER_FUSED_DEFAULT_HIDDEN as the class has it, else that span on the instance,
# which puts 128 inside and 64 outside
AXES = [(HANDLE, [None, "0", "1"]), ("dec_channels", [64, 128, 4096]), ("span", ["default", [128, 128]]), ("grad_enabled", [False, True]),
        ("decoder_frozen", [False, True]), ("planes_require_grad", [False, True]), ("deterministic", [False, True])]
LETTER = {"fused": "F", "layered": "L"}


def _model(pkg, torch, dec_channels):
    kw = dict(dec_density_layers=1, dec_rgb_layers=1, proj_combination="sum") if dec_channels > 256 else dict(
        proj_combination="avg", viewdir_proj_combination="mult", skip_connect_every=3)
    m = pkg.models.TwoDimPlanesModel(use_viewdirs=True, align_corners=True, dec_channels=dec_channels, **kw)
    m.planes_ = torch.nn.ParameterDict({pkg.models.get_plane_name(SID, d): torch.nn.Parameter(torch.zeros(1, 48, 4, 4)) for d in range(4)})
    m.set_cur_scene_id(SID)
    m.train()
    assert not m.is_native_geometry()
    return m


def table(pkg):
    """the rows, in the order of itertools.product over AXES"""
    import torch

    saved = os.environ.get(HANDLE)
    models, rows = {}, []
    try:
        for handle, dec, span, grad, frozen, planes_grad, det in itertools.product(*[values for _, values in AXES]):
            os.environ.pop(HANDLE, None) if handle is None else os.environ.__setitem__(HANDLE, handle)
            m = models.get(dec) or models.setdefault(dec, _model(pkg, torch, dec))
            m.__dict__.pop("GENERIC_TRAIN_DECODER_FUSED_DEFAULT_HIDDEN", None)
            if span != "default":
                m.GENERIC_TRAIN_DECODER_FUSED_DEFAULT_HIDDEN = tuple(span)
            for p in m.decoder_parameters():
                p.requires_grad_(not frozen)
            for p in m.planes_.values():
                p.requires_grad_(planes_grad)
            with torch.set_grad_enabled(grad), pkg.capi.deterministic_scope(det):
                rows.append(LETTER[m.generic_decoder_train_route()])
    finally:
        os.environ.pop(HANDLE, None) if saved is None else os.environ.__setitem__(HANDLE, saved)
    return {"axes": [[name, values] for name, values in AXES], "rows": "".join(rows)}


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
    print("%d rows -> %s; fused: %d" % (len(t["rows"]), OUT, t["rows"].count("F")))
