"""CPU tests of the fused evaluation route of the generic decoder geometries (csrc/generic_fused.hip): the capacity rule
nvsr_generic_fused_supported and the routing decision TwoDimPlanesModel.generic_route().  Neither touches a GPU: the library loads without
a device, and the decision reads the environment, the gradient mode and the geometry only."""
import ctypes as C
import os

import pytest
import torch

from test_oracle import G18_VARIANTS, G22_KW

PROJ = {"sum": 0, "avg": 1, "concat": 2}
VIEW = {"sum": 0, "avg": 1, "mult": 2, "concat": 3, "concat_pos": 4}


@pytest.fixture(scope="module")
def pkg():
    import nvsr_amd

    nvsr_amd.build_extension()
    return nvsr_amd


def supported(pkg, geometry, n_pos=3):
    geo = pkg.capi.DecoderGeometry(*geometry)
    return pkg.capi.lib().nvsr_generic_fused_supported(C.byref(geo), n_pos)


def geometry_of(kw):
    """constructor keywords of TwoDimPlanesModel -> struct nvsr_decoder_geometry (the reference's defaults: 48 channels, 128 wide, 4 + 4 layers)"""
    proj = kw.get("proj_combination", "sum")
    view = kw.get("viewdir_proj_combination") or proj
    c = kw.get("num_plane_channels", 48)
    return [c, kw.get("num_viewdir_plane_channels", c), kw.get("dec_channels", 128), kw.get("dec_density_layers", 4), kw.get("dec_rgb_layers", 4),
            int(kw.get("skip_connect_every") or 0), PROJ[proj], VIEW[view]]


def test_capacity_covers_the_fixture_geometries_and_the_yaml_alternatives(pkg):
    for name, kw in G18_VARIANTS.items():
        assert supported(pkg, geometry_of(dict(dict(skip_connect_every=3), **kw))) == 1, name
    # g22: 'avg' / 'concat_pos' with skip_connect_every 3 at 64 (align_false, bicubic, planes5) and 128 (noise) wide, 3 / 4 / 5 position planes
    for hidden in (64, 128):
        for n_pos in (3, 4, 5):
            assert supported(pkg, geometry_of(dict(G22_KW, dec_channels=hidden)), n_pos) == 1, (hidden, n_pos)
    # config/TrainModels.yml's alternatives beside its defaults
    shipped = dict(proj_combination="avg", viewdir_proj_combination="concat_pos")
    for kw, n_pos in ((dict(shipped, dec_channels=256), 3), (dict(shipped, dec_rgb_layers=8), 3), (dict(shipped, dec_channels=256, dec_rgb_layers=8), 3),
                      (dict(proj_combination="concat", viewdir_proj_combination="concat"), 3), (dict(proj_combination="sum"), 3),
                      (dict(shipped), 4), (dict(shipped, num_plane_channels=24), 3), (dict(shipped, skip_connect_every=3), 3),
                      (dict(proj_combination="concat", viewdir_proj_combination="concat_pos", dec_channels=256), 4),      # Kd = 192, Kr = 240
                      (dict(shipped), 5), (dict(shipped), 8)):
        assert supported(pkg, geometry_of(kw), n_pos) == 1, (kw, n_pos)


def test_capacity_refuses_what_does_not_fit_and_what_is_inconsistent(pkg):
    shipped = dict(proj_combination="avg", viewdir_proj_combination="concat_pos")
    assert supported(pkg, geometry_of(dict(shipped, dec_channels=4096))) == 0
    assert supported(pkg, geometry_of(dict(shipped, dec_channels=257))) == 0            # one past the widest layer the kernel holds
    assert supported(pkg, geometry_of(dict(shipped, num_plane_channels=1024))) == 0
    assert supported(pkg, geometry_of(dict(proj_combination="sum", num_plane_channels=1024))) == 0
    assert supported(pkg, geometry_of(dict(proj_combination="sum", num_plane_channels=512))) == 1
    assert supported(pkg, geometry_of(dict(proj_combination="sum", num_plane_channels=513))) == 0
    assert supported(pkg, [48, 48, 128, 4, 4, 0, 0, 3]) < 0          # 'concat' view features on summed position features (models.py:186-190)
    assert supported(pkg, geometry_of(shipped), 0) < 0 and supported(pkg, geometry_of(shipped), 16) < 0
    assert pkg.capi.lib().nvsr_generic_fused_supported(None, 3) < 0


def test_generic_route_follows_the_handle_the_gradient_mode_and_the_capacity(pkg, monkeypatch):
    monkeypatch.delenv("NVSR_GENERIC_FUSED", raising=False)
    m = pkg.models.TwoDimPlanesModel(use_viewdirs=True, align_corners=True, skip_connect_every=3, **G18_VARIANTS["avg_mult"])
    assert not m.is_native_geometry()
    with torch.no_grad():
        assert m.generic_route() == "fused"
        monkeypatch.setenv("NVSR_GENERIC_FUSED", "0")
        assert m.generic_route() == "layered"                                          # read at every call
        monkeypatch.setenv("NVSR_GENERIC_FUSED", "1")
        assert m.generic_route() == "fused"
    monkeypatch.delenv("NVSR_GENERIC_FUSED")
    with torch.enable_grad():
        assert m.generic_route() == "layered"                                          # the decoder's parameters take gradients: a graph
        for p in m.parameters():
            p.requires_grad_(False)
        assert m.generic_route() == "fused"                                            # gradients on, nothing involved requires them
    # wider than the widths at which the fused route was measured faster: within the capacity, taken only on request
    wide = pkg.models.TwoDimPlanesModel(use_viewdirs=True, align_corners=True, skip_connect_every=3, **G18_VARIANTS["wide256"])
    assert supported(pkg, wide.generic_geometry()) == 1 and wide.dec_channels > wide.GENERIC_FUSED_DEFAULT_MAX_HIDDEN
    with torch.no_grad():
        assert wide.generic_route() == "layered"
        monkeypatch.setenv("NVSR_GENERIC_FUSED", "1")
        assert wide.generic_route() == "fused"
        monkeypatch.delenv("NVSR_GENERIC_FUSED")
    big = pkg.models.TwoDimPlanesModel(use_viewdirs=True, align_corners=True, dec_channels=4096, dec_density_layers=1, dec_rgb_layers=1,
                                       proj_combination="sum")
    with torch.no_grad():
        assert big.generic_route() == "layered"
        monkeypatch.setenv("NVSR_GENERIC_FUSED", "1")
        assert big.generic_route() == "layered"                                        # beyond the capacity: no handle changes that
    assert torch.cuda.is_available() or not torch.cuda.is_initialized()
