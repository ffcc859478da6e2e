"""CPU tests of the fused TRAINING route of the generic decoder geometries (csrc/generic_fused_bwd.hip): the capacity rule
nvsr_generic_backward_fused_supported, the routing decision TwoDimPlanesModel.generic_train_route(), and the float64 helper
tests/generic_train_ref.py against the reference's own autograd (g19).  None touches a GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import load_golden
from test_generic_fused_host import geometry_of, supported as fwd_supported
from test_oracle import G18_VARIANTS, G22_KW, g18_variant

import generic_train_ref


@pytest.fixture(scope="module")
def pkg():
    import nvsr_amd

    nvsr_amd.build_extension()
    return nvsr_amd


def supported(pkg, geometry, n_pos=3):
    geo = pkg.capi.DecoderGeometry(*geometry)
    return pkg.capi.lib().nvsr_generic_backward_fused_supported(C.byref(geo), n_pos)


SHIPPED = dict(proj_combination="avg", viewdir_proj_combination="concat_pos")


def test_capacity_on_the_geometries_of_the_forward_kernel(pkg):
    """the row of the backward is Kr + Kd + hidden + 4 + (density_layers + rgb_layers) ceil(hidden / 32) floats, rounded up to 2 x an odd
    number, at most 1280 (32 rows in 160 KB) -- include/nvsr.h; every answer below follows from that sum"""
    for name, kw in G18_VARIANTS.items():
        assert supported(pkg, geometry_of(dict(dict(skip_connect_every=3), **kw))) == 1, name
    for hidden in (64, 128):
        for n_pos in (3, 4, 5):
            assert supported(pkg, geometry_of(dict(G22_KW, dec_channels=hidden)), n_pos) == 1, (hidden, n_pos)
    assert supported(pkg, geometry_of(dict(SHIPPED, dec_channels=256))) == 1             # 192 + 48 + 256 + 4 + 64 = 564
    assert supported(pkg, geometry_of(dict(SHIPPED, dec_channels=257))) == 0             # one past the widest layer either kernel holds
    assert supported(pkg, geometry_of(dict(SHIPPED, dec_channels=4096))) == 0
    assert supported(pkg, geometry_of(dict(proj_combination="sum", num_plane_channels=512))) == 1      # 512 + 512 + 128 + 4 + 32 = 1188 -> 1190
    assert supported(pkg, geometry_of(dict(proj_combination="sum", num_plane_channels=513))) == 0      # max(Kd, Kr) = 513
    # within the forward's capacity, beyond the backward's: 512 + 512 + 256 + 4 + 64 = 1348 floats
    wide = geometry_of(dict(proj_combination="sum", num_plane_channels=512, dec_channels=256))
    assert fwd_supported(pkg, wide) == 1 and supported(pkg, wide) == 0
    assert supported(pkg, [48, 48, 128, 4, 4, 0, 0, 3]) < 0          # 'concat' view features on summed position features (models.py:186-190)
    assert supported(pkg, geometry_of(SHIPPED), 0) < 0 and supported(pkg, geometry_of(SHIPPED), 16) < 0
    assert pkg.capi.lib().nvsr_generic_backward_fused_supported(None, 3) < 0


def test_capacity_is_never_wider_than_the_forward_kernels(pkg):
    rng = np.random.default_rng(5)
    seen = set()
    for _ in range(400):
        proj = int(rng.integers(0, 3))
        view = int(rng.choice([3, 4] if proj == 2 else [0, 1, 2, 4]))
        c = int(rng.choice([1, 24, 48, 96, 170, 256, 512]))
        geo = [c, c, int(rng.choice([1, 31, 64, 128, 200, 256, 257])), int(rng.integers(1, 65)), int(rng.integers(1, 65)), int(rng.integers(0, 4)), proj, view]
        n_pos = int(rng.integers(1, 16))
        f, b = fwd_supported(pkg, geo, n_pos), supported(pkg, geo, n_pos)
        assert f >= 0 and b in (0, 1) and not (b == 1 and f != 1), (geo, n_pos, f, b)
        seen.add((f, b))
    assert seen == {(0, 0), (1, 0), (1, 1)}


def test_generic_train_route_follows_the_graph_the_decoder_the_mode_the_handle_and_the_capacity(pkg, monkeypatch):
    monkeypatch.delenv("NVSR_GENERIC_TRAIN_FUSED", raising=False)
    monkeypatch.delenv("NVSR_GENERIC_FUSED", raising=False)
    monkeypatch.delenv("NVSR_DETERMINISTIC", raising=False)
    sid = "lego_DS8_PlRes10_6"

    def model(**kw):
        m = pkg.models.TwoDimPlanesModel(use_viewdirs=True, align_corners=True, **kw)
        c = kw.get("num_plane_channels", 48)
        m.planes_ = torch.nn.ParameterDict({pkg.models.get_plane_name(sid, d): torch.nn.Parameter(torch.zeros(1, c, 4, 4)) for d in range(4)})
        m.set_cur_scene_id(sid)
        return m.train()

    m = model(skip_connect_every=3, **G18_VARIANTS["avg_mult"])
    assert not m.is_native_geometry()
    monkeypatch.setenv("NVSR_GENERIC_TRAIN_FUSED", "1")
    assert m.generic_train_route() == "layered"                    # a decoder parameter requires a gradient
    assert m.generic_route() == "layered"
    for p in m.decoder_parameters():
        p.requires_grad_(False)
    assert m.generic_train_route() == "fused"                      # only the planes require gradients, the geometry fits, the handle is 1
    assert m.generic_route() == "layered"                          # ... and generic_route() answers as ever while a graph is recorded
    with torch.no_grad():
        assert m.generic_train_route() == "layered"                # gradients off: nothing to train
        assert m.generic_route() == "fused"
    with pkg.capi.deterministic_scope(True):
        assert m.generic_train_route() == "layered"                # (the layered route refuses there, in front of any launch)
    monkeypatch.setenv("NVSR_GENERIC_TRAIN_FUSED", "0")
    assert m.generic_train_route() == "layered"                    # read at every call
    monkeypatch.delenv("NVSR_GENERIC_TRAIN_FUSED")
    span = m.GENERIC_TRAIN_FUSED_DEFAULT_HIDDEN                    # the default: the measured widths, nowhere above 128 unless measured
    assert m.generic_train_route() == ("fused" if span is not None and span[0] <= 64 <= span[1] else "layered")
    monkeypatch.setenv("NVSR_GENERIC_TRAIN_FUSED", "1")
    next(iter(m.decoder_parameters())).requires_grad_(True)
    assert m.generic_train_route() == "layered"                    # one parameter is enough
    for p in m.planes_.values():
        p.requires_grad_(False)
    for p in m.decoder_parameters():
        p.requires_grad_(False)
    assert m.generic_train_route() == "layered"                    # nothing requires a gradient: no graph
    big = model(dec_channels=4096, dec_density_layers=1, dec_rgb_layers=1, proj_combination="sum")
    for p in big.decoder_parameters():
        p.requires_grad_(False)
    assert big.generic_train_route() == "layered"                  # beyond the capacity: no handle changes that
    assert torch.cuda.is_available() or not torch.cuda.is_initialized()


def test_float64_helper_against_the_references_autograd():
    """tests/generic_train_ref.py against g19 -- the reference's own float32 autograd -- on the five geometries that carry a cotangent: the
    relative L2 distance of the four plane gradients.  Measured here (float32 rounding of the reference, the helper is float64):
        sum_sum 4.12e-7 .. 4.67e-7, avg_mult 3.75e-7 .. 4.87e-7, concat24 4.42e-7 .. 4.80e-7, skip2 3.74e-7 .. 4.25e-7,
        deep5_c24 3.90e-7 .. 4.13e-7;
    asserted at 2 x the largest of them, 4.87e-7, rounded up: 1e-6; the outputs within the project's bound for the forward."""
    g, gg = load_golden("g18_decoder_variants.npz"), load_golden("g19_decoder_variant_grads.npz")
    names = [n for n in G18_VARIANTS if n + ".gout" in gg]
    assert len(names) == 5
    for name in names:
        kw, sd, planes = g18_variant(g, name)
        out, grads = generic_train_ref.plane_gradients(sd, planes, g["box"], g[name + ".x"], gg[name + ".gout"], **kw)
        ref = g[name + ".out"]
        np.testing.assert_allclose(out, ref, rtol=0, atol=2e-5 * max(1.0, float(np.abs(ref).max())), err_msg=name)
        for d in range(4):
            refp = gg[name + ".gplane%d" % d]
            assert grads[d].shape == refp.shape
            err = generic_train_ref.rel_l2(refp, grads[d])
            print("%s plane %d: %.3g" % (name, d, err))
            assert err < 1e-6, (name, d, err)
