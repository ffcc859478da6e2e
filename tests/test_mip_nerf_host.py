"""CPU checks of the Mip-NeRF baseline (MipNeRF_baseline.yml; csrc/mip.hip): the g23 fixture, the C ABI of the new kernels, the model's
dimensions and the errors of the configurations it does not run."""
import sys

import numpy as np
import pytest

from conftest import GOLDEN, load_golden
from nerf_baseline_checks import HOST_SCENE, check_bad_arguments, check_entry_points, check_geometry_refused, host_opts

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)


def test_g23_fixture_keys_and_shapes():
    g = load_golden("g23_mip_nerf.npz")
    n, S1 = g["a.edges"].shape
    S = S1 - 1
    assert g["a.rays"].shape == (n, 11)
    assert g["a.means"].shape == (n, S, 3) and g["a.covs"].shape == (n, S, 3)
    assert g["a.ipe"].shape == (n * S, 36) and g["a.dirs"].shape == (n * S, 27)
    import mip_params
    assert mip_params.SEEDS == (101, 202)
    for i, seed in enumerate(mip_params.SEEDS):
        sd = mip_params.state_dict(seed)
        assert sd["layer1.weight"].shape == (128, 36) and sd["layers_dir.0.weight"].shape == (64, 155)
        assert sum(v.size for v in sd.values()) == 81092
        flat = np.concatenate([v.reshape(-1).astype(np.float64) for v in sd.values()])
        np.testing.assert_allclose([flat.sum(), (flat * flat).sum()], g["b.m%d.checksum" % i], rtol=1e-12)   # the recipe is the fixture's
        np.testing.assert_array_equal(mip_params.checksum(sd), [flat.sum(), (flat * flat).sum()])
        assert g["b.m%d.raw" % i].shape == (n * S, 4)
        for name, shape in mip_params.SHAPES:
            want = min(int(np.prod(shape)), mip_params.KEEP)
            assert g["d.m%d.grad.%s" % (i, name)].shape == (want,) and g["e.m%d.%s" % (i, name)].shape == (want,)
    for tag in ("c.", "c.ndc."):
        assert g[tag + "edges_coarse"].shape == (32, 65) and g[tag + "edges_fine"].shape == (32, 65 + 65)
        assert g[tag + "rgb_fine"].shape == (256, 3) and g[tag + "acc_coarse"].shape == (256,)
    assert g["e.losses"].shape == (3,)
    assert abs(float(g["radius"]) - 8 * 0.00135 * 2 / np.sqrt(12.0)) < 1e-15
    # the fixture exercises what it claims: degree-5 arguments above 100 rad, a near-axis direction, intervals of 1e-5
    assert np.abs(g["a.means"]).max() * 32 > 100
    assert np.diff(g["a.edges"][2]).max() < 2e-5


@pytest.fixture(scope="module")
def pkg_capi():
    import nvsr_amd
    return nvsr_amd.capi


def test_header_declares_the_mip_entry_points(pkg_capi):
    check_entry_points(pkg_capi, "mip", (81092, 767, 708))


def test_mip_entry_points_refuse_bad_arguments_without_a_gpu(pkg_capi):
    check_bad_arguments(pkg_capi, "mip")


def test_flexible_nerf_without_input_xyz_has_the_baseline_dimensions():
    import nvsr_amd
    m = nvsr_amd.models.FlexibleNeRFModel(include_input_xyz=False)
    assert (m.dim_xyz, m.dim_dir) == (36, 27) and m.is_mip_baseline() and not m.is_pe_baseline()
    assert m.layer1.in_features == 36 and m.layers_dir[0].in_features == 155
    assert m.natural_blob().numel() == nvsr_amd.capi.MIP_NERF_NATURAL_FLOATS
    assert sum(p.numel() for p in m.parameters()) == nvsr_amd.capi.MIP_NERF_NATURAL_FLOATS


def test_mip_radius_from_the_scene_id():
    import nvsr_amd
    assert nvsr_amd.train_utils.mip_radius("lego_DS8") == 8 * 0.00135 * 2 / np.sqrt(12.0)
    assert nvsr_amd.train_utils.mip_radius("ship_DS12") == 12 * 0.00135 * 2 / np.sqrt(12.0)
    for bad in ("lego", "lego_DS8_PlRes32", "lego_DS"):
        with pytest.raises(ValueError, match="_DS"):
            nvsr_amd.train_utils.mip_radius(bad)


def test_unsupported_configurations_raise_clearly():
    """positional-encoding NeRF is refused before any GPU work; so is a Mip-NeRF scene id without _DS<d> (before the rays are packed)"""
    import torch
    import nvsr_amd
    tu = nvsr_amd.train_utils
    m = nvsr_amd.models.FlexibleNeRFModel(include_input_xyz=False)
    rays = torch.zeros(2, 4, 3)
    with pytest.raises(NotImplementedError, match="positional-encoding"):
        tu.run_one_iter_of_nerf(4, 4, 2.0, m, m, rays, host_opts("positional_encoding"), "lego_DS8", mode="validation", scene_config=HOST_SCENE)
    with pytest.raises(ValueError, match="_DS"):
        tu.run_one_iter_of_nerf(4, 4, 2.0, m, m, rays, host_opts("mip"), "lego", mode="validation", scene_config=HOST_SCENE)


@pytest.mark.parametrize("kwargs", [dict()] + [dict(include_input_xyz=False, **kw) for kw in (
    dict(num_encoding_fn_xyz=5), dict(num_encoding_fn_xyz=10), dict(num_encoding_fn_dir=3), dict(include_input_dir=False), dict(hidden_size=64),
    dict(num_layers=6), dict(skip_connect_every=2))])
def test_unsupported_mip_geometries_raise_before_gpu_work(kwargs):
    """any FlexibleNeRFModel geometry other than the shipped one (dict(): the default model, PE's geometry) is refused under mip, coarse or
    fine, before the rays are packed and before any coarse depths exist; mip_forward refuses it too"""
    import torch
    import nvsr_amd
    bad = nvsr_amd.models.FlexibleNeRFModel(**kwargs)
    check_geometry_refused(nvsr_amd.models.FlexibleNeRFModel(include_input_xyz=False), bad, "mip", "lego_DS8", "Mip-NeRF")
    with pytest.raises(NotImplementedError, match="Mip-NeRF"):
        bad.mip_forward(torch.zeros(2, 11), torch.zeros(2, 5), 0.001)
