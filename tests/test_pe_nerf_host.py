"""CPU checks of the positional-encoding NeRF baseline (MipNeRF_baseline.yml with encode_position_fn: positional_encoding; csrc/pe.hip): the
g24 fixture, the C ABI of the new entry points, the model's dimensions and the errors of the geometries the kernels are not built for."""
import sys

import numpy as np
import pytest

from conftest import GOLDEN, load_golden
from nerf_baseline_checks import HOST_SCENE, check_bad_arguments, check_entry_points, check_geometry_refused, host_opts

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)


def test_g24_fixture_keys_and_shapes():
    g = load_golden("g24_pe_nerf.npz")
    n, S = g["a.z"].shape
    assert g["a.rays"].shape == (n, 11) and g["a.enc"].shape == (n * S, 39) and g["a.dirs"].shape == (n * S, 27)
    nn_, S_ = g["a.ndc.z"].shape
    assert g["a.ndc.rays"].shape == (nn_, 11) and g["a.ndc.enc"].shape == (nn_ * S_, 39) and g["a.ndc.dirs"].shape == (nn_ * S_, 27)
    import pe_params
    for i, seed in enumerate(pe_params.SEEDS):
        sd = pe_params.state_dict(seed)
        assert sd["layer1.weight"].shape == (128, 39) and sd["layers_dir.0.weight"].shape == (64, 155)
        assert sum(v.size for v in sd.values()) == 81476
        np.testing.assert_allclose(pe_params.checksum(sd), g["b.m%d.checksum" % i], rtol=1e-12)   # the recipe is the fixture's
        assert g["b.m%d.raw" % i].shape == (n * S, 4) and g["b.m%d.ndc.raw" % i].shape == (nn_ * S_, 4)
        for name, shape in pe_params.SHAPES:
            want = min(int(np.prod(shape)), pe_params.KEEP)
            assert g["d.m%d.grad.%s" % (i, name)].shape == (want,) and g["e.m%d.%s" % (i, name)].shape == (want,)
    for tag in ("c.", "c.ndc."):
        assert g[tag + "z_coarse"].shape == (32, 64) and g[tag + "z_fine"].shape == (32, 128)
        assert g[tag + "rgb_fine"].shape == (256, 3) and g[tag + "acc_coarse"].shape == (256,)
        assert (np.diff(g[tag + "z_fine"], axis=-1) >= 0).all()
    assert g["e.losses"].shape == (3,)
    # the fixture exercises what it claims: degree-5 arguments near 200 rad; the first 3 encoding columns are the points
    assert np.abs(g["a.enc"][:, :3]).max() * 32 > 150
    assert str(g["scene_id"]) == "lego"                                            # (no _DS<d>: PE has no cone radius)


@pytest.fixture(scope="module")
def pkg_capi():
    import nvsr_amd
    return nvsr_amd.capi


def test_header_declares_the_pe_entry_points(pkg_capi):
    check_entry_points(pkg_capi, "pe", (81476, 770, 708))


def test_pe_entry_points_refuse_bad_arguments_without_a_gpu(pkg_capi):
    check_bad_arguments(pkg_capi, "pe")


def test_default_flexible_nerf_is_the_pe_baseline():
    import nvsr_amd
    m = nvsr_amd.models.FlexibleNeRFModel()
    assert (m.dim_xyz, m.dim_dir) == (39, 27) and m.is_pe_baseline() and not m.is_mip_baseline()
    assert m.layer1.in_features == 39 and m.layers_dir[0].in_features == 155
    assert m.natural_blob().numel() == nvsr_amd.capi.PE_NERF_NATURAL_FLOATS
    assert sum(p.numel() for p in m.parameters()) == nvsr_amd.capi.PE_NERF_NATURAL_FLOATS
    assert not nvsr_amd.models.FlexibleNeRFModel(include_input_xyz=False).is_pe_baseline()


@pytest.mark.parametrize("kwargs", [dict(include_input_xyz=False), dict(num_encoding_fn_xyz=5), dict(num_encoding_fn_xyz=10),
                                    dict(num_encoding_fn_dir=3), dict(include_input_dir=False), dict(hidden_size=64), dict(num_layers=6),
                                    dict(skip_connect_every=2)])
def test_unsupported_pe_geometries_raise_before_gpu_work(kwargs):
    """any FlexibleNeRFModel geometry other than the shipped one is refused under positional_encoding, coarse or fine, before the rays are
    packed (these are CPU models and CPU rays: reaching a kernel would fail differently)"""
    import torch
    import nvsr_amd
    bad = nvsr_amd.models.FlexibleNeRFModel(**kwargs)
    check_geometry_refused(nvsr_amd.models.FlexibleNeRFModel(), bad, "positional_encoding", "lego", "positional-encoding")
    with pytest.raises(NotImplementedError, match="positional-encoding"):
        bad.pe_forward(torch.zeros(2, 11), torch.zeros(2, 4))


def test_flexible_nerf_without_an_encoding_still_raises():
    import torch
    import nvsr_amd
    m = nvsr_amd.models.FlexibleNeRFModel()
    with pytest.raises(NotImplementedError, match="positional-encoding"):
        nvsr_amd.train_utils.run_one_iter_of_nerf(4, 4, 2.0, m, m, torch.zeros(2, 4, 3), host_opts(None), "lego", mode="validation",
                                                  scene_config=HOST_SCENE)
