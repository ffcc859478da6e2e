"""CPU tests of the low-rank feature planes: the rank formula, the operators' fake implementations, load_scene's wiring and error paths, the
model's path up to the first GPU tensor, and the fixture g26 against the forward bound."""
import os

import numpy as np
import pytest
import torch

import lowrank_checks as lc
from conftest import load_golden


@pytest.fixture(scope="module")
def pkg():
    import nvsr_amd

    nvsr_amd.build_extension()
    return nvsr_amd


def test_plane_rank_dict_is_the_reference_formula(pkg):
    ps, M = pkg.plane_store, pkg.models
    for R in (12, 200, 800):
        for ratio in (0.05, 0.1, 1.0):
            sid = M.get_scene_id("lego", 8, (R, 32))
            d = ps.plane_rank_dict({sid: (R, 32)}, ratio, 3)
            assert d == {M.get_plane_name(sid, k): int(np.ceil(ratio * R)) for k in range(3)}, (R, ratio, d)
            assert M.get_plane_name(sid, 3) not in d, "the view-direction plane is never low-rank"
    assert ps.plane_rank_dict({"s": (12, 6)}, None, 3) is None
    assert ps.plane_rank_dict({"a_PlRes12_6": (12, 6), "b_PlRes800_32": (800, 32)}, 0.1, 2) == {
        "sca_PlRes12_6_D0": 2, "sca_PlRes12_6_D1": 2, "scb_PlRes800_32_D0": 80, "scb_PlRes800_32_D1": 80}
    assert list(ps.plane_rank_dict({"s": (200, 32)}, 0.1, 3).values()) == lc.rank_dict_ref([200] * 3, 0.1) == [20, 20, 20]


def test_fake_tensor_shapes_and_strides(pkg):
    from torch._subclasses.fake_tensor import FakeTensorMode

    with FakeTensorMode():
        fs = [torch.empty(1, 48, 12, 6, device="cuda"), torch.empty(1, 48, 17, 34, device="cuda")]
        planes = torch.ops.nvsr.lowrank_planes(fs, [3, 17])
        assert [tuple(p.shape) for p in planes] == [(1, 48, 12, 12), (1, 48, 17, 17)]
        assert [p.stride() for p in planes] == [(48 * 144, 1, 48 * 12, 48), (48 * 289, 1, 48 * 17, 48)]       # torch.channels_last
        assert all(p.dtype == torch.float32 and pkg.models.is_native_layout(p) for p in planes)
        for grads in (planes, [torch.empty(1, 48, 12, 12, device="cuda"), torch.empty(1, 48, 17, 17, device="cuda")]):
            ds = torch.ops.nvsr.lowrank_planes_backward(grads, fs, [3, 17])
            assert [tuple(d.shape) for d in ds] == [tuple(f.shape) for f in fs] and all(d.is_contiguous() for d in ds)
        out = torch.ops.nvsr.lowrank_planes([f.requires_grad_() for f in fs], [3, 17])
        assert all(o.requires_grad for o in out), "autograd is registered"
        with pytest.raises(Exception, match="rank"):
            torch.ops.nvsr.lowrank_planes(fs, [3, 4])
    assert "lowrank_planes" in pkg.ops.FORWARD_OPS


def test_bad_calls_return_the_status_and_do_not_launch(pkg):
    capi = pkg.capi
    a = capi.LowrankPlanesArgs()
    a.channels = 48
    for n in (0, 16):
        a.num_planes = n
        assert capi.lib().nvsr_lowrank_planes(a, None) == 1 and capi.lib().nvsr_lowrank_planes_backward(a, None) == 1      # NVSR_ERR_SHAPE
    a.num_planes, a.res[0], a.rank[0] = 1, 8, 0
    assert capi.lib().nvsr_lowrank_planes(a, None) == 1
    a.res[0], a.rank[0] = 0, 2
    assert capi.lib().nvsr_lowrank_planes(a, None) == 1
    a.res[0], a.channels = 8, 0
    assert capi.lib().nvsr_lowrank_planes(a, None) == 1
    a.channels = 48
    assert capi.lib().nvsr_lowrank_planes(a, None) == 3                                                                        # NVSR_ERR_NULL


def _write_scene(pkg, tmp_path, sid, shapes):
    planes = {pkg.models.get_plane_name(sid, d): torch.randn(*s) for d, s in enumerate(shapes)}
    os.makedirs(tmp_path / "planes", exist_ok=True)
    box = torch.tensor([[-4.0, -4, -4, -np.pi, -np.pi / 2], [4, 4, 4, np.pi, np.pi / 2]], dtype=torch.float64)
    pkg.plane_store.save_plane_file(pkg.plane_store.plane_file(str(tmp_path / "planes"), sid), planes, box)
    return planes


def _models(pkg):
    kw = dict(use_viewdirs=True, skip_connect_every=3, proj_combination="avg", viewdir_proj_combination="concat_pos", align_corners=True)
    mc = pkg.models.TwoDimPlanesModel(**kw)
    return mc, pkg.models.TwoDimPlanesModel(num_planes_or_rot_mats=mc.rot_mats(), **kw)


def test_load_scene_wires_ranks_and_refuses_wrong_factor_shapes(pkg, tmp_path):
    ps, M = pkg.plane_store, pkg.models
    sid = "lego_DS8_PlRes12_6"
    saved = _write_scene(pkg, tmp_path, sid, [(1, 48, 12, 4), (1, 48, 12, 4), (1, 48, 12, 4), (1, 48, 6, 6)])
    mc, mf = _models(pkg)
    ps.load_scene([mc, mf], str(tmp_path / "planes"), sid, device="cpu", planes_rank_ratio=0.1)       # ceil(1.2) = 2
    names = [M.get_plane_name(sid, d) for d in range(4)]
    assert mc.plane_rank == mf.plane_rank == {n: 2 for n in names[:3]}
    assert mc.generated_planes is mf.generated_planes and mc.generated_planes == {}
    assert mc.planes_ is mf.planes_ and all(torch.equal(mc.planes_[n].detach(), saved[n]) for n in names), "factors are stored and loaded as they are"
    assert tuple(M.create_plane([12, 4], 48, 0.1).shape) == (1, 48, 12, 4)
    # the view-direction plane is used as stored, on any device; a low-rank plane needs the GPU: the path runs up to that point
    assert mc.gen_plane(names[3]) is mc.planes_[names[3]]
    with pytest.raises(pkg.capi.NvsrError, match="GPU only"):
        mc._plane_source(0)
    # explicit ranks; a rank the file's factors do not have names the plane
    ps.load_scene([mc, mf], str(tmp_path / "planes"), sid, device="cpu", plane_rank={names[0]: 2, names[1]: 2})
    assert mc._rank_of(names[2]) is None and mc.gen_plane(names[2]) is mc.planes_[names[2]]
    with pytest.raises(ValueError, match=names[1]):
        ps.load_scene([mc, mf], str(tmp_path / "planes"), sid, device="cpu", plane_rank={names[0]: 2, names[1]: 3})
    with pytest.raises(ValueError, match=names[0]):
        ps.load_scene([mc, mf], str(tmp_path / "planes"), sid, device="cpu", planes_rank_ratio=0.5)
    with pytest.raises(ValueError, match="not both"):
        ps.load_scene([mc, mf], str(tmp_path / "planes"), sid, device="cpu", planes_rank_ratio=0.1, plane_rank={names[0]: 2})
    with pytest.raises(ValueError, match="PlRes"):
        _write_scene(pkg, tmp_path, "lego_DS8", [(1, 48, 12, 4)] * 3 + [(1, 48, 6, 6)])
        ps.load_scene([mc, mf], str(tmp_path / "planes"), "lego_DS8", device="cpu", planes_rank_ratio=0.1)
    # the height must be the resolution the scene id names
    _write_scene(pkg, tmp_path, "lego_DS8_PlRes20_6", [(1, 48, 12, 4)] * 3 + [(1, 48, 6, 6)])
    with pytest.raises(ValueError, match="resolution 20"):
        ps.load_scene([mc, mf], str(tmp_path / "planes"), "lego_DS8_PlRes20_6", device="cpu", planes_rank_ratio=0.1)


def test_plane_rank_no_longer_refused_and_hr_planes_still_are(pkg):
    mc, _ = _models(pkg)
    sid = "lego_DS8_PlRes12_6"
    mc.plane_rank = {pkg.models.get_plane_name(sid, 0): 3}
    mc._refuse_plane_downsampling(pkg.models.get_plane_name(sid, 0))            # (raised NotImplementedError before)
    with pytest.raises(NotImplementedError, match="HR_planes"):
        mc.raw_plane(pkg.models.get_plane_name(sid, 0), downsample=True)
    # a model without the two attributes has the defaults
    assert mc._rank_of("x") is None and mc._generated_dict() is pkg.models._GENERATED_PLANES


def test_fixture_generated_planes_meet_the_forward_bound():
    """the reference's own CPU matmul against float64 of the same factors: pins the bound and the fixture"""
    g = load_golden("g26_lowrank.npz")
    assert list(g["ranks"]) == [3, 5, 12] and os.path.getsize(os.path.join(os.path.dirname(__file__), "golden", "g26_lowrank.npz")) < 1 << 20
    for d in range(3):
        r = int(g["ranks"][d])
        assert g["plane%d" % d].shape == (1, 48, 12, 2 * r) and g["grad_plane%d" % d].shape == g["plane%d" % d].shape
        worst = lc.check_plane(torch.from_numpy(g["generated%d" % d]), torch.from_numpy(g["plane%d" % d]), r, "g26 plane %d" % d)
        print("g26 plane %d: the reference's worst err / bound %.3f" % (d, worst))
        assert float((g["grad_plane%d" % d] != 0).mean()) > 0.5
    assert g["plane3"].shape == (1, 48, 6, 6) and float(g["rgb_fine"].std()) > 0.05
    dec = lc.g26_decoders(g, load_golden("g11_grads.npz"))          # (asserts that g11 is still the file g26 was generated from)
    assert dec["coarse.fc_alpha.0.weight"].shape == (1, 128) and not np.array_equal(dec["fine.fc_alpha.0.bias"], load_golden("g11_grads.npz")["fine.fc_alpha.0.bias"])
