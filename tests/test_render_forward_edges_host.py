"""CPU checks of tests/render_checks.py, the float64 references behind tests/test_render_forward_edges.py: composite64 against the oracle's
independent restatement in C (orc_composite, orc_composite_mip: float32, sequential) under the derived bound plus the rounding of the oracle's
float32 outputs; coarse_depth64 against orc_coarse_z; and the conditions on the inputs of every GPU case, on the float64 reference alone with
forward64's raw standing in for a kernel's: at most 1 % of the elements of any output have a bound wider than include/nvsr.h's tolerance, the
noise-on launches hold empty, partial and full live lists in every workgroup, the knife-edge launch yields all three signs of sn, and the
NaN / inf launch puts its NaNs where the rule says."""
import functools

import numpy as np
import pytest
import torch

import render_checks as rc
import triplane_checks as tc

FUSED = rc.fused_cases()
COMPOSITE = rc.composite_cases()


@functools.lru_cache(maxsize=None)
def _fused(i):
    """case i of the fused kernels -> scene, rays, z, forward64's raw as float32 [N, S, 4]"""
    c = FUSED[i]
    scene, rays, z = rc.make_inputs(c)
    dec = tc.unpack(rc.make_decoder())
    planes = [torch.as_tensor(p).double() for p in rc.make_planes(scene)]
    raw = tc.forward64(dec, planes, rays, z, scene)[0].numpy().reshape(c.N, c.S, 4).astype(np.float32)
    return c, rays, z, raw


def _launches(c, rays, z, raw, mip=False):
    """the launches of the GPU test: (name, noise, white)"""
    on = rc.make_noise(c, raw[..., 3])
    knife, mask = rc.knife_noise(c, raw[..., 3], on, mip)
    nan, where = rc.special_noise(c, z, on)
    return [("plain", None, 0), ("white", None, 1), ("noise", on, 0), ("noise+white", on, 1), ("knife", knife, 0), ("special", nan, 1)], mask, where


def _against_oracle(oracle, tag, raw, z, rd, noise, white, mip):
    ref = rc.composite64(raw, z, rd, noise, white, mip=mip)
    rgb, disp, acc, w, depth = oracle.composite(raw, z, rd, noise=noise, white_background=bool(white), mip_nerf=mip)
    worst = {}
    for name, got in (("weights", w), ("acc", acc), ("depth", depth), ("disp", disp), ("rgb", rgb)):
        v = getattr(ref, name)
        worst[name] = rc.compare(tag, name, got, v, getattr(ref.bound, name) + rc.U * np.abs(v))      # + the oracle's float32 output rounding
    return ref, worst


@pytest.mark.parametrize("i", range(len(FUSED)), ids=[rc.case_id(c) for c in FUSED])
def test_composite64_equals_the_oracle_on_the_fused_cases(oracle, i):
    c, rays, z, raw = _fused(i)
    launches, _, _ = _launches(c, rays, z, raw)
    for name, noise, white in launches:
        _, worst = _against_oracle(oracle, "%s %s" % (rc.case_id(c), name), raw, z, rays[:, 3:6], noise, white, False)
        print("%s %s: oracle err / bound %s" % (rc.case_id(c), name, ", ".join("%s %.3f" % kv for kv in worst.items())))


@pytest.mark.parametrize("mip", [False, True], ids=["plain", "mip"])
@pytest.mark.parametrize("i", range(len(COMPOSITE)), ids=[rc.case_id(c) for c in COMPOSITE])
def test_composite64_equals_the_oracle_on_random_raw(oracle, i, mip):
    c = COMPOSITE[i]
    scene, rays, z = rc.make_inputs(c)
    if mip:
        z = np.concatenate([z, z[:, -1:] + np.float32(0.25)], -1)
    raw = rc.make_raw(c)
    launches, _, where = _launches(c, rays, z[:, :c.S], raw, mip)
    for name, noise, white in launches:
        ref, worst = _against_oracle(oracle, "%s %s" % (rc.case_id(c), name), raw, z, rays[:, 3:6], noise, white, mip)
        share = rc.left_out(ref)
        assert max(share.values()) <= rc.LEFT_OUT_CAP, (name, share)


@pytest.mark.parametrize("lindisp", [0, 1])
@pytest.mark.parametrize("S", [1, 2, 3, 33, 65])
def test_coarse_depth64_equals_the_oracle(oracle, S, lindisp):
    rays = rc.z_rays(np.zeros((293, 11), np.float32), 5)
    assert (rays[:, 6] == rays[:, 7]).any() and rays[:, 6].min() >= 0.5 and rays[:, 7].max() <= 9.0
    z, bound = rc.coarse_depth64(rays[:, 6], rays[:, 7], np.arange(S), S, lindisp)
    got = oracle.coarse_z(rays[:, 6], rays[:, 7], S, lindisp=bool(lindisp)).astype(np.float64)
    assert np.isfinite(bound).all() and bool((bound <= rc.TOLERANCE["depth"] * rays[:, 7:8]).all())
    ratio = np.abs(got - z) / bound
    assert float(ratio.max()) <= 1.0, float(ratio.max())
    # the end points are the ray's own near and far
    if S > 1 and not lindisp:
        assert np.array_equal(got[:, 0], rays[:, 6].astype(np.float64)) and np.array_equal(got[:, -1], rays[:, 7].astype(np.float64))


@pytest.mark.parametrize("i", range(len(FUSED)), ids=[rc.case_id(c) for c in FUSED])
def test_conditions_on_the_inputs_of_the_fused_cases(i):
    c, rays, z, raw = _fused(i)
    tag = rc.case_id(c)
    launches, mask, where = _launches(c, rays, z, raw)
    assert (np.diff(z, axis=-1) == 0).any() or c.S == 1                   # ties: zero-length intervals
    for name, noise, white in launches:
        ref = rc.composite64(raw, z, rays, noise, white)
        share = rc.left_out(ref, far=rays[:, 7])
        print("%s %s: left out %s" % (tag, name, ", ".join("%s %.4f" % kv for kv in share.items())))
        assert max(share.values()) <= rc.LEFT_OUT_CAP, (name, share)
        if name in ("noise", "noise+white"):
            w = ref.weights[rc.ray_class(c.N) != 0]                       # the dictated rays: their lists are the reference's in f32 too
            assert not ((w != 0) & (np.abs(w) < 1e-30)).any(), "%s %s: a weight underflows in f32" % (tag, name)
            rc.assert_live_mix("%s %s" % (tag, name), ref.live, c.S, c.N)
            # a dead sample in the middle of a live list: a zero-length interval between two live samples
            if c.S >= 33:
                w = ref.weights
                assert ((w[:, 1:-1] == 0) & (w[:, :-2] > 0) & (w[:, 2:] > 0)).any(), tag
        if name == "knife":
            sn = ref.sn[mask]
            assert c.N < 8 or ((sn == 0).any() and (sn > 0).any() and (sn < 0).any()), tag
            assert float(np.abs(sn).max()) <= 2.0 ** -18 * max(1.0, float(np.abs(raw[..., 3]).max()))
            if c.N >= 8:
                last = ref.sn[mask[:, -1], -1]                               # the last sample (dist 1e10) of half the rays is on the edge
                assert (last > 0).any() and (last <= 0).any(), tag
                on = mask[:, -1] & (ref.sn[:, -1] * rc.F_1E10 * np.linalg.norm(rays[:, 3:6], axis=1) > 20)
                assert bool((ref.acc[on] > 0.999).all())                    # barely positive times 1e10: opaque
        if name == "special":
            _check_special(tag, c, ref, rc.composite64(raw, z, rays, launches[3][1], 1), where)


def _check_special(tag, c, ref, base, where):
    """the rule, on the reference: NaN noise at (ray, s) -> weights[s:] NaN, weights[:s] those of the launch without it, acc / depth / disp / rgb
    NaN; +inf on a zero-length interval alike (inf * 0); +inf on a positive length: an opaque sample, finite; -inf: a dead sample, finite"""
    nan_rays = set()
    for kind in (5, 6, 7, 2):
        for i, s in where.get(kind, []):
            nan_rays.add(i)
            assert np.isnan(ref.weights[i, s:]).all(), (tag, kind, i)
            assert np.array_equal(ref.weights[i, :s], base.weights[i, :s]), (tag, kind, i)
            for name in ("acc", "depth", "disp"):
                assert np.isnan(getattr(ref, name)[i]), (tag, kind, name, i)
            assert np.isnan(ref.rgb[i]).all(), (tag, kind, i)
    for kind in (1, 3):
        for i, s in where.get(kind, []):
            assert np.isfinite(ref.weights[i]).all() and np.isfinite(ref.rgb[i]).all() and np.isfinite(ref.acc[i]), (tag, kind, i)
            if kind == 3:
                assert ref.weights[i, s] == 0
    others = np.array([i not in nan_rays for i in range(c.N)])
    assert np.isfinite(ref.weights[others]).all() and np.isfinite(ref.acc[others]).all()
    if c.N >= 8:
        assert all(where.get(k) for k in (1, 3, 5, 6, 7)) and (c.S < 2 or where.get(2)), (tag, sorted(where))
    else:
        assert where.get(6), tag
