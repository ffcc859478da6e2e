"""CPU checks of tests/triplane_checks.py, the float64 references behind tests/test_triplane_training_edges.py: the manual backward chain and
the per-texel scatter equal torch autograd through the helper's own float64 forward (grid_sample in double, align_corners=True,
padding_mode='border'), the gate words round-trip, and the inputs of every GPU case have exact taps."""
import numpy as np
import pytest
import torch

import triplane_checks as tc


@pytest.mark.parametrize("N,S,sizes,sort", [(3, 5, tc.SIZES[0], True), (2, 7, tc.SIZES[1], False)])
def test_manual_chain_and_scatter_equal_autograd(N, S, sizes, sort):
    scene = tc.make_scene(sizes)
    rays, z = tc.make_rays(N, S, seed=N, exact=True, sort=sort)
    tc.assert_exact_taps(rays, z, scene)
    dec = tc.unpack(tc.make_decoder(3))
    planes = [torch.as_tensor(p).double().requires_grad_(True) for p in tc.make_planes(scene, 4)]
    g = torch.as_tensor(tc.spread_g_raw(N, S, 5)).reshape(-1, 4)
    raw, Hd, Hr = tc.forward64(dec, planes, rays, z, scene)
    (raw * g.double()).sum().backward()
    assert 0.2 < float((Hd > 0).double().mean()) < 0.8 and 0.2 < float((Hr > 0).double().mean()) < 0.8
    gates = tc.gate_words(Hd.detach(), Hr.detach())
    assert torch.equal(tc.gates_to_masks(gates, N * S), torch.cat([Hd, Hr]).detach().gt(0).double())
    Gd0, Ed0, Gr0, Er0, _, _ = tc.chain_from_gates("f32", dec, g, gates)
    gF, E = tc.feature_gradients("f32", dec, Gd0, Gr0, Ed0, Er0)
    taps = tc.taps_to(tc.all_taps(rays, z, scene, exact=True), "cpu")
    # the manual features equal grid_sample's
    f, _, _ = tc.blend([p.detach() for p in planes], taps)
    x = torch.cat(f, 1)
    for l in range(4):
        x = torch.relu(x @ dec.Wr[l].T + dec.br[l])
    assert float((x - Hr[3].detach()).abs().max()) <= 1e-12 * max(1.0, float(x.abs().max()))
    for d in range(4):
        zero = torch.zeros(scene.ph[d] * scene.pw[d] * tc.C, dtype=torch.float64)
        ref, bound, touched, _ = tc.scatter_reference(zero, taps[d], gF[d], E[d])
        want = planes[d].grad.reshape(-1, tc.C)
        scale = float(want.abs().max())
        assert scale > 0 and float((ref - want).abs().max()) <= 1e-12 * scale, d
        assert bool((want[~touched] == 0).all()) and bool((bound >= 0).all())


def test_every_case_has_exact_taps_where_it_claims_them():
    ids = set()
    for c in tc.cases():
        scene, planes, rays, z, g = tc.case_inputs(c)                     # (asserts the exactness of the exact cases)
        assert g.shape == (c.N, c.S, 4) and np.isfinite(g).all() and float(np.abs(g).max()) < 2.0 ** 40
        assert np.abs(np.linalg.norm(rays[:, 8:11], axis=1) - 1).max() < 1e-6
        ids.add(tc.case_id(c))
    assert len(ids) == len(tc.cases())
    # the exactness the issue states, at the widths it lists
    rays, z = tc.make_rays(64, 33, seed=9)
    for W in (1, 2, 3, 7, 12, 17, 40, 56, 200, 800):
        assert 0.05 < tc.assert_exact_taps(rays, z, tc.make_scene([(W, W), (3, W), (W, 5), (2, 2)])) < 0.25 or W == 1
    # and ordinary coordinates are not exact
    rays, z = tc.make_rays(64, 33, seed=9, exact=False)
    with pytest.raises(AssertionError):
        tc.assert_exact_taps(rays, z, tc.make_scene(tc.SIZES[0]))


def test_tap_error_terms():
    s = tc.make_scene(tc.SIZES[2])
    assert tc.view_tap_error(s) == 2 * tc.U                               # a single view texel: no coordinate error
    s = tc.make_scene(tc.SIZES[0])
    assert 2 * tc.U < tc.view_tap_error(s) < 200 * tc.U                   # 9 x 9: hx = 4
    rays, z = tc.make_rays(8, 5, seed=1, exact=False)
    e = tc.pos_tap_error(rays, z, tc.make_scene(tc.RANDOM_SIZES), 0)
    assert e.shape == (8, 5) and float(e.max()) < 4000 * tc.U
    # the f32 restatement of ordinary coordinates stays within that bound of the float64 one
    sc = tc.make_scene(tc.RANDOM_SIZES)
    a, b = tc.position_taps(rays, z, sc, 0, np.float32), tc.position_taps(rays, z, sc, 0, np.float64)
    same = a.idx == b.idx
    assert float((np.abs(a.w - b.w) * same).max(-1).max()) <= float(e.max())


def test_pow2_undo_follows_the_kernel():
    m = np.float32([0.0, 1e-45, 1.0, 8.0, 15.9, 16.0, 2e-38, 3e38, np.inf])
    un = tc.pow2_undo(m)
    assert un[0] == un[1] == un[8] == 2.0 ** -3                           # e == 0 / 255: eu = 127 - UP
    assert un[2] == 2.0 ** -3 and un[3] == 1.0 and un[4] == 1.0 and un[5] == 2.0
    assert un[6] == 2.0 ** (4 - 127 - 3) and un[7] == 2.0 ** (253 - 127 - 3)
