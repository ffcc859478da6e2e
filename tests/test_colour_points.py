"""GPU tests (-m gpu) of the point-major colour pass (csrc/colour_order.hip: point_order_kernel; csrc/render3.hip: PHASE 3 of render_pass3_body;
include/nvsr.h "The two-phase render pass").

(a) the order kernel alone (nvsr_internal_point_order) against the numpy reference (colour_points_ref.py; itself checked on the CPU by
    test_colour_points_host.py), array for array;
(b) the render pass: the point-major route (the default, NVSR_COLOUR_POINTS=1) against the fused kernel (NVSR_RENDER_ONE_PHASE=1) and against
    the lockstep colour kernels (NVSR_COLOUR_POINTS=0), bit for bit, NaNs in the same places."""
import numpy as np
import pytest
import torch

from colour_order_ref import ORDER_RAYS, ORDER_SHIFT, order_reference
from colour_points_ref import GROUP, POINT_NONE, bands_of_depths, bands_of_indices, check_points, point_order_reference
from two_phase_checks import ARITHS, DEV, N_RAYS, OUTPUTS, _counts_and_noise, _pass, _same, _scene

pytestmark = pytest.mark.gpu

N_SMALL = ORDER_RAYS + 513      # two blocks of the ray order, 19 groups, a ragged last group (one ray)


# ---- (a) the order kernel alone ---------------------------------------------------------------------------------------------------------
def _dictated_counts(N, S, rng):
    """counts per SLOT (the entries name their own slot): group 1 empty, group 2 a total that is a multiple of 256, group 3 exactly one live
    point, slot 5 with all S live; the rest random"""
    c = rng.integers(0, S + 1, N)
    c[GROUP:2 * GROUP] = 0
    c[2 * GROUP:3 * GROUP] = min(S, 2)
    c[3 * GROUP:4 * GROUP] = 0
    c[3 * GROUP + 77] = 1
    c[5] = S
    return c


def _run_order(hip, packed, lists, rays, N, S, nb):
    G = (N + GROUP - 1) // GROUP
    guard = 64
    e = torch.from_numpy(packed.astype(np.int32)).to(DEV)
    l = torch.from_numpy(lists).to(DEV).contiguous()
    r = None if rays is None else torch.from_numpy(rays).to(DEV).contiguous()
    pts = torch.full((G * GROUP * S + guard,), -7, dtype=torch.int32, device=DEV)
    steps = torch.full((G + guard,), -7, dtype=torch.int32, device=DEV)
    offs = torch.full((G + guard,), -7, dtype=torch.int32, device=DEV)
    assert hip.capi.lib().nvsr_internal_point_order(e.data_ptr(), l.data_ptr(), None if r is None else r.data_ptr(), N, S, nb, pts.data_ptr(),
                                                   steps.data_ptr(), offs.data_ptr(), hip.capi.stream()) == 0
    torch.cuda.synchronize()
    pts, steps, offs = pts.cpu().numpy(), steps.cpu().numpy(), offs.cpu().numpy()
    assert np.all(pts[G * GROUP * S:] == -7) and np.all(steps[G:] == -7) and np.all(offs[G:] == -7)      # nothing behind the arrays
    return pts[:G * GROUP * S].reshape(G, GROUP * S), steps[:G], offs[:G]


def _compare(got, want, steps_want, S):
    """the entries of every step the group runs; behind them the buffer is the caller's"""
    for g in range(want.shape[0]):
        n = steps_want[g] * GROUP
        assert np.array_equal(got[g, :n], want[g, :n]), g


@pytest.mark.parametrize("S", [1, 8, 24])
def test_point_order_kernel_equals_the_numpy_reference(hip, S):
    N = N_SMALL
    product = hip.capi.lib().nvsr_internal_point_bands()
    assert product == 0 or product in (4, 8, 16)
    rng = np.random.default_rng(500 + S)
    count = _dictated_counts(N, S, rng)
    identity = (count << ORDER_SHIFT) | (np.arange(N) % ORDER_RAYS)
    ordered = order_reference(count, S, hip.capi.lib().nvsr_internal_colour_order_bins())
    # lists of sample indices (the pass with its depths in registers): c_i sorted indices out of 0..S-1, the rest of the row poisoned
    rank = np.argsort(np.argsort(rng.random((N, S)), 1), 1)
    idx = np.sort(np.where(rank < count[:, None], np.arange(S)[None, :], 1 << 20), 1)
    # lists of depths over near..far = 2..6 (some at and beyond the ends: the clamp), the rest of the row NaN
    z = np.sort(rng.uniform(1.9, 6.1, (N, S)).astype(np.float32), 1)
    z[np.arange(S)[None, :] >= count[:, None]] = np.nan
    rays = np.zeros((N, 11), np.float32)
    rays[:, 6], rays[:, 7] = 2.0, 6.0
    for nb in sorted({product, 4, 16, 0}):
        nbands = nb if 1 <= nb <= S else S
        for packed in (identity, ordered):
            # the entries' rays own the lists: slot j of the identity is ray j
            want = point_order_reference(packed, bands_of_indices(np.minimum(idx, S - 1), S, nbands), S, nbands)
            got = _run_order(hip, packed, idx.astype(np.int32).view(np.float32), None, N, S, nb)
            check_points(np.where(np.arange(GROUP * S)[None, :] < want[1][:, None] * GROUP, got[0], POINT_NONE), got[1], packed, S)
            _compare(got[0], want[0], want[1], S)
            assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), nb
            want = point_order_reference(packed, bands_of_depths(np.nan_to_num(z), rays[:, 6], rays[:, 7], nbands), S, nbands)
            got = _run_order(hip, packed, z, rays, N, S, nb)
            _compare(got[0], want[0], want[1], S)
            assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), nb
    # the dictated groups did what the test thinks (identity entries): empty, a multiple of 256, one point, a full ray
    tot = np.add.reduceat(count, np.arange(0, N, GROUP))
    assert tot[1] == 0 and tot[2] % GROUP == 0 and tot[2] > 0 and tot[3] == 1 and count[5] == S and N % GROUP == 1


# ---- (b) the render pass ----------------------------------------------------------------------------------------------------------------
def _steps_left_behind(hip, N):
    G = (N + GROUP - 1) // GROUP
    t = torch.full((G,), -1, dtype=torch.int32, device=DEV)
    rc = hip.capi.lib().nvsr_internal_copy_point_steps(t.data_ptr(), G, hip.capi.stream())
    torch.cuda.synchronize()
    return rc, t.cpu().numpy()


def _assert_points_agree(hip, model, rays, S, arith, release=True, **kw):
    """point-major == fused == lockstep on every output; the point-major route really ran: its step counts are those of the entries it left"""
    N = rays.shape[0]
    one, _ = _pass(hip, model, rays, S, arith, release=release, NVSR_RENDER_ONE_PHASE="1", **kw)
    lock, _ = _pass(hip, model, rays, S, arith, release=release, NVSR_RENDER_ONE_PHASE="0", NVSR_COLOUR_POINTS="0", **kw)
    assert _steps_left_behind(hip, N)[0] == 1                                    # (NVSR_ERR_SHAPE: the lockstep kernels leave no steps)
    pts, entries = _pass(hip, model, rays, S, arith, release=release, NVSR_RENDER_ONE_PHASE="0", NVSR_COLOUR_POINTS="1", **kw)
    rc, steps = _steps_left_behind(hip, N)
    assert rc == 0
    n = np.zeros(len(steps) * GROUP, np.int64)
    n[:N] = entries >> ORDER_SHIFT
    assert np.array_equal(steps, (n.reshape(-1, GROUP).sum(1) + GROUP - 1) // GROUP)
    for name in OUTPUTS:
        print("%s: point-major differs from fused in %d elements, from lockstep in %d" % (
            name, int((torch.nan_to_num(one[name]) != torch.nan_to_num(pts[name])).sum()), int((torch.nan_to_num(lock[name]) != torch.nan_to_num(pts[name])).sum())))
    for name in OUTPUTS:
        assert _same(one[name], pts[name]), name + " (against the fused kernel)"
        assert _same(lock[name], pts[name]), name + " (against NVSR_COLOUR_POINTS=0)"
    return one, pts, entries


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("S", [8, 24])
def test_point_major_pass_with_depths_in_registers(hip, arith, S):
    """the coarse pass of a frame (nvsr_render_pass3_coarse_z_launch) at a ragged N; white background off and on; each order off"""
    mc, mf, rays = _scene(hip, 21, 96, 96, n_rays=N_SMALL)
    g = torch.Generator(device=DEV).manual_seed(S)
    noise = 0.7 * torch.randn(N_SMALL, S, device=DEV, generator=g)
    for white in (0, 1):
        one, pts, _ = _assert_points_agree(hip, mf, rays, S, arith, noise=noise, white=white, lindisp=white)
        assert torch.isfinite(pts["rgb"]).all()
        w = one["weights"]
        assert 0.02 < float((w == 0).float().mean()) < 0.98                      # dead and live samples: lists of many lengths
    _assert_points_agree(hip, mf, rays, S, arith, noise=noise, NVSR_COLOUR_ORDER="0")
    _assert_points_agree(hip, mf, rays, S, arith, noise=noise, NVSR_COLOUR_GROUP_ORDER="0")


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("S", [24, 40])
def test_point_major_pass_with_depths_read_on_dictated_counts(hip, arith, S):
    """nvsr_render_pass_arith at N_RAYS rays in a random order with the live counts of _counts_and_noise (S = 24: with an emptied group); white
    background off and on; each order off"""
    mc, mf, rays = _scene(hip, 11, 264, 264, n_rays=N_RAYS, sigma=0.05)
    c, noise = _counts_and_noise(S, 300 + S, empty_group=3 if S == 24 else None)
    g = torch.Generator(device=DEV).manual_seed(2)
    z = (2.0 + (torch.arange(S, device=DEV)[None, :] + 0.5 * torch.rand(N_RAYS, 1, device=DEV, generator=g)) * (4.0 / S)).contiguous()
    for white in (0, 1):
        one, pts, entries = _assert_points_agree(hip, mf, rays, S, arith, z=z, noise=noise, white=white)
        assert np.array_equal((one["weights"] != 0).sum(1).cpu().numpy(), c)
        assert np.array_equal(entries, order_reference(c, S, hip.capi.lib().nvsr_internal_colour_order_bins()))
        assert torch.isfinite(pts["rgb"]).all()
    _, _, ident = _assert_points_agree(hip, mf, rays, S, arith, z=z, noise=noise, NVSR_COLOUR_ORDER="0")
    assert np.array_equal(ident, (c << ORDER_SHIFT) | (np.arange(N_RAYS) % ORDER_RAYS))
    if S == 24:
        assert not (ident[3 * GROUP:4 * GROUP] >> ORDER_SHIFT).any()             # the emptied group: a workgroup without a step
    _assert_points_agree(hip, mf, rays, S, arith, z=z, noise=noise, NVSR_COLOUR_GROUP_ORDER="0")


@pytest.mark.parametrize("arith", ARITHS)
def test_point_major_pass_with_every_weight_positive(hip, arith):
    """a density head that answers 0.05 everywhere: every list holds all S samples, every run of a band is S / bands samples or more, and runs
    cross wave and step boundaries -- with the depths read and with the depths in registers"""
    mc, mf, rays = _scene(hip, 6, 264, 264, n_rays=N_RAYS, sigma=0.05)
    S = 24
    g = torch.Generator(device=DEV).manual_seed(2)
    z = (2.0 + (torch.arange(S, device=DEV)[None, :] + 0.5 * torch.rand(N_RAYS, 1, device=DEV, generator=g)) * (4.0 / S)).contiguous()
    for r, zz in ((rays, z), (rays[:N_SMALL].contiguous(), None)):      # (the pass that reads its depths has a minimum ray count)
        one, pts, entries = _assert_points_agree(hip, mf, r, S, arith, z=zz, white=1)
        assert bool((pts["weights"] > 0).all()) and np.all(entries >> ORDER_SHIFT == S) and torch.isfinite(pts["rgb"]).all()


@pytest.mark.parametrize("arith", ARITHS)
def test_a_ray_with_a_nan_density_stays_nan_where_the_fused_route_has_it(hip, arith):
    """NaN noise on one ray: its weights are NaN, NaN weights are live, and its pixel -- no other -- is NaN in all three routes"""
    mc, mf, rays = _scene(hip, 8, 96, 96, n_rays=N_SMALL)
    S, bad = 24, 1000
    g = torch.Generator(device=DEV).manual_seed(5)
    noise = 0.7 * torch.randn(N_SMALL, S, device=DEV, generator=g)
    noise[bad] = float("nan")
    one, pts, entries = _assert_points_agree(hip, mf, rays, S, arith, noise=noise, white=1)
    nan_rays = torch.isnan(pts["rgb"]).any(1)
    assert bool(nan_rays[bad]) and int(nan_rays.sum()) == 1
    assert bool(torch.isnan(pts["weights"][bad]).all())


def test_point_buffers_grow_across_launches_without_a_release(hip):
    """two launches of different N and S on one stream without a release in between, then the first again: the points' and the views' buffers
    grow with the lists; the lists' scratch and the entries left behind answer as tests/test_render_two_phase.py expects"""
    lib = hip.capi.lib()
    Na, Nb = N_SMALL, 2 * ORDER_RAYS + 513
    mc, mf, rays = _scene(hip, 7, 96, 96, n_rays=Nb)
    assert lib.nvsr_release_render_scratch() == 0 and lib.nvsr_render_scratch_bytes() == 0
    largest = 0
    for N, S in ((Na, 8), (Nb, 24), (Na, 8)):
        r = rays[:N].contiguous()
        one, pts, entries = _assert_points_agree(hip, mf, r, S, "f16x2", release=False)
        largest = max(largest, 2 * 4 * N * S + 4 * N)
        assert lib.nvsr_render_scratch_bytes() == largest
        c = (one["weights"] != 0).sum(1).cpu().numpy()
        assert np.array_equal(entries, order_reference(c, S, lib.nvsr_internal_colour_order_bins()))
    t = torch.full((Nb,), -1, dtype=torch.int32, device=DEV)
    assert lib.nvsr_internal_copy_live_counts(t.data_ptr(), Nb, hip.capi.stream()) == 1      # NVSR_ERR_SHAPE: the latest launch had Na rays
    assert lib.nvsr_release_render_scratch() == 0 and lib.nvsr_render_scratch_bytes() == 0
