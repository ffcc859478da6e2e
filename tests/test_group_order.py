"""GPU tests (-m gpu) of the colour pass's order of dispatch (csrc/colour_order.hip: group_order_kernel, the group_trip output of
live_order_kernel; csrc/render3.hip: blk = group_slot[blockIdx.x] in PHASE 2 of render_pass3_body; include/nvsr.h "Order of dispatch of the colour pass").

(a) group_order_kernel alone against the numpy reference (group_order_ref.py; itself checked on the CPU by test_group_order_host.py), with a
    guard band behind the output, the handle on and off, and beyond what the one workgroup sorts;
(b) the product route against the fused kernel (NVSR_RENDER_ONE_PHASE=1), bit for bit, on the dictated counts of test_colour_order.py with one
    group of empty rays added (N = 65536 + 4096 + 37: the last group is ragged), each handle on and off, white background off and on;
(c) what the launch left behind: group_trip is the maxima of the packed entries' groups, group_slot is the reference's."""
import numpy as np
import pytest
import torch

from group_order_ref import GROUP_RAYS, MAX_G, MAX_S, check_group_order, eighths, group_order_reference, group_trips
from two_phase_checks import ARITHS, DEV, N_RAYS, OUTPUTS, _counts_and_noise, _env, _pass, _same, _scene

pytestmark = pytest.mark.gpu


# ---- (a) the kernel alone ----------------------------------------------------------------------------------------------------------------
def _patterns(G, S):
    rng = np.random.default_rng(1000 * S + G)
    one = np.zeros(G, np.int64)
    one[G // 2] = S
    return {"all equal": np.full(G, (S + 1) // 2), "all zero": np.zeros(G, np.int64), "one heavy group among zeros": one,
            "random": rng.integers(0, S + 1, G)}


def _run_alone(hip, trips, S, sorted_):
    G = trips.size
    t = torch.from_numpy(trips.astype(np.int32)).to(DEV)
    out = torch.full((G + 64,), -7, dtype=torch.int32, device=DEV)         # (a guard band behind the output: the kernel writes G entries)
    with _env(NVSR_COLOUR_GROUP_ORDER="1" if sorted_ else "0"):
        assert hip.capi.lib().nvsr_internal_group_order(t.data_ptr(), G, S, out.data_ptr(), hip.capi.stream()) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.all(got[G:] == -7)
    assert np.array_equal(t.cpu().numpy(), trips)                          # the trips are read only
    return got[:G]


@pytest.mark.parametrize("S", [1, 192])
@pytest.mark.parametrize("G", [1, 17, 300, 2500])
def test_group_order_kernel_equals_the_numpy_reference(hip, G, S):
    for name, trips in _patterns(G, S).items():
        got = _run_alone(hip, trips, S, True)
        check_group_order(got, trips, S)
        assert np.array_equal(got, group_order_reference(trips, S)), name
        if name in ("all equal", "all zero"):
            assert np.array_equal(got, eighths(G)), name                   # one run: the density kernels' mapping
        if name == "one heavy group among zeros":
            assert got[0] == G // 2, name
        assert np.array_equal(_run_alone(hip, trips, S, False), eighths(G)), name + " (NVSR_COLOUR_GROUP_ORDER=0)"


def test_group_order_kernel_at_and_beyond_the_limits_of_one_workgroup(hip):
    rng = np.random.default_rng(5)
    t = rng.integers(0, MAX_S + 1, MAX_G)
    assert np.array_equal(_run_alone(hip, t, MAX_S, True), group_order_reference(t, MAX_S))      # the largest case that is sorted
    t = rng.integers(0, 65, MAX_G + 1)
    assert np.array_equal(_run_alone(hip, t, 64, True), eighths(MAX_G + 1))
    t = rng.integers(0, MAX_S + 2, 9)
    assert np.array_equal(_run_alone(hip, t, MAX_S + 1, True), eighths(9))


# ---- (b), (c) the product route ----------------------------------------------------------------------------------------------------------
EMPTY_GROUP = 2      # rays 512..767 of the first block of the order: a group of the density pass's grouping


def _left_behind(hip, G):
    t = torch.full((2 * G + 64,), -7, dtype=torch.int32, device=DEV)
    assert hip.capi.lib().nvsr_internal_copy_group_order(t.data_ptr(), G, hip.capi.stream()) == 0
    torch.cuda.synchronize()
    got = t.cpu().numpy()
    assert np.all(got[2 * G:] == -7)
    return got[:G], got[G:2 * G]


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("S,read_z", [(24, False), (40, True)])
def test_dispatch_order_keeps_the_fused_pixels_on_dictated_counts(hip, arith, S, read_z):
    """(b) and (c): S = 24 with the depths in registers, S = 40 with the depths read"""
    mc, mf, rays = _scene(hip, 11, 264, 264, n_rays=N_RAYS, sigma=0.05)
    N = N_RAYS
    G = (N + GROUP_RAYS - 1) // GROUP_RAYS
    assert N % GROUP_RAYS == 37                                             # a ragged last group
    c, noise = _counts_and_noise(S, 100 + S, empty_group=EMPTY_GROUP)
    g = torch.Generator(device=DEV).manual_seed(2)
    z = (2.0 + (torch.arange(S, device=DEV)[None, :] + 0.5 * torch.rand(N, 1, device=DEV, generator=g)) * (4.0 / S)).contiguous() if read_z else None
    names = OUTPUTS
    for white in (0, 1):
        one, _ = _pass(hip, mf, rays, S, arith, z, noise, white, lindisp=1, release=True, NVSR_RENDER_ONE_PHASE="1")
        assert np.array_equal((one["weights"] != 0).sum(1).cpu().numpy(), c)      # the input did what the test thinks it did
        seen = {}
        for order in ("1", "0"):
            for group in ("1", "0"):
                two, entries = _pass(hip, mf, rays, S, arith, z, noise, white, lindisp=1, release=True, NVSR_RENDER_ONE_PHASE="0", NVSR_COLOUR_ORDER=order,
                                     NVSR_COLOUR_GROUP_ORDER=group)
                slot, trip = _left_behind(hip, G)
                for name in names:
                    print("order %s, group order %s, white %d, %s: %d elements differ"
                          % (order, group, white, name, int((torch.nan_to_num(one[name]) != torch.nan_to_num(two[name])).sum())))
                for name in names:
                    assert _same(one[name], two[name]), "%s (NVSR_COLOUR_ORDER=%s NVSR_COLOUR_GROUP_ORDER=%s)" % (name, order, group)
                assert torch.isfinite(two["rgb"]).all()
                # (c) group_trip: the maxima recomputed from the packed entries; group_slot: the reference's on those trips
                assert np.array_equal(trip, group_trips(entries))
                assert np.array_equal(slot, group_order_reference(trip, S, sorted_=group == "1"))
                if group == "1":
                    check_group_order(slot, trip, S)
                seen[order, group] = (slot, trip)
        # the cases are what they claim: an all-empty group and the ragged one exist, and the sorted dispatch differs from the eighths
        assert seen["0", "1"][1][EMPTY_GROUP] == 0 and (seen["1", "1"][1] == 0).sum() >= 16
        assert seen["0", "1"][1][G - 1] == c[(G - 1) * GROUP_RAYS:].max()
        assert not np.array_equal(seen["1", "1"][0], seen["1", "0"][0]) and not np.array_equal(seen["0", "1"][0], seen["0", "0"][0])
        assert np.bincount(seen["1", "1"][1]).max() >= 16                   # (runs of equal trips longer than 8: dealt in pieces)
        assert np.array_equal(seen["1", "0"][0], eighths(G))
