"""GPU tests (-m gpu) of the colour pass's ray order (csrc/colour_order.hip: live_order_kernel; csrc/render3.hip: PHASE 2 of render_pass3_body; include/nvsr.h
"The two-phase render pass").

(a) the ordering kernel alone against the numpy reference (colour_order_ref.py; itself checked on the CPU by test_colour_order_host.py);
(b) the product route against the fused kernel (NVSR_RENDER_ONE_PHASE=1), bit for bit, on rays in a random order whose live counts the test
    dictates through the density noise -- the new grouping then differs from the old one as much as it can;
(c) the packed entries the launch left behind: ordered by default, the identity with NVSR_COLOUR_ORDER=0, the same pixels in both."""
import numpy as np
import pytest
import torch

from colour_order_ref import ORDER_RAYS, ORDER_SHIFT, check_packed, order_reference
from two_phase_checks import ARITHS, DEV, N_RAYS, OUTPUTS, _counts_and_noise, _pass, _same, _scene

pytestmark = pytest.mark.gpu

# ---- (a) the ordering kernel alone ------------------------------------------------------------------------------------------------------
def _patterns(N, S):
    rng = np.random.default_rng(1000 * S + N)
    one = np.zeros(N, np.int64)
    one[N // 2] = S
    return {"all equal": np.full(N, (S + 1) // 2), "all 0": np.zeros(N, np.int64), "all S": np.full(N, S),
            "increasing": np.arange(N) if N <= S + 1 else np.arange(N) * S // (N - 1),      # (strictly where 0..S has room for it, else a ramp)
            "random": rng.integers(0, S + 1, N), "one full ray among zeros": one}


@pytest.mark.parametrize("S", [1, 192])
@pytest.mark.parametrize("N", [1, 255, 4096, 4096 + 513])
def test_ordering_kernel_equals_the_numpy_reference(hip, N, S):
    f = hip.capi.lib().nvsr_internal_live_order
    bins = hip.capi.lib().nvsr_internal_colour_order_bins()
    assert bins >= 1
    for name, count in _patterns(N, S).items():
        t = torch.zeros(N + 64, dtype=torch.int32, device=DEV)         # (a guard band behind the array: the kernel writes N entries)
        t[:N] = torch.from_numpy(count.astype(np.int32)).to(DEV)
        t[N:] = -7
        assert f(t.data_ptr(), N, S, hip.capi.stream()) == 0
        torch.cuda.synchronize()
        got = t.cpu().numpy()
        assert np.all(got[N:] == -7), name
        check_packed(got[:N], count, S, bins)
        assert np.array_equal(got[:N], order_reference(count, S, bins)), name
        if name in ("all equal", "all 0", "all S"):
            assert np.array_equal(got[:N] & (ORDER_RAYS - 1), np.arange(N) % ORDER_RAYS), name      # stability: the identity


# ---- (b), (c) the product route ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("S,read_z", [(24, False), (40, True)])
def test_ordered_colour_pass_equals_fused_on_dictated_counts(hip, arith, S, read_z):
    """(b) and (c): S = 24 with the depths in registers, S = 40 with the depths read; white background off and on"""
    mc, mf, rays = _scene(hip, 11, 264, 264, n_rays=N_RAYS, sigma=0.05)      # a 264 x 264 view, N_RAYS of its rays in a random order
    N = N_RAYS
    c, noise = _counts_and_noise(S, 100 + S)
    # evenly spaced depths with a per-ray offset (two random depths may coincide: a sample of zero length has weight 0 whatever its density)
    g = torch.Generator(device=DEV).manual_seed(2)
    z = (2.0 + (torch.arange(S, device=DEV)[None, :] + 0.5 * torch.rand(N, 1, device=DEV, generator=g)) * (4.0 / S)).contiguous() if read_z else None
    bins = hip.capi.lib().nvsr_internal_colour_order_bins()
    names = OUTPUTS
    for white in (0, 1):
        one, _ = _pass(hip, mf, rays, S, arith, z, noise, white, lindisp=1, release=True, NVSR_RENDER_ONE_PHASE="1")
        two, entries = _pass(hip, mf, rays, S, arith, z, noise, white, lindisp=1, release=True, NVSR_RENDER_ONE_PHASE="0", NVSR_COLOUR_ORDER="1")
        same, ident = _pass(hip, mf, rays, S, arith, z, noise, white, lindisp=1, release=True, NVSR_RENDER_ONE_PHASE="0", NVSR_COLOUR_ORDER="0")
        # the input did what the test thinks it did: ray i has exactly c_i weights that are not zero
        assert np.array_equal((one["weights"] != 0).sum(1).cpu().numpy(), c)
        for name in names:
            print("ordered vs fused, white %d, %s: %d elements differ" % (white, name, int((torch.nan_to_num(one[name]) != torch.nan_to_num(two[name])).sum())))
        for name in names:
            assert _same(one[name], two[name]), name
            assert _same(one[name], same[name]), name + " (NVSR_COLOUR_ORDER=0)"
        assert torch.isfinite(two["rgb"]).all()
        # (c) the ordered route ran: the entries are the reference's; without the order every entry names its own slot
        check_packed(entries, c, S, bins)
        assert np.array_equal(entries, order_reference(c, S, bins))
        assert not np.array_equal(entries & (ORDER_RAYS - 1), np.arange(N) % ORDER_RAYS)
        assert np.array_equal(ident, (c << ORDER_SHIFT) | (np.arange(N) % ORDER_RAYS))
