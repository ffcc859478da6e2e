"""GPU tests (-m gpu) of the colour pass's ray order (csrc/render3.hip: live_order_kernel and PHASE 2 of render_pass3_body; include/nvsr.h
"The two-phase render pass").

(a) the ordering kernel alone against the numpy reference (colour_order_ref.py; itself checked on the CPU by test_colour_order_host.py);
(b) the product route against the fused kernel (NVSR_RENDER_ONE_PHASE=1), bit for bit, on rays in a random order whose live counts the test
    dictates through the density noise -- the new grouping then differs from the old one as much as it can;
(c) the packed entries the launch left behind: ordered by default, the identity with NVSR_COLOUR_ORDER=0, the same pixels in both."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from colour_order_ref import ORDER_RAYS, ORDER_SHIFT, check_packed, order_reference
from test_hip_parity import DEV

pytestmark = pytest.mark.gpu

ARITHS = ["f16x2", "bf16x3"]


class _env:
    """environment variables for the launches inside the block (the library reads them at every launch)"""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _same(a, b):
    """torch.equal with NaNs: in the same places, and every number equal"""
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0))


def _bins(hip):
    f = hip.capi.lib().nvsr_internal_colour_order_bins
    f.restype, f.argtypes = C.c_int, []
    return int(f())


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
    lib = hip.capi.lib()
    f = lib.nvsr_internal_live_order
    f.restype, f.argtypes = C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_void_p]
    bins = _bins(hip)
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
N_RAYS = 65536 + 4096 + 37


def _scene(hip, seed):
    """a decoder whose density head answers +0.05 everywhere, and N_RAYS rays of a 264 x 264 view in a seeded random order"""
    from bench import make_synthetic_scene
    mc, mf, sid, pose = make_synthetic_scene(DEV, plane_res=64, view_res=16, seed=seed)
    H = W = 264
    focal = 0.5 * W / np.tan(0.5 * 0.6911112)
    ro, rd = hip.nerf_helpers.get_ray_bundle(H, W, focal, pose)
    rays = hip.train_utils.pack_rays(ro, rd, 2.0, 6.0)
    g = torch.Generator(device="cpu").manual_seed(seed)
    rays = rays[torch.randperm(H * W, generator=g)[:N_RAYS].to(DEV)].contiguous()
    with torch.no_grad():
        mf.fc_alpha["0"].weight.zero_()
        mf.fc_alpha["0"].bias.fill_(0.05)
    return mf, rays


def _counts_and_noise(S, seed):
    """ray i has c_i live samples at random positions: half the rays are empty, the rest spread over 1..S, one full ray per block of the
    order.  The noise is -1000 on a dead sample (sigma + noise <= 0: w = +0.0 exactly) and 0 on a live one (sigma = 0.05: w > 0)."""
    rng = np.random.default_rng(seed)
    c = np.where(rng.random(N_RAYS) < 0.5, 0, rng.integers(1, S + 1, N_RAYS))
    for b0 in range(0, N_RAYS, ORDER_RAYS):
        c[b0 + rng.integers(0, min(ORDER_RAYS, N_RAYS - b0))] = S
    rank = np.argsort(np.argsort(rng.random((N_RAYS, S)), 1), 1)
    live = rank < c[:, None]
    noise = torch.from_numpy(np.where(live, 0.0, -1000.0).astype(np.float32)).to(DEV).contiguous()
    return c, noise


def _pass(hip, model, rays, S, arith, z, noise, white, **env):
    """one render pass by the C ABI (tests/test_render_two_phase.py: with `z` nvsr_render_pass_arith, without it the coarse pass with its
    depths in registers) and, on the two-phase route, the packed entries it left in the scratch"""
    capi = hip.capi
    lib = capi.lib()
    N = rays.shape[0]
    assert N >= capi.fused_min_rays()
    sc, keep = model.native_scene()
    packed = model.packed_decoder()
    out = dict(rgb=torch.full((N, 3), float("nan"), device=DEV), disp=torch.full((N,), float("nan"), device=DEV),
               acc=torch.full((N,), float("nan"), device=DEV), weights=torch.full((N, S), float("nan"), device=DEV),
               depth=torch.full((N,), float("nan"), device=DEV))
    assert lib.nvsr_release_render_scratch() == 0
    with _env(**env):
        if z is not None:
            capi.call("nvsr_render_pass_arith", C.byref(sc), capi.ptr(packed), N, S, capi.ptr(rays), capi.ptr(z), capi.ptr(noise), int(white),
                      capi.ptr(out["rgb"]), capi.ptr(out["disp"]), capi.ptr(out["acc"]), capi.ptr(out["weights"]), capi.ptr(out["depth"]), None,
                      capi.ARITHMETIC[arith], capi.stream())
        else:
            f = lib.nvsr_render_pass3_coarse_z_launch
            f.restype = C.c_int
            f.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 7
            st = f(capi.ARITHMETIC[arith], C.cast(C.byref(sc), C.c_void_p), capi.ptr(packed), N, S, capi.ptr(rays), 1, capi.ptr(noise), int(white),
                   capi.ptr(out["rgb"]), capi.ptr(out["disp"]), capi.ptr(out["acc"]), capi.ptr(out["weights"]), capi.ptr(out["depth"]), None,
                   capi.stream())
            assert st == 0
        torch.cuda.synchronize()
    entries = None
    if env.get("NVSR_RENDER_ONE_PHASE") != "1":
        assert lib.nvsr_render_scratch_bytes() == 2 * 4 * N * S + 4 * N, "the two-phase route did not run"
        g = lib.nvsr_internal_copy_live_counts
        g.restype, g.argtypes = C.c_int, [C.c_void_p, C.c_int64, C.c_void_p]
        t = torch.full((N,), -1, dtype=torch.int32, device=DEV)
        assert g(t.data_ptr(), N, capi.stream()) == 0
        torch.cuda.synchronize()
        entries = t.cpu().numpy()
    else:
        assert lib.nvsr_render_scratch_bytes() == 0
    return out, entries


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("S,read_z", [(24, False), (40, True)])
def test_ordered_colour_pass_equals_fused_on_dictated_counts(hip, arith, S, read_z):
    """(b) and (c): S = 24 with the depths in registers, S = 40 with the depths read; white background off and on"""
    mf, rays = _scene(hip, 11)
    N = N_RAYS
    c, noise = _counts_and_noise(S, 100 + S)
    # evenly spaced depths with a per-ray offset (two random depths may coincide: a sample of zero length has weight 0 whatever its density)
    g = torch.Generator(device=DEV).manual_seed(2)
    z = (2.0 + (torch.arange(S, device=DEV)[None, :] + 0.5 * torch.rand(N, 1, device=DEV, generator=g)) * (4.0 / S)).contiguous() if read_z else None
    bins = _bins(hip)
    names = ("rgb", "disp", "acc", "depth", "weights")
    for white in (0, 1):
        one, _ = _pass(hip, mf, rays, S, arith, z, noise, white, NVSR_RENDER_ONE_PHASE="1")
        two, entries = _pass(hip, mf, rays, S, arith, z, noise, white, NVSR_RENDER_ONE_PHASE="0", NVSR_COLOUR_ORDER="1")
        same, ident = _pass(hip, mf, rays, S, arith, z, noise, white, NVSR_RENDER_ONE_PHASE="0", NVSR_COLOUR_ORDER="0")
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
