"""Shared plumbing of the GPU tests of the two-phase render pass -- tests/test_render_two_phase.py (csrc/render3.hip: the density and colour
kernels), tests/test_colour_order.py and tests/test_group_order.py (csrc/colour_order.hip: the two orders and the scratch).  A plain helper
module like triplane_checks.py (not collected, not a conftest): environment handles, the bit-for-bit comparison, scenes, dictated live counts
and one render pass by the C ABI."""
import ctypes as C
import os

import numpy as np
import torch

from colour_order_ref import ORDER_RAYS
from group_order_ref import GROUP_RAYS

DEV = "cuda:0"
ARITHS = ["f16x2", "bf16x3"]
OUTPUTS = ("rgb", "disp", "acc", "depth", "weights")
N_RAYS = 65536 + 4096 + 37      # of the dictated counts: 17 blocks of the ray order and a ragged one, a ragged last group


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


def _scene(hip, seed, H, W, plane_res=64, n_rays=None, sigma=None):
    """bench.py's synthetic scene and the packed rays of an H x W view -> (coarse model, fine model, rays).  n_rays: that many of the rays, in
    a seeded random order.  sigma: the fine model's density head answers this everywhere."""
    from bench import make_synthetic_scene
    mc, mf, sid, pose = make_synthetic_scene(DEV, plane_res=plane_res, view_res=16, seed=seed)
    focal = 0.5 * W / np.tan(0.5 * 0.6911112)
    ro, rd = hip.nerf_helpers.get_ray_bundle(H, W, focal, pose)
    rays = hip.train_utils.pack_rays(ro, rd, 2.0, 6.0)
    if n_rays is not None:
        g = torch.Generator(device="cpu").manual_seed(seed)
        rays = rays[torch.randperm(H * W, generator=g)[:n_rays].to(DEV)].contiguous()
    if sigma is not None:
        with torch.no_grad():
            mf.fc_alpha["0"].weight.zero_()
            mf.fc_alpha["0"].bias.fill_(sigma)
    return mc, mf, rays


def _counts_and_noise(S, seed, empty_group=None):
    """ray i of N_RAYS has c_i live samples at random positions: half the rays are empty, the rest spread over 1..S, one full ray per block of
    the order.  The noise is -1000 on a dead sample (sigma + noise <= 0: w = +0.0 exactly) and 0 on a live one (sigma = 0.05: w > 0).
    empty_group: that group of 256 consecutive rays is emptied -- with NVSR_COLOUR_ORDER=0 its workgroup has trip 0; with the order the
    blocks' last groups hold empty rays only."""
    rng = np.random.default_rng(seed)
    c = np.where(rng.random(N_RAYS) < 0.5, 0, rng.integers(1, S + 1, N_RAYS))
    for b0 in range(0, N_RAYS, ORDER_RAYS):
        c[b0 + rng.integers(0, min(ORDER_RAYS, N_RAYS - b0))] = S
    if empty_group is not None:
        c[empty_group * GROUP_RAYS:(empty_group + 1) * GROUP_RAYS] = 0
    rank = np.argsort(np.argsort(rng.random((N_RAYS, S)), 1), 1)
    live = rank < c[:, None]
    noise = torch.from_numpy(np.where(live, 0.0, -1000.0).astype(np.float32)).to(DEV).contiguous()
    return c, noise


def _pass(hip, model, rays, S, arith, z=None, noise=None, white=0, lindisp=0, release=False, **env):
    """One render pass by the C ABI under the environment handles `env`: with `z` nvsr_render_pass_arith (depths read; weights requested: the
    coarse kernel), without it the coarse pass with its depths in registers (nvsr_render_pass3_coarse_z_launch, which has no minimum ray
    count).  Outputs start as NaN: an element a route does not write fails.  -> (outputs, the packed entries the launch left in the scratch, or
    None with NVSR_RENDER_ONE_PHASE=1).  release: the scratch is released first, and afterwards holds this launch's lists or nothing."""
    capi = hip.capi
    lib = capi.lib()
    N = rays.shape[0]
    assert z is None or N >= capi.fused_min_rays()
    sc, keep = model.native_scene()
    packed = model.packed_decoder()
    out = dict(rgb=torch.full((N, 3), float("nan"), device=DEV), disp=torch.full((N,), float("nan"), device=DEV),
               acc=torch.full((N,), float("nan"), device=DEV), weights=torch.full((N, S), float("nan"), device=DEV),
               depth=torch.full((N,), float("nan"), device=DEV))
    if release:
        assert lib.nvsr_release_render_scratch() == 0
    with _env(**env):
        if z is not None:
            capi.call("nvsr_render_pass_arith", C.byref(sc), capi.ptr(packed), N, S, capi.ptr(rays), capi.ptr(z), capi.ptr(noise), int(white),
                      capi.ptr(out["rgb"]), capi.ptr(out["disp"]), capi.ptr(out["acc"]), capi.ptr(out["weights"]), capi.ptr(out["depth"]), None,
                      capi.ARITHMETIC[arith], capi.stream())
        else:
            capi.call("nvsr_render_pass3_coarse_z_launch", capi.ARITHMETIC[arith], C.byref(sc), capi.ptr(packed), N, S, capi.ptr(rays), int(lindisp),
                      capi.ptr(noise), int(white), capi.ptr(out["rgb"]), capi.ptr(out["disp"]), capi.ptr(out["acc"]), capi.ptr(out["weights"]),
                      capi.ptr(out["depth"]), None, capi.stream())
        torch.cuda.synchronize()
    entries = None
    if env.get("NVSR_RENDER_ONE_PHASE") != "1":
        if release:
            assert lib.nvsr_render_scratch_bytes() == 2 * 4 * N * S + 4 * N, "the two-phase route did not run"
        t = torch.full((N,), -1, dtype=torch.int32, device=DEV)
        assert lib.nvsr_internal_copy_live_counts(t.data_ptr(), N, capi.stream()) == 0, "the two-phase route did not run"
        torch.cuda.synchronize()
        entries = t.cpu().numpy()
    elif release:
        assert lib.nvsr_render_scratch_bytes() == 0
    return out, entries
