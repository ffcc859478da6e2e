"""GPU tests of the one-decoder render route (models.fine.type == 'use_same': nvsr_render_rays_shared_arith, csrc/aux.hip), stage by stage and
on a diverged model, on a small frame of make_synthetic_scene (64 x 64 planes, a 16 x 16 view plane) through the C ABI on buffers the test owns.

  the stages ........ the route is rebuilt from entry points that have tests of their own --
                          nvsr_render_pass3_coarse_z_launch with raw_out   (test_render_forward_edges.py)
                          nvsr_importance_resample_rays, nvsr_sample_pdf   (the resampler tests of test_hip_parity.py, test_hip_round3.py)
                          nvsr_render_pass_arith with raw_out on z_new     (test_render_forward_edges.py)
                          nvsr_shared_merge                                (test_shared_merge.py)
                          nvsr_composite_rays                              (test_render_forward_edges.py)
                      -- and all six outputs of the route (rgb, disp, acc; coarse and fine) equal the sequence's byte for byte: the same kernels
                      on the same inputs, no tolerance.  The merged depths also equal the resampler's own merged list bit for bit.  At
                      N = nvsr_fused_min_rays() and N + 1 (with an odd Nc: N Nc is no multiple of 4 and the round4 offsets of the workspace
                      matter), 15 + 33 and 64 + 128 (63 + 128 at N + 1) samples, white background on and off, both spacings, density noise.
                      That the shared route ran: its rgb_f differs in at least one bit from the NVSR_NO_SHARED_DECODER=1 run of the same inputs.
  a diverged model .. one NaN texel in a position plane (a tenth of the pixels NaN in f16x2): the NaN masks of all six outputs equal those of the two-decoder route
                      (NVSR_NO_SHARED_DECODER=1), rgb_f agrees to 2e-5 outside the mask.  The workspace holds a finite, plausible number
                      everywhere before the call.  A pixel whose depths hold a NaN is NaN whatever the merge gathered, so the outputs alone
                      cannot show a slot of the merged decoder outputs that was never written: the test also looks at the route's last
                      sub-buffer (raw_m, the layout nvsr_render_shared_workspace_floats describes) for an element that still holds the fill.
"""
import ctypes as C
import time
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from nerf_baseline_checks import DEV

pytestmark = pytest.mark.gpu

T0 = time.time()
OUTPUTS = ("rgb_c", "disp_c", "acc_c", "rgb_f", "disp_f", "acc_f")
FILL = 0.7311                          # what the workspace of the diverged frame holds before the call: a plausible logit, density and depth
# (rays over nvsr_fused_min_rays(), Nc, Nf)
FRAMES = [(0, 64, 128), (0, 15, 33), (1, 15, 33), (1, 63, 128)]
# (white background, lindisp, density noise)
SETTINGS = [(0, 0, 0), (1, 1, 0), (1, 0, 1), (0, 1, 1)]
ARITHS = ["f16x2", "bf16x3"]


def _bits(t):
    return t.contiguous().view(torch.int32)


def round4(n):
    return (n + 3) // 4 * 4


class Frame:
    """the scene, the packed decoder and the packed rays of N + 1 pixels on the device"""

    def __init__(self, hip):
        from bench import make_synthetic_scene
        self.hip, self.capi = hip, hip.capi
        mc, _, sid, pose = make_synthetic_scene(DEV, plane_res=64, view_res=16, seed=3)
        mc.set_cur_scene_id(sid)
        with torch.no_grad():
            planes, self.consts = mc.scene_args()
            self.planes = [p.detach().clone() for p in planes]
            self.packed = mc.packed_decoder().detach().clone()
        self.N0 = hip.capi.fused_min_rays()
        W = 256
        H = -(-(self.N0 + 1) // W)
        focal = 0.5 * W / np.tan(0.5 * 0.6911112)
        ro, rd = hip.nerf_helpers.get_ray_bundle(H, W, focal, pose)
        self.rays = hip.train_utils.pack_rays(ro, rd, 2.0, 6.0)[:self.N0 + 1].contiguous()
        g = torch.Generator(device=DEV).manual_seed(5)
        self.noise = 0.5 * torch.randn(self.N0 + 1, 256, device=DEV, generator=g)

    def scene(self, planes):
        sc = self.capi.Scene()
        for d, p in enumerate(planes):
            assert p.is_contiguous() and p.dtype == torch.float32
            sc.planes[d] = p.data_ptr()
            sc.ph[d], sc.pw[d] = p.shape[0], p.shape[1]
        for i in range(5):
            sc.lo[i], sc.range[i] = self.consts[i], self.consts[5 + i]
        for d in range(3):
            for j in range(6):
                sc.proj[d][j] = self.consts[10 + 6 * d + j]
        return sc

    def inputs(self, N, Nc, Nf, noise):
        S = Nc + Nf
        return (self.rays[:N], self.noise[:N, :Nc].contiguous() if noise else None, self.noise[:N, 256 - S:].contiguous() if noise else None)

    def outputs(self, N):
        nan = lambda *s: torch.full(s, float("nan"), device=DEV)
        return NS(rgb_c=nan(N, 3), disp_c=nan(N), acc_c=nan(N), rgb_f=nan(N, 3), disp_f=nan(N), acc_f=nan(N))

    def route(self, planes, N, Nc, Nf, lindisp, white, noise, arith, fill=None):
        """nvsr_render_rays_shared_arith -> the six outputs and the workspace"""
        capi, p = self.capi, self.capi.ptr
        rays, n_c, n_f = self.inputs(N, Nc, Nf, noise)
        sc, o = self.scene(planes), self.outputs(N)
        ws = torch.full((capi.lib().nvsr_render_shared_workspace_floats(N, Nc, Nf),), float("nan") if fill is None else fill, device=DEV)
        capi.call("nvsr_render_rays_shared_arith", C.byref(sc), p(self.packed), N, Nc, Nf, p(rays), int(lindisp), int(white), None, None, p(n_c), p(n_f),
                  p(o.rgb_c), p(o.disp_c), p(o.acc_c), p(o.rgb_f), p(o.disp_f), p(o.acc_f), p(ws), capi.ARITHMETIC[arith], capi.stream())
        torch.cuda.synchronize()
        return o, ws

    def stages(self, planes, N, Nc, Nf, lindisp, white, noise, arith):
        """the same frame from the six entry points -> the six outputs, the merged depths and the resampler's merged depths"""
        capi, p, st = self.capi, self.capi.ptr, self.capi.stream()
        rays, n_c, n_f = self.inputs(N, Nc, Nf, noise)
        sc, o, S, code = self.scene(planes), self.outputs(N), Nc + Nf, capi.ARITHMETIC[arith]
        nan = lambda *s: torch.full(s, float("nan"), device=DEV)
        w_c, raw_c = nan(N, Nc), nan(N, Nc, 4)
        capi.call("nvsr_render_pass3_coarse_z_launch", code, C.byref(sc), p(self.packed), N, Nc, p(rays), int(lindisp), p(n_c), int(white), p(o.rgb_c),
                  p(o.disp_c), p(o.acc_c), p(w_c), None, p(raw_c), st)
        z_f = nan(N, S)
        capi.call("nvsr_importance_resample_rays", N, Nc, Nf, p(rays), int(lindisp), p(w_c), None, p(z_f), st)
        z_c = nan(N, Nc)
        capi.call("nvsr_coarse_z", N, Nc, p(rays), int(lindisp), None, p(z_c), st)
        mid, w_mid, z_new = (0.5 * (z_c[:, 1:] + z_c[:, :-1])).contiguous(), w_c[:, 1:-1].contiguous(), nan(N, Nf)
        capi.call("nvsr_sample_pdf", N, Nc - 1, Nf, p(mid), p(w_mid), None, p(z_new), st)
        raw_new, t = nan(N, Nf, 4), self.outputs(N)
        capi.call("nvsr_render_pass_arith", C.byref(sc), p(self.packed), N, Nf, p(rays), p(z_new), None, int(white), p(t.rgb_f), p(t.disp_f), p(t.acc_f),
                  None, None, p(raw_new), code, st)
        z_m, raw_m = nan(N, S), nan(N, S, 4)
        capi.call("nvsr_shared_merge", N, Nc, Nf, p(rays), int(lindisp), p(z_new), p(raw_c), p(raw_new), p(z_m), p(raw_m), st)
        capi.call("nvsr_composite_rays", N, S, p(raw_m), p(z_m), p(rays), p(n_f), int(white), p(o.rgb_f), p(o.disp_f), p(o.acc_f), None, None, st)
        torch.cuda.synchronize()
        return o, z_m, z_f


@pytest.fixture(scope="module")
def frame(hip):
    f = Frame(hip)
    yield f
    hip.capi.lib().nvsr_release_render_scratch()
    if hip.capi._range_flag is not None:             # the NaN frame raises the f16x2 range flag of a process that registered one
        hip.capi._range_flag.reset()


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("setting", SETTINGS, ids=lambda s: "white%d-lindisp%d-noise%d" % s)
@pytest.mark.parametrize("shape", FRAMES, ids=lambda s: "N+%d-%dx%d" % s)
def test_route_equals_its_stages(frame, monkeypatch, shape, setting, arith):
    (extra, Nc, Nf), (white, lindisp, noise) = shape, setting
    N = frame.N0 + extra
    assert extra == 0 or (N * Nc) % 4 != 0
    monkeypatch.delenv("NVSR_NO_SHARED_DECODER", raising=False)
    got, _ = frame.route(frame.planes, N, Nc, Nf, lindisp, white, noise, arith)
    want, z_m, z_f = frame.stages(frame.planes, N, Nc, Nf, lindisp, white, noise, arith)
    for name in OUTPUTS:
        g, w = getattr(got, name), getattr(want, name)
        assert name.startswith("disp") or torch.isfinite(g).all(), name          # (disp is NaN where acc == 0, like the reference's)
        assert torch.equal(_bits(g), _bits(w)), "%s: %d elements differ from the stage sequence's" % (name, int((_bits(g) != _bits(w)).sum()))
    assert torch.equal(_bits(z_m), _bits(z_f)), "the merged depths are not the resampler's merged list"
    monkeypatch.setenv("NVSR_NO_SHARED_DECODER", "1")
    two, _ = frame.route(frame.planes, N, Nc, Nf, lindisp, white, noise, arith)
    assert torch.equal(_bits(two.rgb_c), _bits(got.rgb_c))
    d = float((two.rgb_f - got.rgb_f).abs().max())
    print("shared_route | N+%d %dx%d white%d lindisp%d noise%d %s | rgb_f against the two-decoder route: max %.2e, %d elements differ in a bit" % (
        extra, Nc, Nf, white, lindisp, noise, arith, d, int((_bits(two.rgb_f) != _bits(got.rgb_f)).sum())))
    assert not torch.equal(_bits(two.rgb_f), _bits(got.rgb_f)), "the shared route was not taken"


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("shape", [(0, 64, 128), (1, 15, 33)], ids=lambda s: "N+%d-%dx%d" % s)
def test_diverged_model_renders_like_the_two_decoder_route(frame, monkeypatch, shape, arith):
    extra, Nc, Nf = shape
    N, S = frame.N0 + extra, Nc + Nf
    planes = [p.clone() for p in frame.planes]
    planes[0][32, 32, :] = float("nan")
    monkeypatch.delenv("NVSR_NO_SHARED_DECODER", raising=False)
    got, ws = frame.route(planes, N, Nc, Nf, 0, 1, 0, arith, fill=FILL)
    monkeypatch.setenv("NVSR_NO_SHARED_DECODER", "1")
    two, _ = frame.route(planes, N, Nc, Nf, 0, 1, 0, arith, fill=FILL)
    bad = torch.isnan(got.rgb_f).any(-1)
    n_bad = int(bad.sum())
    print("shared_route | diverged N+%d %dx%d %s | %d of %d pixels NaN" % (extra, Nc, Nf, arith, n_bad, N))
    # (bf16x3: the decoder's ReLU is fmaxf, which returns its non-NaN operand -- the NaN features never reach an output, no pixel of the frame is
    # NaN in either route and the comparison below is one of two finite frames; f16x2's ReLU lets a NaN through, pair_core.h)
    assert n_bad < N // 2 and (n_bad > 0 or arith != "f16x2")
    for name in OUTPUTS:
        g, t = getattr(got, name), getattr(two, name)
        assert torch.equal(torch.isnan(g), torch.isnan(t)), "%s: %d elements NaN in one route only" % (name, int((torch.isnan(g) != torch.isnan(t)).sum()))
    assert torch.equal(_bits(got.rgb_c.nan_to_num(nan=-1.0)), _bits(two.rgb_c.nan_to_num(nan=-1.0)))      # (a NaN's sign and payload differ with the kernel)
    d = float((got.rgb_f - two.rgb_f)[~bad].abs().max())
    assert d <= 2e-5, d
    # the merged decoder outputs, last in the workspace: w_c, z_new, z_m (each rounded up to 4 floats), raw_c, raw_new, raw_m [N,S,4]
    off = round4(N * Nc) + round4(N * Nf) + round4(N * S) + 4 * N * Nc + 4 * N * Nf
    raw_m = ws[off:off + 4 * N * S].view(N, S, 4)
    left = (raw_m == FILL).all(-1)
    assert not left.any(), "%d elements of the merged decoder outputs on %d rays were never written" % (int(left.sum()), int(left.any(-1).sum()))


def test_wall_time_of_this_file():
    print("shared_route wall | %.1f s since the module was imported" % (time.time() - T0))
