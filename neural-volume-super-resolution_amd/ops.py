"""`torch.ops.nvsr.*`: the hot path as PyTorch custom operators (torch.library) on top of the C ABI of include/nvsr.h.

Every operator is a thin shell: it allocates the outputs, turns tensors into raw device pointers and calls ONE entry point of
libnvsr_hip.so on the current stream (ctypes, capi.py) -- no arithmetic happens in Python.  Each has a fake (meta) implementation, so
the operators trace under FakeTensor / torch.compile / torch.export, and the differentiable ones carry their backward as another
operator of this library (`register_autograd`).  The host mirror (nerf_helpers / volume_rendering_utils / train_utils / models) is
written against these operators; they are the product path, not a side door.

Conventions
  * a scene is passed as `planes` = 4 CHANNEL-LAST [H,W,48] tensors (position planes D0..D2, view-direction plane) and `consts` = 28
    python floats: lo[5], range[5], proj[3][6] (struct nvsr_scene, include/nvsr.h);
  * `arithmetic` is the NVSR_ARITH_* code of the decoder GEMMs / SR convolutions for THIS call (-1 = the process default): a per-call
    argument, nothing global (capi.arith_code turns 'f32' / 'bf16x3' / 'f16x2' / None into it; render_pass and render_rays also take
    capi.RENDER_ARITHMETIC['f16'], the convolution operators capi.CONV_ARITHMETIC['f16']);
  * operators cannot return None: an output that was not asked for comes back as an empty tensor.

Reference functions behind the operators: models.py:381-421 (decoder), train_utils.py:71-182 (render passes), volume_rendering_utils.py:6-51
(compositing), nerf_helpers.py:668-702 (importance sampling), models.py:769-822,884-926 (EDSR / PlanesSR)."""
import ctypes as C
import os
from types import SimpleNamespace
from typing import List, Optional, Sequence, Tuple

import torch
from torch import Tensor
from torch.library import custom_op

from . import capi

PACK_ALL_ARITHMETICS = capi.PACK_ALL_ARITHMETICS

PC = capi.PLANE_CHANNELS
# decoder-gradient record: up to this many points of a pass (19 GB of record) the forward itself records the layer inputs and the backward
# never recomputes; beyond, the chunked recomputing path runs RECORD_RAYS rays at a time (train_utils re-exports both)
RECORD_FORWARD_MAX_POINTS = 1 << 21
RECORD_RAYS = 8192


def _f(*shape, like):
    return torch.empty(shape, dtype=torch.float32, device=like.device)


def _c(t):
    """float32 + contiguous (None passes through): the kernels take dense row-major buffers"""
    return None if t is None else capi.f32c(t)


def _none_if_empty(t):
    return None if (t is None or t.numel() == 0) else t


def _scene(planes, consts, channels=None):
    """struct nvsr_scene from 4 channel-last planes + the 28 host constants (channels: (C, Cv) of a non-default decoder geometry)"""
    assert len(planes) == 4 and len(consts) == 28
    sc = capi.Scene()
    for d, p in enumerate(planes):
        capi.require_cuda(p)
        cc = PC if channels is None else channels[0 if d < 3 else 1]
        assert p.dtype == torch.float32 and p.dim() == 3 and p.shape[2] == cc and p.is_contiguous(), "planes must be channel-last [H,W,%d] f32" % cc
        sc.planes[d] = p.data_ptr()
        sc.ph[d], sc.pw[d] = p.shape[0], p.shape[1]
    for i in range(5):
        sc.lo[i] = consts[i]
        sc.range[i] = consts[5 + i]
    for d in range(3):
        for j in range(6):
            sc.proj[d][j] = consts[10 + 6 * d + j]
    return sc


def scene_consts(sc):
    """the 28 floats of a capi.Scene (lo, range, proj) as the operators take them"""
    return [float(sc.lo[i]) for i in range(5)] + [float(sc.range[i]) for i in range(5)] + [float(sc.proj[d][j]) for d in range(3) for j in range(6)]


# =====================================================================================================================================
# layout / packing
# =====================================================================================================================================
@custom_op("nvsr::plane_to_channel_last", mutates_args=(), device_types="cuda")
def plane_to_channel_last(plane: Tensor) -> Tensor:
    """[1,C,H,W] or [C,H,W] (reference layout, models.py:436-439) -> channel-last [H,W,C] copy"""
    p = capi.f32c(plane)
    Cc, H, W = p.shape[-3:]
    out = _f(H, W, Cc, like=p)
    capi.call("nvsr_plane_to_channel_last", capi.ptr(p), capi.ptr(out), Cc, H, W, capi.stream())
    return out


@plane_to_channel_last.register_fake
def _(plane):
    Cc, H, W = plane.shape[-3:]
    return plane.new_empty((H, W, Cc), dtype=torch.float32)


@custom_op("nvsr::plane_from_channel_last", mutates_args=(), device_types="cuda")
def plane_from_channel_last(plane_hwc: Tensor) -> Tensor:
    """channel-last [H,W,C] -> [1,C,H,W]"""
    p = capi.f32c(plane_hwc)
    H, W, Cc = p.shape
    out = _f(1, Cc, H, W, like=p)
    capi.call("nvsr_plane_from_channel_last", capi.ptr(p), capi.ptr(out), Cc, H, W, capi.stream())
    return out


@plane_from_channel_last.register_fake
def _(plane_hwc):
    H, W, Cc = plane_hwc.shape
    return plane_hwc.new_empty((1, Cc, H, W), dtype=torch.float32)


plane_to_channel_last.register_autograd(lambda ctx, g: torch.ops.nvsr.plane_from_channel_last(g).reshape(ctx.shape),
                                        setup_context=lambda ctx, inputs, output: setattr(ctx, "shape", inputs[0].shape))
plane_from_channel_last.register_autograd(lambda ctx, g: torch.ops.nvsr.plane_to_channel_last(g))


@custom_op("nvsr::pack_decoder", mutates_args=(), device_types="cuda")
def pack_decoder(natural: Tensor) -> Tensor:
    """decoder parameters in state-dict order (models.py:169-195) -> MFMA-fragment blob of the forward kernels"""
    nat = capi.f32c(natural)
    assert nat.numel() == capi.DECODER_NATURAL_FLOATS
    packed = _f(capi.DECODER_PACKED_FLOATS, like=nat)
    capi.call("nvsr_pack_decoder", capi.ptr(nat), capi.ptr(packed), capi.stream())
    return packed


@pack_decoder.register_fake
def _(natural):
    return natural.new_empty((capi.DECODER_PACKED_FLOATS,), dtype=torch.float32)


@custom_op("nvsr::pack_decoder_bwd", mutates_args=(), device_types="cuda")
def pack_decoder_bwd(natural: Tensor) -> Tensor:
    """-> fragments of the transposed layers (backward kernels)"""
    nat = capi.f32c(natural)
    assert nat.numel() == capi.DECODER_NATURAL_FLOATS
    packed = _f(capi.DECODER_PACKED_BWD_FLOATS, like=nat)
    capi.call("nvsr_pack_decoder_bwd", capi.ptr(nat), capi.ptr(packed), capi.stream())
    return packed


@pack_decoder_bwd.register_fake
def _(natural):
    return natural.new_empty((capi.DECODER_PACKED_BWD_FLOATS,), dtype=torch.float32)


# =====================================================================================================================================
# sampling helpers (train_utils.py:95-109,144-155; nerf_helpers.py:668-702)
# =====================================================================================================================================
@custom_op("nvsr::coarse_z", mutates_args=(), device_types="cuda")
def coarse_z(rays: Tensor, Nc: int, lindisp: bool, t_rand: Optional[Tensor]) -> Tensor:
    rays, t_rand = _c(rays), _c(t_rand)
    N = rays.shape[0]
    z = _f(N, Nc, like=rays)
    if N:
        capi.call("nvsr_coarse_z", N, Nc, capi.ptr(rays), int(lindisp), capi.ptr(t_rand), capi.ptr(z), capi.stream())
    return z


@coarse_z.register_fake
def _(rays, Nc, lindisp, t_rand):
    return rays.new_empty((rays.shape[0], Nc))


@custom_op("nvsr::importance_resample", mutates_args=(), device_types="cuda")
def importance_resample(z_coarse: Tensor, weights: Tensor, Nf: int, u: Optional[Tensor]) -> Tensor:
    """z_mid -> sample_pdf_2(z_mid, w[1:-1], Nf, det = (u is None)) -> sort(cat(z, samples)): [N, Nc+Nf]; no gradient (train_utils.py:153)"""
    z_coarse, weights, u = _c(z_coarse), _c(weights), _c(u)
    N, Nc = z_coarse.shape
    z_f = _f(N, Nc + Nf, like=z_coarse)
    if N:
        capi.call("nvsr_importance_resample", N, Nc, Nf, capi.ptr(z_coarse), capi.ptr(weights), capi.ptr(u), capi.ptr(z_f), capi.stream())
    return z_f


@importance_resample.register_fake
def _(z_coarse, weights, Nf, u):
    return z_coarse.new_empty((z_coarse.shape[0], z_coarse.shape[1] + Nf))


# =====================================================================================================================================
# tri-plane decoder (models.py:381-421) and the render passes (train_utils.py:71-182)
# =====================================================================================================================================
@custom_op("nvsr::triplane_decode", mutates_args=(), device_types="cuda")
def triplane_decode(planes: Sequence[Tensor], consts: Sequence[float], packed: Tensor, x: Tensor, arith: int = -1) -> Tensor:
    """TwoDimPlanesModel.forward on points: x [P,6] = [xyz, viewdir] -> [P,4] = [rgb_raw, sigma_raw].  arith: NVSR_ARITH_* (-1 = the process
    default): the limb modes run the training forward's kernel on tiles of 32 points, 0 the exact-f32 MFMA kernel"""
    x = _c(x)
    sc = _scene(planes, consts)
    P = x.shape[0]
    out = _f(P, 4, like=x)
    if P:
        capi.call("nvsr_triplane_decode_arith", C.byref(sc), capi.ptr(packed), P, capi.ptr(x), capi.ptr(out), int(arith), capi.stream())
    return out


@triplane_decode.register_fake
def _(planes, consts, packed, x, arith=-1):
    return x.new_empty((x.shape[0], 4))


def _scene_ext(planes, consts, channels, align_corners, bicubic=False):
    """struct nvsr_scene_ext from N + 1 channel-last planes (N position planes, then the view-direction plane) + 10 + 6 N host constants
    (lo, range, the N 3x2 projections)"""
    n_pos = len(planes) - 1
    assert 1 <= n_pos <= capi.MAX_POSITION_PLANES, "1 .. %d position planes" % capi.MAX_POSITION_PLANES
    assert len(consts) == 10 + 6 * n_pos, "scene constants: lo[5], range[5] and a 3x2 projection per position plane"
    sc = capi.SceneExt()
    sc.num_position_planes, sc.align_corners, sc.plane_interp = n_pos, int(bool(align_corners)), int(bool(bicubic))
    for d, p in enumerate(planes):
        capi.require_cuda(p)
        cc = channels[0 if d < n_pos else 1]
        assert p.dtype == torch.float32 and p.dim() == 3 and p.shape[2] == cc and p.is_contiguous(), "planes must be channel-last [H,W,%d] f32" % cc
        sc.planes[d] = p.data_ptr()
        sc.ph[d], sc.pw[d] = p.shape[0], p.shape[1]
    _scene_box(sc, consts)
    for d in range(n_pos):
        for j in range(6):
            sc.proj[d][j] = consts[10 + 6 * d + j]
    return sc


def _scene_box(sc, consts):
    """lo[5] and range[5] of a capi.SceneExt from the head of the scene constants"""
    for i in range(5):
        sc.lo[i] = consts[i]
        sc.range[i] = consts[5 + i]
    return sc


def _generic_geometry(geometry, n_pos, natural=None):
    """(struct nvsr_decoder_geometry, floats of its natural blob); raises for an inconsistent geometry and for a `natural` of another size"""
    geo = capi.DecoderGeometry(*[int(v) for v in geometry])
    n = capi.lib().nvsr_generic_decoder_natural_floats_ext(C.byref(geo), int(n_pos))
    if n < 0:
        raise capi.NvsrError("this decoder geometry is inconsistent (the reference's own layer sizes do not admit it)")
    assert natural is None or natural.numel() == n, "natural blob: %d floats, the geometry needs %d" % (natural.numel(), n)
    return geo, n


def _generic_setup(planes, consts, natural, geometry, align_corners, coord_noise, P, bicubic=False):
    """the geometry with the natural blob's size checked, coord_noise [P,3] validated, the scene -> (geo, n_pos, floats of natural, scene)"""
    n_pos = len(planes) - 1
    geo, n = _generic_geometry(geometry, n_pos, natural)
    if coord_noise is not None:
        assert tuple(coord_noise.shape) == (P, 3) and coord_noise.dtype == torch.float32, "coord_noise: [P,3] f32"
        capi.require_cuda(coord_noise)
    return geo, n_pos, n, _scene_ext(planes, consts, (geo.plane_channels, geo.viewdir_channels), align_corners, bicubic)


# what each capacity check of _generic_call asks and says: capacity -> (entry, takes `arith`, message)
_ARITH_CAPACITY = ("the fused generic kernel does not take this decoder geometry in this arithmetic (nvsr_generic_fused_supported_arith: "
                   "beyond its capacity, or not 'f32' / 'f16x2')")
_GENERIC_CAPACITY = {
    "fused": ("nvsr_generic_fused_supported", False, "this decoder geometry is beyond the fused generic kernel's capacity "
              "(nvsr_generic_fused_supported); torch.ops.nvsr.triplane_decode_generic runs it layer by layer"),
    "arith": ("nvsr_generic_fused_supported_arith", True, _ARITH_CAPACITY),
    "occupancy": ("nvsr_generic_fused_supported_arith", True, _ARITH_CAPACITY + ": no occupancy grid for it"),
    "backward": ("nvsr_generic_backward_fused_supported", False, "this decoder geometry is beyond the fused generic backward's capacity "
                 "(nvsr_generic_backward_fused_supported); torch.ops.nvsr.triplane_decode_generic_backward runs it layer by layer"),
    "backward_arith": ("nvsr_generic_backward_fused_supported_arith", True, "the fused generic backward does not take this decoder geometry in this "
                       "arithmetic (nvsr_generic_backward_fused_supported_arith: beyond its capacity, or not 'f32' / 'f16x2'); "
                       "torch.ops.nvsr.triplane_decode_generic_backward runs every geometry layer by layer"),
}


def _generic_call(planes, consts, natural, geometry, align_corners, bicubic, x=None, coord_noise=None, capacity=None, arith=0, packed=None,
                  grad=None, packed_bwd=None):
    """The paragraph every generic operator opens with.  Makes natural, x [P,6], coord_noise [P,3], packed and grad (g_out / d_out [P,4]) f32 and
    contiguous -- the kernels take dense row-major buffers, and a view must never reach them; _generic_setup; then the `capacity` the operator
    needs (None: every geometry runs; 'fused': the f32 kernel; 'arith' / 'occupancy': the forward kernel in `arith`; 'backward': the fused
    backward; 'backward_arith': the fused backward in `arith`) and, in 'f16x2', the packed size (and the transposed blob's, packed_bwd).
    -> a namespace that holds the contiguous tensors until the call is made: geo, n_pos, n (floats of natural), sc, P, grad, arith and head =
    the arguments (scene, geometry, natural[, packed in the arith entries][, packed_bwd], P, x, coord_noise or NULL) every decode entry starts with."""
    s = SimpleNamespace(natural=_c(natural), x=_c(x), packed=_c(packed), grad=_c(grad), coord_noise=_c(coord_noise), arith=int(arith),
                        packed_bwd=_c(packed_bwd))
    s.P = 0 if x is None else s.x.shape[0]
    s.geo, s.n_pos, s.n, s.sc = _generic_setup(planes, consts, s.natural, geometry, align_corners, s.coord_noise, s.P, bicubic)
    assert s.grad is None or tuple(s.grad.shape) == (s.P, 4), "the output's gradient: [P,4]"
    lib, geo = capi.lib(), C.byref(s.geo)
    if capacity is not None:
        entry, by_arith, message = _GENERIC_CAPACITY[capacity]
        if getattr(lib, entry)(geo, s.n_pos, *([s.arith] if by_arith else [])) != 1:
            raise capi.NvsrError(message)
        if by_arith and s.arith == capi.ARITHMETIC["f16x2"]:
            assert s.packed.numel() == lib.nvsr_generic_packed_floats_ext(geo, s.n_pos), "packed blob of another geometry"
            assert packed_bwd is None or s.packed_bwd.numel() == lib.nvsr_generic_packed_bwd_floats_ext(geo, s.n_pos), \
                "transposed packed blob of another geometry"
    s.head = (C.byref(s.sc), geo, capi.ptr(s.natural)) + ((capi.ptr(s.packed),) if packed is not None else ()) + \
             ((capi.ptr(s.packed_bwd),) if packed_bwd is not None else ()) + (s.P, capi.ptr(s.x), capi.ptr(s.coord_noise))
    return s


@custom_op("nvsr::triplane_decode_generic", mutates_args=(), device_types="cuda")
def triplane_decode_generic(planes: Sequence[Tensor], consts: Sequence[float], natural: Tensor, geometry: Sequence[int], x: Tensor,
                            align_corners: bool = True, coord_noise: Optional[Tensor] = None, bicubic: bool = False) -> Tensor:
    """TwoDimPlanesModel.forward for ANY decoder geometry the reference's layer sizes admit (csrc/generic.hip).
    geometry = [plane_channels, viewdir_channels, hidden, density_layers, rgb_layers, skip_connect_every (0 = None), proj_combination
    (0 sum, 1 avg, 2 concat), viewdir_combination (0 sum, 1 avg, 2 mult, 3 concat, 4 concat_pos)]; natural = the parameters in
    state-dict order; planes channel-last: N position planes [H,W,plane_channels], then [H,W,viewdir_channels]; consts = lo[5], range[5],
    N 3x2 projections; align_corners / bicubic: grid_sample's align_corners and mode; coord_noise [P,3]: added to the normalised positions
    (point_coords_noise, models.py:291-293)."""
    s = _generic_call(planes, consts, natural, geometry, align_corners, bicubic, x, coord_noise)
    out = _f(s.P, 4, like=x)
    if s.P:
        ws = _f(capi.lib().nvsr_generic_decode_workspace_floats_ext(C.byref(s.geo), s.n_pos, s.P), like=x)
        capi.call("nvsr_generic_decode_ext", *s.head, capi.ptr(out), capi.ptr(ws), capi.stream())
    return out


@triplane_decode_generic.register_fake
def _(planes, consts, natural, geometry, x, align_corners=True, coord_noise=None, bicubic=False):
    return x.new_empty((x.shape[0], 4))


@custom_op("nvsr::triplane_decode_generic_fused", mutates_args=(), device_types="cuda")
def triplane_decode_generic_fused(planes: Sequence[Tensor], consts: Sequence[float], natural: Tensor, geometry: Sequence[int], x: Tensor,
                                  align_corners: bool = True, coord_noise: Optional[Tensor] = None, bicubic: bool = False) -> Tensor:
    """triplane_decode_generic in ONE launch, for evaluation (csrc/generic_fused.hip): the input features, every layer of both decoders and both
    heads with the activations in LDS; same arguments, the same bits in the result, no workspace and no registered autograd (training with
    decoder-weight gradients keeps triplane_decode_generic unless TwoDimPlanesModel.generic_decoder_train_route() pairs this forward with
    triplane_decode_generic_fused_backward_record; planes-only training pairs it with triplane_decode_generic_fused_backward,
    TwoDimPlanesModel.generic_train_route()).  Raises for a geometry beyond the kernel's capacity (nvsr_generic_fused_supported, include/nvsr.h: hidden <= 256,
    first-layer inputs <= 512 columns, 32 points' rows in 160 KB of LDS) -- TwoDimPlanesModel.generic_route() picks the operator."""
    s = _generic_call(planes, consts, natural, geometry, align_corners, bicubic, x, coord_noise, "fused")
    out = _f(s.P, 4, like=x)
    if s.P:
        capi.call("nvsr_generic_decode_fused_ext", *s.head, capi.ptr(out), capi.stream())
    return out


@triplane_decode_generic_fused.register_fake
def _(planes, consts, natural, geometry, x, align_corners=True, coord_noise=None, bicubic=False):
    return x.new_empty((x.shape[0], 4))


@custom_op("nvsr::pack_generic_decoder", mutates_args=(), device_types="cuda")
def pack_generic_decoder(natural: Tensor, geometry: Sequence[int], n_pos: int) -> Tensor:
    """the hidden layers of a generic geometry's natural blob -> the f16-limb fragments of the fused evaluation kernel in 'f16x2'
    (csrc/generic_fused_limb.hip; include/nvsr.h has the layout).  Evaluation only: no autograd."""
    nat = capi.f32c(natural)
    geo, _ = _generic_geometry(geometry, n_pos, nat)
    packed = _f(capi.lib().nvsr_generic_packed_floats_ext(C.byref(geo), int(n_pos)), like=nat)
    capi.call("nvsr_pack_generic_decoder_ext", C.byref(geo), int(n_pos), capi.ptr(nat), capi.ptr(packed), capi.stream())
    return packed


@pack_generic_decoder.register_fake
def _(natural, geometry, n_pos):
    geo, _ = _generic_geometry(geometry, n_pos, natural)
    return natural.new_empty((capi.lib().nvsr_generic_packed_floats_ext(C.byref(geo), int(n_pos)),), dtype=torch.float32)


@custom_op("nvsr::triplane_decode_generic_fused_arith", mutates_args=(), device_types="cuda")
def triplane_decode_generic_fused_arith(planes: Sequence[Tensor], consts: Sequence[float], natural: Tensor, packed: Tensor, geometry: Sequence[int],
                                        x: Tensor, align_corners: bool = True, coord_noise: Optional[Tensor] = None, bicubic: bool = False,
                                        arith: int = 2) -> Tensor:
    """triplane_decode_generic_fused with the arithmetic of the hidden layers as an argument: capi.ARITHMETIC['f16x2'] runs them in two f16
    limbs from `packed` (pack_generic_decoder of the same natural blob), capi.ARITHMETIC['f32'] is triplane_decode_generic_fused (`packed`
    is not read).  Every other code raises: the mode is chosen by name, never inherited.  Beyond f16x2's ranges the result is NaN and the
    range flag (capi.range_flag) is raised.  Evaluation only: no autograd."""
    s = _generic_call(planes, consts, natural, geometry, align_corners, bicubic, x, coord_noise, "arith", arith, packed)
    out = _f(s.P, 4, like=x)
    if s.P:
        capi.call("nvsr_generic_decode_fused_arith_ext", *s.head, capi.ptr(out), s.arith, capi.stream())
    return out


@triplane_decode_generic_fused_arith.register_fake
def _(planes, consts, natural, packed, geometry, x, align_corners=True, coord_noise=None, bicubic=False, arith=2):
    return x.new_empty((x.shape[0], 4))


def _generic_list_phase(entry, raw, planes, consts, natural, packed, geometry, x, index, count, align_corners, coord_noise, bicubic, arith, max_count):
    """a phase of the fused kernel on the points x[index[i]], i < count, written IN PLACE into raw [P,4] (`entry`: the colour phase or the
    listed density phase): the list's checks, the launch size n = max_count or min(len(index), P), the shared setup, the call"""
    P = x.shape[0]
    capi.require_cuda(raw, index, count)
    assert raw.dtype == torch.float32 and tuple(raw.shape) == (P, 4) and raw.is_contiguous(), "raw: contiguous [P,4] f32 (written in place)"
    assert index.dtype == torch.int32 and index.dim() == 1 and index.is_contiguous(), "index: contiguous int32 [n]"
    assert count.dtype == torch.int32 and count.numel() == 1, "count: int32 [1]"
    n = min(index.numel(), P) if max_count < 0 else int(max_count)
    assert n <= index.numel() and n <= P, "max_count: at most len(index) and P"
    s = _generic_call(planes, consts, natural, geometry, align_corners, bicubic, x, coord_noise, "arith", arith, packed)
    if n:
        capi.call(entry, *s.head, capi.ptr(index), capi.ptr(count), n, capi.ptr(raw), s.arith, capi.stream())


@custom_op("nvsr::triplane_density_generic_fused_arith", mutates_args=(), device_types="cuda")
def triplane_density_generic_fused_arith(planes: Sequence[Tensor], consts: Sequence[float], natural: Tensor, packed: Tensor, geometry: Sequence[int],
                                         x: Tensor, align_corners: bool = True, coord_noise: Optional[Tensor] = None, bicubic: bool = False,
                                         arith: int = 0) -> Tensor:
    """the DENSITY phase of triplane_decode_generic_fused_arith (same arguments; `packed` is read in 'f16x2' only and may be empty otherwise):
    the density decoder on all P points -> raw [P,4] = [+0, +0, +0, sigma_raw] per row, sigma_raw with the one-launch operator's bits.  A
    compositor reads the tensor as it is; triplane_colour_generic_fused_arith completes it.  Evaluation only: no autograd."""
    s = _generic_call(planes, consts, natural, geometry, align_corners, bicubic, x, coord_noise, "arith", arith, packed)
    raw = _f(s.P, 4, like=x)
    if s.P:
        capi.call("nvsr_generic_decode_fused_density_arith_ext", *s.head, capi.ptr(raw), s.arith, capi.stream())
    return raw


@triplane_density_generic_fused_arith.register_fake
def _(planes, consts, natural, packed, geometry, x, align_corners=True, coord_noise=None, bicubic=False, arith=0):
    return x.new_empty((x.shape[0], 4))


@custom_op("nvsr::triplane_colour_generic_fused_arith", mutates_args=("raw",), device_types="cuda")
def triplane_colour_generic_fused_arith(raw: Tensor, planes: Sequence[Tensor], consts: Sequence[float], natural: Tensor, packed: Tensor,
                                        geometry: Sequence[int], x: Tensor, index: Tensor, count: Tensor, align_corners: bool = True,
                                        coord_noise: Optional[Tensor] = None, bicubic: bool = False, arith: int = 0, max_count: int = -1) -> None:
    """the COLOUR phase: the colour decoder on the points x[index[i]], i < count, written IN PLACE into raw[index[i], 0:3] with the one-launch
    operator's bits; column 3 and every other row of raw [P,4] stay as they are.  index: int32 [>= max_count] on the device, distinct, any
    order; count: int32 [1] on the device, read by the kernel (generic_live_list makes both; no host synchronisation); max_count: what the
    launch is sized for, -1 = min(len(index), P).  Entries of index at or beyond count are not read.  Evaluation only: no autograd."""
    _generic_list_phase("nvsr_generic_decode_fused_colour_arith_ext", raw, planes, consts, natural, packed, geometry, x, index, count, align_corners,
                        coord_noise, bicubic, arith, max_count)


@triplane_colour_generic_fused_arith.register_fake
def _(raw, planes, consts, natural, packed, geometry, x, index, count, align_corners=True, coord_noise=None, bicubic=False, arith=0, max_count=-1):
    return None


@custom_op("nvsr::generic_live_list", mutates_args=(), device_types="cuda")
def generic_live_list(w: Tensor) -> Tuple[Tensor, Tensor]:
    """weights of any shape (P values) -> (index int32 [P], count int32 [1]): index[:count] = the flat positions p with not (w[p] == 0) in
    ascending order (NaN is live, +0.0 and -0.0 are dead), both on the device (csrc/generic_live.hip: no atomics, the same list on every run).
    index[count:] is not written."""
    w = _c(w)
    P = w.numel()
    index = torch.empty((P,), dtype=torch.int32, device=w.device)
    count = torch.empty((1,), dtype=torch.int32, device=w.device)
    nbytes = capi.lib().nvsr_generic_live_list_workspace_bytes(P)
    if nbytes < 0:
        raise capi.NvsrError("generic_live_list: at most 2^31 - 1 weights")
    ws = torch.empty((nbytes // 4,), dtype=torch.int32, device=w.device)
    capi.call("nvsr_generic_live_list", P, capi.ptr(w), capi.ptr(index), capi.ptr(count), capi.ptr(ws), capi.stream())
    return index, count


@generic_live_list.register_fake
def _(w):
    return w.new_empty((w.numel(),), dtype=torch.int32), w.new_empty((1,), dtype=torch.int32)


# ---- occupancy grid of a generic geometry (include/nvsr.h, "generic decoder, occupancy grid"): opt-in, evaluation only ---------------------
@custom_op("nvsr::generic_occupancy_build", mutates_args=(), device_types="cuda")
def generic_occupancy_build(planes: Sequence[Tensor], consts: Sequence[float], natural: Tensor, packed: Tensor, geometry: Sequence[int], G: int,
                            K: int, threshold: float, dilate: int, align_corners: bool = True, bicubic: bool = False, arith: int = 0) -> Tensor:
    """occupancy_build for ANY decoder geometry the fused generic kernel holds: the same grid layout, probes, marks and dilation, with the
    density phase (triplane_density_generic_fused_arith, `arith` = 'f32' or 'f16x2'; `packed` is read in 'f16x2' only) as the decoder.
    -> int32 [ceil(G^3 / 32)]"""
    s = _generic_call(planes, consts, natural, geometry, align_corners, bicubic, capacity="occupancy", arith=arith, packed=packed)
    words = capi.lib().nvsr_occupancy_words(int(G))
    if words <= 0:
        raise capi.NvsrError("nvsr_generic_occupancy_build_ext failed: %s" % capi._STATUS[1])
    grid = torch.empty(words, dtype=torch.int32, device=natural.device)
    ws = _f(max(int(capi.lib().nvsr_occupancy_workspace_floats(int(G), int(K))), 4), like=natural)
    capi.call("nvsr_generic_occupancy_build_ext", *s.head[:4], int(G), int(K), float(threshold), int(dilate), s.arith, capi.ptr(grid), capi.ptr(ws),
              capi.stream())
    return grid


@generic_occupancy_build.register_fake
def _(planes, consts, natural, packed, geometry, G, K, threshold, dilate, align_corners=True, bicubic=False, arith=0):
    return natural.new_empty(((G ** 3 + 31) // 32,), dtype=torch.int32)


@custom_op("nvsr::generic_occupancy_keep", mutates_args=(), device_types="cuda")
def generic_occupancy_keep(consts: Sequence[float], x: Tensor, grid: Tensor, G: int, raw: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """the keep mask of points x [P,6] under `grid` (G^3 bits) in the box of `consts` (lo[5], range[5], then the projections, which are not
    read) -> (keep f32 [P], raw f32 [P,4]).  keep[p] = 1.0 iff a normalised coordinate of the point is NaN or lies outside the box (|n| > 1),
    or the bit of its cell is set; else 0.0, and the row of raw is [+0, +0, +0, capi.CULLED_SIGMA].  Kept rows are not written: they are
    those of a copy of the `raw` handed in, or uninitialised without one -- triplane_density_list_generic_fused_arith fills them.
    generic_live_list(keep) gives the ascending kept list."""
    x = _c(x)
    P = x.shape[0]
    assert x.dim() == 2 and x.shape[1] == 6, "x: [P,6]"
    assert len(consts) >= 10 and (len(consts) - 10) % 6 == 0, "scene constants: lo[5], range[5] (and the projections)"
    grid = _grid(grid, int(G))
    if raw is None:
        out = _f(P, 4, like=x)
    else:
        assert raw.dtype == torch.float32 and tuple(raw.shape) == (P, 4), "raw: [P,4] f32"
        out = raw.contiguous().clone()
    keep = _f(P, like=x)
    sc = _scene_box(capi.SceneExt(), consts)
    sc.num_position_planes = max((len(consts) - 10) // 6, 1)
    if P:
        capi.call("nvsr_generic_occupancy_keep", C.byref(sc), P, capi.ptr(x), capi.ptr(grid), int(G), capi.ptr(keep), capi.ptr(out), capi.stream())
    return keep, out


@generic_occupancy_keep.register_fake
def _(consts, x, grid, G, raw=None):
    return x.new_empty((x.shape[0],)), x.new_empty((x.shape[0], 4))


@custom_op("nvsr::triplane_density_list_generic_fused_arith", mutates_args=("raw",), device_types="cuda")
def triplane_density_list_generic_fused_arith(raw: Tensor, planes: Sequence[Tensor], consts: Sequence[float], natural: Tensor, packed: Tensor,
                                              geometry: Sequence[int], x: Tensor, index: Tensor, count: Tensor, align_corners: bool = True,
                                              coord_noise: Optional[Tensor] = None, bicubic: bool = False, arith: int = 0, max_count: int = -1) -> None:
    """the DENSITY phase on the points x[index[i]], i < count: the row [+0, +0, +0, sigma_raw] written IN PLACE into raw[index[i]], sigma_raw
    with the one-launch operator's bits; every other row of raw [P,4] stays as it is.  index, count, max_count: as for
    triplane_colour_generic_fused_arith (the kept list of generic_occupancy_keep through generic_live_list).  Evaluation only: no autograd."""
    _generic_list_phase("nvsr_generic_decode_fused_density_list_arith_ext", raw, planes, consts, natural, packed, geometry, x, index, count,
                        align_corners, coord_noise, bicubic, arith, max_count)


@triplane_density_list_generic_fused_arith.register_fake
def _(raw, planes, consts, natural, packed, geometry, x, index, count, align_corners=True, coord_noise=None, bicubic=False, arith=0, max_count=-1):
    return None


def _gradient_planes(planes, want):
    """the plane gradients of a generic backward: zeros like the plane where wanted, an empty tensor where not -> (the tensors, their pointers
    as the C entry's float* const* with NULL for a plane that is not wanted, whether any is wanted)"""
    want = [bool(w) for w in want]
    assert len(want) == len(planes)
    g_pl = [torch.zeros_like(pl) if w else _f(0, like=pl) for pl, w in zip(planes, want)]
    return g_pl, (C.c_void_p * len(planes))(*[g.data_ptr() if w else None for g, w in zip(g_pl, want)]), any(want)


@custom_op("nvsr::triplane_decode_generic_backward", mutates_args=(), device_types="cuda")
def triplane_decode_generic_backward(planes: Sequence[Tensor], consts: Sequence[float], natural: Tensor, geometry: Sequence[int], x: Tensor,
                                     g_out: Tensor, want_natural: bool, want_planes: Sequence[bool], align_corners: bool = True,
                                     coord_noise: Optional[Tensor] = None, bicubic: bool = False) -> List[Tensor]:
    """Backward of triplane_decode_generic (csrc/generic.hip; the reference: torch.autograd through models.py:381-421): g_out [P,4] ->
    [d_natural, d_plane0 .. d_planeN] (channel-last like the planes; a gradient that is not wanted comes back as an empty tensor)."""
    s = _generic_call(planes, consts, natural, geometry, align_corners, bicubic, x, coord_noise, grad=g_out)
    g_pl, d_planes, any_plane = _gradient_planes(planes, want_planes)
    g_nat = torch.zeros(s.n if want_natural else 0, dtype=torch.float32, device=x.device)
    if s.P and (want_natural or any_plane):
        ws = _f(capi.lib().nvsr_generic_decode_backward_workspace_floats_ext(C.byref(s.geo), s.n_pos, s.P), like=x)
        capi.call("nvsr_generic_decode_backward_ext", *s.head, capi.ptr(s.grad), capi.ptr(g_nat) if want_natural else None, d_planes, capi.ptr(ws),
                  capi.stream())
    return [g_nat] + g_pl


@triplane_decode_generic_backward.register_fake
def _(planes, consts, natural, geometry, x, g_out, want_natural, want_planes, align_corners=True, coord_noise=None, bicubic=False):
    return [natural.new_empty(natural.numel() if want_natural else 0)] + [pl.new_empty(pl.shape if w else (0,)) for pl, w in zip(planes, want_planes)]


@custom_op("nvsr::triplane_decode_generic_fused_backward", mutates_args=(), device_types="cuda")
def triplane_decode_generic_fused_backward(planes: Sequence[Tensor], consts: Sequence[float], natural: Tensor, geometry: Sequence[int], x: Tensor,
                                           d_out: Tensor, need_planes: Sequence[bool], align_corners: bool = True,
                                           coord_noise: Optional[Tensor] = None, bicubic: bool = False) -> List[Tensor]:
    """The PLANE gradients of triplane_decode_generic in ONE launch, exact f32, for a decoder whose parameters take no gradient
    (csrc/generic_fused_bwd.hip; the reference: torch.autograd through models.py:381-421): d_out [P,4] -> [d_plane0 .. d_planeN], channel-last
    like the planes; a gradient that is not wanted comes back as an empty tensor and costs no atomics.  No workspace.  Raises for a geometry
    beyond the kernel's capacity (nvsr_generic_backward_fused_supported, include/nvsr.h) -- TwoDimPlanesModel.generic_train_route() picks the
    operator; triplane_decode_generic_backward runs every geometry, and the decoder's gradients, layer by layer."""
    s = _generic_call(planes, consts, natural, geometry, align_corners, bicubic, x, coord_noise, "backward", grad=d_out)
    g_pl, d_planes, any_plane = _gradient_planes(planes, need_planes)
    if s.P and any_plane:
        capi.call("nvsr_generic_decode_backward_fused_ext", *s.head, capi.ptr(s.grad), d_planes, capi.stream())
    return g_pl


@triplane_decode_generic_fused_backward.register_fake
def _(planes, consts, natural, geometry, x, d_out, need_planes, align_corners=True, coord_noise=None, bicubic=False):
    return [pl.new_empty(pl.shape if w else (0,)) for pl, w in zip(planes, need_planes)]


@custom_op("nvsr::triplane_decode_generic_fused_backward_record", mutates_args=(), device_types="cuda")
def triplane_decode_generic_fused_backward_record(planes: Sequence[Tensor], consts: Sequence[float], natural: Tensor, geometry: Sequence[int],
                                                  x: Tensor, d_out: Tensor, want_natural: bool, want_planes: Sequence[bool],
                                                  align_corners: bool = True, coord_noise: Optional[Tensor] = None,
                                                  bicubic: bool = False) -> List[Tensor]:
    """triplane_decode_generic_backward on the fused backward (csrc/generic_fused_bwd.hip, nvsr_generic_decode_backward_fused_record_ext; the
    reference: torch.autograd through models.py:381-421), exact f32: per chunk one launch that scatters the planes' gradients and records the
    decoder inputs, every hidden activation and every gated dZ with the layered route's bits, then the layered route's weight-gradient
    contractions on that record.  d_out [P,4] -> [d_natural, d_plane0 .. d_planeN] (a gradient that is not wanted comes back as an empty
    tensor).  d_natural is the layered operator's up to the order of its float atomics (bit for bit for P <= 512).  Raises for a geometry
    beyond the kernel's capacity (nvsr_generic_backward_fused_supported) -- TwoDimPlanesModel.generic_decoder_train_route() picks the operator."""
    s = _generic_call(planes, consts, natural, geometry, align_corners, bicubic, x, coord_noise, "backward", grad=d_out)
    g_pl, d_planes, any_plane = _gradient_planes(planes, want_planes)
    g_nat = torch.zeros(s.n if want_natural else 0, dtype=torch.float32, device=x.device)
    if s.P and (want_natural or any_plane):
        ws = None
        if want_natural:
            ws = _f(capi.lib().nvsr_generic_backward_fused_record_workspace_floats_ext(C.byref(s.geo), s.n_pos, s.P), like=x)
        capi.call("nvsr_generic_decode_backward_fused_record_ext", *s.head, capi.ptr(s.grad), capi.ptr(g_nat) if want_natural else None, d_planes,
                  capi.ptr(ws), capi.stream())
    return [g_nat] + g_pl


@triplane_decode_generic_fused_backward_record.register_fake
def _(planes, consts, natural, geometry, x, d_out, want_natural, want_planes, align_corners=True, coord_noise=None, bicubic=False):
    return [natural.new_empty(natural.numel() if want_natural else 0)] + [pl.new_empty(pl.shape if w else (0,)) for pl, w in zip(planes, want_planes)]


@custom_op("nvsr::pack_generic_decoder_bwd", mutates_args=(), device_types="cuda")
def pack_generic_decoder_bwd(natural: Tensor, geometry: Sequence[int], n_pos: int) -> Tensor:
    """the hidden layers of a generic geometry's natural blob -> the TRANSPOSED f16-limb fragments of the fused backward in 'f16x2'
    (csrc/generic_fused_bwd_limb.hip; include/nvsr.h has the layout).  No autograd: the decoder is frozen where this blob is read."""
    nat = capi.f32c(natural)
    geo, _ = _generic_geometry(geometry, n_pos, nat)
    packed = _f(capi.lib().nvsr_generic_packed_bwd_floats_ext(C.byref(geo), int(n_pos)), like=nat)
    capi.call("nvsr_pack_generic_decoder_bwd_ext", C.byref(geo), int(n_pos), capi.ptr(nat), capi.ptr(packed), capi.stream())
    return packed


@pack_generic_decoder_bwd.register_fake
def _(natural, geometry, n_pos):
    geo, _ = _generic_geometry(geometry, n_pos, natural)
    return natural.new_empty((capi.lib().nvsr_generic_packed_bwd_floats_ext(C.byref(geo), int(n_pos)),), dtype=torch.float32)


@custom_op("nvsr::triplane_decode_generic_fused_backward_arith", mutates_args=(), device_types="cuda")
def triplane_decode_generic_fused_backward_arith(planes: Sequence[Tensor], consts: Sequence[float], natural: Tensor, packed: Tensor, packed_bwd: Tensor,
                                                 geometry: Sequence[int], x: Tensor, d_out: Tensor, need_planes: Sequence[bool],
                                                 align_corners: bool = True, coord_noise: Optional[Tensor] = None, bicubic: bool = False,
                                                 arith: int = 2) -> List[Tensor]:
    """triplane_decode_generic_fused_backward with the arithmetic of the hidden layers as an argument: capi.ARITHMETIC['f16x2'] is the backward of
    triplane_decode_generic_fused_arith in 'f16x2' -- the forward recomputed in two f16 limbs from `packed`, the transposed layers in two f16
    limbs from `packed_bwd` (pack_generic_decoder_bwd of the same natural blob) under one exact power-of-two scale per point and layer
    (csrc/generic_fused_bwd_limb.hip); capi.ARITHMETIC['f32'] is triplane_decode_generic_fused_backward (the blobs are not read).  Every other
    code raises: the mode is chosen by name.  Beyond f16x2's ranges, or with a non-finite cotangent, the gradients are NaN and the range flag
    (capi.range_flag) is raised."""
    s = _generic_call(planes, consts, natural, geometry, align_corners, bicubic, x, coord_noise, "backward_arith", arith, packed, d_out, packed_bwd)
    g_pl, d_planes, any_plane = _gradient_planes(planes, need_planes)
    if s.P and any_plane:
        capi.call("nvsr_generic_decode_backward_fused_arith_ext", *s.head, capi.ptr(s.grad), d_planes, s.arith, capi.stream())
    return g_pl


@triplane_decode_generic_fused_backward_arith.register_fake
def _(planes, consts, natural, packed, packed_bwd, geometry, x, d_out, need_planes, align_corners=True, coord_noise=None, bicubic=False, arith=2):
    return [pl.new_empty(pl.shape if w else (0,)) for pl, w in zip(planes, need_planes)]


@custom_op("nvsr::ray_points", mutates_args=(), device_types="cuda")
def ray_points(rays: Tensor, z: Tensor) -> Tensor:
    """run_network's model input (train_utils.py:15-64,111): [N*S,6] = [ro + rd * z, viewdir] from packed rays [N,11] and depths [N,S]"""
    rays, z = _c(rays), _c(z)
    N, S = z.shape
    x = _f(N * S, 6, like=rays)
    if N:
        capi.call("nvsr_ray_points", N, S, capi.ptr(rays), capi.ptr(z), capi.ptr(x), capi.stream())
    return x


@ray_points.register_fake
def _(rays, z):
    return rays.new_empty((z.shape[0] * z.shape[1], 6))


@custom_op("nvsr::render_pass", mutates_args=(), device_types="cuda")
def render_pass(planes: Sequence[Tensor], consts: Sequence[float], packed: Tensor, rays: Tensor, z: Tensor, noise: Optional[Tensor],
                white: bool, want_weights: bool, arithmetic: int) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """run_network + model + volume_render_radiance_field of one pass, fused (no [N,S,*] tensor reaches HBM):
    rays [N,11], z [N,S] -> rgb [N,3], disp [N], acc [N], weights [N,S] (empty unless want_weights)"""
    rays, z, noise = _c(rays), _c(z), _c(noise)
    sc = _scene(planes, consts)
    N, S = z.shape
    rgb, disp, acc = _f(N, 3, like=rays), _f(N, like=rays), _f(N, like=rays)
    w = _f(N, S, like=rays) if want_weights else _f(0, like=rays)
    if N:
        capi.call("nvsr_render_pass_arith", C.byref(sc), capi.ptr(packed), N, S, capi.ptr(rays), capi.ptr(z), capi.ptr(noise), int(white),
                  capi.ptr(rgb), capi.ptr(disp), capi.ptr(acc), capi.ptr(w) if want_weights else None, None, None, arithmetic, capi.stream())
    return rgb, disp, acc, w


@render_pass.register_fake
def _(planes, consts, packed, rays, z, noise, white, want_weights, arithmetic):
    N, S = z.shape
    return rays.new_empty((N, 3)), rays.new_empty((N,)), rays.new_empty((N,)), rays.new_empty((N, S) if want_weights else (0,))


@custom_op("nvsr::render_rays", mutates_args=(), device_types="cuda")
def render_rays(planes: Sequence[Tensor], consts: Sequence[float], packed_coarse: Tensor, packed_fine: Optional[Tensor], rays: Tensor,
                Nc: int, Nf: int, lindisp: bool, white: bool, t_rand: Optional[Tensor], u: Optional[Tensor], noise_coarse: Optional[Tensor],
                noise_fine: Optional[Tensor], arithmetic: int) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    """predict_and_render_radiance for a ray block (inference): coarse depths -> coarse pass -> importance resampling -> fine pass.
    -> rgb_c, disp_c, acc_c, rgb_f, disp_f, acc_f (the fine ones empty when Nf == 0)"""
    rays, t_rand, u, noise_coarse, noise_fine = _c(rays), _c(t_rand), _c(u), _c(noise_coarse), _c(noise_fine)
    sc = _scene(planes, consts)
    N = rays.shape[0]
    rgb_c, disp_c, acc_c = _f(N, 3, like=rays), _f(N, like=rays), _f(N, like=rays)
    if Nf > 0:
        rgb_f, disp_f, acc_f = _f(N, 3, like=rays), _f(N, like=rays), _f(N, like=rays)
    else:
        rgb_f, disp_f, acc_f = _f(0, 3, like=rays), _f(0, like=rays), _f(0, like=rays)
    # one decoder for both passes (models.fine.type == 'use_same'): the fine pass evaluates the importance samples only (nvsr.h) -- but in
    # 'f16' (one f16 limb), which the shared route does not have: such a frame takes the two-decoder route with the blob given twice
    if N and Nf > 0 and packed_fine is not None and packed_fine.data_ptr() == packed_coarse.data_ptr() and arithmetic != capi.RENDER_ARITHMETIC["f16"]:
        ws = _f(capi.lib().nvsr_render_shared_workspace_floats(N, Nc, Nf), like=rays)
        capi.call("nvsr_render_rays_shared_arith", C.byref(sc), capi.ptr(packed_coarse), N, Nc, Nf, capi.ptr(rays), int(lindisp), int(white),
                  capi.ptr(t_rand), capi.ptr(u), capi.ptr(noise_coarse), capi.ptr(noise_fine), capi.ptr(rgb_c), capi.ptr(disp_c), capi.ptr(acc_c),
                  capi.ptr(rgb_f), capi.ptr(disp_f), capi.ptr(acc_f), capi.ptr(ws), arithmetic, capi.stream())
    elif N:
        ws = _f(capi.lib().nvsr_render_workspace_floats(N, Nc, Nf), like=rays)
        capi.call("nvsr_render_rays_arith", C.byref(sc), capi.ptr(packed_coarse), capi.ptr(packed_fine), N, Nc, Nf, capi.ptr(rays), int(lindisp),
                  int(white), capi.ptr(t_rand), capi.ptr(u), capi.ptr(noise_coarse), capi.ptr(noise_fine), capi.ptr(rgb_c), capi.ptr(disp_c),
                  capi.ptr(acc_c), capi.ptr(rgb_f) if Nf > 0 else None, capi.ptr(disp_f) if Nf > 0 else None,
                  capi.ptr(acc_f) if Nf > 0 else None, capi.ptr(ws), arithmetic, capi.stream())
    return rgb_c, disp_c, acc_c, rgb_f, disp_f, acc_f


@render_rays.register_fake
def _(planes, consts, packed_coarse, packed_fine, rays, Nc, Nf, lindisp, white, t_rand, u, noise_coarse, noise_fine, arithmetic):
    N = rays.shape[0]
    M = N if Nf > 0 else 0
    e = rays.new_empty
    return e((N, 3)), e((N,)), e((N,)), e((M, 3)), e((M,)), e((M,))


# ---- occupancy grid (csrc/occupancy.hip; include/nvsr.h, "Occupancy grid"): opt-in, evaluation only -------------------------------------
def _grid(grid, G):
    """a grid tensor of an operator: int32 [ceil(G^3 / 32)] on the GPU, or None"""
    if grid is None:
        return None
    capi.require_cuda(grid)
    assert grid.dtype == torch.int32 and grid.is_contiguous() and grid.numel() == (G ** 3 + 31) // 32, "grid: int32 [ceil(G^3 / 32)]"
    return grid


@custom_op("nvsr::occupancy_build", mutates_args=(), device_types="cuda")
def occupancy_build(planes: Sequence[Tensor], consts: Sequence[float], packed: Tensor, G: int, K: int, threshold: float, dilate: int,
                    arith: int = -1) -> Tensor:
    """The occupancy grid of (planes, decoder): G^3 bits over the scene's box, cell (ix, iy, iz) = bit i & 31 of word i >> 5, i = (iz G + iy) G + ix.
    A bit is set iff one of the cell's K^3 probes has sigma_raw > threshold (or NaN), then `dilate` rounds of a 3x3x3 OR.  Approximate by
    nature: K, threshold and dilate are the caller's knobs.  -> int32 [ceil(G^3 / 32)]"""
    sc = _scene(planes, consts)
    words = capi.lib().nvsr_occupancy_words(int(G))
    if words <= 0:
        raise capi.NvsrError("nvsr_occupancy_build failed: %s" % capi._STATUS[1])
    grid = torch.empty(words, dtype=torch.int32, device=packed.device)
    ws = _f(max(int(capi.lib().nvsr_occupancy_workspace_floats(int(G), int(K))), 4), like=packed)
    capi.call("nvsr_occupancy_build", C.byref(sc), capi.ptr(packed), int(G), int(K), float(threshold), int(dilate), int(arith), capi.ptr(grid), capi.ptr(ws),
              capi.stream())
    return grid


@occupancy_build.register_fake
def _(planes, consts, packed, G, K, threshold, dilate, arith=-1):
    return packed.new_empty(((G ** 3 + 31) // 32,), dtype=torch.int32)


@custom_op("nvsr::render_pass_occupancy", mutates_args=(), device_types="cuda")
def render_pass_occupancy(planes: Sequence[Tensor], consts: Sequence[float], packed: Tensor, rays: Tensor, z: Optional[Tensor], S: int, lindisp: bool,
                          white: bool, want_weights: bool, grid: Tensor, G: int, arithmetic: int) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """render_pass with the density decoder run only on the samples whose cell of `grid` is set (limb arithmetics, no noise).  z [N,S], or
    None: the S un-jittered coarse depths, formed in the kernel (lindisp; the weights are then always written)
    -> rgb [N,3], disp [N], acc [N], weights [N,S] (empty unless want_weights)"""
    rays, z = _c(rays), _c(z)
    sc = _scene(planes, consts)
    N = rays.shape[0]
    assert z is None or tuple(z.shape) == (N, S)
    want_weights = bool(want_weights) or z is None
    rgb, disp, acc = _f(N, 3, like=rays), _f(N, like=rays), _f(N, like=rays)
    w = _f(N, S, like=rays) if want_weights else _f(0, like=rays)
    if N:
        capi.call("nvsr_render_pass_occupancy_arith", C.byref(sc), capi.ptr(packed), N, int(S), capi.ptr(rays), capi.ptr(z), int(lindisp), int(white),
                  capi.ptr(rgb), capi.ptr(disp), capi.ptr(acc), capi.ptr(w) if want_weights else None, None, capi.ptr(_grid(grid, G)), int(G), arithmetic,
                  capi.stream())
    return rgb, disp, acc, w


@render_pass_occupancy.register_fake
def _(planes, consts, packed, rays, z, S, lindisp, white, want_weights, grid, G, arithmetic):
    N = rays.shape[0]
    return rays.new_empty((N, 3)), rays.new_empty((N,)), rays.new_empty((N,)), rays.new_empty((N, S) if (want_weights or z is None) else (0,))


@custom_op("nvsr::render_rays_occupancy", mutates_args=(), device_types="cuda")
def render_rays_occupancy(planes: Sequence[Tensor], consts: Sequence[float], packed_coarse: Tensor, packed_fine: Optional[Tensor], rays: Tensor,
                          Nc: int, Nf: int, lindisp: bool, white: bool, t_rand: Optional[Tensor], u: Optional[Tensor], grid_coarse: Optional[Tensor],
                          G_coarse: int, grid_fine: Optional[Tensor], G_fine: int,
                          arithmetic: int) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    """render_rays (without noise) with an occupancy grid per pass; a pass whose grid is None runs the plain route, and below
    capi.fused_min_rays() rays the grids are ignored.  Two decoders always: the shared-decoder frame has no occupancy route."""
    rays, t_rand, u = _c(rays), _c(t_rand), _c(u)
    sc = _scene(planes, consts)
    N = rays.shape[0]
    rgb_c, disp_c, acc_c = _f(N, 3, like=rays), _f(N, like=rays), _f(N, like=rays)
    M = N if Nf > 0 else 0
    rgb_f, disp_f, acc_f = _f(M, 3, like=rays), _f(M, like=rays), _f(M, like=rays)
    if N:
        ws = _f(capi.lib().nvsr_render_workspace_floats(N, Nc, Nf), like=rays)
        capi.call("nvsr_render_rays_occupancy_arith", C.byref(sc), capi.ptr(packed_coarse), capi.ptr(packed_fine), N, Nc, Nf, capi.ptr(rays), int(lindisp),
                  int(white), capi.ptr(t_rand), capi.ptr(u), capi.ptr(rgb_c), capi.ptr(disp_c), capi.ptr(acc_c), capi.ptr(rgb_f) if Nf > 0 else None,
                  capi.ptr(disp_f) if Nf > 0 else None, capi.ptr(acc_f) if Nf > 0 else None, capi.ptr(ws), capi.ptr(_grid(grid_coarse, G_coarse)),
                  int(G_coarse), capi.ptr(_grid(grid_fine, G_fine)), int(G_fine), arithmetic, capi.stream())
    return rgb_c, disp_c, acc_c, rgb_f, disp_f, acc_f


@render_rays_occupancy.register_fake
def _(planes, consts, packed_coarse, packed_fine, rays, Nc, Nf, lindisp, white, t_rand, u, grid_coarse, G_coarse, grid_fine, G_fine, arithmetic):
    N = rays.shape[0]
    M = N if Nf > 0 else 0
    e = rays.new_empty
    return e((N, 3)), e((N,)), e((N,)), e((M, 3)), e((M,)), e((M,))


@custom_op("nvsr::decode_rays", mutates_args=(), device_types="cuda")
def decode_rays(planes: Sequence[Tensor], consts: Sequence[float], packed: Tensor, rays: Tensor, z: Tensor, want_gates: bool,
                want_record: bool, arithmetic: int) -> Tuple[Tensor, Tensor, Tensor]:
    """decoder outputs of every sample of every ray, tiled over (ray block, sample): raw [N,S,4]; with want_gates the ReLU gates of every
    layer ([N,S,32] int32, 128 B per point) and with want_record the layer inputs (9.2 KB per point) the backward operators consume"""
    rays, z = _c(rays), _c(z)
    sc = _scene(planes, consts)
    N, S = z.shape
    raw = _f(N, S, 4, like=rays)
    gates = torch.empty((N, S, 32) if (want_gates or want_record) else (0,), dtype=torch.int32, device=rays.device)
    rec = _f(capi.lib().nvsr_decoder_record_floats(N, S) if want_record else 0, like=rays)
    if N:
        capi.call("nvsr_decode_rays_arith", C.byref(sc), capi.ptr(packed), N, S, capi.ptr(rays), capi.ptr(z), capi.ptr(raw),
                  capi.ptr(_none_if_empty(gates)), capi.ptr(_none_if_empty(rec)), arithmetic, capi.stream())
    return raw, gates, rec


@decode_rays.register_fake
def _(planes, consts, packed, rays, z, want_gates, want_record, arithmetic):
    N, S = z.shape
    nrec = capi.lib().nvsr_decoder_record_floats(int(N), int(S)) if want_record else 0      # (host-side size arithmetic of the library)
    return (rays.new_empty((N, S, 4)), rays.new_empty((N, S, 32) if (want_gates or want_record) else (0,), dtype=torch.int32),
            rays.new_empty((nrec,)))


def _decode_rays_backward_launch(planes, consts, packed, packed_bwd, rays, z, g_raw, gates, record, need, arithmetic, grads):
    """the gate-driven backward scattering into `grads` (channel-last gradient planes, ADDED to; entries of planes that need no gradient ignored)"""
    rays, z, g_raw = _c(rays), _c(z), _c(g_raw)
    sc = _scene(planes, consts)
    N, S = z.shape
    if N == 0 or (not any(need) and record is None):
        return
    gptrs = (C.c_void_p * 4)(*[g.data_ptr() if need[d] else None for d, g in enumerate(grads)]) if any(need) else None
    # per-tile rows of the view-direction plane's gradient (summed per ray before they touch the plane)
    view_ws = _f(N * S * PC, like=rays) if (gptrs is not None and need[3]) else None
    capi.call("nvsr_render_pass_backward_gates_arith", C.byref(sc), capi.ptr(packed), capi.ptr(packed_bwd), N, S, capi.ptr(rays), capi.ptr(z),
              capi.ptr(g_raw), capi.ptr(gates), gptrs, capi.ptr(view_ws), capi.ptr(record), arithmetic, capi.stream())


def zero_planes_like(planes, need, like):
    """zero gradient planes laid out like `planes` (empty tensors where need[d] is False) for decode_rays_backward_: contiguous planes are
    carved out of ONE zero-filled allocation (one fill kernel per step instead of four; every plane starts on a 16-byte boundary).  (An
    operator may not RETURN tensors that share a storage, so the functional decode_rays_backward fills its four planes one by one.)"""
    wanted = [p for d, p in enumerate(planes) if need[d]]
    if len(wanted) < 2 or not all(p.is_contiguous() and p.dtype == torch.float32 for p in wanted):
        return [torch.zeros_like(p) if need[d] else _f(0, like=like) for d, p in enumerate(planes)]
    sizes = [(p.numel() + 3) // 4 * 4 for p in wanted]
    flat = torch.zeros(sum(sizes), dtype=torch.float32, device=wanted[0].device)
    out, off = [], 0
    for d, p in enumerate(planes):
        if not need[d]:
            out.append(_f(0, like=like))
            continue
        out.append(flat[off: off + p.numel()].view(p.shape))
        off += (p.numel() + 3) // 4 * 4
    return out


def _check_grads_layout(who, planes, need, grads, contiguous):
    """the gradient planes an in-place backward adds into: float32 CUDA tensors shaped like the planes `need` names, with the planes' strides
    (the atomic kernel indexes both alike) or, contiguous=True, dense (nvsr_rows_scatter's layout)"""
    for d, (g, p) in enumerate(zip(grads, planes)):
        if need[d] and (g.shape != p.shape or g.dtype != torch.float32 or not g.is_cuda
                        or not (g.is_contiguous() if contiguous else g.stride() == p.stride())):
            raise ValueError("%s: grads[%d] must be a %sfloat32 CUDA tensor %s planes[%d]"
                             % (who, d, "contiguous " if contiguous else "", "shaped like" if contiguous else "laid out like", d))


@custom_op("nvsr::decode_rays_backward", mutates_args=("record",), device_types="cuda")
def decode_rays_backward(planes: Sequence[Tensor], consts: Sequence[float], packed: Tensor, packed_bwd: Tensor, rays: Tensor, z: Tensor,
                         g_raw: Tensor, gates: Tensor, record: Optional[Tensor], need: Sequence[bool], arithmetic: int) -> List[Tensor]:
    """gate-driven backward of decode_rays: g_raw [N,S,4] -> gradient planes (channel-last, zeros where need[d] is False -> empty tensor);
    with `record` (the forward's) the pre-activation gradients are added to it for decoder_weight_grad.  `arithmetic` must be the
    forward's."""
    grads = [torch.zeros_like(p) if need[d] else _f(0, like=rays) for d, p in enumerate(planes)]
    _decode_rays_backward_launch(planes, consts, packed, packed_bwd, rays, z, g_raw, gates, record, need, arithmetic, grads)
    return grads


@decode_rays_backward.register_fake
def _(planes, consts, packed, packed_bwd, rays, z, g_raw, gates, record, need, arithmetic):
    return [torch.empty_like(p) if need[d] else rays.new_empty((0,)) for d, p in enumerate(planes)]


@custom_op("nvsr::decode_rays_backward_", mutates_args=("record", "grads"), device_types="cuda")
def decode_rays_backward_(planes: Sequence[Tensor], consts: Sequence[float], packed: Tensor, packed_bwd: Tensor, rays: Tensor, z: Tensor,
                          g_raw: Tensor, gates: Tensor, record: Optional[Tensor], need: Sequence[bool], arithmetic: int,
                          grads: Sequence[Tensor]) -> None:
    """decode_rays_backward ACCUMULATING into existing gradient planes (`grads`: what the functional form returned for an earlier pass over
    the same planes): the fine pass of a training step scatters into the coarse pass's buffers instead of zero-filling a second set of
    full-size planes and adding the two (the reference's autograd accumulates into one .grad the same way)."""
    _check_grads_layout("decode_rays_backward_", planes, need, grads, contiguous=False)
    _decode_rays_backward_launch(planes, consts, packed, packed_bwd, rays, z, g_raw, gates, record, need, arithmetic, grads)


@decode_rays_backward_.register_fake
def _(planes, consts, packed, packed_bwd, rays, z, g_raw, gates, record, need, arithmetic, grads):
    return None


@custom_op("nvsr::decode_rays_backward_recompute", mutates_args=(), device_types="cuda")
def decode_rays_backward_recompute(planes: Sequence[Tensor], consts: Sequence[float], packed: Tensor, packed_bwd: Tensor, rays: Tensor,
                                   z: Tensor, g_raw: Tensor, need: Sequence[bool], want_decoder_grad: bool, arithmetic: int) -> List[Tensor]:
    """backward of a decode pass that recomputes the forward (exact-f32 kernel), RECORD_RAYS rays at a time: the memory-bounded path for
    decoder gradients of very large batches, and the path for passes that published no gates.
    -> [g_plane0..3 (empty where not needed), g_natural (empty unless want_decoder_grad)]"""
    if capi.deterministic():
        capi.refuse_deterministic("decode_rays_backward_recompute (the backward of a pass that published no gates)")
    rays, z, g_raw = _c(rays), _c(z), _c(g_raw)
    sc = _scene(planes, consts)
    N, S = z.shape
    grads = [torch.zeros_like(p) if need[d] else _f(0, like=rays) for d, p in enumerate(planes)]
    gnat = torch.zeros(capi.DECODER_NATURAL_FLOATS, dtype=torch.float32, device=rays.device) if want_decoder_grad else _f(0, like=rays)
    if N == 0 or (not any(need) and not want_decoder_grad):
        return grads + [gnat]
    gptrs = (C.c_void_p * 4)(*[g.data_ptr() if need[d] else None for d, g in enumerate(grads)]) if any(need) else None
    view_ws = _f(N * S * PC, like=rays) if (gptrs is not None and need[3]) else None
    st = capi.stream()
    if not want_decoder_grad:
        capi.call("nvsr_render_pass_backward_ex", C.byref(sc), capi.ptr(packed), capi.ptr(packed_bwd), N, S, capi.ptr(rays), capi.ptr(z),
                  capi.ptr(g_raw), gptrs, None, capi.ptr(view_ws), st)
        return grads + [gnat]
    step = min(N, RECORD_RAYS)
    record = _f(capi.lib().nvsr_decoder_record_floats(step, S), like=rays)
    for a in range(0, N, step):
        n = min(step, N - a)
        capi.call("nvsr_render_pass_backward_ex", C.byref(sc), capi.ptr(packed), capi.ptr(packed_bwd), n, S, capi.ptr(rays[a:]), capi.ptr(z[a:]),
                  capi.ptr(g_raw[a:]), gptrs, capi.ptr(record), capi.ptr(view_ws), st)
        # the recomputing kernel is the exact-f32 one; its record is contracted in the caller's arithmetic (both are held to 1e-5 of float64)
        capi.call("nvsr_decoder_weight_grad_arith", n, S, capi.ptr(record), capi.ptr(gnat), arithmetic, st)
    return grads + [gnat]


@decode_rays_backward_recompute.register_fake
def _(planes, consts, packed, packed_bwd, rays, z, g_raw, need, want_decoder_grad, arithmetic):
    return [torch.empty_like(p) if need[d] else rays.new_empty((0,)) for d, p in enumerate(planes)] + \
        [rays.new_empty((capi.DECODER_NATURAL_FLOATS if want_decoder_grad else 0,))]


# =====================================================================================================================================
# the deterministic route (capi.deterministic): the same gradients in a fixed order, for the limb arithmetics
# =====================================================================================================================================
def _require_limb_arithmetic(arithmetic, who):
    if capi.resolve_decoder_arithmetic(None if arithmetic == capi.ARITH_INHERIT else arithmetic) == capi.ARITHMETIC["f32"]:
        capi.refuse_deterministic("%s in the 'f32' arithmetic" % who)


def rows_scatter_workspace(M, like):
    """an uninitialised workspace for rows_scatter of M rows"""
    return torch.empty(capi.lib().nvsr_rows_scatter_workspace_bytes(int(M)), dtype=torch.uint8, device=like.device)


@custom_op("nvsr::rows_scatter", mutates_args=("g", "workspace"), device_types="cuda")
def rows_scatter(rows: Tensor, texel: Tensor, weight: Tensor, g: Tensor, workspace: Optional[Tensor]) -> None:
    """ordered scatter (include/nvsr.h, nvsr_rows_scatter): rows [M,48] f32, texel [M,4] int32, weight [M,4] f32 are ADDED into the
    channel-last plane g [H,W,48]: per texel the entries e = 4 m + j that name it are summed in ascending e from +0.0f, the sum is added to
    g once; a texel no entry names keeps its bits.  workspace: uint8, at least nvsr_rows_scatter_workspace_bytes(M), or None (allocated
    here); always passed (torch's bookkeeping of a mutated argument indexes it by position)."""
    M = rows.shape[0]
    capi.require_cuda(rows, texel, weight, g)
    if not (rows.dtype == weight.dtype == g.dtype == torch.float32 and texel.dtype == torch.int32 and rows.is_contiguous() and texel.is_contiguous()
            and weight.is_contiguous() and g.is_contiguous() and rows.shape == (M, PC) and texel.shape == (M, 4) and weight.shape == (M, 4)
            and g.dim() == 3 and g.shape[2] == PC):
        raise ValueError("rows_scatter: rows [M,%d] f32, texel [M,4] int32, weight [M,4] f32, g [H,W,%d] f32, all contiguous" % (PC, PC))
    if M == 0:
        return
    ws = rows_scatter_workspace(M, rows) if workspace is None else workspace
    capi.call("nvsr_rows_scatter", M, capi.ptr(rows), capi.ptr(texel), capi.ptr(weight), g.shape[0], g.shape[1], capi.ptr(g), capi.ptr(ws),
              ws.numel() * ws.element_size(), capi.stream())


@rows_scatter.register_fake
def _(rows, texel, weight, g, workspace):
    return None


def _rows_backward_launch(sc, packed, packed_bwd, rays, z, g_raw, gates, record, want, arithmetic):
    """the ROWS variant of the gate-driven backward: -> (rows[3] of [N*S,48] or None, the view plane's workspace or None) for the planes
    `want` names; with `record` the pre-activation gradients are added to it"""
    N, S = z.shape
    rows = [_f(N * S, PC, like=rays) if want[d] else None for d in range(3)]
    rptrs = (C.c_void_p * 3)(*[None if r is None else r.data_ptr() for r in rows]) if any(want[:3]) else None
    view_ws = _f(capi.lib().nvsr_view_grad_workspace_floats(N, S), like=rays) if want[3] else None
    capi.call("nvsr_render_pass_backward_rows_arith", C.byref(sc), capi.ptr(packed), capi.ptr(packed_bwd), N, S, capi.ptr(rays), capi.ptr(z),
              capi.ptr(g_raw), capi.ptr(gates), rptrs, capi.ptr(view_ws), capi.ptr(record), arithmetic, capi.stream())
    return rows, view_ws


def _rows_scatter_tail(sc, planes, rays, z, rows, view_ws, need, grads, want_view_rows=False):
    """what follows the rows launch on the ordered route, ADDING into `grads`: per wanted position plane taps + ordered scatter, then the view
    plane (reduce-only kernel, taps per ray, ordered scatter with M = N).  -> view_rows [N,48] (None unless the view plane needs its
    gradient or want_view_rows asks for the rows alone)"""
    N, S = z.shape
    M, st = N * S, capi.stream()
    if any(need):
        texel = torch.empty((M, 4), dtype=torch.int32, device=rays.device)
        weight = _f(M, 4, like=rays)
        ws = rows_scatter_workspace(M, rays)
    for d in range(3):
        if need[d]:
            capi.call("nvsr_internal_plane_taps", C.byref(sc), d, N, S, capi.ptr(rays), capi.ptr(z), capi.ptr(texel), capi.ptr(weight), st)
            capi.call("nvsr_rows_scatter", M, capi.ptr(rows[d]), capi.ptr(texel), capi.ptr(weight), planes[d].shape[0], planes[d].shape[1],
                      capi.ptr(grads[d]), capi.ptr(ws), ws.numel(), st)
    view_rows = None
    if need[3] or want_view_rows:
        view_rows = _f(N, PC, like=rays)
        capi.call("nvsr_view_rows_reduce", N, S, capi.ptr(view_ws), capi.ptr(view_rows), st)
    if need[3]:
        capi.call("nvsr_internal_plane_taps", C.byref(sc), 3, N, S, capi.ptr(rays), None, capi.ptr(texel), capi.ptr(weight), st)
        capi.call("nvsr_rows_scatter", N, capi.ptr(view_rows), capi.ptr(texel), capi.ptr(weight), planes[3].shape[0], planes[3].shape[1],
                  capi.ptr(grads[3]), capi.ptr(ws), ws.numel(), st)
    return view_rows


@custom_op("nvsr::decode_rays_backward_det", mutates_args=("record",), device_types="cuda")
def decode_rays_backward_det(planes: Sequence[Tensor], consts: Sequence[float], packed: Tensor, packed_bwd: Tensor, rays: Tensor, z: Tensor,
                             g_raw: Tensor, gates: Tensor, record: Optional[Tensor], need: Sequence[bool], arithmetic: int) -> List[Tensor]:
    """decode_rays_backward without float atomics: the same gradient planes, every texel summed in a fixed order (two calls on the same inputs
    return the same bits).  Limb arithmetics only ('f32' raises)."""
    _require_limb_arithmetic(arithmetic, "decode_rays_backward_det")
    return decode_rays_backward_with_points(planes, consts, packed, packed_bwd, rays, z, g_raw, gates, record, need, arithmetic, points=False)[0]


@decode_rays_backward_det.register_fake
def _(planes, consts, packed, packed_bwd, rays, z, g_raw, gates, record, need, arithmetic):
    return [torch.empty_like(p) if need[d] else rays.new_empty((0,)) for d, p in enumerate(planes)]


@custom_op("nvsr::decode_rays_backward_det_", mutates_args=("record", "grads"), device_types="cuda")
def decode_rays_backward_det_(planes: Sequence[Tensor], consts: Sequence[float], packed: Tensor, packed_bwd: Tensor, rays: Tensor, z: Tensor,
                              g_raw: Tensor, gates: Tensor, record: Optional[Tensor], need: Sequence[bool], arithmetic: int,
                              grads: Sequence[Tensor]) -> None:
    """decode_rays_backward_det ACCUMULATING into existing gradient planes: every texel this pass touches receives g + s, s being the sum
    the functional form would have returned for it -- pass 2 onto pass 1's planes equals the sum of the two functional results bit for bit."""
    _require_limb_arithmetic(arithmetic, "decode_rays_backward_det_")
    _check_grads_layout("decode_rays_backward_det_", planes, need, grads, contiguous=True)
    decode_rays_backward_with_points(planes, consts, packed, packed_bwd, rays, z, g_raw, gates, record, need, arithmetic, grads, points=False)


@decode_rays_backward_det_.register_fake
def _(planes, consts, packed, packed_bwd, rays, z, g_raw, gates, record, need, arithmetic, grads):
    return None


@custom_op("nvsr::decoder_weight_grad_det", mutates_args=("workspace",), device_types="cuda")
def decoder_weight_grad_det(record: Tensor, N: int, S: int, arithmetic: int, workspace: Optional[Tensor]) -> Tensor:
    """decoder_weight_grad without float atomics: every slab of rows writes its partial blob into the workspace (f32, at least
    nvsr_decoder_weight_grad_det_workspace_floats(N, S), or None: allocated here; always passed), a reduce kernel adds the slabs in
    ascending order."""
    _require_limb_arithmetic(arithmetic, "decoder_weight_grad_det")
    gnat = torch.zeros(capi.DECODER_NATURAL_FLOATS, dtype=torch.float32, device=record.device)
    if N:
        need = capi.lib().nvsr_decoder_weight_grad_det_workspace_floats(N, S)
        ws = _f(need, like=record) if workspace is None else workspace
        if ws.dtype != torch.float32 or ws.numel() < need or not ws.is_contiguous():
            raise ValueError("decoder_weight_grad_det: workspace must hold %d contiguous float32" % need)
        capi.call("nvsr_decoder_weight_grad_det_arith", N, S, capi.ptr(record), capi.ptr(gnat), capi.ptr(ws), arithmetic, capi.stream())
    return gnat


@decoder_weight_grad_det.register_fake
def _(record, N, S, arithmetic, workspace):
    return record.new_empty((capi.DECODER_NATURAL_FLOATS,))


# =====================================================================================================================================
# input gradients (csrc/points_grad.hip): the rows of the ordered route, chained to the sample positions and view directions
# =====================================================================================================================================
@custom_op("nvsr::triplane_points_grad", mutates_args=(), device_types="cuda")
def triplane_points_grad(planes: Sequence[Tensor], consts: Sequence[float], rays: Tensor, z: Tensor, rows: Sequence[Tensor],
                         view_rows: Tensor) -> Tuple[Tensor, Tensor]:
    """include/nvsr.h, nvsr_triplane_points_grad: rays [N,11], z [N,S], rows = three tensors [N*S,48] f32 (dL/d feature of position plane d
    per point; an EMPTY tensor: plane d adds nothing), view_rows [N,48] (or empty) -> (d_points [N*S,3], d_viewdir [N,3]).  Fixed
    summation order, no atomics: the same inputs give the same bits."""
    capi.require_cuda(rays, z, view_rows, *rows)
    if not (rays.dtype == z.dtype == torch.float32 and rays.is_contiguous() and z.is_contiguous() and rays.dim() == 2 and rays.shape[1] == 11
            and z.dim() == 2 and z.shape[0] == rays.shape[0] and z.shape[1] >= 1):
        raise ValueError("triplane_points_grad: rays [N,11] f32, z [N,S >= 1] f32, both contiguous")
    N, S = z.shape
    if len(rows) != 3:
        raise ValueError("triplane_points_grad: rows is a list of three tensors ([N*S,%d] f32 or empty)" % PC)
    for name, t, shape in [("rows[%d]" % d, r, (N * S, PC)) for d, r in enumerate(rows)] + [("view_rows", view_rows, (N, PC))]:
        if t.numel() == 0:
            continue
        if t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != shape:
            raise ValueError("triplane_points_grad: %s must be a contiguous float32 tensor %s, or an empty one" % (name, list(shape)))
    sc = _scene(planes, consts)
    d_points, d_viewdir = _f(N * S, 3, like=rays), _f(N, 3, like=rays)
    if N:
        rptrs = (C.c_void_p * 3)(*[r.data_ptr() if r.numel() else None for r in rows])
        capi.call("nvsr_triplane_points_grad", C.byref(sc), N, S, capi.ptr(rays), capi.ptr(z), rptrs, capi.ptr(_none_if_empty(view_rows)),
                  capi.ptr(d_points), capi.ptr(d_viewdir), capi.stream())
    return d_points, d_viewdir


@triplane_points_grad.register_fake
def _(planes, consts, rays, z, rows, view_rows):
    N, S = z.shape
    return rays.new_empty((N * S, 3)), rays.new_empty((N, 3))


def decode_rays_backward_rows(planes, consts, packed, packed_bwd, rays, z, g_raw, gates, arithmetic):
    """the ROWS backward alone, for the three position planes (no view workspace, no record): -> rows, three [N*S,48] tensors.  Limb
    arithmetics only; N >= 1."""
    _require_limb_arithmetic(arithmetic, "decode_rays_backward_rows")
    rays, z, g_raw = _c(rays), _c(z), _c(g_raw)
    return _rows_backward_launch(_scene(planes, consts), packed, packed_bwd, rays, z, g_raw, gates, None, (True, True, True, False), arithmetic)[0]


def decode_rays_backward_with_points(planes, consts, packed, packed_bwd, rays, z, g_raw, gates, record, need, arithmetic, grads=None, points=True):
    """the launcher of the ordered route, one stream, in this order: ONE rows launch (with `record` the pre-activation gradients are added to
    it), then per position plane `need` names taps + ordered scatter, then the view plane (reduce-only kernel, taps per ray, ordered scatter
    with M = N); points=True: the points need their gradient too -- the rows of all four planes, which also feed triplane_points_grad.
    grads: existing gradient planes to ADD into (a second pass onto the first pass's planes); None: fresh zero-filled ones.
    -> (gradient planes as decode_rays_backward_det returns them, d_points [N*S,3], d_viewdir [N,3]; both None without `points`)"""
    _require_limb_arithmetic(arithmetic, "the input gradient of a model call" if points else "the gate-driven backward")
    rays, z, g_raw = _c(rays), _c(z), _c(g_raw)
    sc = _scene(planes, consts)
    N, S = z.shape
    if grads is None:
        grads = [torch.zeros_like(p) if need[d] else _f(0, like=rays) for d, p in enumerate(planes)]
    if not points and (N == 0 or (not any(need) and record is None)):
        return grads, None, None
    if N == 0:
        return grads, _f(0, 3, like=rays), _f(0, 3, like=rays)
    rows, view_ws = _rows_backward_launch(sc, packed, packed_bwd, rays, z, g_raw, gates, record, (True,) * 4 if points else need, arithmetic)
    view_rows = _rows_scatter_tail(sc, planes, rays, z, rows, view_ws, need, grads, want_view_rows=points)
    if not points:
        return grads, None, None
    d_points, d_viewdir = torch.ops.nvsr.triplane_points_grad(planes, consts, rays, z, rows, view_rows)
    return grads, d_points, d_viewdir


ATOMIC, ORDERED, ORDERED_POINTS = "atomic", "ordered", "ordered with points"


def gate_route(det, points):
    """the route of a gate-driven backward: points (or rays) that need a gradient take the ordered route once, whatever the deterministic mode
    says; otherwise the mode decides between the ordered scatter and the float atomics"""
    return ORDERED_POINTS if points else ORDERED if det else ATOMIC


def gate_backward_(nv, route, planes, consts, packed, packed_bwd, rays, z, g_raw, gates, record, need, arithmetic, grads):
    """the gate-driven backward of one pass on `route` (gate_route), ADDING into the gradient planes `grads` (zero_planes_like: entries of
    planes that need no gradient are ignored) and, with `record`, the gradient half into it; nv: the operator namespace (torch.ops.nvsr, or
    `direct`).  -> (d_points [N*S,3], d_viewdir [N,3]) on ORDERED_POINTS, else None"""
    if route == ORDERED_POINTS:
        return decode_rays_backward_with_points(planes, consts, packed, packed_bwd, rays, z, g_raw, gates, record, need, arithmetic, grads)[1:]
    op = nv.decode_rays_backward_det_ if route == ORDERED else nv.decode_rays_backward_
    op(planes, consts, packed, packed_bwd, rays, z, g_raw, gates, record, need, arithmetic, grads)
    return None


# =====================================================================================================================================
# depth and surface-normal maps of a rendered view (csrc/normals.hip): opt-in, evaluation only
# =====================================================================================================================================
@custom_op("nvsr::render_pass_geometry", mutates_args=(), device_types="cuda")
def render_pass_geometry(planes: Sequence[Tensor], consts: Sequence[float], packed: Tensor, rays: Tensor, z: Tensor, noise: Optional[Tensor],
                         white: bool, arithmetic: int) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """render_pass's call with the compositor's weights AND its expected depth requested:
    rays [N,11], z [N,S] -> rgb [N,3], disp [N], acc [N], weights [N,S], depth [N] (sum_s w_s z_s)"""
    rays, z, noise = _c(rays), _c(z), _c(noise)
    sc = _scene(planes, consts)
    N, S = z.shape
    rgb, disp, acc, w, depth = _f(N, 3, like=rays), _f(N, like=rays), _f(N, like=rays), _f(N, S, like=rays), _f(N, like=rays)
    if N:
        capi.call("nvsr_render_pass_arith", C.byref(sc), capi.ptr(packed), N, S, capi.ptr(rays), capi.ptr(z), capi.ptr(noise), int(white),
                  capi.ptr(rgb), capi.ptr(disp), capi.ptr(acc), capi.ptr(w), capi.ptr(depth), None, arithmetic, capi.stream())
    return rgb, disp, acc, w, depth


@render_pass_geometry.register_fake
def _(planes, consts, packed, rays, z, noise, white, arithmetic):
    N, S = z.shape
    return rays.new_empty((N, 3)), rays.new_empty((N,)), rays.new_empty((N,)), rays.new_empty((N, S)), rays.new_empty((N,))


def _check_live(who, index, rays, z):
    capi.require_cuda(index, rays, z)
    if not (index.dtype == torch.int32 and index.dim() == 1 and index.is_contiguous() and rays.dtype == z.dtype == torch.float32
            and rays.is_contiguous() and z.is_contiguous() and rays.dim() == 2 and rays.shape[1] == 11 and z.dim() == 2
            and z.shape[0] == rays.shape[0] and z.shape[1] >= 1):
        raise ValueError("%s: index [M] int32, rays [N,11] f32, z / weights [N,S >= 1] f32, all contiguous" % who)


@custom_op("nvsr::live_ray_points", mutates_args=(), device_types="cuda")
def live_ray_points(index: Tensor, rays: Tensor, z: Tensor) -> Tensor:
    """include/nvsr.h, nvsr_live_ray_points: index [M] int32 (entries p = ray * S + s of a live list), rays [N,11], z [N,S] -> one-sample rays
    [M,11] = [o + d z[p], 0 x 5, viewdir]; the row of an index outside [0, N * S) stays 0."""
    _check_live("live_ray_points", index, rays, z)
    N, S = z.shape
    M = index.shape[0]
    live = torch.zeros((M, 11), dtype=torch.float32, device=rays.device)
    capi.call("nvsr_live_ray_points", N, S, M, capi.ptr(index), capi.ptr(rays), capi.ptr(z), capi.ptr(live), capi.stream())
    return live


@live_ray_points.register_fake
def _(index, rays, z):
    return rays.new_empty((index.shape[0], 11))


@custom_op("nvsr::normals_composite", mutates_args=("normal",), device_types="cuda")
def normals_composite(planes: Sequence[Tensor], consts: Sequence[float], index: Tensor, live_rays: Tensor, rows: Sequence[Tensor], weights: Tensor,
                      normal: Tensor) -> None:
    """include/nvsr.h, nvsr_normals_composite: index [M] int32 ASCENDING, live_rays [M,11] (live_ray_points of the same entries), rows = three
    tensors [M,48] f32 (the ROWS backward of g_raw = (0, 0, 0, 1) on the one-sample rays), weights [N,S]; normal [N,3] is ADDED INTO, per ray
    in ascending list order: slabs of one list launched in ascending order give the bits of one launch."""
    N, S = weights.shape[0], (weights.shape[1] if weights.dim() == 2 else 0)
    M = index.shape[0] if index.dim() == 1 else -1
    capi.require_cuda(index, live_rays, weights, normal, *rows)
    ok = (index.dtype == torch.int32 and M >= 0 and index.is_contiguous() and weights.dim() == 2 and S >= 1 and len(rows) == 3
          and all(t.dtype == torch.float32 and t.is_contiguous() for t in (live_rays, weights, normal, *rows))
          and tuple(live_rays.shape) == (M, 11) and tuple(normal.shape) == (N, 3) and all(tuple(r.shape) == (M, PC) for r in rows))
    if not ok:
        raise ValueError("normals_composite: index [M] int32, live_rays [M,11], rows three [M,%d], weights [N,S >= 1], normal [N,3]: f32, contiguous" % PC)
    sc = _scene(planes, consts)
    rptrs = (C.c_void_p * 3)(*[r.data_ptr() for r in rows])
    capi.call("nvsr_normals_composite", C.byref(sc), N, S, M, capi.ptr(index), capi.ptr(live_rays), rptrs, capi.ptr(weights), capi.ptr(normal),
              capi.stream())


@normals_composite.register_fake
def _(planes, consts, index, live_rays, rows, weights, normal):
    return None


def normals_of_pass(planes, consts, packed, packed_bwd, rays, z, weights, arith, slab_points=1 << 20, timers=None):
    """normal [N,3] = sum_s w_s n_s of one pass (include/nvsr.h, "surface normals"): the live list of `weights` once, its count read on the
    host once (the only host read), then per slab of slab_points list entries live_ray_points, decode_rays with gates on the one-sample rays,
    the rows backward of g_raw = (0, 0, 0, 1) (three position planes, no view workspace, no record) and normals_composite.  A slab of 2^20
    points holds 604 MB of rows; any slab size gives the same bits.  Limb arithmetics only.
    timers: a dict of lists that receives (start, end) device events per stage ('decode', 'rows', 'composite'; tools/normals_time.py)."""
    if capi.resolve_decoder_arithmetic(None if arith == capi.ARITH_INHERIT else arith) not in (capi.ARITHMETIC["f16x2"], capi.ARITHMETIC["bf16x3"]):
        raise NotImplementedError("normals_of_pass: the limb arithmetics 'f16x2' / 'bf16x3' only")
    rays, z, weights = _c(rays), _c(z), _c(weights)
    N = z.shape[0]
    normal = torch.zeros((N, 3), dtype=torch.float32, device=rays.device)
    if N == 0:
        return normal
    nv = torch.ops.nvsr
    index, count = nv.generic_live_list(weights)
    M = int(count.item())

    def timed(stage, fn):
        if timers is None:
            return fn()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        out = fn()
        ev[1].record()
        timers.setdefault(stage, []).append(ev)
        return out

    for a in range(0, M, int(slab_points)):
        idx = index[a: min(a + int(slab_points), M)]
        m = idx.shape[0]
        live = nv.live_ray_points(idx, rays, z)
        z0 = torch.zeros((m, 1), dtype=torch.float32, device=rays.device)
        gates = timed("decode", lambda: nv.decode_rays(planes, consts, packed, live, z0, True, False, arith)[1])
        g_raw = torch.zeros((m, 1, 4), dtype=torch.float32, device=rays.device)
        g_raw[..., 3] = 1.0
        rows = timed("rows", lambda: decode_rays_backward_rows(planes, consts, packed, packed_bwd, live, z0, g_raw, gates, arith))
        timed("composite", lambda: nv.normals_composite(planes, consts, idx, live, rows, weights, normal))
    return normal


@custom_op("nvsr::decoder_weight_grad", mutates_args=(), device_types="cuda")
def decoder_weight_grad(record: Tensor, N: int, S: int, arithmetic: int) -> Tensor:
    """one contraction over all points of the record -> weight / bias gradients in state-dict order"""
    gnat = torch.zeros(capi.DECODER_NATURAL_FLOATS, dtype=torch.float32, device=record.device)
    if N:
        capi.call("nvsr_decoder_weight_grad_arith", N, S, capi.ptr(record), capi.ptr(gnat), arithmetic, capi.stream())
    return gnat


@decoder_weight_grad.register_fake
def _(record, N, S, arithmetic):
    return record.new_empty((capi.DECODER_NATURAL_FLOATS,))


# =====================================================================================================================================
# the two NeRF baselines below share the layer engine (csrc/nerf_mlp.h): their backward, weight-gradient and autograd glue differ only in
# the C prefix ("mip" / "pe"), the capi sizes and where `natural` sits among the forward op's inputs
# =====================================================================================================================================
def _nerf_backward(prefix, grad_record_floats, natural, record, g_raw, arithmetic):
    natural, record, g_raw = _c(natural), _c(record), _c(g_raw)
    P = record.shape[0]
    assert g_raw.numel() == 4 * P
    grec = _f(P, grad_record_floats, like=record)
    if P:
        capi.call("nvsr_%s_nerf_backward_arith" % prefix, P, capi.ptr(natural), capi.ptr(record), capi.ptr(g_raw), capi.ptr(grec), arithmetic,
                  capi.stream())
    return grec


def _nerf_weight_grad(prefix, natural_floats, record, grad_record):
    record, grad_record = _c(record), _c(grad_record)
    P = record.shape[0]
    g = _f(natural_floats, like=record)
    ws = _f(max(1, int(getattr(capi.lib(), "nvsr_%s_nerf_wgrad_workspace_floats" % prefix)(P))), like=record)
    capi.call("nvsr_%s_nerf_weight_grad" % prefix, P, capi.ptr(record), capi.ptr(grad_record), capi.ptr(ws), capi.ptr(g), capi.stream())
    return g


def _register_nerf_autograd(op, prefix, nat):
    """autograd of nvsr::<prefix>_nerf, whose inputs are (..., natural, want_record, arithmetic) with `natural` at index `nat`"""
    def setup(ctx, inputs, output):
        ctx.save_for_backward(inputs[nat], output[1])
        ctx.want_record, ctx.arithmetic = inputs[nat + 1], inputs[nat + 2]
        ctx.mark_non_differentiable(output[1])

    def backward(ctx, g_raw, g_rec):
        natural, record = ctx.saved_tensors
        if not ctx.want_record:
            raise RuntimeError("nvsr::%s_nerf was called with want_record=False: no record for its backward" % prefix)
        g_nat = None
        if ctx.needs_input_grad[nat] and g_raw is not None:
            grec = getattr(torch.ops.nvsr, prefix + "_nerf_backward")(natural, record, g_raw, ctx.arithmetic)
            g_nat = getattr(torch.ops.nvsr, prefix + "_nerf_weight_grad")(record, grec)
        return (None,) * nat + (g_nat, None, None)

    op.register_autograd(backward, setup_context=setup)


# =====================================================================================================================================
# the Mip-NeRF baseline (mip.py, models.py:14-108; csrc/mip.hip): integrated positional encoding + FlexibleNeRFModel, forward and training
# =====================================================================================================================================
@custom_op("nvsr::mip_encode", mutates_args=(), device_types="cuda")
def mip_encode(rays: Tensor, edges: Tensor, radius: float) -> Tensor:
    """rays [N,11], edges [N,S+1] -> [N*S, 63] = [36 IPE columns | 27 direction columns] (what the fused forward computes on chip)"""
    rays, edges = _c(rays), _c(edges)
    N, S = edges.shape[0], edges.shape[1] - 1
    out = _f(N * S, 63, like=rays)
    if N:
        capi.call("nvsr_mip_encode", N, S, capi.ptr(rays), capi.ptr(edges), float(radius), capi.ptr(out), capi.stream())
    return out


@mip_encode.register_fake
def _(rays, edges, radius):
    return rays.new_empty((edges.shape[0] * (edges.shape[1] - 1), 63))


@custom_op("nvsr::mip_nerf", mutates_args=(), device_types="cuda")
def mip_nerf(rays: Tensor, edges: Tensor, radius: float, natural: Tensor, want_record: bool, arithmetic: int) -> Tuple[Tensor, Tensor]:
    """encoding + FlexibleNeRFModel over the S intervals of every ray -> raw [N,S,4], record [N*S, MIP_NERF_RECORD_FLOATS] (empty unless
    want_record).  Differentiable in `natural` (state-dict order) when want_record."""
    rays, edges, natural = _c(rays), _c(edges), _c(natural)
    assert natural.numel() == capi.MIP_NERF_NATURAL_FLOATS
    N, S = edges.shape[0], edges.shape[1] - 1
    raw = _f(N, S, 4, like=rays)
    rec = _f(N * S, capi.MIP_NERF_RECORD_FLOATS, like=rays) if want_record else _f(0, like=rays)
    if N:
        capi.call("nvsr_mip_nerf_forward_arith", N, S, capi.ptr(rays), capi.ptr(edges), float(radius), capi.ptr(natural), capi.ptr(raw),
                  capi.ptr(rec) if want_record else None, arithmetic, capi.stream())
    return raw, rec


@mip_nerf.register_fake
def _(rays, edges, radius, natural, want_record, arithmetic):
    N, S = edges.shape[0], edges.shape[1] - 1
    return rays.new_empty((N, S, 4)), rays.new_empty((N * S, capi.MIP_NERF_RECORD_FLOATS) if want_record else (0,))


@custom_op("nvsr::mip_nerf_backward", mutates_args=(), device_types="cuda")
def mip_nerf_backward(natural: Tensor, record: Tensor, g_raw: Tensor, arithmetic: int) -> Tensor:
    """g_raw [P,4] (any shape with P * 4 elements) -> the pre-activation gradient of every layer [P, MIP_NERF_GRAD_RECORD_FLOATS]"""
    return _nerf_backward("mip", capi.MIP_NERF_GRAD_RECORD_FLOATS, natural, record, g_raw, arithmetic)


@mip_nerf_backward.register_fake
def _(natural, record, g_raw, arithmetic):
    return record.new_empty((record.shape[0], capi.MIP_NERF_GRAD_RECORD_FLOATS))


@custom_op("nvsr::mip_nerf_weight_grad", mutates_args=(), device_types="cuda")
def mip_nerf_weight_grad(record: Tensor, grad_record: Tensor) -> Tensor:
    """sum over the points of every layer's G^T X and G -> the gradient of the natural blob (fixed summation order: bit-reproducible)"""
    return _nerf_weight_grad("mip", capi.MIP_NERF_NATURAL_FLOATS, record, grad_record)


@mip_nerf_weight_grad.register_fake
def _(record, grad_record):
    return record.new_empty((capi.MIP_NERF_NATURAL_FLOATS,))


_register_nerf_autograd(mip_nerf, "mip", 3)


# =====================================================================================================================================
# the positional-encoding NeRF baseline (train_utils.py:71-182 with mip_nerf=False, nerf_helpers.py:552-575, models.py:14-108;
# csrc/pe.hip): points ro + rd z, positional encoding + FlexibleNeRFModel, forward and training
# =====================================================================================================================================
@custom_op("nvsr::pe_encode", mutates_args=(), device_types="cuda")
def pe_encode(rays: Tensor, z: Tensor) -> Tensor:
    """rays [N,11], z [N,S] -> [N*S, 66] = [39 position columns | 27 direction columns] (what the fused forward computes on chip)"""
    rays, z = _c(rays), _c(z)
    N, S = z.shape
    out = _f(N * S, 66, like=rays)
    if N:
        capi.call("nvsr_pe_encode", N, S, capi.ptr(rays), capi.ptr(z), capi.ptr(out), capi.stream())
    return out


@pe_encode.register_fake
def _(rays, z):
    return rays.new_empty((z.shape[0] * z.shape[1], 66))


@custom_op("nvsr::pe_nerf", mutates_args=(), device_types="cuda")
def pe_nerf(rays: Tensor, z: Tensor, natural: Tensor, want_record: bool, arithmetic: int) -> Tuple[Tensor, Tensor]:
    """encoding + FlexibleNeRFModel at the S depths of every ray -> raw [N,S,4], record [N*S, PE_NERF_RECORD_FLOATS] (empty unless
    want_record).  Differentiable in `natural` (state-dict order) when want_record."""
    rays, z, natural = _c(rays), _c(z), _c(natural)
    assert natural.numel() == capi.PE_NERF_NATURAL_FLOATS
    N, S = z.shape
    raw = _f(N, S, 4, like=rays)
    rec = _f(N * S, capi.PE_NERF_RECORD_FLOATS, like=rays) if want_record else _f(0, like=rays)
    if N:
        capi.call("nvsr_pe_nerf_forward_arith", N, S, capi.ptr(rays), capi.ptr(z), capi.ptr(natural), capi.ptr(raw),
                  capi.ptr(rec) if want_record else None, arithmetic, capi.stream())
    return raw, rec


@pe_nerf.register_fake
def _(rays, z, natural, want_record, arithmetic):
    N, S = z.shape
    return rays.new_empty((N, S, 4)), rays.new_empty((N * S, capi.PE_NERF_RECORD_FLOATS) if want_record else (0,))


@custom_op("nvsr::pe_nerf_backward", mutates_args=(), device_types="cuda")
def pe_nerf_backward(natural: Tensor, record: Tensor, g_raw: Tensor, arithmetic: int) -> Tensor:
    """g_raw [P,4] (any shape with P * 4 elements) -> the pre-activation gradient of every layer [P, PE_NERF_GRAD_RECORD_FLOATS]"""
    return _nerf_backward("pe", capi.PE_NERF_GRAD_RECORD_FLOATS, natural, record, g_raw, arithmetic)


@pe_nerf_backward.register_fake
def _(natural, record, g_raw, arithmetic):
    return record.new_empty((record.shape[0], capi.PE_NERF_GRAD_RECORD_FLOATS))


@custom_op("nvsr::pe_nerf_weight_grad", mutates_args=(), device_types="cuda")
def pe_nerf_weight_grad(record: Tensor, grad_record: Tensor) -> Tensor:
    """sum over the points of every layer's G^T X and G -> the gradient of the natural blob (fixed summation order: bit-reproducible)"""
    return _nerf_weight_grad("pe", capi.PE_NERF_NATURAL_FLOATS, record, grad_record)


@pe_nerf_weight_grad.register_fake
def _(record, grad_record):
    return record.new_empty((capi.PE_NERF_NATURAL_FLOATS,))


_register_nerf_autograd(pe_nerf, "pe", 2)


# =====================================================================================================================================
# compositing (volume_rendering_utils.py:6-51)
# =====================================================================================================================================
@custom_op("nvsr::composite", mutates_args=(), device_types="cuda")
def composite(raw: Tensor, z: Tensor, rd: Tensor, noise: Optional[Tensor], white: bool, mip: bool) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """raw [N,S,4], z [N,S] (mip: the S+1 interval edges), rd [N,3] -> rgb [N,3], disp [N], acc [N], weights [N,S], depth [N]"""
    raw, z, rd, noise = _c(raw), _c(z), _c(rd), _c(noise)
    N = z.shape[0]
    S = z.shape[1] - (1 if mip else 0)
    rgb, disp, acc, depth, w = _f(N, 3, like=raw), _f(N, like=raw), _f(N, like=raw), _f(N, like=raw), _f(N, S, like=raw)
    if N:
        capi.call("nvsr_composite_mip" if mip else "nvsr_composite", N, S, capi.ptr(raw), capi.ptr(z), capi.ptr(rd), capi.ptr(noise), int(white),
                  capi.ptr(rgb), capi.ptr(disp), capi.ptr(acc), capi.ptr(w), capi.ptr(depth), capi.stream())
    return rgb, disp, acc, w, depth


@composite.register_fake
def _(raw, z, rd, noise, white, mip):
    N = z.shape[0]
    S = z.shape[1] - (1 if mip else 0)
    e = raw.new_empty
    return e((N, 3)), e((N,)), e((N,)), e((N, S)), e((N,))


@custom_op("nvsr::composite_rays", mutates_args=(), device_types="cuda")
def composite_rays(raw: Tensor, z: Tensor, rays: Tensor, noise: Optional[Tensor], white: bool, want_weights: bool) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """composite with the ray directions taken from packed rays [N,11] -> rgb, disp, acc, weights (empty unless want_weights)"""
    raw, z, rays, noise = _c(raw), _c(z), _c(rays), _c(noise)
    N, S = z.shape
    rgb, disp, acc = _f(N, 3, like=raw), _f(N, like=raw), _f(N, like=raw)
    w = _f(N, S, like=raw) if want_weights else _f(0, like=raw)
    if N:
        capi.call("nvsr_composite_rays", N, S, capi.ptr(raw), capi.ptr(z), capi.ptr(rays), capi.ptr(noise), int(white), capi.ptr(rgb),
                  capi.ptr(disp), capi.ptr(acc), capi.ptr(w) if want_weights else None, None, capi.stream())
    return rgb, disp, acc, w


@composite_rays.register_fake
def _(raw, z, rays, noise, white, want_weights):
    N, S = z.shape
    e = raw.new_empty
    return e((N, 3)), e((N,)), e((N,)), e((N, S) if want_weights else (0,))


@custom_op("nvsr::composite_backward", mutates_args=(), device_types="cuda")
def composite_backward(raw: Tensor, z: Tensor, rd: Tensor, noise: Optional[Tensor], white: bool, mip: bool, g_rgb: Tensor,
                       g_acc: Optional[Tensor], g_depth: Optional[Tensor] = None) -> Tensor:
    """gradient of rgb_map / acc_map / depth_map with respect to the radiance field: -> g_raw [N,S,4]; S <= 512"""
    raw, z, rd, noise, g_rgb, g_acc, g_depth = _c(raw), _c(z), _c(rd), _c(noise), _c(g_rgb), _c(g_acc), _c(g_depth)
    N = z.shape[0]
    S = z.shape[1] - (1 if mip else 0)
    g_raw = torch.empty_like(raw)          # (the kernel writes all four channels of every sample)
    if N:
        if S > 512:
            raise NotImplementedError("nvsr_composite_backward handles up to 512 samples per ray")
        capi.call("nvsr_composite_backward_depth", N, S, capi.ptr(raw), capi.ptr(z), capi.ptr(rd), capi.ptr(noise), int(white), capi.ptr(g_rgb),
                  capi.ptr(g_acc), capi.ptr(g_depth), int(mip), capi.ptr(g_raw), capi.stream())
    return g_raw


@composite_backward.register_fake
def _(raw, z, rd, noise, white, mip, g_rgb, g_acc, g_depth=None):
    return torch.empty_like(raw)


@custom_op("nvsr::composite_backward_rays", mutates_args=(), device_types="cuda")
def composite_backward_rays(raw: Tensor, z: Tensor, rays: Tensor, noise: Optional[Tensor], white: bool, mip: bool, g_rgb: Tensor,
                            g_acc: Optional[Tensor], g_depth: Optional[Tensor] = None) -> Tensor:
    """composite_backward with the ray directions taken from packed rays [N,11] (the backward of composite_rays; no [N,3] copy)"""
    raw, z, rays, noise, g_rgb, g_acc, g_depth = _c(raw), _c(z), _c(rays), _c(noise), _c(g_rgb), _c(g_acc), _c(g_depth)
    N = z.shape[0]
    S = z.shape[1] - (1 if mip else 0)
    assert rays.shape == (N, 11)
    g_raw = torch.empty_like(raw)
    if N:
        if S > 512:
            raise NotImplementedError("nvsr_composite_backward handles up to 512 samples per ray")
        capi.call("nvsr_composite_backward_rays", N, S, capi.ptr(raw), capi.ptr(z), capi.ptr(rays), capi.ptr(noise), int(white), capi.ptr(g_rgb),
                  capi.ptr(g_acc), capi.ptr(g_depth), int(mip), capi.ptr(g_raw), capi.stream())
    return g_raw


@composite_backward_rays.register_fake
def _(raw, z, rays, noise, white, mip, g_rgb, g_acc, g_depth=None):
    return torch.empty_like(raw)


def fold_disp_grad(g_disp, q, acc, depth, g_acc, g_depth):
    """disp_map = 1 / max(1e-10, q), q = depth_map / acc_map (volume_rendering_utils.py:46): the incoming gradient of disp_map as additions to
    those of depth_map and acc_map (per-ray scalars; torch.max passes the gradient to the larger operand, q = NaN (acc = 0) passes none)
    -> (g_acc, g_depth)"""
    live = q > 1e-10
    dq = torch.where(live, -capi.f32c(g_disp) / (q * q), torch.zeros_like(q))
    gd = torch.where(live, dq / acc, torch.zeros_like(q))
    ga = torch.where(live, -dq * depth / (acc * acc), torch.zeros_like(q))
    return (ga if g_acc is None else g_acc + ga), (gd if g_depth is None else g_depth + gd)


def _composite_setup(ctx, inputs, output):
    raw, z, rd, noise, white, mip = inputs
    ctx.save_for_backward(raw, z, rd, noise, output[2], output[4])      # + acc_map, depth_map: disp_map's chain rule
    ctx.white, ctx.mip = white, mip
    ctx.mark_non_differentiable(output[3])


def _composite_bwd(ctx, g_rgb, g_disp, g_acc, g_w, g_depth):
    # rgb_map, acc_map, depth_map and disp_map = 1 / max(1e-10, depth_map / acc_map) are differentiable like the reference's
    # (volume_rendering_utils.py:38-46); the per-sample weights output is not (nothing downstream of the reference's renderer uses it).
    # disp's gradient is folded into those of depth and acc here -- per-ray scalars, plumbing; the kernel sums over the samples.
    raw, z, rd, noise, acc, depth = ctx.saved_tensors
    g_rgb = torch.zeros((z.shape[0], 3), dtype=torch.float32, device=raw.device) if g_rgb is None else capi.f32c(g_rgb)
    g_acc = None if g_acc is None else capi.f32c(g_acc)
    g_depth = None if g_depth is None else capi.f32c(g_depth)
    if g_disp is not None:
        g_acc, g_depth = fold_disp_grad(g_disp, depth / acc, acc, depth, g_acc, g_depth)
    return torch.ops.nvsr.composite_backward(raw, z, rd, noise, ctx.white, ctx.mip, g_rgb, g_acc, g_depth), None, None, None, None, None


composite.register_autograd(_composite_bwd, setup_context=_composite_setup)


# =====================================================================================================================================
# feature-plane super-resolution (models.py:769-822 EDSR, :884-926 PlanesSR).  geometry = [Cin, Cout, hidden, n_blocks, n_up]
# =====================================================================================================================================
def _edsr_out_size(H, W, nb, n_up):
    h, w = H - 2 - 4 * nb - 2, W - 2 - 4 * nb - 2
    for _ in range(n_up):
        h, w = (h - 2) * 2, (w - 2) * 2
    return h - 2, w - 2


@custom_op("nvsr::pack_edsr", mutates_args=(), device_types="cuda")
def pack_edsr(natural: Tensor, geometry: Sequence[int], dgrad: bool, arithmetic: int = PACK_ALL_ARITHMETICS) -> Tensor:
    """conv weights in state-dict order -> MFMA-fragment blob (dgrad: of the flipped, transposed kernels of the data gradient).
    arithmetic: PACK_ALL_ARITHMETICS = every fragment region; an NVSR_ARITH_* code = only the regions a launch in that arithmetic reads
    (nvsr_pack_edsr_arith: a fifth of the bytes, for weights that change every iteration); the other regions are uninitialised memory, so the
    blob serves launches in THAT arithmetic only (EDSR.packed_weights keys its cache on it)"""
    nat = capi.f32c(natural)
    lib = capi.lib()
    assert nat.numel() == lib.nvsr_edsr_natural_floats(*geometry)
    n = (lib.nvsr_edsr_packed_dgrad_floats if dgrad else lib.nvsr_edsr_packed_floats)(*geometry)
    assert n > 0
    packed = _f(n, like=nat)
    if os.environ.get("NVSR_PACK_POISON") == "1":          # (tests / tools: NaN words wherever the packer does not write)
        packed.fill_(float("nan"))
    capi.call("nvsr_pack_edsr_dgrad_arith" if dgrad else "nvsr_pack_edsr_arith", capi.ptr(nat), *geometry, capi.ptr(packed), int(arithmetic), capi.stream())
    return packed


@pack_edsr.register_fake
def _(natural, geometry, dgrad, arithmetic=PACK_ALL_ARITHMETICS):
    lib = capi.lib()
    return natural.new_empty(((lib.nvsr_edsr_packed_dgrad_floats if dgrad else lib.nvsr_edsr_packed_floats)(*[int(g) for g in geometry]),))


@custom_op("nvsr::edsr", mutates_args=(), device_types="cuda")
def edsr(x: Tensor, packed: Tensor, geometry: Sequence[int], arithmetic: int) -> Tensor:
    """EDSR.forward: x [B,Cin,H,W] -> [B,Cout,Ho,Wo] (un-padded 3x3 convolutions, fused ReLU / residual / PixelShuffle epilogues)"""
    x = _c(x)
    cin, cout, hid, nb, n_up = geometry
    B, Cin, H, W = x.shape
    assert Cin == cin
    Ho, Wo = _edsr_out_size(H, W, nb, n_up)
    if Ho < 1 or Wo < 1:
        raise capi.NvsrError("EDSR: input smaller than the receptive field")
    out = _f(B, cout, Ho, Wo, like=x)
    ws = _f(B * capi.lib().nvsr_edsr_workspace_floats(hid, nb, n_up, H, W), like=x)
    capi.call("nvsr_edsr_forward_batch_arith", capi.ptr(x), B, Cin, H, W, capi.ptr(packed), cout, hid, nb, n_up, capi.ptr(out), capi.ptr(ws),
              arithmetic, capi.stream())
    return out


@edsr.register_fake
def _(x, packed, geometry, arithmetic):
    cin, cout, hid, nb, n_up = geometry
    Ho, Wo = _edsr_out_size(x.shape[2], x.shape[3], nb, n_up)
    return x.new_empty((x.shape[0], cout, Ho, Wo))


@custom_op("nvsr::edsr_train", mutates_args=(), device_types="cuda")
def edsr_train(x: Tensor, natural: Tensor, packed: Tensor, packed_dgrad: Tensor, geometry: Sequence[int], arithmetic: int) -> Tuple[Tensor, Tensor]:
    """EDSR.forward that keeps every layer's input (`acts`) for the backward; differentiable in x and `natural` (the conv weights in
    state-dict order; `packed` / `packed_dgrad` are their fragment blobs).  x [1,Cin,H,W]"""
    x = _c(x)
    cin, cout, hid, nb, n_up = geometry
    assert x.shape[0] == 1 and x.shape[1] == cin, "the training forward runs one plane at a time"
    H, W = x.shape[2:]
    Ho, Wo = _edsr_out_size(H, W, nb, n_up)
    out = _f(1, cout, Ho, Wo, like=x)
    acts = _f(capi.lib().nvsr_edsr_acts_floats(cin, cout, hid, nb, n_up, H, W), like=x)
    capi.call("nvsr_edsr_forward_train_arith", capi.ptr(x), cin, H, W, capi.ptr(packed), cout, hid, nb, n_up, capi.ptr(out), capi.ptr(acts),
              arithmetic, capi.stream())
    return out, acts


@edsr_train.register_fake
def _(x, natural, packed, packed_dgrad, geometry, arithmetic):
    cin, cout, hid, nb, n_up = geometry
    Ho, Wo = _edsr_out_size(x.shape[2], x.shape[3], nb, n_up)
    return x.new_empty((1, cout, Ho, Wo)), x.new_empty((capi.lib().nvsr_edsr_acts_floats(cin, cout, hid, nb, n_up, int(x.shape[2]), int(x.shape[3])),))


@custom_op("nvsr::edsr_backward", mutates_args=(), device_types="cuda")
def edsr_backward(x: Tensor, acts: Tensor, packed_dgrad: Tensor, geometry: Sequence[int], d_out: Tensor, need_dx: bool, arithmetic: int) -> Tuple[Tensor, Tensor]:
    """-> (weight gradients in state-dict order, dx (empty unless need_dx)); deterministic"""
    x, d_out = _c(x), _c(d_out)
    cin, cout, hid, nb, n_up = geometry
    H, W = x.shape[2:]
    lib = capi.lib()
    gnat = torch.zeros(lib.nvsr_edsr_natural_floats(*geometry), dtype=torch.float32, device=x.device)
    dx = torch.empty_like(x) if need_dx else _f(0, like=x)
    ws = _f(lib.nvsr_edsr_backward_workspace_floats(cin, cout, hid, nb, n_up, H, W), like=x)
    capi.call("nvsr_edsr_backward_arith", capi.ptr(x), cin, H, W, capi.ptr(acts), capi.ptr(packed_dgrad), cout, hid, nb, n_up, capi.ptr(d_out),
              capi.ptr(gnat), capi.ptr(dx) if need_dx else None, capi.ptr(ws), arithmetic, capi.stream())
    return gnat, dx


@edsr_backward.register_fake
def _(x, acts, packed_dgrad, geometry, d_out, need_dx, arithmetic):
    cin, cout, hid, nb, n_up = geometry
    n = 9 * (hid * cin + (2 * nb + 1) * hid * hid + n_up * 4 * hid * hid + cout * hid)
    return x.new_empty((n,)), (torch.empty_like(x) if need_dx else x.new_empty((0,)))


def _edsr_train_setup(ctx, inputs, output):
    x, natural, packed, packed_dgrad, geometry, arithmetic = inputs
    ctx.save_for_backward(x, output[1], packed_dgrad)
    ctx.geometry, ctx.arithmetic = list(geometry), arithmetic
    ctx.mark_non_differentiable(output[1])


def _edsr_train_bwd(ctx, d_out, d_acts):
    x, acts, packed_dgrad = ctx.saved_tensors
    gnat, dx = torch.ops.nvsr.edsr_backward(x, acts, packed_dgrad, ctx.geometry, capi.f32c(d_out), ctx.needs_input_grad[0], ctx.arithmetic)
    return (dx if ctx.needs_input_grad[0] else None), (gnat if ctx.needs_input_grad[1] else None), None, None, None, None


edsr_train.register_autograd(_edsr_train_bwd, setup_context=_edsr_train_setup)


def _roi_c(roi):
    return None if roi is None else (C.c_float * 4)(*[float(v) for v in roi])


@custom_op("nvsr::planes_sr", mutates_args=(), device_types="cuda")
def planes_sr(lr: Sequence[Tensor], packed: Tensor, geometry: Sequence[int], pad: int, over: int, roi: Optional[Sequence[float]],
              mean: Optional[Tensor], std: Optional[Tensor], arithmetic: int, align_corners: bool = True, bicubic: bool = False) -> List[Tensor]:
    """PlanesSR.forward for B equally sized LR planes [C,R0,R1] in ONE batched pass: crop + replicate pad -> EDSR -> crop over-padding
    -> + bilinear x sf of the LR plane (F.interpolate's align_corners as given), NaN outside the ROI.  roi: None (full plane) or
    [ymin, xmin, ymax, xmax] in [-1, 1].  -> B tensors [1,C,sf R0,sf R1]"""
    lr = [_c(t) for t in lr]
    cin, cout, hid, nb, n_up = geometry
    B = len(lr)
    Cc, R0, R1 = lr[0].shape[-3:]
    assert Cc == cin == cout and all(tuple(t.shape[-3:]) == (Cc, R0, R1) for t in lr)
    roi_c = _roi_c(roi)
    nws = capi.lib().nvsr_planes_sr_workspace_floats(Cc, R0, R1, hid, nb, n_up, pad, roi_c)
    if nws < 0:
        raise capi.NvsrError("PlanesSR: region of interest too small for the network")
    sf = 1 << n_up
    outs = [_f(1, Cc, R0 * sf, R1 * sf, like=lr[0]) for _ in lr]
    ws = _f(B * nws, like=lr[0])
    # (align_corners / interpolation of the residual are arguments of the call: no process-wide state between this thread and a backward thread)
    lr_ptrs = (C.c_void_p * B)(*[t.data_ptr() for t in lr])
    out_ptrs = (C.c_void_p * B)(*[t.data_ptr() for t in outs])
    capi.call("nvsr_planes_sr_batch_ex", lr_ptrs, B, Cc, R0, R1, capi.ptr(packed), hid, nb, n_up, pad, over, roi_c, capi.ptr(mean),
              capi.ptr(std), out_ptrs, capi.ptr(ws), arithmetic, int(bool(align_corners)), int(bool(bicubic)), capi.stream())
    return outs


@planes_sr.register_fake
def _(lr, packed, geometry, pad, over, roi, mean, std, arithmetic, align_corners=True, bicubic=False):
    sf = 1 << geometry[4]
    Cc, R0, R1 = lr[0].shape[-3:]
    return [t.new_empty((1, Cc, R0 * sf, R1 * sf)) for t in lr]


@custom_op("nvsr::planes_sr_train", mutates_args=(), device_types="cuda")
def planes_sr_train(lr: Tensor, natural: Tensor, packed: Tensor, packed_dgrad: Tensor, geometry: Sequence[int], pad: int, over: int,
                    roi: Optional[Sequence[float]], mean: Optional[Tensor], std: Optional[Tensor], arithmetic: int,
                    align_corners: bool = True, bicubic: bool = False) -> Tuple[Tensor, Tensor]:
    """planes_sr of one plane that keeps the prepared input + activation record (`keep`); differentiable in `lr` and `natural`"""
    lr = _c(lr)
    cin, cout, hid, nb, n_up = geometry
    Cc, R0, R1 = lr.shape[-3:]
    roi_c = _roi_c(roi)
    lib = capi.lib()
    nws = lib.nvsr_planes_sr_workspace_floats(Cc, R0, R1, hid, nb, n_up, pad, roi_c)
    nkeep = lib.nvsr_planes_sr_keep_floats(Cc, R0, R1, hid, nb, n_up, pad, roi_c)
    if nws < 0 or nkeep < 0:
        raise capi.NvsrError("PlanesSR: region of interest too small for the network")
    sf = 1 << n_up
    out, ws, keep = _f(1, Cc, R0 * sf, R1 * sf, like=lr), _f(nws, like=lr), _f(nkeep, like=lr)
    # (the B = 1 case of the batch entry point: same kernels plane by plane, the residual's settings are arguments of the call)
    lr_ptrs, out_ptrs = (C.c_void_p * 1)(lr.data_ptr()), (C.c_void_p * 1)(out.data_ptr())
    capi.call("nvsr_planes_sr_train_batch_arith", lr_ptrs, 1, Cc, R0, R1, capi.ptr(packed), hid, nb, n_up, pad, over, roi_c, capi.ptr(mean),
              capi.ptr(std), out_ptrs, capi.ptr(ws), capi.ptr(keep), arithmetic, int(bool(align_corners)), int(bool(bicubic)), capi.stream())
    return out, keep


@planes_sr_train.register_fake
def _(lr, natural, packed, packed_dgrad, geometry, pad, over, roi, mean, std, arithmetic, align_corners=True, bicubic=False):
    cin, cout, hid, nb, n_up = geometry
    sf = 1 << n_up
    Cc, R0, R1 = lr.shape[-3:]
    nkeep = capi.lib().nvsr_planes_sr_keep_floats(int(Cc), int(R0), int(R1), hid, nb, n_up, pad, _roi_c(roi))
    return lr.new_empty((1, Cc, R0 * sf, R1 * sf)), lr.new_empty((nkeep,))


@custom_op("nvsr::planes_sr_backward", mutates_args=(), device_types="cuda")
def planes_sr_backward(keep: Tensor, packed_dgrad: Tensor, plane_shape: Sequence[int], geometry: Sequence[int], pad: int, over: int,
                       roi: Optional[Sequence[float]], std: Optional[Tensor], d_out: Tensor, need_lr: bool, arithmetic: int,
                       align_corners: bool = True, bicubic: bool = False) -> Tuple[Tensor, Tensor]:
    """-> (EDSR weight gradients in state-dict order, d_lr [1,C,R0,R1] (empty unless need_lr))"""
    d_out = _c(d_out)
    cin, cout, hid, nb, n_up = geometry
    Cc, R0, R1 = plane_shape
    roi_c = _roi_c(roi)
    lib = capi.lib()
    gnat = torch.zeros(lib.nvsr_edsr_natural_floats(*geometry), dtype=torch.float32, device=keep.device)
    d_lr = torch.zeros((1, Cc, R0, R1), dtype=torch.float32, device=keep.device) if need_lr else _f(0, like=keep)
    ws = _f(lib.nvsr_planes_sr_batch_backward_workspace_floats(1, Cc, R0, R1, hid, nb, n_up, pad, roi_c), like=keep)
    d_out_ptrs = (C.c_void_p * 1)(d_out.data_ptr())
    d_lr_ptrs = (C.c_void_p * 1)(d_lr.data_ptr() if need_lr else None)
    capi.call("nvsr_planes_sr_backward_batch_arith", 1, Cc, R0, R1, capi.ptr(keep), capi.ptr(packed_dgrad), hid, nb, n_up, pad, over, roi_c, capi.ptr(std),
              d_out_ptrs, capi.ptr(gnat), d_lr_ptrs if need_lr else None, capi.ptr(ws), arithmetic, int(bool(align_corners)), int(bool(bicubic)),
              capi.stream())
    return gnat, d_lr


@planes_sr_backward.register_fake
def _(keep, packed_dgrad, plane_shape, geometry, pad, over, roi, std, d_out, need_lr, arithmetic, align_corners=True, bicubic=False):
    cin, cout, hid, nb, n_up = geometry
    n = 9 * (hid * cin + (2 * nb + 1) * hid * hid + n_up * 4 * hid * hid + cout * hid)
    Cc, R0, R1 = plane_shape
    return keep.new_empty((n,)), keep.new_empty((1, Cc, R0, R1) if need_lr else (0,))


def _planes_sr_train_setup(ctx, inputs, output):
    lr, natural, packed, packed_dgrad, geometry, pad, over, roi, mean, std, arithmetic, align_corners, bicubic = inputs
    ctx.save_for_backward(output[1], packed_dgrad, std)
    ctx.mark_non_differentiable(output[1])
    ctx.args = (list(lr.shape[-3:]), list(geometry), pad, over, None if roi is None else list(roi), arithmetic, lr.shape, bool(align_corners), bool(bicubic))


def _planes_sr_train_bwd(ctx, d_out, d_keep):
    keep, packed_dgrad, std = ctx.saved_tensors
    shape, geometry, pad, over, roi, arithmetic, lr_shape, align_corners, bicubic = ctx.args
    gnat, d_lr = torch.ops.nvsr.planes_sr_backward(keep, packed_dgrad, shape, geometry, pad, over, roi, std, capi.f32c(d_out),
                                                   ctx.needs_input_grad[0], arithmetic, align_corners, bicubic)
    return ((d_lr.reshape(lr_shape) if ctx.needs_input_grad[0] else None), (gnat if ctx.needs_input_grad[1] else None)) + (None,) * 11


planes_sr_train.register_autograd(_planes_sr_train_bwd, setup_context=_planes_sr_train_setup)



# ---- the regions of interest of B planes through the SR network at once (training; include/nvsr.h "SR training on the regions of interest of B
# planes at once").  Buffers are allocated at the capacity of FULL planes whatever the regions are: a training iteration's regions change with
# every batch of rays, and exact sizes would hand the caching allocator a new set of multi-GB block sizes per iteration (measured on the refine
# workload: the iteration waited ~40 ms for the allocator); with one size per buffer the blocks of the previous iteration are reused as they are.
def _rois_c(rois, B):
    if rois is None:
        return None
    assert len(rois) == 4 * B
    return (C.c_float * (4 * B))(*[float(v) for v in rois])


@custom_op("nvsr::planes_sr_train_batch", mutates_args=(), device_types="cuda")
def planes_sr_train_batch(lr: Sequence[Tensor], packed: Tensor, geometry: Sequence[int], pad: int, over: int, rois: Optional[Sequence[float]],
                          mean: Optional[Tensor], std: Optional[Tensor], arithmetic: int, align_corners: bool, bicubic: bool) -> List[Tensor]:
    """planes_sr_train of B equally sized planes [C,R0,R1], every one on its own region of interest (rois: 4 floats per plane, or None), one
    launch per layer for all of them.  -> [out_0 .. out_{B-1} ([1,C,sf R0,sf R1] each, NaN outside the region), keep]"""
    lr = [_c(t) for t in lr]
    cin, cout, hid, nb, n_up = geometry
    B = len(lr)
    Cc, R0, R1 = lr[0].shape[-3:]
    assert Cc == cin == cout and all(tuple(t.shape[-3:]) == (Cc, R0, R1) for t in lr)
    lib = capi.lib()
    rois_c = _rois_c(rois, B)
    if lib.nvsr_planes_sr_batch_keep_floats(B, Cc, R0, R1, hid, nb, n_up, pad, rois_c) < 0:
        raise capi.NvsrError("PlanesSR: region of interest too small for the network")
    nkeep = lib.nvsr_planes_sr_batch_keep_floats(B, Cc, R0, R1, hid, nb, n_up, pad, None)
    nws = lib.nvsr_planes_sr_batch_workspace_floats(B, Cc, R0, R1, hid, nb, n_up, pad, None)
    sf = 1 << n_up
    outs = [_f(1, Cc, R0 * sf, R1 * sf, like=lr[0]) for _ in lr]
    ws, keep = _f(nws, like=lr[0]), _f(nkeep, like=lr[0])
    lr_ptrs = (C.c_void_p * B)(*[t.data_ptr() for t in lr])
    out_ptrs = (C.c_void_p * B)(*[t.data_ptr() for t in outs])
    capi.call("nvsr_planes_sr_train_batch_arith", lr_ptrs, B, Cc, R0, R1, capi.ptr(packed), hid, nb, n_up, pad, over, rois_c, capi.ptr(mean), capi.ptr(std),
              out_ptrs, capi.ptr(ws), capi.ptr(keep), arithmetic, int(bool(align_corners)), int(bool(bicubic)), capi.stream())
    return outs + [keep]


@planes_sr_train_batch.register_fake
def _(lr, packed, geometry, pad, over, rois, mean, std, arithmetic, align_corners, bicubic):
    cin, cout, hid, nb, n_up = geometry
    sf = 1 << n_up
    Cc, R0, R1 = lr[0].shape[-3:]
    nkeep = capi.lib().nvsr_planes_sr_batch_keep_floats(len(lr), int(Cc), int(R0), int(R1), hid, nb, n_up, pad, None)
    return [t.new_empty((1, Cc, R0 * sf, R1 * sf)) for t in lr] + [lr[0].new_empty((nkeep,))]


@custom_op("nvsr::planes_sr_backward_batch", mutates_args=(), device_types="cuda")
def planes_sr_backward_batch(keep: Tensor, packed_dgrad: Tensor, plane_shape: Sequence[int], geometry: Sequence[int], pad: int, over: int,
                             rois: Optional[Sequence[float]], std: Optional[Tensor], d_out: Sequence[Tensor], need_lr: Sequence[bool], arithmetic: int,
                             align_corners: bool, bicubic: bool) -> List[Tensor]:
    """-> [EDSR weight gradients in state-dict order (summed over the planes), d_lr_0 .. d_lr_{B-1} ([1,C,R0,R1]; empty where not needed)]"""
    d_out = [_c(t) for t in d_out]
    cin, cout, hid, nb, n_up = geometry
    Cc, R0, R1 = plane_shape
    B = len(d_out)
    lib = capi.lib()
    rois_c = _rois_c(rois, B)
    gnat = torch.zeros(lib.nvsr_edsr_natural_floats(*geometry), dtype=torch.float32, device=keep.device)
    d_lr = [torch.zeros((1, Cc, R0, R1), dtype=torch.float32, device=keep.device) if n else _f(0, like=keep) for n in need_lr]
    ws = _f(lib.nvsr_planes_sr_batch_backward_workspace_floats(B, Cc, R0, R1, hid, nb, n_up, pad, None), like=keep)
    d_out_ptrs = (C.c_void_p * B)(*[t.data_ptr() for t in d_out])
    d_lr_ptrs = (C.c_void_p * B)(*[(t.data_ptr() if n else None) for t, n in zip(d_lr, need_lr)])
    capi.call("nvsr_planes_sr_backward_batch_arith", B, Cc, R0, R1, capi.ptr(keep), capi.ptr(packed_dgrad), hid, nb, n_up, pad, over, rois_c, capi.ptr(std),
              d_out_ptrs, capi.ptr(gnat), d_lr_ptrs if any(need_lr) else None, capi.ptr(ws), arithmetic, int(bool(align_corners)), int(bool(bicubic)),
              capi.stream())
    return [gnat] + d_lr


@planes_sr_backward_batch.register_fake
def _(keep, packed_dgrad, plane_shape, geometry, pad, over, rois, std, d_out, need_lr, arithmetic, align_corners, bicubic):
    cin, cout, hid, nb, n_up = geometry
    n = 9 * (hid * cin + (2 * nb + 1) * hid * hid + n_up * 4 * hid * hid + cout * hid)
    Cc, R0, R1 = plane_shape
    return [keep.new_empty((n,))] + [keep.new_empty((1, Cc, R0, R1) if k else (0,)) for k in need_lr]


def planes_sr_backward_batch_marked(keep, packed_dgrad, plane_shape, geometry, pad, over, rois, std, d_out, need_lr, arithmetic, align_corners, bicubic,
                                    bucket_sync):
    """planes_sr_backward_batch with the weight-gradient blob handed to `bucket_sync` (distributed.OverlappedSRGradSync) bucket by bucket WHILE the
    backward runs: the library records one event per bucket as soon as that part of the blob is final (nvsr_planes_sr_backward_batch_marks; the
    layers finish from the last to the first, the blob is in state-dict order: buckets are suffixes), bucket_sync starts the all-reduce of the
    bucket behind its event on the collective stream, and the iteration's stream waits for the collectives (and scales by 1 / world) before the
    blob goes back to autograd.  Not a registered operator: events and a process group are not tensors; called from PlanesSRBatchFn.backward only."""
    d_out = [_c(t) for t in d_out]
    cin, cout, hid, nb, n_up = geometry
    Cc, R0, R1 = plane_shape
    B = len(d_out)
    lib = capi.lib()
    rois_c = _rois_c(rois, B)
    gnat = torch.zeros(lib.nvsr_edsr_natural_floats(*geometry), dtype=torch.float32, device=keep.device)
    d_lr = [torch.zeros((1, Cc, R0, R1), dtype=torch.float32, device=keep.device) if n else _f(0, like=keep) for n in need_lr]
    ws = _f(lib.nvsr_planes_sr_batch_backward_workspace_floats(B, Cc, R0, R1, hid, nb, n_up, pad, None), like=keep)
    d_out_ptrs = (C.c_void_p * B)(*[t.data_ptr() for t in d_out])
    d_lr_ptrs = (C.c_void_p * B)(*[(t.data_ptr() if n else None) for t, n in zip(d_lr, need_lr)])
    sizes = [9 * hid * cin] + [9 * hid * hid] * (2 * nb + 1) + [9 * 4 * hid * hid] * n_up + [9 * cout * hid]       # floats per layer, state-dict order
    marks = bucket_sync.plan(sizes, gnat)            # [(first layer of the bucket, lo, hi, torch.cuda.Event)], last bucket of the blob first
    layers = (C.c_int32 * len(marks))(*[m[0] for m in marks])
    events = (C.c_void_p * len(marks))(*[m[3].cuda_event for m in marks])
    capi.call("nvsr_planes_sr_backward_batch_marks", B, Cc, R0, R1, capi.ptr(keep), capi.ptr(packed_dgrad), hid, nb, n_up, pad, over, rois_c, capi.ptr(std),
              d_out_ptrs, capi.ptr(gnat), d_lr_ptrs if any(need_lr) else None, capi.ptr(ws), arithmetic, int(bool(align_corners)), int(bool(bicubic)),
              len(marks), layers, events, capi.stream())
    bucket_sync.reduce_marked(gnat, marks)           # collectives behind their events; the current stream then waits for them and scales
    return [gnat] + d_lr


class PlanesSRBatchFn(torch.autograd.Function):
    """PlanesSR on the regions of interest of B planes as ONE autograd node: inputs (cfg, natural weights blob, lr_0 .. lr_{B-1}) -> B
    super-resolved planes; the backward returns ONE weight-gradient blob (torch's cat / reshape backward hands the slices to the
    convolutions' parameters once per iteration instead of once per plane) and the LR planes' gradients.
    cfg["bucket_sync"] (data-parallel training; distributed.OverlappedSRGradSync): the blob comes back ALREADY averaged over the ranks -- its
    buckets were all-reduced while the backward was still computing the layers in front of them."""

    @staticmethod
    def forward(ctx, cfg, natural, *lrs):
        res = direct.planes_sr_train_batch(list(lrs), cfg["packed"], cfg["geometry"], cfg["pad"], cfg["over"], cfg["rois"], cfg["mean"], cfg["std"],
                                           cfg["arithmetic"], cfg["align_corners"], cfg["bicubic"])
        outs, keep = res[:-1], res[-1]
        ctx.cfg = cfg
        ctx.shapes = [t.shape for t in lrs]
        ctx.save_for_backward(keep, cfg["packed_dgrad"])
        return tuple(outs)

    @staticmethod
    def backward(ctx, *d_outs):
        keep, packed_dgrad = ctx.saved_tensors
        cfg = ctx.cfg
        need = ctx.needs_input_grad
        need_lr = [bool(n) for n in need[2:]]
        args = (keep, packed_dgrad, list(ctx.shapes[0][-3:]), cfg["geometry"], cfg["pad"], cfg["over"], cfg["rois"], cfg["std"],
                [capi.f32c(g) for g in d_outs], need_lr, cfg["arithmetic"], cfg["align_corners"], cfg["bicubic"])
        sync = cfg.get("bucket_sync")
        if sync is not None and need[1] and sync.active():
            res = planes_sr_backward_batch_marked(*args, sync)
        else:
            res = direct.planes_sr_backward_batch(*args)
        return (None, res[0] if need[1] else None) + tuple(g.reshape(sh) if n else None for g, sh, n in zip(res[1:], ctx.shapes, need_lr))


# operators whose forward is checked with torch.library.opcheck in the GPU tests
# =====================================================================================================================================
# cumprod_exclusive (nerf_helpers.py:409-430) -- differentiable like the reference's torch helper
# =====================================================================================================================================
@custom_op("nvsr::cumprod_exclusive", mutates_args=(), device_types="cuda")
def cumprod_exclusive(x: Tensor) -> Tensor:
    """out[..., 0] = 1, out[..., i] = x[..., 0] * ... * x[..., i-1]"""
    x = _c(x)
    out = torch.empty_like(x)
    if x.numel():
        capi.call("nvsr_cumprod_exclusive", x.numel() // x.shape[-1], x.shape[-1], capi.ptr(x), capi.ptr(out), capi.stream())
    return out


@cumprod_exclusive.register_fake
def _(x):
    return torch.empty_like(x, memory_format=torch.contiguous_format)


@custom_op("nvsr::cumprod_exclusive_backward", mutates_args=(), device_types="cuda")
def cumprod_exclusive_backward(x: Tensor, out: Tensor, g_out: Tensor) -> Tensor:
    x, out, g_out = _c(x), _c(out), _c(g_out)
    g = torch.empty_like(x)
    if x.numel():
        capi.call("nvsr_cumprod_exclusive_backward", x.numel() // x.shape[-1], x.shape[-1], capi.ptr(x), capi.ptr(out), capi.ptr(g_out), capi.ptr(g),
                  capi.stream())
    return g


@cumprod_exclusive_backward.register_fake
def _(x, out, g_out):
    return torch.empty_like(x, memory_format=torch.contiguous_format)


def _cumprod_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[0], output)


def _cumprod_bwd(ctx, g):
    x, out = ctx.saved_tensors
    return torch.ops.nvsr.cumprod_exclusive_backward(x, out, capi.f32c(g))


cumprod_exclusive.register_autograd(_cumprod_bwd, setup_context=_cumprod_setup)


# =====================================================================================================================================
# low-rank feature planes (models.py:223-230 gen_plane; csrc/lowrank.hip)
# =====================================================================================================================================
def _lowrank_check(factors, ranks):
    """-> [(C, R, r)] of factors [1,C,R,2r] / [C,R,2r]; the kernels' own argument checks (plane count, C, R, r >= 1) stay in the library"""
    assert len(factors) == len(ranks), "one rank per factor tensor"
    dims = []
    for f, r in zip(factors, ranks):
        assert f.dim() in (3, 4) and (f.dim() == 3 or f.shape[0] == 1), "a factor tensor is [1,C,R,2r]"
        Cc, R, W = f.shape[-3:]
        assert W == 2 * int(r), "factor width %d is not 2 x rank %d" % (W, int(r))
        dims.append((int(Cc), int(R), int(r)))
    assert len({d[0] for d in dims}) <= 1, "the planes of one call have the same number of channels"
    return dims


def _lowrank_args(dims, factors, planes, d_factors=None):
    a = capi.LowrankPlanesArgs()
    a.num_planes, a.channels = len(dims), dims[0][0] if dims else 0
    for p, (_, R, r) in enumerate(dims[:capi.MAX_POSITION_PLANES]):      # (a longer list is refused by the library's status)
        a.factors[p], a.planes[p] = factors[p].data_ptr(), planes[p].data_ptr()
        a.d_factors[p] = d_factors[p].data_ptr() if d_factors is not None else None
        a.res[p], a.rank[p] = R, r
    return a


@custom_op("nvsr::lowrank_planes", mutates_args=(), device_types="cuda")
def lowrank_planes(factors: Sequence[Tensor], ranks: Sequence[int]) -> List[Tensor]:
    """factors [1,C,R,2r] (U | V along the last axis) -> planes [1,C,R,R], plane[0,c] = U[0,c] @ V[0,c]^T, in torch.channels_last memory (the
    layout the render kernels sample: models.is_native_layout); all planes in one launch"""
    dims = _lowrank_check(factors, ranks)
    fs = [capi.f32c(f) for f in factors]
    outs = [torch.empty((1, Cc, R, R), dtype=torch.float32, device=f.device, memory_format=torch.channels_last) for f, (Cc, R, _) in zip(fs, dims)]
    capi.call("nvsr_lowrank_planes", _lowrank_args(dims, fs, outs), capi.stream())
    return outs


@lowrank_planes.register_fake
def _(factors, ranks):
    return [torch.empty((1, Cc, R, R), dtype=torch.float32, device=f.device, memory_format=torch.channels_last)
            for f, (Cc, R, _) in zip(factors, _lowrank_check(factors, ranks))]


@custom_op("nvsr::lowrank_planes_backward", mutates_args=(), device_types="cuda")
def lowrank_planes_backward(grads: Sequence[Tensor], factors: Sequence[Tensor], ranks: Sequence[int]) -> List[Tensor]:
    """grads: dL/d plane [1,C,R,R] per plane (channels_last memory is read in place, anything else goes through plane_to_channel_last)
    -> dL/d factors, shaped like the factors; fixed-order sums, no atomics"""
    dims = _lowrank_check(factors, ranks)
    assert len(grads) == len(factors)
    fs = [capi.f32c(f) for f in factors]
    gs = []
    for g, (Cc, R, _) in zip(grads, dims):
        assert tuple(g.shape[-3:]) == (Cc, R, R), "a plane gradient is [1,C,R,R]"
        capi.require_cuda(g)
        g4 = g.reshape(1, Cc, R, R) if g.dim() == 3 else g
        hwc = g4.permute(0, 2, 3, 1)[0]
        gs.append(hwc if (g4.dtype == torch.float32 and hwc.is_contiguous()) else plane_to_channel_last(g4))
    outs = [torch.empty(f.shape, dtype=torch.float32, device=f.device) for f in fs]
    capi.call("nvsr_lowrank_planes_backward", _lowrank_args(dims, fs, gs, outs), capi.stream())
    return outs


@lowrank_planes_backward.register_fake
def _(grads, factors, ranks):
    _lowrank_check(factors, ranks)
    return [f.new_empty(f.shape, dtype=torch.float32) for f in factors]


def _lowrank_setup(ctx, inputs, output):
    ctx.save_for_backward(*inputs[0])
    ctx.ranks = list(inputs[1])
    ctx.shapes = [tuple(o.shape) for o in output]


def _lowrank_bwd(ctx, grads):
    # a plane nobody sampled has no gradient: its factor gets a zero gradient (one launch serves all planes)
    factors = list(ctx.saved_tensors)
    gs = [torch.zeros(s, dtype=torch.float32, device=f.device, memory_format=torch.channels_last) if g is None else g
          for g, s, f in zip(grads, ctx.shapes, factors)]
    return torch.ops.nvsr.lowrank_planes_backward(gs, factors, ctx.ranks), None


lowrank_planes.register_autograd(_lowrank_bwd, setup_context=_lowrank_setup)


# =====================================================================================================================================
# ray and camera-pose gradients of a training render (csrc/ray_grad.hip): the four backward entries, then the differentiable
# forms of the ray generator, the NDC warp and the packer -- today's entries with today's arguments, their backward registered on top
# =====================================================================================================================================
def _check_f32(who, **named):
    """every named (tensor, shape) is a contiguous float32 CUDA tensor of exactly that shape (None passes)"""
    for name, (t, shape) in named.items():
        if t is None:
            continue
        capi.require_cuda(t)
        if t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != tuple(shape):
            raise ValueError("%s: %s must be a contiguous float32 tensor %s" % (who, name, list(shape)))


@custom_op("nvsr::rays_grad", mutates_args=("d_rays",), device_types="cuda")
def rays_grad(rays: Tensor, z: Tensor, d_points: Optional[Tensor], d_viewdir: Optional[Tensor], raw: Tensor, noise: Optional[Tensor],
              g_raw: Tensor, d_rays: Tensor, accumulate: bool) -> None:
    """include/nvsr.h, nvsr_rays_grad: one pass's share of d loss / d rays, WRITTEN into d_rays [N,11] (accumulate: added onto it; columns
    6..7 are +0 either way).  rays [N,11], z [N,S], d_points [N*S,3] or None, d_viewdir [N,3] or None, raw / g_raw [N,S,4], noise [N,S] or
    None.  Fixed summation order, no atomics."""
    if not (z.dim() == 2 and z.shape[1] >= 1):
        raise ValueError("rays_grad: z is [N,S >= 1]")
    N, S = z.shape
    _check_f32("rays_grad", rays=(rays, (N, 11)), z=(z, (N, S)), d_points=(d_points, (N * S, 3)), d_viewdir=(d_viewdir, (N, 3)),
               raw=(raw, (N, S, 4)), noise=(noise, (N, S)), g_raw=(g_raw, (N, S, 4)), d_rays=(d_rays, (N, 11)))
    if N:
        capi.call("nvsr_rays_grad", N, S, capi.ptr(rays), capi.ptr(z), capi.ptr(d_points), capi.ptr(d_viewdir), capi.ptr(raw), capi.ptr(noise),
                  capi.ptr(g_raw), int(bool(accumulate)), capi.ptr(d_rays), capi.stream())


@rays_grad.register_fake
def _(rays, z, d_points, d_viewdir, raw, noise, g_raw, d_rays, accumulate):
    return None


@custom_op("nvsr::pack_rays_backward", mutates_args=(), device_types="cuda")
def pack_rays_backward(d_rays: Tensor, view_src: Tensor, view_is_rd: bool) -> Tuple[Tensor, Tensor, Tensor]:
    """include/nvsr.h, nvsr_pack_rays_backward: d_rays [N,11], the forward's view source [N,3] -> (d_ro, d_rd, d_view_src), each [N,3];
    view_is_rd: the view chain is added to d_rd and d_view_src comes back empty"""
    if d_rays.dim() != 2:
        raise ValueError("pack_rays_backward: d_rays is [N,11]")
    N = d_rays.shape[0]
    _check_f32("pack_rays_backward", d_rays=(d_rays, (N, 11)), view_src=(view_src, (N, 3)))
    d_ro, d_rd = _f(N, 3, like=d_rays), _f(N, 3, like=d_rays)
    d_vs = _f(0, like=d_rays) if view_is_rd else _f(N, 3, like=d_rays)
    if N:
        capi.call("nvsr_pack_rays_backward", N, capi.ptr(d_rays), capi.ptr(view_src), int(bool(view_is_rd)), capi.ptr(d_ro), capi.ptr(d_rd),
                  capi.ptr(_none_if_empty(d_vs)), capi.stream())
    return d_ro, d_rd, d_vs


@pack_rays_backward.register_fake
def _(d_rays, view_src, view_is_rd):
    N = d_rays.shape[0]
    return d_rays.new_empty((N, 3)), d_rays.new_empty((N, 3)), d_rays.new_empty((0,) if view_is_rd else (N, 3))


@custom_op("nvsr::ndc_rays_backward", mutates_args=(), device_types="cuda")
def ndc_rays_backward(H: int, W: int, focal: float, near: float, ro: Tensor, rd: Tensor, d_ro_out: Tensor, d_rd_out: Tensor) -> Tuple[Tensor, Tensor]:
    """include/nvsr.h, nvsr_ndc_rays_backward: the forward's inputs ro, rd [N,3] and the gradients of its outputs -> (d_ro, d_rd)"""
    if ro.dim() != 2:
        raise ValueError("ndc_rays_backward: ro is [N,3]")
    N = ro.shape[0]
    _check_f32("ndc_rays_backward", ro=(ro, (N, 3)), rd=(rd, (N, 3)), d_ro_out=(d_ro_out, (N, 3)), d_rd_out=(d_rd_out, (N, 3)))
    if H < 1 or W < 1:
        raise ValueError("ndc_rays_backward: H, W >= 1")
    d_ro, d_rd = _f(N, 3, like=ro), _f(N, 3, like=ro)
    if N:
        capi.call("nvsr_ndc_rays_backward", H, W, float(focal), float(near), N, capi.ptr(ro), capi.ptr(rd), capi.ptr(d_ro_out), capi.ptr(d_rd_out),
                  capi.ptr(d_ro), capi.ptr(d_rd), capi.stream())
    return d_ro, d_rd


@ndc_rays_backward.register_fake
def _(H, W, focal, near, ro, rd, d_ro_out, d_rd_out):
    return ro.new_empty(ro.shape), ro.new_empty(ro.shape)


@custom_op("nvsr::ray_bundle_backward", mutates_args=(), device_types="cuda")
def ray_bundle_backward(H: int, W: int, focal_x: float, focal_y: float, offset: float, row_col: Optional[Tensor], padding: int, d_ro: Tensor,
                        d_rd: Tensor) -> Tensor:
    """include/nvsr.h, nvsr_ray_bundle_backward: d_ro, d_rd [N,3] of the rays of row_col [N,2] int32 (None: of the whole padded grid,
    N = (H + 2 padding)(W + 2 padding)) -> d_c2w [4,4], row 3 zero.  Two stages in a fixed order over a workspace allocated here."""
    if d_ro.dim() != 2:
        raise ValueError("ray_bundle_backward: d_ro is [N,3]")
    N = d_ro.shape[0]
    _check_f32("ray_bundle_backward", d_ro=(d_ro, (N, 3)), d_rd=(d_rd, (N, 3)))
    if H < 1 or W < 1 or padding < 0:
        raise ValueError("ray_bundle_backward: H, W >= 1, padding >= 0")
    if row_col is None:
        if N != (H + 2 * padding) * (W + 2 * padding):
            raise ValueError("ray_bundle_backward: without row_col the gradients cover the whole padded grid, %d rays" % ((H + 2 * padding) * (W + 2 * padding)))
    else:
        capi.require_cuda(row_col)
        if row_col.dtype != torch.int32 or not row_col.is_contiguous() or tuple(row_col.shape) != (N, 2):
            raise ValueError("ray_bundle_backward: row_col must be a contiguous int32 tensor [N,2]")
    d_c2w = torch.zeros((4, 4), dtype=torch.float32, device=d_ro.device) if N == 0 else _f(4, 4, like=d_ro)
    if N:
        ws = _f(capi.lib().nvsr_ray_bundle_backward_workspace_floats(N), like=d_ro)
        capi.call("nvsr_ray_bundle_backward", H, W, float(focal_x), float(focal_y), float(offset), N, capi.ptr(row_col), padding, capi.ptr(d_ro),
                  capi.ptr(d_rd), capi.ptr(d_c2w), capi.ptr(ws), capi.stream())
    return d_c2w


@ray_bundle_backward.register_fake
def _(H, W, focal_x, focal_y, offset, row_col, padding, d_ro, d_rd):
    return d_ro.new_empty((4, 4))


def _c2w_check(who, c2w):
    capi.require_cuda(c2w)
    if c2w.dtype != torch.float32 or not c2w.is_contiguous() or c2w.dim() != 2 or c2w.shape[1] != 4 or c2w.shape[0] not in (3, 4):
        raise ValueError("%s: c2w must be a contiguous float32 tensor [3,4] or [4,4]" % who)


@custom_op("nvsr::ray_bundle", mutates_args=(), device_types="cuda")
def ray_bundle(H: int, W: int, focal_x: float, focal_y: float, c2w: Tensor, padding: int, offset: float) -> Tuple[Tensor, Tensor]:
    """nvsr_get_ray_bundle as nerf_helpers.get_ray_bundle calls it, differentiable in c2w -> (ro, rd), each [H+2p, W+2p, 3]"""
    _c2w_check("ray_bundle", c2w)
    ro = _f(H + 2 * padding, W + 2 * padding, 3, like=c2w)
    rd = torch.empty_like(ro)
    capi.call("nvsr_get_ray_bundle", H, W, float(focal_x), float(focal_y), capi.ptr(c2w), padding, float(offset), capi.ptr(ro), capi.ptr(rd),
              capi.stream())
    return ro, rd


@ray_bundle.register_fake
def _(H, W, focal_x, focal_y, c2w, padding, offset):
    return c2w.new_empty((H + 2 * padding, W + 2 * padding, 3)), c2w.new_empty((H + 2 * padding, W + 2 * padding, 3))


@custom_op("nvsr::ray_bundle_at", mutates_args=(), device_types="cuda")
def ray_bundle_at(H: int, W: int, focal_x: float, focal_y: float, c2w: Tensor, offset: float, row_col: Tensor) -> Tuple[Tensor, Tensor]:
    """nvsr_get_ray_bundle_at as training.get_ray_bundle_at calls it, differentiable in c2w -> (ro, rd), each [N,3]"""
    _c2w_check("ray_bundle_at", c2w)
    capi.require_cuda(row_col)
    if row_col.dtype != torch.int32 or not row_col.is_contiguous() or row_col.dim() != 2 or row_col.shape[1] != 2:
        raise ValueError("ray_bundle_at: row_col must be a contiguous int32 tensor [N,2]")
    N = row_col.shape[0]
    ro = _f(N, 3, like=c2w)
    rd = torch.empty_like(ro)
    if N:
        capi.call("nvsr_get_ray_bundle_at", H, W, float(focal_x), float(focal_y), capi.ptr(c2w), float(offset), N, capi.ptr(row_col), capi.ptr(ro),
                  capi.ptr(rd), capi.stream())
    return ro, rd


@ray_bundle_at.register_fake
def _(H, W, focal_x, focal_y, c2w, offset, row_col):
    return c2w.new_empty((row_col.shape[0], 3)), c2w.new_empty((row_col.shape[0], 3))


def _zeros_if_none(g, like):
    return torch.zeros_like(like) if g is None else _c(g)


def _ray_bundle_setup(ctx, inputs, output):
    H, W, fx, fy, c2w, padding, offset = inputs
    ctx.args, ctx.rows, ctx.row_col_saved = (H, W, fx, fy, offset, padding), c2w.shape[0], False


def _ray_bundle_at_setup(ctx, inputs, output):
    H, W, fx, fy, c2w, offset, row_col = inputs
    ctx.args, ctx.rows, ctx.row_col_saved = (H, W, fx, fy, offset, 0), c2w.shape[0], True
    ctx.save_for_backward(row_col)                   # (under autograd's version check: an in-place change before backward raises)


def _ray_bundle_bwd(ctx, g_ro, g_rd):
    H, W, fx, fy, offset, padding = ctx.args
    row_col = ctx.saved_tensors[0] if ctx.row_col_saved else None
    present = g_ro if g_ro is not None else g_rd      # (one of the two is: autograd does not call a backward without a gradient)
    g = torch.ops.nvsr.ray_bundle_backward(H, W, fx, fy, offset, row_col, padding, _zeros_if_none(g_ro, present).reshape(-1, 3),
                                           _zeros_if_none(g_rd, present).reshape(-1, 3))[:ctx.rows]
    return (None, None, None, None, g, None, None)


ray_bundle.register_autograd(_ray_bundle_bwd, setup_context=_ray_bundle_setup)
ray_bundle_at.register_autograd(_ray_bundle_bwd, setup_context=_ray_bundle_at_setup)


@custom_op("nvsr::ndc_rays", mutates_args=(), device_types="cuda")
def ndc_rays(H: int, W: int, focal: float, near: float, ro: Tensor, rd: Tensor) -> Tuple[Tensor, Tensor]:
    """nvsr_ndc_rays as nerf_helpers.ndc_rays calls it, differentiable in ro and rd (any leading shape, last axis 3)"""
    _check_f32("ndc_rays", ro=(ro, ro.shape), rd=(rd, ro.shape))
    o, d = torch.empty_like(ro), torch.empty_like(rd)
    if ro.numel():
        capi.call("nvsr_ndc_rays", H, W, float(focal), float(near), ro.numel() // 3, capi.ptr(ro), capi.ptr(rd), capi.ptr(o), capi.ptr(d), capi.stream())
    return o, d


@ndc_rays.register_fake
def _(H, W, focal, near, ro, rd):
    return torch.empty_like(ro), torch.empty_like(rd)


def _ndc_setup(ctx, inputs, output):
    ctx.args = inputs[:4]
    ctx.save_for_backward(inputs[4], inputs[5])


def _ndc_bwd(ctx, g_o, g_d):
    ro, rd = ctx.saved_tensors
    d_ro, d_rd = torch.ops.nvsr.ndc_rays_backward(*ctx.args, ro.reshape(-1, 3), rd.reshape(-1, 3), _zeros_if_none(g_o, ro).reshape(-1, 3),
                                                  _zeros_if_none(g_d, rd).reshape(-1, 3))
    return None, None, None, None, d_ro.reshape(ro.shape), d_rd.reshape(rd.shape)


ndc_rays.register_autograd(_ndc_bwd, setup_context=_ndc_setup)


@custom_op("nvsr::pack_rays", mutates_args=(), device_types="cuda")
def pack_rays(ro: Tensor, rd: Tensor, view_src: Optional[Tensor], near: float, far: float) -> Tensor:
    """nvsr_pack_rays as train_utils.pack_rays calls it, differentiable in ro, rd and the view source (None: the directions themselves)
    -> rays [N,11]"""
    N = ro.shape[0]
    _check_f32("pack_rays", ro=(ro, (N, 3)), rd=(rd, (N, 3)), view_src=(view_src, (N, 3)))
    rays = _f(N, 11, like=ro)
    if N:
        capi.call("nvsr_pack_rays", N, capi.ptr(ro), capi.ptr(rd), capi.ptr(rd if view_src is None else view_src), float(near), float(far),
                  capi.ptr(rays), capi.stream())
    return rays


@pack_rays.register_fake
def _(ro, rd, view_src, near, far):
    return ro.new_empty((ro.shape[0], 11))


def _pack_setup(ctx, inputs, output):
    ro, rd, view_src, _, _ = inputs
    ctx.view_is_rd = view_src is None
    ctx.save_for_backward(rd if view_src is None else view_src)


def _pack_bwd(ctx, g):
    d_ro, d_rd, d_vs = torch.ops.nvsr.pack_rays_backward(_c(g), ctx.saved_tensors[0], ctx.view_is_rd)
    return d_ro, d_rd, (None if ctx.view_is_rd else d_vs), None, None


pack_rays.register_autograd(_pack_bwd, setup_context=_pack_setup)


FORWARD_OPS = ["plane_to_channel_last", "plane_from_channel_last", "pack_decoder", "coarse_z", "importance_resample", "triplane_decode",
               "triplane_decode_generic", "triplane_decode_generic_fused", "pack_generic_decoder", "triplane_decode_generic_fused_arith",
               "pack_generic_decoder_bwd", "ray_points", "lowrank_planes", "ray_bundle", "ray_bundle_at", "ndc_rays", "pack_rays",
               "triplane_density_generic_fused_arith", "triplane_colour_generic_fused_arith", "generic_live_list",
               "generic_occupancy_build", "generic_occupancy_keep", "triplane_density_list_generic_fused_arith",
               "render_pass_geometry", "live_ray_points", "render_pass", "render_rays", "decode_rays", "composite", "composite_rays", "edsr", "planes_sr", "cumprod_exclusive"]


class _Direct:
    """The operators' Python bodies without the dispatcher round trip (torch.ops.nvsr.X(...) costs tens of microseconds of host time per call
    in schema matching and boxing; a 1.7 ms training step makes a dozen of them).  For callers that need none of what the dispatcher adds --
    train_utils._RenderRaysFn runs them inside an autograd.Function, where gradient mode is off and the tensors are already CUDA float32 --
    and only there: everything else goes through torch.ops.nvsr (fake implementations, registered autograd, opcheck)."""

    def __getattr__(self, name):
        op = globals()[name]
        fn = getattr(op, "_init_fn", op)          # (CustomOpDef keeps the decorated function; fall back to the operator itself)
        setattr(self, name, fn)
        return fn


direct = _Direct()
