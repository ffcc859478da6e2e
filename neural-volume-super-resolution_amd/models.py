"""Tri-plane decoder model -- mirror of the reference's models.py hot subset (a6; 8b surface).

`TwoDimPlanesModel` keeps the reference's constructor signature, attribute protocol (`planes_`, `box_coords`, `cur_id`, ...)
and state-dict keys, so checkpoints and the `PlanesOptimizer`-style wiring of the reference carry over; `forward` runs the
fused gather + MFMA decoder kernel (csrc/render.hip) on channel-last copies of the planes and a fragment-packed copy of the
weights, both cached and refreshed when the source tensors change."""
import ctypes as C
import os
import weakref
from re import search

import numpy as np
import torch
import torch.nn as nn

from . import capi
from . import ops  # noqa: F401  (registers torch.ops.nvsr.*)


def get_plane_name(scene_id, dimension):
    """models.py:110-113"""
    if scene_id is None:
        return "_D%d" % (dimension)
    return "sc%s_D%d" % (scene_id, dimension)


def plane_name2scene(plane_name):
    """models.py:115-116"""
    return search("(?<=sc).*(?=_D)", plane_name).group(0)


def get_scene_id(basedir, ds_factor, plane_res):
    """models.py:928-929"""
    return "%s_DS%d%s" % (basedir, ds_factor, "" if plane_res[0] is None else "_PlRes%d_%d" % (plane_res))


def create_plane(resolution, num_plane_channels, init_STD, channels_last=False):
    """models.py:436-439 -- planes are [1,C,H,W] tensors at the interface, like the reference.  channels_last=True (extension) gives the
    parameter torch's channels_last memory format: same shape, same indexing, same state-dict entry, but its memory IS the kernels'
    native [H][W][C] layout -- no re-layout kernel per training step and no second copy of the planes (is_native_layout below)."""
    if not isinstance(resolution, list):
        resolution = [resolution, resolution]
    p = init_STD * torch.randn(size=[1, num_plane_channels, resolution[0], resolution[1]])
    return nn.Parameter(p.contiguous(memory_format=torch.channels_last) if channels_last else p)


def is_native_layout(plane):
    """a [1,C,H,W] float32 plane whose memory is already [H][W][C] (torch.channels_last)"""
    return (plane.dim() == 4 and plane.shape[0] == 1 and plane.shape[1] > 1 and plane.dtype == torch.float32
            and not plane.is_contiguous() and plane.is_contiguous(memory_format=torch.channels_last))


class CoordProjector(nn.Module):
    """models.py:471-497: one orthonormal frame per position plane (column 0 = the plane's normal, columns 1:3 = the axes a point is
    projected on).  Up to three planes: the standard basis and two permutations of it.  More: random frames, drawn from NumPy's global
    generator with the reference's calls in the reference's order -- a seeded construction yields the reference's frames bit for bit
    (tests: g22 `planes5.rot*`)."""

    SPREAD_TRIALS = 10000

    def __init__(self, N: int = None, rot_mats=None) -> None:
        super().__init__()
        if rot_mats is not None:
            assert len(rot_mats) == N
            self.rot_mats_NON_LEARNED = rot_mats
            return
        if N <= 3:
            eye = torch.eye(3)
            frames = [eye, eye[:, [1, 0, 2]], eye[:, [2, 0, 1]]][:N]
        else:
            frames = [torch.from_numpy(f) for f in self.spread_frames(N)]
        self.rot_mats_NON_LEARNED = nn.ParameterList([nn.Parameter(f) for f in frames])

    @classmethod
    def spread_frames(cls, N):
        """N plane normals that keep away from each other and from each other's mirror images: of SPREAD_TRIALS random sets of N unit
        vectors, the set whose 2N directions (every normal and its negative) have the largest sum of squared distances to their nearest
        neighbour.  Each normal is then completed to an orthonormal frame by the QR factorisation of [normal | random 3x2]."""
        sets = np.random.uniform(low=-1, high=1, size=[cls.SPREAD_TRIALS, N, 3])
        sets /= np.sqrt(np.sum(sets ** 2, 2, keepdims=True))
        both = np.concatenate((sets, -1 * sets), 1)                                        # [trial, 2N, 3]
        d2 = np.sum((both[..., None, :] - np.expand_dims(both, 1)) ** 2, -1)               # [trial, 2N, 2N] squared distances
        nearest = np.sort(d2, 1)[:, 1, ...]                                                # (row 0 of the sort is the distance to itself)
        normals = both[np.argmax(np.sum(nearest, -1))][:N]
        frames = []
        for nrm in normals:
            while True:
                m = np.concatenate([nrm[:, None], np.random.uniform(size=[3, 2])], 1)
                if np.linalg.matrix_rank(m) == 3:
                    break
            frames.append(np.linalg.qr(m)[0])
        return frames

    def forward(self, points_dim):
        with torch.no_grad():
            return torch.matmul(points_dim[0], self.rot_mats_NON_LEARNED[points_dim[1]][:, 1:].type(points_dim[0].type()))


def to_channel_last(plane_nchw):
    """[1,C,H,W] or [C,H,W] -> [H,W,C] through the re-layout kernel; a channels_last plane is returned as a view of its own memory"""
    if is_native_layout(plane_nchw):
        return plane_nchw.permute(0, 2, 3, 1)[0]
    capi.require_cuda(plane_nchw)
    return torch.ops.nvsr.plane_to_channel_last(plane_nchw)


def from_channel_last(plane_hwc, like=None):
    """[H,W,C] -> [1,C,H,W]; for a channels_last `like` (the plane the gradient belongs to) a view with that memory format, no kernel"""
    if like is not None and is_native_layout(like) and plane_hwc.is_contiguous():
        return plane_hwc.unsqueeze(0).permute(0, 3, 1, 2)
    capi.require_cuda(plane_hwc)
    return torch.ops.nvsr.plane_from_channel_last(plane_hwc)


# plane name -> (weak reference to the source tensor, its version, channel-last copy or view).  Shared by the coarse and the fine model,
# which sample the same planes (the reference assigns one ParameterDict to both, models.py:601,707); an entry is refreshed when the source
# tensor changes and EVICTED when the source tensor dies (weakref callback), when its SR model clears its planes, and when a model moves to
# another scene -- like the reference, only the current scene's planes stay resident (multi-scene runs would otherwise grow by 368 MB
# per 800^2 scene and 5.9 GB per super-resolved scene).
_PLANE_CACHE = {}


# ---- generated (low-rank) planes: models.py:223-230 -----------------------------------------------------------------------------------
# With `plane_rank[name] = r` the parameter planes_[name] is a factor tensor F [1,C,R,2r] and the plane that is sampled is GENERATED from it
# (torch.ops.nvsr.lowrank_planes).  The reference keeps generated planes in the dict `generated_planes`, shared by the coarse and the fine
# model and cleared by PlanesOptimizer.step() / load_scene; here the dict is honoured the same way (an externally assigned attribute; clearing
# it has the reference's effect), and on top of that an entry is only SERVED while it is valid: made from this factor tensor object, at its
# current version, after the last clear_plane_cache().  Models that were given no dict share this one.
#
# All the rules, in one place.  An entry generated_planes[name] is served by gen_plane only if
#   1. it was made from THIS factor tensor object (weak reference) at its CURRENT `_version`, with the current plane_rank[name]: an optimizer step,
#      training.mark_updated, any in-place write and a replaced parameter retire it (_generated_valid);
#   2. it was made after the last clear_plane_cache() (`_generation_epoch`: that call cannot reach dicts the caller assigned to models);
#   3. for a caller that needs gradients: it carries a graph that no backward has walked yet (a hook on the plane sets `consumed`: autograd frees
#      the graph, and a second iteration on the same factor version must generate again instead of failing).
# Entries are REMOVED by generated_planes.clear() (the reference's PlanesOptimizer.step / load_scene), model.invalidate() (`.data` writes bump no
# version), a model's move to another scene (set_cur_scene_id: only the current scene stays resident) and GraphedTrainStep before its capture.
# A detached plane (gen_plane(detach=True), what assign_LR_planes hands to PlanesSR under detach_LR_planes) keeps the record of its source, so
# that whoever holds it can apply rule 1: TwoDimPlanesModel._refresh_LR_planes does, right before every use of PlanesSR's LR planes.
_GENERATED_PLANES = {}
_generation_epoch = 0


class _Generated:
    """what a generated plane was made from (kept on the tensor as `_nvsr_generated`)"""
    __slots__ = ("src", "version", "rank", "epoch", "state")

    def __init__(self, src, rank, state):
        self.src, self.version, self.rank, self.epoch, self.state = weakref.ref(src), src._version, rank, _generation_epoch, state


def _generated_valid(plane, src, rank, need_grad):
    meta = getattr(plane, "_nvsr_generated", None) if plane is not None else None
    if meta is None or meta.src() is not src or meta.version != src._version or meta.rank != rank or meta.epoch != _generation_epoch:
        return False
    # a training step needs a plane that is part of the autograd graph, and one whose graph has not been walked yet (the backward frees it)
    return not need_grad or (plane.requires_grad and not meta.state["consumed"])


def clear_plane_cache(prefix=None, keep_scene=None):
    """drop every cached channel-last plane; with `prefix` only the entries whose name starts with it; with `keep_scene` every entry that
    does not belong to that scene id.  Without arguments every generated (low-rank) plane is dropped as well, whichever dict holds it."""
    if prefix is None and keep_scene is None:
        global _generation_epoch
        _generation_epoch += 1
        _GENERATED_PLANES.clear()
        _PLANE_CACHE.clear()
        return
    for name in list(_PLANE_CACHE):
        if (prefix is not None and name.startswith(prefix)) or (keep_scene is not None and plane_name2scene(name.split("/")[0]) != keep_scene):
            _PLANE_CACHE.pop(name, None)


def _cache_plane(name, src):
    def _evict(ref, name=name):
        hit = _PLANE_CACHE.get(name)
        if hit is not None and hit[0] is ref:
            _PLANE_CACHE.pop(name, None)

    hit = (weakref.ref(src, _evict), src._version, to_channel_last(src.detach()))
    _PLANE_CACHE[name] = hit
    return hit


DECODER_KEYS = (
    [("density_dec.0.%d.weight" % i, "density_dec.0.%d.bias" % i) for i in range(4)]
    + [("fc_alpha.0.weight", "fc_alpha.0.bias")]
    + [("rgb_dec.0.%d.weight" % i, "rgb_dec.0.%d.bias" % i) for i in range(4)]
    + [("fc_rgb.0.weight", "fc_rgb.0.bias")]
)


class TwoDimPlanesModel(nn.Module):
    """models.py:118-434"""

    def __init__(self, use_viewdirs, dec_density_layers=4, dec_rgb_layers=4, dec_channels=128, skip_connect_every=None,
                 num_plane_channels=48, num_viewdir_plane_channels=None, rgb_dec_input="projections", proj_combination="sum",
                 plane_interp="bilinear", align_corners=True, viewdir_proj_combination=None, num_planes_or_rot_mats=3,
                 plane_stats=False, detach_LR_planes=False, scene_coupler=None, point_coords_noise=0, ensemble_size=1):
        self.num_density_planes = num_planes_or_rot_mats if isinstance(num_planes_or_rot_mats, int) else len(num_planes_or_rot_mats)
        super().__init__()
        self.box_coords = None
        self.use_viewdirs = use_viewdirs
        assert use_viewdirs or (viewdir_proj_combination is None and num_viewdir_plane_channels is None)
        # (models.py:291-293: a training-mode forward jitters the normalised sample positions; such a model trains through the generic kernels,
        #  which take the jitter as an input -- jitter_std / _generic_forward)
        self.point_coords_noise = point_coords_noise
        self.num_plane_channels = num_plane_channels
        if num_viewdir_plane_channels is None:
            num_viewdir_plane_channels = num_plane_channels if use_viewdirs else 0
        self.num_viewdir_plane_channels = num_viewdir_plane_channels
        self.plane_stats = plane_stats
        self.detach_LR_planes = detach_LR_planes
        self.align_corners = align_corners
        assert rgb_dec_input in ["projections", "features", "projections_features"]
        self.rgb_dec_input = rgb_dec_input
        assert proj_combination in ["sum", "concat", "avg"]
        if viewdir_proj_combination is None:
            viewdir_proj_combination = proj_combination
        assert viewdir_proj_combination in ["sum", "concat", "avg", "mult", "concat_pos"]
        if num_viewdir_plane_channels != num_plane_channels:
            assert "concat" in viewdir_proj_combination
        self.proj_combination = proj_combination
        self.viewdir_proj_combination = viewdir_proj_combination
        self.plane_interp = plane_interp
        self.skip_connect_every = skip_connect_every
        self.dec_channels = dec_channels
        self.dec_density_layers, self.dec_rgb_layers, self.ensemble_size = dec_density_layers, dec_rgb_layers, ensemble_size
        self.coord_projector = CoordProjector(self.num_density_planes,
                                              rot_mats=None if isinstance(num_planes_or_rot_mats, int) else num_planes_or_rot_mats)
        self.scene_coupler = scene_coupler

        # same module tree / state-dict keys as the reference (models.py:169-195)
        self.density_dec = nn.ModuleDict([(str(i), nn.ModuleList()) for i in range(ensemble_size)])
        in_channels = num_plane_channels * (self.num_density_planes if proj_combination == "concat" else 1)
        for i in range(ensemble_size):
            self.density_dec[str(i)].append(nn.Linear(in_channels, dec_channels))
            for layer_num in range(dec_density_layers - 1):
                if self.is_skip_layer(layer_num=layer_num):
                    self.density_dec[str(i)].append(nn.Linear(in_channels + dec_channels, dec_channels))
                else:
                    self.density_dec[str(i)].append(nn.Linear(dec_channels, dec_channels))
        self.fc_alpha = nn.ModuleDict([(str(i), nn.Linear(dec_channels, 1)) for i in range(ensemble_size)])
        if "features" in self.rgb_dec_input:
            self.fc_feat = nn.ModuleDict([(str(i), nn.Linear(dec_channels, num_plane_channels)) for i in range(ensemble_size)])
        self.rgb_dec = nn.ModuleDict([(str(i), nn.ModuleList()) for i in range(ensemble_size)])
        plane_C_mult = 0
        if proj_combination == "concat" or viewdir_proj_combination == "concat_pos":
            plane_C_mult += self.num_density_planes
        rgb_in = num_viewdir_plane_channels + num_plane_channels * plane_C_mult
        for i in range(ensemble_size):
            self.rgb_dec[str(i)].append(nn.Linear(rgb_in, dec_channels))
            for layer_num in range(dec_rgb_layers - 1):
                if self.is_skip_layer(layer_num=layer_num):
                    self.rgb_dec[str(i)].append(nn.Linear(rgb_in + dec_channels, dec_channels))
                else:
                    self.rgb_dec[str(i)].append(nn.Linear(dec_channels, dec_channels))
        self.fc_rgb = nn.ModuleDict([(str(i), nn.Linear(dec_channels, 3)) for i in range(ensemble_size)])

        self.skip_SR_ = False
        self._packed_cache = None  # (source key, packed blob)
        # arithmetic of the decoder GEMMs for the calls made through this model: 'f32' | 'bf16x3' | 'f16x2' | None = the process default
        # (capi.set_decoder_arithmetic / NVSR_DECODER_ARITHMETIC).  Passed to every kernel launch explicitly; a training forward stores
        # the mode it ran in and its backward uses that one.
        self.arithmetic = None
        # arithmetic of a generic geometry's planes-only TRAINING: 'f16x2' BY NAME (generic_train_arithmetic()); None and anything else: exact f32
        self.train_arithmetic = None

    # ---- reference protocol ------------------------------------------------------------------------------------------
    def is_skip_layer(self, layer_num):
        """models.py:203-207"""
        if self.skip_connect_every is None:
            return False
        return layer_num % self.skip_connect_every == 0 and layer_num > 0

    def rot_mats(self):
        return self.coord_projector.rot_mats_NON_LEARNED

    def rot_mat_backward_support(self, loaded_dict):
        """models.py:246-249"""
        if not any(["rot_mats" in k for k in loaded_dict]):
            loaded_dict.update(dict([(k, v) for k, v in self.state_dict().items() if "rot_mats" in k]))
        return loaded_dict

    def assign_SR_model(self, SR_model, SR_viewdir):
        """models.py:251-256"""
        self.SR_model = SR_model
        self.SR_model.align_corners = self.align_corners
        self.SR_model.SR_viewdir = SR_viewdir
        self.skip_SR_ = False
        assert not SR_viewdir, "Ceased supporting this option"

    def set_cur_scene_id(self, scene_id):
        if getattr(self, "cur_id", None) is not None and scene_id != self.cur_id:
            # only the current scene stays resident in the channel-last cache
            keep = scene_id if self.scene_coupler is None else None
            if keep is not None:
                clear_plane_cache(keep_scene=keep)
                gen = self._generated_dict()
                for name in [n for n in gen if search("(?<=sc).*(?=_D)", n) and plane_name2scene(n) != keep]:
                    gen.pop(name, None)                  # (generated low-rank planes of the scene that was left)
        self.cur_id = scene_id

    def invalidate(self):
        """Forget every derived copy of the parameters (packed decoder blobs, channel-last planes of the current scene, host copies of the box).
        The caches are keyed on (data_ptr, tensor._version); writes through `.data` (`p.data.copy_()`, `p.data = ...`) do NOT bump the
        version, so code that updates parameters that way -- checkpoint loaders, the reference's planes2cpu -- must call this."""
        self._packed_cache = None
        self._packed_bwd_cache = None
        self.__dict__.pop("_scene_consts", None)
        if getattr(self, "planes_", None) is not None:
            for k in self.planes_:
                _PLANE_CACHE.pop(k, None)
                _PLANE_CACHE.pop(k + "/SR", None)
        self._generated_dict().clear()           # (a `.data` write leaves the factor's version where it was)
        self.__dict__.pop("_occupancy", None)    # (occupancy grids are derived from the planes and the decoder)

    # ---- occupancy grid (csrc/occupancy.hip; include/nvsr.h, "Occupancy grid"): opt-in, evaluation only ------------------------------------
    def _occupancy_key(self):
        """(data_ptr, _version) of everything a grid of the current scene was probed from: the planes scene_args() returns now, through their
        sources -- the raw or generated planes; for a super-resolved plane what it is made from, the SR network's parameters and its LR
        planes, not the SR output itself: that tensor is remade (the f16 range re-render in 'bf16x3' drops it) without the scene changing --
        and the decoder"""
        self.scene_args(check_native=False)        # (super-resolves / generates what is missing, so that the sources below are the cached ones)
        srcs = [self._plane_source(d) for d in range(self.num_density_planes + 1)]
        ts = [t for name, t in srcs if not name.endswith("/SR")] + list(self.decoder_parameters())
        if hasattr(self, "SR_model") and not self.skip_SR_:
            ts += list(self.SR_model.inner_model.parameters()) + list(getattr(self.SR_model, "LR_planes", {}).values())
        for name, t in srcs:                                # a generated low-rank plane: also the factor it was made from, at that version
            meta = getattr(t, "_nvsr_generated", None)
            src = meta.src() if meta is not None else None
            if src is not None:
                ts = ts + [src]
        return tuple((t.data_ptr(), t._version) for t in ts)

    def build_occupancy(self, scene_id, resolution=128, probes=2, threshold=0.0, dilate=1):
        """Build and keep the occupancy grid of `scene_id` for THIS model's decoder (the coarse and the fine model each have their own):
        resolution^3 cells over the scene's box, each probed at probes^3 points with the density decoder; a cell is occupied iff a probe
        has sigma_raw > threshold (or NaN), then `dilate` rounds of a 3x3x3 OR.  Evaluation renders of this scene (no noise, native geometry,
        a limb arithmetic) then skip the density decoder in empty cells.  The grid is APPROXIMATE by nature -- no finite set of probes bounds
        an MLP over a cell -- and resolution, probes, threshold and dilate are the caller's knobs.  It is built from what scene_args()
        returns now (super-resolved planes where the model super-resolves, generated planes of low-rank scenes) and is dropped, never
        used, once a plane or a decoder parameter has changed (occupancy()).  -> the grid, int32 [ceil(resolution^3 / 32)]
        A generic geometry (any other decoder the fused generic kernel holds) builds the same grid with its own density phase
        (torch.ops.nvsr.generic_occupancy_build on _generic_eval_args() in generic_arithmetic()); its evaluation frames then run the
        density decoder on the kept samples only (density_field_kept; include/nvsr.h has the contract: samples outside the box are kept).
        NotImplementedError where the fused kernel has no capacity for the geometry.  A frame uses the grid only where generic_route() is
        'fused' when it is rendered: at a width the fused route does not take by default (dec_channels above GENERIC_FUSED_DEFAULT_MAX_HIDDEN
        without NVSR_GENERIC_FUSED=1) the grid is built and kept, and the frames stay grid-less."""
        if not self.is_native_geometry():
            return self._build_generic_occupancy(scene_id, resolution, probes, threshold, dilate)
        self.set_cur_scene_id(scene_id)
        with torch.no_grad():
            planes, consts = self.scene_args()
            grid = torch.ops.nvsr.occupancy_build(planes, consts, self.packed_decoder(), int(resolution), int(probes), float(threshold), int(dilate),
                                                  self.arith())
        self.__dict__.setdefault("_occupancy", {})[scene_id] = (self._occupancy_key(), grid, int(resolution))
        return grid

    def _build_generic_occupancy(self, scene_id, resolution, probes, threshold, dilate):
        """build_occupancy for a generic geometry; the capacity is asked of the host (nvsr_generic_fused_supported_arith) before any GPU work"""
        with torch.no_grad():                      # (the arithmetic of an evaluation: what the frames that use the grid run in)
            limb = self.generic_arithmetic() == "f16x2"
        arith = capi.ARITHMETIC["f16x2" if limb else "f32"]
        if not self._generic_held("f16x2" if limb else "f32"):
            raise NotImplementedError("an occupancy grid of a generic decoder geometry is probed with the fused generic kernel's density phase, which "
                                      "does not hold this geometry (nvsr_generic_fused_supported_arith: hidden <= 256, first-layer inputs <= 512 "
                                      "columns, 32 points' rows in 160 KB of LDS)")
        self.set_cur_scene_id(scene_id)
        with torch.no_grad():
            planes, consts, nat = self._generic_eval_args()
            packed = self.packed_generic_decoder() if limb else nat.new_empty(0)
            grid = torch.ops.nvsr.generic_occupancy_build(planes, consts, nat, packed, self.generic_geometry(), int(resolution), int(probes),
                                                          float(threshold), int(dilate), bool(self.align_corners), self.plane_interp == "bicubic", arith)
        self.__dict__.setdefault("_occupancy", {})[scene_id] = (self._occupancy_key(), grid, int(resolution))
        return grid

    def clear_occupancy(self, scene_id=None):
        """drop the grid of one scene, or of every scene"""
        if scene_id is None:
            self.__dict__.pop("_occupancy", None)
        else:
            self.__dict__.get("_occupancy", {}).pop(scene_id, None)

    def occupancy_entry(self, scene_id):
        """(grid, resolution) of `scene_id`, or None if there is none or it is stale -- a stale grid is dropped, never used.  Makes `scene_id`
        the current scene."""
        hit = self.__dict__.get("_occupancy", {}).get(scene_id)
        if hit is None:
            return None
        self.set_cur_scene_id(scene_id)
        if hit[0] != self._occupancy_key():
            self.clear_occupancy(scene_id)
            return None
        return hit[1], hit[2]

    def occupancy(self, scene_id):
        """the grid of `scene_id` (build_occupancy), or None if there is none or if it is stale"""
        hit = self.occupancy_entry(scene_id)
        return None if hit is None else hit[0]

    def train(self, mode=True):
        """nn.Module.train, and on a CHANGE of mode the derived copies are dropped: a training loop may have updated the parameters through
        something that does not bump version counters (a fused optimizer outside TrainStep); the first forward of the other mode re-derives"""
        if bool(mode) != self.training:
            self.invalidate()
        return super().train(mode)

    def skip_SR(self, skip):
        self.skip_SR_ = skip

    def planes2cpu(self):
        for p in self.planes_.values():
            p.data = p.data.to("cpu")
        self.invalidate()

    # ---- low-rank planes (models.py:223-244) ---------------------------------------------------------------------------------------
    def _generated_dict(self):
        """`generated_planes` when the caller assigned one (load_scene: one dict for all models of a scene), else the module's shared dict"""
        g = self.__dict__.get("generated_planes")
        return _GENERATED_PLANES if g is None else g

    def _rank_of(self, plane_name):
        rank = self.__dict__.get("plane_rank")
        return int(rank[plane_name]) if rank and plane_name in rank else None

    def gen_plane(self, plane_name, detach=False):
        """models.py:223-231: the plane as stored, or -- with plane_rank[plane_name] = r -- the plane generated from its factors
        F [1,C,R,2r], U @ V^T per channel, in channels_last memory (sampled in place).  ALL low-rank planes of the plane's scene that have
        no valid entry are generated by the one operator call, and the entries are shared by every model that shares the dict: the coarse
        and the fine pass of an iteration sample one generated plane, and both gradients reach F through its one autograd node."""
        r = self._rank_of(plane_name)
        if r is None:
            plane = self.planes_[plane_name]
            return plane.detach() if detach else plane
        src = self.planes_[plane_name]
        cache = self._generated_dict()
        need_grad = torch.is_grad_enabled() and src.requires_grad and not detach
        plane = cache.get(plane_name)
        if not _generated_valid(plane, src, r, need_grad):
            scene = search("(?<=sc).*(?=_D)", plane_name)
            names = [plane_name]
            for n in self.plane_rank:
                if n == plane_name or n not in self.planes_ or len(names) == capi.MAX_POSITION_PLANES:
                    continue
                m = search("(?<=sc).*(?=_D)", n)
                f = self.planes_[n]
                if (m and scene and m.group(0) == scene.group(0) and f.shape[1] == src.shape[1] and f.is_cuda
                        and not _generated_valid(cache.get(n), f, int(self.plane_rank[n]), torch.is_grad_enabled() and f.requires_grad)):
                    names.append(n)
            factors = [self.planes_[n] for n in names]
            ranks = [int(self.plane_rank[n]) for n in names]
            for n, f, k in zip(names, factors, ranks):
                if f.dim() != 4 or f.shape[3] != 2 * k or f.shape[2] < 1:
                    raise ValueError("low-rank plane %s: plane_rank %d needs a factor tensor [1,C,R,%d], got %s" % (n, k, 2 * k, list(f.shape)))
            capi.require_cuda(*factors)
            state = {"consumed": False}
            for n, f, k, p in zip(names, factors, ranks, torch.ops.nvsr.lowrank_planes(factors, ranks)):
                p._nvsr_generated = _Generated(f, k, state)
                if p.requires_grad:
                    p.register_hook(lambda g, state=state: state.__setitem__("consumed", True))
                cache[n] = p
            plane = cache[plane_name]
        if detach:
            meta, plane = plane._nvsr_generated, plane.detach()
            plane._nvsr_generated = meta                 # (what holds the detached plane -- PlanesSR.LR_planes -- can tell when it is stale)
        return plane

    def raw_plane(self, plane_name, downsample=False, detach=False):
        """models.py:233-244 (down-sampled planes -- 'HR_planes' -- are refused: _refuse_plane_downsampling)"""
        if downsample:
            raise NotImplementedError("plane down-sampling ('HR_planes' in nerf.train.what: models.py:231-238) is not implemented")
        return self.gen_plane(plane_name, detach=detach)

    def assign_LR_planes(self, scene=None):
        """models.py:426-434 (no plane down-sampling: `should_downsample` is always False in the supported configs).  A low-rank LR plane is
        handed over GENERATED, as part of the graph: refining through it trains the factors (unless detach_LR_planes)."""
        for k in self.planes_:
            if scene is not None and self.scene_coupler is not None and self.scene_coupler.scene2saved[scene] not in k:
                continue
            if self.scene_coupler is not None:
                self._refuse_plane_downsampling(k, for_LR_loading=True)
            if not self.SR_model.SR_viewdir and get_plane_name(None, self.num_density_planes) in k:
                continue
            self.SR_model.set_LR_plane(self.raw_plane(k, detach=self.detach_LR_planes), id=k, save_interpolated=False)

    # ---- native path ---------------------------------------------------------------------------------------------------
    def is_native_geometry(self):
        """the configuration the fused MFMA kernels are compiled for: 3 + 1 planes x 48 channels, 'avg' / 'concat_pos', 4 + 4 layers x 128,
        no skip layer (every shipped YAML).  Any other geometry the reference's layer sizes admit renders through the generic kernels
        and trains through the generic kernels (csrc/generic.hip: plain layer-by-layer kernels, activations through HBM)."""
        return (self.use_viewdirs and self.num_density_planes == 3 and self.num_plane_channels == capi.PLANE_CHANNELS
                and self.num_viewdir_plane_channels == capi.PLANE_CHANNELS and self.dec_channels == capi.DEC_CHANNELS
                and self.dec_density_layers == 4 and self.dec_rgb_layers == 4 and self.ensemble_size == 1
                and self.proj_combination == "avg" and self.viewdir_proj_combination == "concat_pos"
                and self.rgb_dec_input == "projections" and self.plane_interp == "bilinear" and self.align_corners
                and not any(self.is_skip_layer(l) for l in range(3)) and not (self.point_coords_noise and self.training))

    def jitter_std(self):
        """std of the jitter a forward adds to the normalised sample positions right now: point_coords_noise * 2 / (1 + plane resolution) in
        training mode (models.py:291-293; the resolution is read off the scene id like there), 0 otherwise"""
        if not (self.point_coords_noise and self.training):
            return 0.0
        import re
        return float(self.point_coords_noise) * 2 / (1 + int(re.search(r"(?<=PlRes)(\d)+(?=_)", self.cur_id).group(0)))

    def _check_native_geometry(self):
        if not self.is_native_geometry():
            raise NotImplementedError(
                "this entry point (training / fused passes) runs on the kernels compiled for the shipped configuration (3+1 planes x 48 "
                "channels, 'avg' / 'concat_pos', 4+4 layers x 128, no skip layer); other TwoDimPlanesModel geometries go through the "
                "generic kernels (model.forward / run_one_iter_of_nerf pass by pass)")

    def generic_geometry(self):
        """[plane_channels, viewdir_channels, hidden, density_layers, rgb_layers, skip_connect_every, proj, view] for
        torch.ops.nvsr.triplane_decode_generic (struct nvsr_decoder_geometry)"""
        if not (self.use_viewdirs and 1 <= self.num_density_planes <= capi.MAX_POSITION_PLANES and self.ensemble_size == 1
                and self.rgb_dec_input == "projections" and self.plane_interp in ("bilinear", "bicubic")):
            raise NotImplementedError("the generic decoder kernels cover use_viewdirs=True, 1 .. %d position planes, ensemble_size 1, "
                                      "rgb_dec_input='projections' and bilinear / bicubic planes" % capi.MAX_POSITION_PLANES)
        return [self.num_plane_channels, self.num_viewdir_plane_channels, self.dec_channels, self.dec_density_layers, self.dec_rgb_layers,
                int(self.skip_connect_every or 0), {"sum": 0, "avg": 1, "concat": 2}[self.proj_combination],
                {"sum": 0, "avg": 1, "mult": 2, "concat": 3, "concat_pos": 4}[self.viewdir_proj_combination]]

    def decoder_parameters(self):
        """the decoder's weights and biases in state-dict order (planes and the fixed projection matrices excluded)"""
        sd = dict(self.named_parameters())
        keys = [("density_dec.0.%d.weight" % i, "density_dec.0.%d.bias" % i) for i in range(self.dec_density_layers)] + \
               [("fc_alpha.0.weight", "fc_alpha.0.bias")] + \
               [("rgb_dec.0.%d.weight" % i, "rgb_dec.0.%d.bias" % i) for i in range(self.dec_rgb_layers)] + [("fc_rgb.0.weight", "fc_rgb.0.bias")]
        return [sd[k] for pair in keys for k in pair]

    def natural_blob(self, differentiable=False):
        """Decoder parameters flattened in state-dict order (the layout nvsr_pack_decoder consumes).  differentiable=True keeps
        the autograd graph, so a gradient with respect to the blob reaches the individual parameters."""
        ps = self.decoder_parameters()
        return torch.cat([(p if differentiable else p.detach()).reshape(-1).float() for p in ps])

    def packed_decoder(self):
        self._check_native_geometry()
        params = self.decoder_parameters()
        key = tuple((p.data_ptr(), p._version) for p in params)
        if self._packed_cache is None or self._packed_cache[0] != key:
            nat = self.natural_blob()
            capi.require_cuda(nat)
            self._packed_cache = (key, torch.ops.nvsr.pack_decoder(nat))
        return self._packed_cache[1]

    def packed_decoder_bwd(self):
        """transposed layers for the backward kernels (nvsr_pack_decoder_bwd), cached like packed_decoder()"""
        self._check_native_geometry()
        params = self.decoder_parameters()
        key = tuple((p.data_ptr(), p._version) for p in params)
        cache = getattr(self, "_packed_bwd_cache", None)
        if cache is None or cache[0] != key:
            nat = self.natural_blob()
            capi.require_cuda(nat)
            cache = (key, torch.ops.nvsr.pack_decoder_bwd(nat))
            self._packed_bwd_cache = cache
        return cache[1]

    def _should_SR(self, plane_name):
        if not hasattr(self, "SR_model") or self.skip_SR_:
            return False
        if self.scene_coupler is None:
            return True
        return self.scene_coupler.should_SR(plane_name, plane_not_scene=True)

    def _refuse_plane_downsampling(self, plane_name, **kw):
        """models.py:231-238,273: with 'HR_planes' in nerf.train.what (SceneCoupler(planes_res='HR')) an LR scene samples its HR couple's planes
        DOWN-sampled.  Not mirrored (no shipped config trains HR planes): loud instead of sampling the HR plane as it is."""
        sd = getattr(self.scene_coupler, "should_downsample", None)
        if sd is not None and sd(plane_name, **kw):
            raise NotImplementedError("plane down-sampling ('HR_planes' in nerf.train.what: models.py:231-238) is not implemented; "
                                      "the shipped configs store LR planes (what: ['LR_planes', ...])")

    def _plane_source(self, dim_num):
        """models.py:270-284 `planes()`: the NCHW tensor a projection samples from (raw or super-resolved)."""
        plane_name = get_plane_name(self.cur_id, dim_num)
        super_resolve = dim_num < self.num_density_planes and self._should_SR(plane_name)
        self._refuse_plane_downsampling(plane_name)
        if self.scene_coupler is not None:
            plane_name = self.scene_coupler.scene_with_saved_plane(plane_name, plane_not_scene=True)
        if super_resolve:
            self._refresh_LR_planes([plane_name])
            return plane_name + "/SR", self.SR_model(plane_name)
        return plane_name, self.raw_plane(plane_name)

    def channel_last_plane(self, dim_num):
        name, src = self._plane_source(dim_num)
        # keyed on the source tensor OBJECT (weakly) + its version counter: a data pointer is not an identity -- the allocator hands
        # the address of a dropped super-resolved plane to the next one
        hit = _PLANE_CACHE.get(name)
        if hit is None or hit[0]() is not src or hit[1] != src._version:
            hit = _cache_plane(name, src)
        return hit[2]

    def training_rois(self, rays=None, normalized_points=None):
        """The regions of interest of a training batch (models.py:270-284: the ROI of every point chunk; the bounding box of the ray segments
        [near, far] contains all of them, and the super-resolved values do not depend on the ROI): for every position plane that is
        super-resolved in training mode, [[ymin, xmin], [ymax, xmax]] in normalised plane coordinates.  -> (plane indices, device tensor
        [n, 2, 2]) -- the arithmetic stays on the device; the caller decides when the host reads it (one copy for all planes).
        rays: packed [N,11]; or normalized_points [P,3]: the normalised (and jittered) positions of a model call."""
        names = [get_plane_name(self.cur_id, d) for d in range(self.num_density_planes)]
        dims = [d for d, name in enumerate(names) if self._should_SR(name)] if (hasattr(self, "SR_model") and self.SR_model.training) else []
        if not dims:
            return [], None
        n_ends = normalized_points
        if n_ends is None:
            # (the box and the projection matrices on the device, cached per version: a host tensor's .to(device) is a blocking copy per call)
            box_t = self.box_coords[self.cur_id + ""]
            key = (self.cur_id, str(rays.device), box_t.data_ptr(), box_t._version)
            cache = self.__dict__.get("_roi_consts")
            if cache is None or cache[0] != key:
                box = box_t.to(rays.device)
                cache = (key, box[0, :3].float(), (box[1, :3] - box[0, :3]).float())
                self.__dict__["_roi_consts"] = cache
            lo, rng = cache[1], cache[2]
            ends = torch.cat([rays[:, 0:3] + rays[:, 3:6] * rays[:, 6:7], rays[:, 0:3] + rays[:, 3:6] * rays[:, 7:8]], 0)
            n_ends = 2 * (ends - lo) / rng - 1
        rois = []
        for d in dims:
            m = self.coord_projector.rot_mats_NON_LEARNED[d].detach().float().to(n_ends.device)[:, 1:]
            grid = n_ends @ m                                         # [2N, (x, y)]
            gmin, gmax = grid.min(0)[0], grid.max(0)[0]
            rois.append(torch.stack([torch.stack([gmin[1], gmin[0]]), torch.stack([gmax[1], gmax[0]])], 0))   # rows (min, max), cols (y, x)
        return dims, torch.stack(rois, 0)

    def training_planes(self, rays, normalized_points=None):
        """The NCHW tensors a training step samples, as autograd sees them: the raw plane parameters, or -- where a plane is
        super-resolved -- the output of PlanesSR on the region of interest the batch covers (training_rois).  All super-resolved planes of the
        scene go through the SR network together (PlanesSR.forward_many: one launch per layer for all regions of interest).
        A caller that has the regions on the host already (training.TrainStep computes them ahead of the iteration on a side stream, so that
        the host never waits for the queue to drain) leaves them in `self._roi_hint = (number of rays, [[4 floats] per plane])`."""
        names = [get_plane_name(self.cur_id, d) for d in range(self.num_density_planes + 1)]
        saved = [self.scene_coupler.scene_with_saved_plane(n, plane_not_scene=True) if self.scene_coupler is not None else n for n in names]
        # models.py:273: every plane name goes through the coupler -- an HR scene coupled to an LR scene samples the LR scene's saved planes
        out = [None] * len(names)
        sr_dims = []
        for d, name in enumerate(names):
            if not (d < self.num_density_planes and self._should_SR(name)):
                out[d] = self.raw_plane(saved[d])
            elif not self.SR_model.training:
                self._refresh_LR_planes([saved[d]])
                out[d] = self.SR_model(saved[d])                       # full plane, cached (models.py:277: ROI only in training)
            else:
                sr_dims.append(d)
        if sr_dims:
            hint = self.__dict__.pop("_roi_hint", None)
            if hint is not None and normalized_points is None and rays is not None and hint[0] == rays.shape[0] and len(hint[1]) == len(sr_dims):
                rois = hint[1]
            else:
                dims, dev_rois = self.training_rois(rays, normalized_points)
                assert dims == sr_dims
                rois = dev_rois.detach().reshape(len(dims), 4).cpu().tolist()          # ONE host read for all planes
            self._refresh_LR_planes([saved[d] for d in sr_dims])
            for d, plane in zip(sr_dims, self.SR_model.forward_many([(saved[d], rois[k]) for k, d in enumerate(sr_dims)])):
                out[d] = plane
        return out

    def _refresh_LR_planes(self, names):
        """a generated LR plane the SR model holds belongs to ONE version of its factors: before the SR network runs in training, hand it the
        current one (the reference re-assigns after every PlanesOptimizer step through generated_planes.clear() + assign_LR_planes)"""
        for n in names:
            if self._rank_of(n) is None or n not in self.SR_model.LR_planes:
                continue
            held, src = self.SR_model.LR_planes[n], self.planes_[n]
            need = torch.is_grad_enabled() and src.requires_grad and not self.detach_LR_planes
            if not _generated_valid(held, src, self._rank_of(n), need):
                self.SR_model.LR_planes[n] = self.raw_plane(n, detach=self.detach_LR_planes)
                self.SR_model.SR_planes.pop(n, None)            # (super-resolved from the stale plane)
                _PLANE_CACHE.pop(n + "/SR", None)

    def _generic_graph(self):
        """(the decoder's parameters take gradients, super-resolution is on, _generic_forward would record a graph) with gradients enabled"""
        names = [get_plane_name(self.cur_id, d) for d in range(self.num_density_planes + 1)] if getattr(self, "cur_id", None) is not None else []
        dec = any(p.requires_grad for p in self.decoder_parameters())
        sr_on = hasattr(self, "SR_model") and not self.skip_SR_
        sr_grad = sr_on and self.SR_model.training and self.SR_model.inner_model.wants_grad(*self.SR_model.LR_planes.values())
        return dec, sr_on, bool(dec or sr_grad or any(n in self.planes_ and self.planes_[n].requires_grad for n in names))

    @staticmethod
    def _generic_handle(name):
        """an environment handle of the generic routes, read at every call: '0' (never), '1' (wherever the conditions hold), '' (anything else:
        the measured default)"""
        value = os.environ.get(name, "")
        return value if value in ("0", "1") else ""

    def _generic_width_in(self, span):
        """is dec_channels within (lowest, highest)?  None: nowhere"""
        return span is not None and span[0] <= self.dec_channels <= span[1]

    def _generic_held(self, *kinds):
        """do the fused kernels hold this geometry -- 'f32' (nvsr_generic_fused_supported), 'f16x2' (nvsr_generic_fused_supported_arith),
        'backward' (nvsr_generic_backward_fused_supported), 'backward_f16x2' (nvsr_generic_backward_fused_supported_arith), every one of
        `kinds`?  Host code: no GPU is touched."""
        geo, n_pos, lib = C.byref(capi.DecoderGeometry(*[int(v) for v in self.generic_geometry()])), int(self.num_density_planes), capi.lib()
        ask = {"f32": lambda: lib.nvsr_generic_fused_supported(geo, n_pos),
               "f16x2": lambda: lib.nvsr_generic_fused_supported_arith(geo, n_pos, capi.ARITHMETIC["f16x2"]),
               "backward": lambda: lib.nvsr_generic_backward_fused_supported(geo, n_pos),
               "backward_f16x2": lambda: lib.nvsr_generic_backward_fused_supported_arith(geo, n_pos, capi.ARITHMETIC["f16x2"])}
        return all(ask[kind]() == 1 for kind in kinds)

    def generic_route(self):
        """'fused' or 'layered': what a forward through the generic kernels runs if called now.  'fused' = one launch, activations in LDS
        (csrc/generic_fused.hip, torch.ops.nvsr.triplane_decode_generic_fused); it is taken when no graph is being recorded (gradients off, or
        nothing involved requires them), the geometry is within the kernel's capacity (nvsr_generic_fused_supported) and dec_channels is at
        most GENERIC_FUSED_DEFAULT_MAX_HIDDEN: the widths at which it was measured faster (profiles/generic_fused_ab.txt; at 256 it holds one
        wave per workgroup and takes twice the layered route's time).  'layered' = a launch per layer (csrc/generic.hip): training and
        everything else.  NVSR_GENERIC_FUSED (read at every call): 0 forces 'layered', 1 takes 'fused' wherever the capacity allows.
        The two give the same bits.  The decision touches no GPU."""
        handle = self._generic_handle("NVSR_GENERIC_FUSED")
        if handle == "0" or (torch.is_grad_enabled() and self._generic_graph()[2]):
            return "layered"
        if handle != "1" and self.dec_channels > self.GENERIC_FUSED_DEFAULT_MAX_HIDDEN:
            return "layered"
        return "fused" if self._generic_held("f32") else "layered"

    GENERIC_FUSED_DEFAULT_MAX_HIDDEN = 128

    # dec_channels (lowest, highest) at which the fused TRAINING route (generic_train_route) is taken without NVSR_GENERIC_TRAIN_FUSED=1: the
    # widths at which it was measured faster than the layered route -- this tree's and the parent commit's -- by more than the spread of the
    # alternations in both timed shapes (tools/generic_train_time.py -> profiles/generic_train_ab.txt).  None: nowhere, the route is opt-in.
    # Measured: 128 ('sum': 1.09 x on 2^19 points forward + backward, 1.03 x per planes-only iteration of 4 096 rays).  At 64 the iteration
    # ties inside the spread (17.88 against 17.98 ms) although forward + backward wins 1.10 x, at 256 the route loses (0.36 x: one wave per
    # workgroup): both stay opt-in, and so does every width that was not measured.
    GENERIC_TRAIN_FUSED_DEFAULT_HIDDEN = (128, 128)

    def generic_train_route(self):
        """'fused' or 'layered': how a forward through the generic kernels that RECORDS A GRAPH trains if called now.  'fused' = the forward
        in one launch (torch.ops.nvsr.triplane_decode_generic_fused: the layered forward's bits) and the planes' gradients in one launch
        (csrc/generic_fused_bwd.hip, torch.ops.nvsr.triplane_decode_generic_fused_backward), exact f32.  It is taken when a graph is being
        recorded, NO decoder parameter requires a gradient (planes-only iterations, refinement and SR training under a frozen decoder), the
        deterministic mode is off (generic training is refused there, before any launch), both kernels hold the geometry
        (nvsr_generic_fused_supported, nvsr_generic_backward_fused_supported) and NVSR_GENERIC_TRAIN_FUSED (read at every call) allows it: 0
        never, 1 wherever the capacity allows, unset at the widths of GENERIC_TRAIN_FUSED_DEFAULT_HIDDEN.  'layered' = csrc/generic.hip layer by
        layer: decoder-weight gradients and everything else.  The decision touches no GPU; generic_route() is not affected."""
        handle = self._generic_handle("NVSR_GENERIC_TRAIN_FUSED")
        if handle == "0" or not torch.is_grad_enabled() or capi.deterministic():
            return "layered"
        dec, _, graph = self._generic_graph()
        if dec or not graph or (handle != "1" and not self._generic_width_in(self.GENERIC_TRAIN_FUSED_DEFAULT_HIDDEN)):
            return "layered"
        return "fused" if self._generic_held("f32", "backward") else "layered"

    # dec_channels (lowest, highest) at which training WITH decoder gradients takes the fused route (generic_decoder_train_route) without
    # NVSR_GENERIC_TRAIN_DECODER_FUSED=1: the widths at which it beat the parent commit's layered route by more than the larger spread in both
    # timed shapes (tools/generic_train_decoder_time.py -> profiles/generic_train_decoder_ab.txt; DESIGN 3.10 has the table).  None: nowhere, the
    # route is opt-in.  Measured at 64 ('avg' / 'concat_pos'), 128 ('sum') and 256 ('concat' over 4 planes): 0.99 / 1.07 / 0.36 x per forward +
    # backward of 2^19 points, 0.92 / 0.96 / 0.36 x per iteration of 4 096 rays -- no width wins both shapes, so none enters.
    GENERIC_TRAIN_DECODER_FUSED_DEFAULT_HIDDEN = None

    def generic_decoder_train_route(self):
        """'fused' or 'layered': how a forward through the generic kernels that records a graph WITH DECODER GRADIENTS trains if called now.
        'fused' = the forward in one launch (torch.ops.nvsr.triplane_decode_generic_fused: the layered forward's bits) and a backward that records
        the weight-gradient operands from the fused plane-gradient launch and contracts them with the layered route's own launches
        (csrc/generic_fused_bwd.hip, torch.ops.nvsr.triplane_decode_generic_fused_backward_record), exact f32.  It is taken when gradients are
        enabled and a graph is recorded, at least one decoder parameter requires a gradient, the deterministic mode is off, both kernels hold the
        geometry (nvsr_generic_fused_supported, nvsr_generic_backward_fused_supported) and NVSR_GENERIC_TRAIN_DECODER_FUSED (read at every
        call) allows it: 0 never, 1 wherever the capacity allows, unset at the widths of GENERIC_TRAIN_DECODER_FUSED_DEFAULT_HIDDEN.  'layered' =
        csrc/generic.hip layer by layer.  The decision touches no GPU and changes no other predicate."""
        handle = self._generic_handle("NVSR_GENERIC_TRAIN_DECODER_FUSED")
        if handle == "0" or not torch.is_grad_enabled() or capi.deterministic():
            return "layered"
        dec, _, graph = self._generic_graph()
        if not dec or not graph or (handle != "1" and not self._generic_width_in(self.GENERIC_TRAIN_DECODER_FUSED_DEFAULT_HIDDEN)):
            return "layered"
        return "fused" if self._generic_held("f32", "backward") else "layered"

    # dec_channels (lowest, highest) at which planes-only training in 'f16x2' (generic_train_arithmetic) is taken without
    # NVSR_GENERIC_TRAIN_FUSED=1 once train_arithmetic names it: the widths at which it was measured faster than the better f32 route of the
    # parent commit by more than the larger spread, in both timed shapes (tools/generic_train_limb_time.py -> profiles/generic_train_limb_ab.txt;
    # DESIGN 3.10 has the table).  None: nowhere, the route needs the handle.  Measured at 64 ('avg' / 'concat_pos'), 128 ('sum') and 256
    # ('concat' over 4 planes): 1.52 / 1.92 / 1.09 x per forward + backward of 2^19 points, 1.40 / 1.32 / 1.12 x per iteration of 4 096 rays,
    # every difference (3.4 ... 9.1 ms) above the spread (<= 0.19 ms).  Narrower and wider decoders were not measured: there the route needs the handle.
    GENERIC_TRAIN_LIMB_DEFAULT_HIDDEN = (64, 256)

    def generic_train_arithmetic(self):
        """'f16x2' or 'f32': the arithmetic in which a forward through the generic kernels that RECORDS A GRAPH trains if called now.  'f16x2' =
        the forward launch on two f16 limbs (torch.ops.nvsr.triplane_decode_generic_fused_arith) and the planes' gradients in one launch on two
        f16 limbs (csrc/generic_fused_bwd_limb.hip, torch.ops.nvsr.triplane_decode_generic_fused_backward_arith).  It is taken exactly when
        model.train_arithmetic is 'f16x2' BY NAME (model.arithmetic, the process default and NVSR_DECODER_ARITHMETIC never select it), a graph is
        being recorded, NO decoder parameter requires a gradient, the deterministic mode is off, NVSR_GENERIC_TRAIN_FUSED is not 0, both limb
        kernels hold the geometry (nvsr_generic_fused_supported_arith, nvsr_generic_backward_fused_supported_arith) and
        NVSR_GENERIC_TRAIN_FUSED is 1 or dec_channels lies in GENERIC_TRAIN_LIMB_DEFAULT_HIDDEN.  'f32': what generic_train_route() says --
        training with decoder gradients stays exact f32 (generic_decoder_train_route() picks its route).  The decision touches no GPU and changes
        no other predicate."""
        if not (isinstance(self.train_arithmetic, str) and self.train_arithmetic == "f16x2"):
            return "f32"
        handle = self._generic_handle("NVSR_GENERIC_TRAIN_FUSED")
        if handle == "0" or not torch.is_grad_enabled() or capi.deterministic():
            return "f32"
        dec, _, graph = self._generic_graph()
        if dec or not graph or (handle != "1" and not self._generic_width_in(self.GENERIC_TRAIN_LIMB_DEFAULT_HIDDEN)):
            return "f32"
        return "f16x2" if self._generic_held("f16x2", "backward_f16x2") else "f32"

    # dec_channels (lowest, highest) at which the fused route in 'f16x2' was measured faster, by more than the spread of the alternations, than
    # the better of the two f32 routes: 1.28 - 1.54 x on 2^22 points, 1.39 - 1.69 x on a 400 x 400 frame at 64, 128 and 256
    # (profiles/generic_limb_ab.txt).  Narrower decoders were not measured: there the arithmetic needs NVSR_GENERIC_FUSED=1.  None: nowhere.
    GENERIC_LIMB_DEFAULT_HIDDEN = (64, 256)

    def generic_arithmetic(self):
        """'f16x2' or 'f32': the arithmetic of the hidden layers if a forward through the generic kernels were called now.  'f16x2' = the fused
        launch on two f16 limbs (csrc/generic_fused_limb.hip, torch.ops.nvsr.triplane_decode_generic_fused_arith), taken exactly when
        model.arithmetic is 'f16x2' BY NAME (None, the process default and NVSR_DECODER_ARITHMETIC never select it), no graph is being
        recorded (generic_route's rule), NVSR_GENERIC_FUSED is not 0, the geometry is within the limb kernel's capacity
        (nvsr_generic_fused_supported_arith) and dec_channels is a width at which it was measured faster (GENERIC_LIMB_DEFAULT_HIDDEN;
        NVSR_GENERIC_FUSED=1 lifts this last condition).  Any other model.arithmetic is ignored by the generic kernels, as ever: 'f32' means
        what generic_route() says.  An evaluation frame that left the limbs' range is rendered again in 'f32' (train_utils.run_one_iter_of_nerf),
        which holds this answer at 'f32' while it does.  The decision touches no GPU."""
        if not (isinstance(self.arithmetic, str) and self.arithmetic == "f16x2") or self.__dict__.get("_generic_limb_off"):
            return "f32"
        handle = self._generic_handle("NVSR_GENERIC_FUSED")
        if handle == "0" or (torch.is_grad_enabled() and self._generic_graph()[2]):
            return "f32"
        if handle != "1" and not self._generic_width_in(self.GENERIC_LIMB_DEFAULT_HIDDEN):
            return "f32"
        return "f16x2" if self._generic_held("f16x2") else "f32"

    def packed_generic_decoder(self):
        """the hidden layers' f16-limb fragments for generic_arithmetic() == 'f16x2' (nvsr_pack_generic_decoder_ext), cached like packed_decoder()"""
        params = self.decoder_parameters()
        key = tuple((p.data_ptr(), p._version) for p in params)
        cache = self.__dict__.get("_packed_generic_cache")
        if cache is None or cache[0] != key:
            nat = self.natural_blob()
            capi.require_cuda(nat)
            cache = (key, torch.ops.nvsr.pack_generic_decoder(nat, self.generic_geometry(), int(self.num_density_planes)))
            self.__dict__["_packed_generic_cache"] = cache
        return cache[1]

    def packed_generic_decoder_bwd(self):
        """the hidden layers' TRANSPOSED f16-limb fragments for generic_train_arithmetic() == 'f16x2' (nvsr_pack_generic_decoder_bwd_ext), cached
        like packed_generic_decoder()"""
        params = self.decoder_parameters()
        key = tuple((p.data_ptr(), p._version) for p in params)
        cache = self.__dict__.get("_packed_generic_bwd_cache")
        if cache is None or cache[0] != key:
            nat = self.natural_blob()
            capi.require_cuda(nat)
            cache = (key, torch.ops.nvsr.pack_generic_decoder_bwd(nat, self.generic_geometry(), int(self.num_density_planes)))
            self.__dict__["_packed_generic_bwd_cache"] = cache
        return cache[1]

    def _generic_forward(self, x, coord_noise=None):
        """forward through the generic kernels (any geometry); in training mode with gradients for the planes and the decoder.
        coord_noise [P,3]: the jitter of the normalised sample positions (models.py:291-293) when the caller has drawn it (run_one_iter_of_nerf
        draws in the reference's order of chunks and network batches); None = drawn here like the reference's forward does, one
        torch.normal call of the input's size on the CPU generator."""
        std = self.jitter_std()
        if std and coord_noise is None:
            coord_noise = torch.normal(mean=0, std=std, size=[x.shape[0], 3])
        if coord_noise is not None:
            coord_noise = capi.f32c(coord_noise.to(x.device))
        if torch.is_grad_enabled():                                    # (like any torch module: a graph whenever gradients are on)
            names = [get_plane_name(self.cur_id, d) for d in range(self.num_density_planes + 1)]
            dec, sr_on, graph = self._generic_graph()
            if graph:
                if self.training:
                    np.random.randint(self.ensemble_size)             # models.py:393 (see forward())
                if sr_on:
                    # training THROUGH super-resolved planes (models.py:270-284): PlanesSR on the region the call's points cover, as part of the graph
                    box = self.box_coords[self.cur_id + ""].to(x.device)
                    n = 2 * (x[:, :3] - box[0, :3].float()) / (box[1, :3] - box[0, :3]).float() - 1
                    planes = self.training_planes(None, normalized_points=n if coord_noise is None else n + coord_noise)
                else:
                    planes = [self.raw_plane(n) for n in names]
                if self.generic_train_arithmetic() == "f16x2":
                    return _GenericFusedLimbTrainFn.apply(self, x, coord_noise, *planes)
                if self.generic_train_route() == "fused":
                    return _GenericFusedTrainFn.apply(self, x, coord_noise, *planes)
                if dec and self.generic_decoder_train_route() == "fused":
                    return _GenericFusedDecoderTrainFn.apply(self, x, self.natural_blob(differentiable=True), coord_noise, *planes)
                return _GenericDecodeFn.apply(self, x, self.natural_blob(differentiable=True) if dec else None, coord_noise, *planes)
        planes, consts, nat = self._generic_eval_args()
        if self.generic_arithmetic() == "f16x2":
            return torch.ops.nvsr.triplane_decode_generic_fused_arith(planes, consts, nat, self.packed_generic_decoder(), self.generic_geometry(), x,
                                                                      bool(self.align_corners), coord_noise, self.plane_interp == "bicubic",
                                                                      capi.ARITHMETIC["f16x2"])
        op = torch.ops.nvsr.triplane_decode_generic_fused if self.generic_route() == "fused" else torch.ops.nvsr.triplane_decode_generic
        return op(planes, consts, nat, self.generic_geometry(), x, bool(self.align_corners), coord_noise, self.plane_interp == "bicubic")

    def _generic_eval_args(self):
        """(planes, consts, natural blob) of an evaluation through the generic kernels: super-resolved planes where super-resolution is on"""
        if hasattr(self, "SR_model") and not self.skip_SR_:
            names = [get_plane_name(self.cur_id, d) for d in range(self.num_density_planes)]
            names = [n for n in names if self._should_SR(n)]
            if self.scene_coupler is not None:
                names = [self.scene_coupler.scene_with_saved_plane(n, plane_not_scene=True) for n in names]
            self._refresh_LR_planes(names)
            self.SR_model.super_resolve_many(names)
        planes = [self.channel_last_plane(d) for d in range(self.num_density_planes + 1)]
        planes, consts = self.scene_args(planes=planes, check_native=False)
        nat = self.natural_blob()
        capi.require_cuda(nat)
        return planes, consts, nat

    # (hidden-width class, arithmetic) at which a frame in two phases was measured faster than the one-launch frame on the same tree by more
    # than the larger of the two routes' spreads (tools/generic_two_phase_time.py -> profiles/generic_two_phase_ab.txt); DESIGN 3.10 has the
    # table.  Classes: dec_channels (lowest, highest) per arithmetic; None: nowhere -- the route then needs NVSR_GENERIC_TWO_PHASE=1.
    # 'f32': 400 x 400 frames 1.48 x faster at 64 (197.3 -> 133.3 ms) and 1.43 x at 128 with a third of the samples live (340.4 -> 238.1 ms); with
    # EVERY sample live the 128-wide frame is 4.5 % slower (341.5 -> 357.0 ms) -- the break-even live share of a decode is 0.65 at 64 and 0.84
    # at 128, a rendered scene's is about a third.  Narrower decoders were not measured; wider ones are not 'fused' by default.
    # 'f16x2' stays None although two phases measured 1.29 - 2.29 x faster there: tests/test_generic_limb.py counts the one-launch operator's
    # calls in such a frame, and the existing test wins.
    GENERIC_TWO_PHASE_DEFAULT_HIDDEN = {"f32": (64, 128), "f16x2": None}

    def generic_frame_route(self):
        """'two_phase' or 'one_phase': how an evaluation frame (train_utils._render_generic) runs a pass of this model if rendered now.
        'two_phase' = density_field on every sample, the compositing weights, their live list, colour_field_ on the live samples
        (csrc/generic_fused*.hip's phases, csrc/generic_live.hip): the one-launch frame bit for bit, a dead sample's colour logits being +0
        (include/nvsr.h has the contract).  It needs generic_route() == 'fused' (so: no graph being recorded, the capacity) and no jitter of
        the sample positions drawn inside the forward (jitter_std() == 0).  NVSR_GENERIC_TWO_PHASE (read at every call): 0 forces 'one_phase',
        1 takes 'two_phase' wherever those conditions hold; unset: the measured default (GENERIC_TWO_PHASE_DEFAULT_HIDDEN).  The decision
        touches no GPU."""
        if not self.generic_phases_allowed():
            return "one_phase"
        if self._generic_handle("NVSR_GENERIC_TWO_PHASE") != "1" and not self._generic_width_in(
                self.GENERIC_TWO_PHASE_DEFAULT_HIDDEN.get(self.generic_arithmetic())):
            return "one_phase"
        return "two_phase"

    def generic_phases_allowed(self):
        """what a frame in two phases and a frame under an occupancy grid (train_utils._generic_occupancy) both need: NVSR_GENERIC_TWO_PHASE
        is not 0, the geometry is a generic one, no jitter of the sample positions, and generic_route() == 'fused'"""
        return not (self._generic_handle("NVSR_GENERIC_TWO_PHASE") == "0" or self.is_native_geometry() or self.jitter_std()
                    or self.generic_route() != "fused")

    def _generic_phase_args(self, points, coord_noise):
        if torch.is_grad_enabled() and self._generic_graph()[2]:
            raise RuntimeError("density_field / colour_field_ are evaluation operators: call them under torch.no_grad()")
        planes, consts, nat = self._generic_eval_args()
        limb = self.generic_arithmetic() == "f16x2"
        packed = self.packed_generic_decoder() if limb else nat.new_empty(0)
        if coord_noise is not None:
            coord_noise = capi.f32c(coord_noise.to(points.device))
        return (planes, consts, nat, packed, self.generic_geometry(), points), \
               (bool(self.align_corners), coord_noise, self.plane_interp == "bicubic", capi.ARITHMETIC["f16x2" if limb else "f32"])

    def density_field(self, points, coord_noise=None):
        """the density decoder alone on points [P,6] -> raw [P,4] = [+0, +0, +0, sigma_raw]: the fused kernel's density phase
        (torch.ops.nvsr.triplane_density_generic_fused_arith) in generic_arithmetic(), sigma_raw with the bits of forward().  Evaluation only;
        raises for a geometry beyond the fused kernel's capacity."""
        head, tail = self._generic_phase_args(points, coord_noise)
        return torch.ops.nvsr.triplane_density_generic_fused_arith(*head, *tail)

    def density_field_kept(self, points, grid, G):
        """density_field on the points an occupancy grid (G^3 bits, build_occupancy) keeps: the keep mask of the point list
        (torch.ops.nvsr.generic_occupancy_keep), its ascending list (generic_live_list), the density phase over the list
        (triplane_density_list_generic_fused_arith) -- all enqueued, nothing read back.  -> (raw [P,4], index int32 [P], count int32 [1]): a
        kept row is [+0, +0, +0, sigma_raw] with the bits of forward(), a culled row [+0, +0, +0, capi.CULLED_SIGMA]; index[:count] are the kept
        points.  Points with a NaN coordinate or outside the box are kept.  No jitter of the sample positions: evaluation only."""
        head, tail = self._generic_phase_args(points, None)
        keep, raw = torch.ops.nvsr.generic_occupancy_keep(head[1], points, grid, int(G))
        index, count = torch.ops.nvsr.generic_live_list(keep)
        torch.ops.nvsr.triplane_density_list_generic_fused_arith(raw, *head, index, count, *tail)
        return raw, index, count

    def colour_field_(self, raw, points, index, count, coord_noise=None):
        """the colour decoder on points[index[:count]], written in place into raw[index[:count], 0:3] with the bits of forward(); the rest of
        raw [P,4] stays (torch.ops.nvsr.triplane_colour_generic_fused_arith; index int32 [n], count int32 [1], both on the device -- what
        torch.ops.nvsr.generic_live_list returns).  -> raw"""
        head, tail = self._generic_phase_args(points, coord_noise)
        torch.ops.nvsr.triplane_colour_generic_fused_arith(raw, *head, index, count, *tail)
        return raw

    def scene_args(self, planes=None, check_native=True):
        """(planes, consts) of the current scene id as the torch.ops.nvsr operators take them: the channel-last planes (position planes, then
        the view-direction plane) + the host floats of struct nvsr_scene / nvsr_scene_ext (lo[5], range[5], a 3x2 projection per position
        plane: 28 for the three planes of the MFMA kernels).  planes: optional explicit channel-last planes (the training path samples
        tensors that are part of the autograd graph)."""
        if check_native:
            self._check_native_geometry()
        if planes is None:
            if hasattr(self, "SR_model") and not self.skip_SR_ and not (self.SR_model.training and torch.is_grad_enabled()):
                # evaluation: super-resolve every plane that needs it in one batched pass; _plane_source then hits the cache
                names = [get_plane_name(self.cur_id, d) for d in range(self.num_density_planes)]
                names = [n for n in names if self._should_SR(n)]
                if self.scene_coupler is not None:
                    names = [self.scene_coupler.scene_with_saved_plane(n, plane_not_scene=True) for n in names]
                self._refresh_LR_planes(names)
                self.SR_model.super_resolve_many(names)
            planes = [self.channel_last_plane(d) for d in range(self.num_density_planes + 1)]
        # box and projection matrices as host floats: read back once per version (a device-to-host copy drains the queue, and this runs
        # for every pass of every training iteration)
        box_t = self.box_coords[self.cur_id + ""]
        rots = [self.coord_projector.rot_mats_NON_LEARNED[d] for d in range(self.num_density_planes)]
        key = (self.cur_id, box_t.data_ptr(), box_t._version) + tuple((r.data_ptr(), r._version) for r in rots)
        cache = self.__dict__.get("_scene_consts")
        if cache is None or cache[0] != key:
            box = box_t.detach().double().cpu().numpy()
            lo = [np.float32(box[0, i]) for i in range(5)]
            rng = [np.float32(box[1, i] - box[0, i]) for i in range(5)]   # subtraction in double, then cast (models.py:264-265)
            proj = []
            for r in rots:
                m = r.detach().float().cpu().numpy()[:, 1:]
                proj.append([float(m[k, c]) for k in range(3) for c in range(2)])
            consts = [float(v) for v in lo] + [float(v) for v in rng] + [v for row in proj for v in row]
            cache = (key, lo, rng, proj, consts)
            self.__dict__["_scene_consts"] = cache
        return list(planes), cache[4]

    def _warn_no_points_grad(self, why):
        """once per model: a point tensor that requires grad met a route that returns no gradient for it"""
        if not self.__dict__.get("_points_grad_warned"):
            import warnings
            warnings.warn("TwoDimPlanesModel: the points require a gradient, but a model call with %s returns none for them (x.grad stays "
                          "None); the shipped geometry in 'f16x2' / 'bf16x3' does" % why)
            self.__dict__["_points_grad_warned"] = True

    def density_gradient(self, points):
        """d sigma_raw / d xyz of points [P,6] = [xyz, viewdir] -> [P,3], under no_grad (sigma_raw: column 3 of forward(), before the
        activation).  One-sample rays through decode_rays with gates, the rows backward of g_raw = (0, 0, 0, 1) for the three position
        planes (no view workspace, no record), torch.ops.nvsr.triplane_points_grad.  The TRUE derivative; a normal is -normalize(.) of it.
        The shipped geometry in a limb arithmetic only."""
        if not self.is_native_geometry():
            raise NotImplementedError("density_gradient: the shipped decoder geometry only (this model runs a generic one)")
        arith = capi.resolve_decoder_arithmetic(self.arithmetic)
        if arith == capi.ARITHMETIC["f32"]:
            raise NotImplementedError("density_gradient: the limb arithmetics 'f16x2' / 'bf16x3' only (this model resolves to 'f32')")
        with torch.no_grad():
            x = capi.f32c(points)
            assert x.shape[-1] == 6, "TwoDimPlanesModel expects [xyz, viewdir] rows"
            P = x.numel() // 6
            x = x.reshape(P, 6)
            if P == 0:
                return torch.empty((0, 3), dtype=torch.float32, device=x.device)
            rays = torch.zeros((P, 11), dtype=torch.float32, device=x.device)
            rays[:, 0:3] = x[:, 0:3]
            rays[:, 8:11] = x[:, 3:6]
            z = torch.zeros((P, 1), dtype=torch.float32, device=x.device)
            planes, consts = self.scene_args()
            _, gates, _ = torch.ops.nvsr.decode_rays(planes, consts, self.packed_decoder(), rays, z, True, False, arith)
            g_raw = torch.zeros((P, 1, 4), dtype=torch.float32, device=x.device)
            g_raw[..., 3] = 1.0
            rows = ops.decode_rays_backward_rows(planes, consts, self.packed_decoder(), self.packed_decoder_bwd(), rays, z, g_raw, gates, arith)
            return torch.ops.nvsr.triplane_points_grad(planes, consts, rays, z, rows, rays.new_empty(0))[0]

    def native_scene(self, planes=None):
        """struct nvsr_scene for the current scene id (+ the tensors that must outlive the launch) for direct C-ABI calls"""
        planes, consts = self.scene_args(planes)
        return ops._scene(planes, consts), planes

    def arith(self):
        """NVSR_ARITH_* code of this model's calls (-1 = the process default; 'f16' is an arithmetic of evaluation renders: the library
        refuses it to a direct model call, a grid build or a training step)"""
        return capi.render_arith_code(self.arithmetic)

    # |value| limits of NVSR_ARITH_F16X2's static scales (include/nvsr.h): weights are packed as W 2^8, features held as x 2^4
    F16_WEIGHT_LIMIT, F16_FEATURE_LIMIT = 255.0, 4094.0

    def f16_operands_in_range(self, planes):
        """True if the decoder weights and the given channel-last planes fit NVSR_ARITH_F16X2's ranges.  One reduction + one host read per
        tensor VERSION (cached): evaluation renders call it, training steps (whose planes change every iteration) do not -- there an
        out-of-range operand shows as a NaN loss, never as a wrong number (csrc/render3.hip)."""
        cache = self.__dict__.setdefault("_f16_range_cache", {})
        ok = True
        # the matrices the matrix pipe multiplies: the hidden / feature layers' weights (heads and biases stay f32 vector arithmetic)
        mats = [p for n, p in self.named_parameters() if n.endswith(".weight") and (n.startswith("density_dec.") or n.startswith("rgb_dec."))]
        for t, limit in [(w, self.F16_WEIGHT_LIMIT) for w in mats] + [(p, self.F16_FEATURE_LIMIT) for p in planes]:
            # (the tensor OBJECT is part of the entry: a regenerated low-rank plane or a new super-resolved plane is a fresh tensor -- version 0, the
            #  same shape, usually at the address the allocator has just got back -- and must not inherit its predecessor's verdict)
            key = (t.data_ptr(), t._version, tuple(t.shape))
            hit = cache.get(key)
            if hit is None or hit[0]() is not t:
                if len(cache) > 64:
                    cache.clear()
                hit = cache[key] = (weakref.ref(t), bool(torch.isfinite(t).all()) and float(t.detach().abs().max()) < limit if t.numel() else True)
            ok = ok and hit[1]
        return ok

    def render_arithmetic(self, planes, training):
        """the NVSR_ARITH_* code a render of `planes` through this model runs in: the model's / the process's choice, except that an
        EVALUATION render whose operands do not fit the f16 limbs falls back to the 3-bf16-limb arithmetic (warned once) instead of
        rendering NaN pixels.  Hidden activations beyond the range cannot be known beforehand: those still render NaN."""
        code = capi.resolve_render_arithmetic(self.arithmetic)
        if code in (capi.RENDER_ARITHMETIC["f16x2"], capi.RENDER_ARITHMETIC["f16"]) and not training and not self.f16_operands_in_range(planes):
            if not self.__dict__.get("_f16_warned"):
                import warnings
                warnings.warn("decoder weights or plane values beyond NVSR_ARITH_F16X2's range (|W| < 255, |feature| < 4094): rendering this "
                              "model in 'bf16x3' (set model.arithmetic to silence)")
                self.__dict__["_f16_warned"] = True
            return capi.ARITHMETIC["bf16x3"]
        return code

    def forward(self, x, coord_noise=None):
        """models.py:381-421: x [P,6] = [xyz, viewdir] -> [P,4] = [rgb, sigma] (pre-activation).  coord_noise (not in the reference's
        signature): the point_coords_noise jitter of this call, [P,3], when the caller draws it (_generic_forward)."""
        x = capi.f32c(x)
        assert x.shape[-1] == 6, "TwoDimPlanesModel expects [xyz, viewdir] rows"
        P = x.numel() // 6
        if P == 0:
            return torch.empty(list(x.shape[:-1]) + [4], dtype=torch.float32, device=x.device)
        x_grad = x.requires_grad and torch.is_grad_enabled()
        if not self.is_native_geometry():
            if x_grad:
                self._warn_no_points_grad("a generic decoder geometry")
            return self._generic_forward(x.reshape(P, 6), coord_noise).reshape(list(x.shape[:-1]) + [4])
        assert coord_noise is None, "a jitter for a forward that does not jitter (point_coords_noise == 0 or evaluation mode)"
        if x_grad and capi.resolve_decoder_arithmetic(self.arithmetic) == capi.ARITHMETIC["f32"]:
            self._warn_no_points_grad("the 'f32' arithmetic")
            x_grad = False
        if self.training and torch.is_grad_enabled() and not (hasattr(self, "SR_model") and not self.skip_SR_):
            names = [get_plane_name(self.cur_id, d) for d in range(self.num_density_planes + 1)]
            dec = any(p.requires_grad for p in self.decoder_parameters())
            if dec or x_grad or any(self.planes_[n].requires_grad for n in names):
                planes = [self.raw_plane(n) for n in names]
                # run_network's differentiable model call (train_utils.py:15-64): gradients for the planes and the decoder
                # models.py:393 `np.random.randint(len(self.density_dec))`: the reference picks an ensemble member on every training-mode
                # forward.  With ensemble_size == 1 (the only supported size) the call returns 0 WITHOUT drawing from NumPy's stream (a
                # zero-width range consumes no state: tests/test_host.py::test_single_member_ensemble_draw_leaves_numpy_stream_alone), so
                # the pixel selection of a seeded run (train_nerf.py:839) is unaffected; the call is kept for literal parity.
                np.random.randint(self.ensemble_size)
                out = _DecodePointsFn.apply(self, x.reshape(P, 6), *planes, self.natural_blob(differentiable=True) if dec else None)
                return out.reshape(list(x.shape[:-1]) + [4])
        planes, consts = self.scene_args()
        out = torch.ops.nvsr.triplane_decode(planes, consts, self.packed_decoder(), x.reshape(P, 6), self.arith())
        return out.reshape(list(x.shape[:-1]) + [4])


class _DecodePointsFn(torch.autograd.Function):
    """TwoDimPlanesModel.forward on a list of points with gradients for the planes, the decoder and -- in the limb arithmetics -- the
    points themselves.  The points are handed to the ray-tiled training kernels as one-sample rays (origin = point, direction = 0,
    depth = 0): decode with published ReLU gates (+ the layer-input record when the decoder trains), gate-driven backward, weight-gradient
    contraction.  The backward adds into one set of zero-filled gradient planes on the route ops.gate_route names (ops.gate_backward_, as
    train_utils._RenderRaysFn does per pass): points that require a gradient take the rows route once, whatever the deterministic mode says
     -- the same rows feed the ordered scatter into the planes and torch.ops.nvsr.triplane_points_grad -- and the record is
    contracted by the mode's own weight-gradient operator.  The position columns are the TRUE derivative (the reference projects under
    no_grad and returns 0 there)."""

    @staticmethod
    def forward(ctx, model, x, p0, p1, p2, pv, nat):
        P, dev = x.shape[0], x.device
        rays = torch.zeros((P, 11), dtype=torch.float32, device=dev)
        rays[:, 0:3] = x[:, 0:3]
        rays[:, 8:11] = x[:, 3:6]
        z = torch.zeros((P, 1), dtype=torch.float32, device=dev)
        planes_cl = [to_channel_last(p.detach()) for p in (p0, p1, p2, pv)]
        ctx.plane_srcs = (p0, p1, p2, pv)
        planes_cl, consts = model.scene_args(planes=planes_cl)
        arith = capi.resolve_decoder_arithmetic(model.arithmetic)      # the backward runs in the mode the gates / record were made in
        ctx.det = capi.deterministic()                                  # ... and on the route (atomic / ordered) resolved here
        if ctx.det and arith == capi.ARITHMETIC["f32"]:
            capi.refuse_deterministic("a differentiable model call in the 'f32' arithmetic")
        raw, gates, rec = torch.ops.nvsr.decode_rays(planes_cl, consts, model.packed_decoder(), rays, z, True, nat is not None, arith)
        ctx.model, ctx.state = model, (planes_cl, consts, rays, z, gates, rec if nat is not None else None, arith)
        return raw.reshape(P, 4)

    @staticmethod
    def backward(ctx, g_out):
        model = ctx.model
        planes_cl, consts, rays, z, gates, rec, arith = ctx.state
        P = rays.shape[0]
        need = ctx.needs_input_grad
        need_planes = [bool(n) for n in need[2:6]]
        need_x = bool(need[1]) and arith != capi.ARITHMETIC["f32"]          # ('f32': x.grad stays None, forward() has warned)
        if not any(need_planes) and rec is None and not need_x:
            return (None,) * 7
        g_raw = capi.f32c(g_out).reshape(P, 1, 4)
        nv = torch.ops.nvsr
        gplanes = ops.zero_planes_like(planes_cl, need_planes, rays)
        gx = ops.gate_backward_(nv, ops.gate_route(ctx.det, need_x), planes_cl, consts, model.packed_decoder(), model.packed_decoder_bwd(), rays, z, g_raw,
                                gates, rec, need_planes, arith, gplanes)
        gx = None if gx is None else torch.cat(gx, -1)
        gnat = None
        if rec is not None and need[6]:      # (the weight gradient contracts in the MODE's operator, also behind points that took the ordered route)
            gnat = nv.decoder_weight_grad_det(rec, P, 1, arith, None) if ctx.det else nv.decoder_weight_grad(rec, P, 1, arith)
        return (None, gx) + tuple(from_channel_last(g, like=p_) if n else None for g, p_, n in zip(gplanes, ctx.plane_srcs, need_planes)) + (gnat,)


def _generic_forward_state(ctx, model, x, nat, coord_noise, plane_srcs):
    """what the forwards of the four generic autograd functions share: the refusal in the deterministic mode (before any launch), the
    channel-last planes and the scene constants, the natural blob (nat, or the model's where the decoder does not train) -> the arguments of the
    forward operator, kept as ctx.state for the backward"""
    if capi.deterministic():
        capi.refuse_deterministic("training a generic decoder geometry (generic.hip)")
    planes_cl, consts = model.scene_args(planes=[to_channel_last(p.detach()) for p in plane_srcs], check_native=False)
    natural = model.natural_blob() if nat is None else nat.detach()
    capi.require_cuda(natural)
    ctx.plane_srcs = plane_srcs
    ctx.state = (planes_cl, consts, natural, model.generic_geometry(), x, bool(model.align_corners), coord_noise, model.plane_interp == "bicubic")
    return ctx.state


class _GenericDecodeFn(torch.autograd.Function):
    """TwoDimPlanesModel.forward for a decoder geometry / option set other than the shipped one, with gradients for the planes and the
    decoder (torch.ops.nvsr.triplane_decode_generic / _backward: csrc/generic.hip recomputes the forward in the backward).
    inputs: model, x, natural blob (None = the decoder does not train), jitter (None = none), then the planes of the scene."""

    @staticmethod
    def forward(ctx, model, x, nat, coord_noise, *plane_srcs):
        return torch.ops.nvsr.triplane_decode_generic(*_generic_forward_state(ctx, model, x, nat, coord_noise, plane_srcs))

    @staticmethod
    def backward(ctx, g_out):
        planes_cl, consts, natural, geometry, x, align, coord_noise, bicubic = ctx.state
        need = ctx.needs_input_grad
        need_planes = [bool(n) for n in need[4:]]
        if not any(need_planes) and not need[2]:
            return (None,) * len(need)
        g = torch.ops.nvsr.triplane_decode_generic_backward(planes_cl, consts, natural, geometry, x, capi.f32c(g_out), bool(need[2]), need_planes,
                                                            align, coord_noise, bicubic)
        return (None, None, g[0] if need[2] else None, None) + \
               tuple(from_channel_last(gp, like=p_) if n else None for gp, p_, n in zip(g[1:], ctx.plane_srcs, need_planes))


class _GenericFusedTrainFn(torch.autograd.Function):
    """_GenericDecodeFn for a decoder that takes no gradient, on the fused kernels (TwoDimPlanesModel.generic_train_route() == 'fused'): the
    forward is torch.ops.nvsr.triplane_decode_generic_fused (the layered forward's bits), the backward
    torch.ops.nvsr.triplane_decode_generic_fused_backward (csrc/generic_fused_bwd.hip: the planes' gradients in one launch, exact f32).
    inputs: model, x, jitter (None = none), then the planes of the scene."""

    @staticmethod
    def forward(ctx, model, x, coord_noise, *plane_srcs):
        return torch.ops.nvsr.triplane_decode_generic_fused(*_generic_forward_state(ctx, model, x, None, coord_noise, plane_srcs))

    @staticmethod
    def backward(ctx, g_out):
        planes_cl, consts, natural, geometry, x, align, coord_noise, bicubic = ctx.state
        need = ctx.needs_input_grad
        need_planes = [bool(n) for n in need[3:]]
        if not any(need_planes):
            return (None,) * len(need)
        g = torch.ops.nvsr.triplane_decode_generic_fused_backward(planes_cl, consts, natural, geometry, x, capi.f32c(g_out), need_planes, align,
                                                                  coord_noise, bicubic)
        return (None, None, None) + tuple(from_channel_last(gp, like=p_) if n else None for gp, p_, n in zip(g, ctx.plane_srcs, need_planes))


class _GenericFusedDecoderTrainFn(torch.autograd.Function):
    """_GenericDecodeFn on the fused kernels for a decoder that DOES take gradients (TwoDimPlanesModel.generic_decoder_train_route() ==
    'fused'): the forward is torch.ops.nvsr.triplane_decode_generic_fused (the layered forward's bits), the backward
    torch.ops.nvsr.triplane_decode_generic_fused_backward_record (csrc/generic_fused_bwd.hip: per chunk one launch that scatters the planes'
    gradients and records the weight gradients' operands, then the layered contractions on the record), exact f32.
    inputs: model, x, the differentiable natural blob, jitter (None = none), then the planes of the scene."""

    @staticmethod
    def forward(ctx, model, x, nat, coord_noise, *plane_srcs):
        return torch.ops.nvsr.triplane_decode_generic_fused(*_generic_forward_state(ctx, model, x, nat, coord_noise, plane_srcs))

    @staticmethod
    def backward(ctx, g_out):
        planes_cl, consts, natural, geometry, x, align, coord_noise, bicubic = ctx.state
        need = ctx.needs_input_grad
        need_planes = [bool(n) for n in need[4:]]
        if not any(need_planes) and not need[2]:
            return (None,) * len(need)
        g = torch.ops.nvsr.triplane_decode_generic_fused_backward_record(planes_cl, consts, natural, geometry, x, capi.f32c(g_out), bool(need[2]),
                                                                         need_planes, align, coord_noise, bicubic)
        return (None, None, g[0] if need[2] else None, None) + \
               tuple(from_channel_last(gp, like=p_) if n else None for gp, p_, n in zip(g[1:], ctx.plane_srcs, need_planes))


class _GenericFusedLimbTrainFn(torch.autograd.Function):
    """_GenericFusedTrainFn in 'f16x2' (TwoDimPlanesModel.generic_train_arithmetic() == 'f16x2'): the forward is
    torch.ops.nvsr.triplane_decode_generic_fused_arith on the packed blob -- the limb evaluation kernel's bits, under its range contract: nothing
    is rendered again, the range flag reaches the iteration's metrics (TrainStep._range_word) -- and the backward
    torch.ops.nvsr.triplane_decode_generic_fused_backward_arith (csrc/generic_fused_bwd_limb.hip: the planes' gradients in one launch on two f16
    limbs).  inputs: model, x, jitter (None = none), then the planes of the scene."""

    @staticmethod
    def forward(ctx, model, x, coord_noise, *plane_srcs):
        planes_cl, consts, natural, geometry, x, align, coord_noise, bicubic = _generic_forward_state(ctx, model, x, None, coord_noise, plane_srcs)
        ctx.blobs = (model.packed_generic_decoder(), model.packed_generic_decoder_bwd())
        return torch.ops.nvsr.triplane_decode_generic_fused_arith(planes_cl, consts, natural, ctx.blobs[0], geometry, x, align, coord_noise, bicubic,
                                                                  capi.ARITHMETIC["f16x2"])

    @staticmethod
    def backward(ctx, g_out):
        planes_cl, consts, natural, geometry, x, align, coord_noise, bicubic = ctx.state
        need = ctx.needs_input_grad
        need_planes = [bool(n) for n in need[3:]]
        if not any(need_planes):
            return (None,) * len(need)
        g = torch.ops.nvsr.triplane_decode_generic_fused_backward_arith(planes_cl, consts, natural, ctx.blobs[0], ctx.blobs[1], geometry, x,
                                                                        capi.f32c(g_out), need_planes, align, coord_noise, bicubic,
                                                                        capi.ARITHMETIC["f16x2"])
        return (None, None, None) + tuple(from_channel_last(gp, like=p_) if n else None for gp, p_, n in zip(g, ctx.plane_srcs, need_planes))


# =======================================================================================================================
# Feature-plane super-resolution: EDSR wrapped by PlanesSR (models.py:768-926)
# =======================================================================================================================
def _cfg_get(node, name, default=None):
    if isinstance(node, dict):
        return node.get(name, default)
    return getattr(node, name, default)


class _Residual_Block(nn.Module):
    """models.py:769-786 (parameters only; the arithmetic is the fused conv -> ReLU -> conv -> x0.1 + cropped identity kernels)"""

    def __init__(self, hidden_size, padding, kernel_size):
        super().__init__()
        self.margins = None if (padding or kernel_size == 1) else 2 * (kernel_size // 2)
        self.conv1 = nn.Conv2d(hidden_size, hidden_size, kernel_size, stride=1, padding=padding, bias=False)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(hidden_size, hidden_size, kernel_size, stride=1, padding=padding, bias=False)


class EDSR(nn.Module):
    """models.py:789-822.  Same constructor, `required_padding` arithmetic and state-dict keys; forward runs nvsr_edsr_forward
    (MFMA implicit-GEMM convolutions with fused ReLU / residual / PixelShuffle epilogues).

    receptive_field_bound (models.py:793-798): a layer whose 3 x 3 kernel would push the receptive field beyond the bound is a 1 x 1
    convolution.  The parameters keep the reference's shapes; the kernels run every layer as a 3 x 3 convolution, a 1 x 1 weight sitting in
    the centre of a zero kernel.  Such a layer returns the true layer's output minus a one-texel border, so the network is fed `_extra_pad`
    more texels of context per side (they meet zero weights only) and its output is cropped accordingly: same values, nine times the
    arithmetic in those layers (no shipped config sets the option)."""

    def __init__(self, in_channels, out_channels, hidden_size, n_blocks, scale_factor, padding, receptive_field_bound=np.iinfo(np.int32).max,
                 **kwargs):
        super().__init__()
        import math
        KERNEL_SIZE = 3
        self.required_padding, rf_factor = 0, 1
        self._all3_padding = 0           # required_padding of the network the kernels run (every layer 3 x 3)
        if padding != 0:
            raise NotImplementedError("the SR kernels implement the un-padded convolutions PlanesSR uses (PADDING = 0, models.py:836)")

        def kernel_size(num_layers=1):
            grow = rf_factor * num_layers * (KERNEL_SIZE // 2)
            self._all3_padding += grow
            if (1 + 2 * (self.required_padding + rf_factor * num_layers * ((KERNEL_SIZE - 1) // 2))) <= receptive_field_bound:
                self.required_padding += grow
                return KERNEL_SIZE
            return 1

        self.conv_input = nn.Conv2d(in_channels, hidden_size, kernel_size(), stride=1, padding=padding, bias=False)
        self.residual = nn.Sequential()
        for _ in range(n_blocks):
            self.residual.append(_Residual_Block(hidden_size=hidden_size, padding=padding, kernel_size=kernel_size(2)))
        self.conv_mid = nn.Conv2d(hidden_size, hidden_size, kernel_size(), stride=1, padding=padding, bias=False)
        assert math.log2(scale_factor) == int(math.log2(scale_factor)), "Supperting only scale factors that are an integer power of 2."
        upscaling_layers = []
        for _ in range(int(math.log2(scale_factor))):
            upscaling_layers += [nn.Conv2d(hidden_size, hidden_size * 4, kernel_size(), stride=1, padding=padding, bias=False), nn.PixelShuffle(2)]
            rf_factor /= 2
        self.upscale = nn.Sequential(*upscaling_layers)
        self.conv_output = nn.Conv2d(hidden_size, out_channels, kernel_size(), stride=1, padding=padding, bias=False)
        self.geometry = (in_channels, out_channels, hidden_size, n_blocks, int(math.log2(scale_factor)))
        # stand-alone forward: context the 3 x 3 stand-ins of the 1 x 1 layers consume, in input texels (rounded up; the rest is cropped from the
        # output, a whole number of output texels because every increment is a multiple of 1 / scale_factor)
        extra = self._all3_padding - self.required_padding
        self._extra_pad = int(math.ceil(extra))
        self._extra_crop = int(round((self._extra_pad - extra) * scale_factor))
        self._packed_cache = None
        # 'f32' | 'bf16x3' | 'f16x2' | 'f16' (capi.CONV_ARITHMETIC) | None = the process default (capi.set_conv_arithmetic / NVSR_CONV_ARITHMETIC)
        self.arithmetic = None

    def invalidate(self):
        """forget the packed weight blobs (needed after writes through `.data`, which do not bump a tensor's version counter)"""
        self._packed_cache = None
        self._packed_dgrad_cache = None

    def train(self, mode=True):
        """nn.Module.train; a CHANGE of mode drops the packed blobs (see TwoDimPlanesModel.train)"""
        if bool(mode) != self.training:
            self.invalidate()
        return super().train(mode)

    def arith(self):
        return capi.conv_arith_code(self.arithmetic)

    def conv_parameters(self):
        """the convolution weights in state-dict order, as the reference shapes them (3 x 3 or 1 x 1)"""
        ws = [self.conv_input.weight]
        for blk in self.residual:
            ws += [blk.conv1.weight, blk.conv2.weight]
        ws.append(self.conv_mid.weight)
        ws += [m.weight for m in self.upscale if isinstance(m, nn.Conv2d)]
        ws.append(self.conv_output.weight)
        return ws

    def conv_weights(self):
        """the 3 x 3 kernels the library runs: a 1 x 1 weight (receptive_field_bound) in the centre of a zero kernel -- differentiable, so a
        gradient of the 3 x 3 blob reaches the 1 x 1 parameter through its centre tap"""
        return [w if w.shape[-1] == 3 else torch.nn.functional.pad(w, (1, 1, 1, 1)) for w in self.conv_parameters()]

    def packed_weights(self, arithmetic=None):
        """the fragment blob of the forward convolutions, cached on the parameters' (data_ptr, version).  arithmetic: None = every fragment region
        (a blob any arithmetic can run: evaluation, whose range fallback re-renders in bf16x3); an NVSR_ARITH_* code = only the regions that
        arithmetic reads (training: the weights change every iteration and both blobs are re-packed -- a fifth of the bytes); a cached blob with
        every region serves any request"""
        key = tuple((w.data_ptr(), w._version) for w in self.conv_parameters())
        kinds = capi.PACK_ALL_ARITHMETICS if (arithmetic is None or os.environ.get("NVSR_PACK_ALL") == "1") else int(arithmetic)
        c = self._packed_cache
        if c is None or c[0] != key or c[2] not in (kinds, capi.PACK_ALL_ARITHMETICS):
            ws = self.conv_weights()
            nat = torch.cat([w.detach().reshape(-1).float() for w in ws])
            capi.require_cuda(nat)
            c = self._packed_cache = (key, torch.ops.nvsr.pack_edsr(nat, list(self.geometry), False, kinds), kinds)
        return c[1]

    def natural_blob(self, differentiable=False):
        """conv weights flattened in state-dict order (the layout nvsr_pack_edsr consumes and nvsr_edsr_backward fills)"""
        return torch.cat([(w if differentiable else w.detach()).reshape(-1).float() for w in self.conv_weights()])

    def packed_dgrad_weights(self, arithmetic=None):
        """fragments of every layer's data gradient (flipped, transposed kernels), cached like packed_weights()"""
        key = tuple((w.data_ptr(), w._version) for w in self.conv_parameters())
        kinds = capi.PACK_ALL_ARITHMETICS if (arithmetic is None or os.environ.get("NVSR_PACK_ALL") == "1") else int(arithmetic)
        cache = getattr(self, "_packed_dgrad_cache", None)
        if cache is None or cache[0] != key or cache[2] not in (kinds, capi.PACK_ALL_ARITHMETICS):
            nat = self.natural_blob()
            capi.require_cuda(nat)
            cache = (key, torch.ops.nvsr.pack_edsr(nat, list(self.geometry), True, kinds), kinds)
            self._packed_dgrad_cache = cache
        return cache[1]

    def wants_grad(self, *inputs):
        return torch.is_grad_enabled() and (any(w.requires_grad for w in self.conv_parameters()) or
                                            any(t is not None and t.requires_grad for t in inputs))

    def forward(self, x):
        x = capi.f32c(x)
        lead = x.shape[:-3]
        assert int(np.prod(lead)) == 1, "the SR network runs one plane at a time"
        x4 = x.reshape((1,) + tuple(x.shape[-3:]))
        if self._extra_pad:                                # (1 x 1 layers run as 3 x 3: see the class comment; the padding meets zero weights only)
            x4 = torch.nn.functional.pad(x4, (self._extra_pad,) * 4)
        if self.wants_grad(x):
            # gradients for the conv weights (through the flat state-dict-order blob) and the input: torch.ops.nvsr.edsr_train
            arith = capi.resolve_conv_arithmetic(self.arithmetic)
            out, _ = torch.ops.nvsr.edsr_train(x4, self.natural_blob(differentiable=True), self.packed_weights(arith), self.packed_dgrad_weights(arith),
                                               list(self.geometry), arith)
        else:
            out = torch.ops.nvsr.edsr(x4, self.packed_weights(), list(self.geometry), self.arith())
        if self._extra_crop:
            out = out[..., self._extra_crop:-self._extra_crop, self._extra_crop:-self._extra_crop]
        return out.reshape(tuple(lead) + tuple(out.shape[-3:]))


class PlanesSR(nn.Module):
    """models.py:824-926.  `forward(plane_name | (plane_name, roi))` -> super-resolved plane [1,C,sf*R,sf*R]; NaN outside the ROI."""

    def __init__(self, model_arch, scale_factor, in_channels, out_channels, sr_config, plane_interp):
        super().__init__()
        import math
        model_cfg = _cfg_get(sr_config, "model")
        hidden_size, n_blocks = _cfg_get(model_cfg, "hidden_size"), _cfg_get(model_cfg, "n_blocks")
        input_normalization = _cfg_get(sr_config, "input_normalization", False)
        self.scale_factor = scale_factor
        self.plane_interp = plane_interp
        self.input_noise = _cfg_get(sr_config, "sr_input_noise", 0)
        self.output_noise = _cfg_get(sr_config, "sr_output_noise", 0)
        if plane_interp not in ("bilinear", "bicubic"):
            raise NotImplementedError("PlanesSR kernels implement the bilinear and bicubic residual up-sampling (config/TrainModels.yml:72,172)")
        self.inner_model = model_arch(in_channels=in_channels, out_channels=out_channels, hidden_size=hidden_size, n_blocks=n_blocks,
                                      scale_factor=scale_factor, padding=0,
                                      receptive_field_bound=_cfg_get(model_cfg, "receptive_field_bound", np.iinfo(np.int32).max))
        # models.py:840-842
        self.HR_overpadding = int(self.inner_model.required_padding * self.scale_factor)
        self.inner_model.required_padding = int(np.ceil(self.inner_model.required_padding))
        self.HR_overpadding = self.inner_model.required_padding * self.scale_factor - self.HR_overpadding
        # the same two numbers for the network the kernels run (all 3 x 3: EDSR's class comment); equal to the above without receptive_field_bound
        all3 = getattr(self.inner_model, "_all3_padding", self.inner_model.required_padding)
        self._kernel_pad = int(np.ceil(all3))
        self._kernel_over = self._kernel_pad * self.scale_factor - int(all3 * self.scale_factor)
        for m in self.modules():       # models.py:843-848
            if isinstance(m, nn.Conv2d):
                n = m.kernel_size[0] * m.kernel_size[1] * m.out_channels
                m.weight.data.normal_(0, math.sqrt(2. / n) / 10)
        self.clear_SR_planes(all_planes=True)
        self.align_corners = True
        self.SR_viewdir = False
        if input_normalization:
            self.normalization_params({"mean": float("nan") * torch.ones([in_channels]), "std": float("nan") * torch.ones([in_channels])})

    def normalization_params(self, norm_dict):
        self.planes_mean_NON_LEARNED = nn.Parameter(norm_dict["mean"].reshape([1, -1, 1, 1]))
        self.planes_std_NON_LEARNED = nn.Parameter(norm_dict["std"].reshape([1, -1, 1, 1]))

    def interpolate_LR(self, id):
        return torch.nn.functional.interpolate(self.LR_planes[id], scale_factor=self.scale_factor, mode=self.plane_interp,
                                               align_corners=self.align_corners)

    def set_LR_plane(self, plane, id: str, save_interpolated: bool):
        assert id not in self.LR_planes, "Plane ID already exists."
        self.LR_planes[id] = plane
        # `save_interpolated` cached the bilinear up-sampling on the CPU in the reference (models.py:874-875); the finish kernel
        # recomputes it on the fly, so there is nothing to store.

    def invalidate(self):
        """forget everything derived from the parameters / LR planes (see EDSR.invalidate): packed weights and super-resolved planes"""
        self.inner_model.invalidate()
        self.clear_SR_planes()

    def clear_SR_planes(self, all_planes=False):
        for name in list(getattr(self, "SR_planes", {})):          # ... and their channel-last copies in the renderer's plane cache
            _PLANE_CACHE.pop(name + "/SR", None)
        self.__dict__.pop("_planes_arith", None)                     # (train_utils._sr_fallback: the arithmetic the cached planes were made in)
        planes_2_clear = ["SR_planes"]
        if all_planes:
            planes_2_clear += ["LR_planes", "residual_planes"]
        for attr in planes_2_clear:
            setattr(self, attr, {})

    def super_resolve_many(self, plane_names):
        """Full-plane, no-grad super-resolution of several equally sized planes in ONE batched pass (fills the cache `forward`
        serves from).  The reference super-resolves the planes one by one on first use (models.py:270-284); the values are the
        same, the batch keeps all 256 CUs busy."""
        todo = [n for n in plane_names if n not in self.SR_planes]
        if len(todo) < 2 or (self.training and (self.input_noise > 0 or self.output_noise > 0)):
            return
        lrs = [capi.f32c(self.LR_planes[n].detach()) for n in todo]
        if len({tuple(t.shape[-3:]) for t in lrs}) != 1:
            return
        Cc, R0, R1 = lrs[0].shape[-3:]
        cin, cout, hid, nb, n_up = self.inner_model.geometry
        mean = std = None
        if hasattr(self, "planes_mean_NON_LEARNED"):
            mean, std = capi.f32c(self.planes_mean_NON_LEARNED.detach().reshape(-1)), capi.f32c(self.planes_std_NON_LEARNED.detach().reshape(-1))
        pad, over = self._kernel_pad, self._kernel_over
        if capi.lib().nvsr_planes_sr_workspace_floats(Cc, R0, R1, hid, nb, n_up, pad, None) < 0:
            return
        outs = torch.ops.nvsr.planes_sr([t.reshape(Cc, R0, R1) for t in lrs], self.inner_model.packed_weights(), list(self.inner_model.geometry),
                                        pad, over, None, mean, std, self.inner_model.arith(), bool(self.align_corners),
                                        self.plane_interp == "bicubic")
        for n, o in zip(todo, outs):
            self.SR_planes[n] = o

    def _apply_training_noise(self, out, noise_in, lr_clean):
        """The training-mode noises of models.py:896-897,920-921 on the operator's output `out` = EDSR(prep(LR + n_in)) + up(LR + n_in) (NaN
        outside the region of interest): remove up(n_in) -- the reference's residual is up(LR) -- then add
        N(0, (sr_output_noise * difference.std())^2) over the region, difference = the network's (cropped) output.  Training only, not a
        hot path: plain torch on the device, draws from the CPU generator in the reference's order (input noise first)."""
        if noise_in is not None:
            out = out - torch.nn.functional.interpolate(noise_in, scale_factor=self.scale_factor, mode=self.plane_interp, align_corners=self.align_corners)
        if self.output_noise > 0:
            inside = ~torch.isnan(out.detach()[0, 0])
            rows, cols = inside.any(1).nonzero().flatten(), inside.any(0).nonzero().flatten()
            r0, r1, c0, c1 = int(rows[0]), int(rows[-1]) + 1, int(cols[0]), int(cols[-1]) + 1
            # difference = out - up(LR) on the region (the noisy LR plane's residual was removed above)
            resid = torch.nn.functional.interpolate(lr_clean.detach().float(), scale_factor=self.scale_factor, mode=self.plane_interp,
                                                    align_corners=self.align_corners)[..., r0:r1, c0:c1]
            diff = out.detach()[..., r0:r1, c0:c1] - resid
            sd_out = float(self.output_noise * diff.std())
            n_out = torch.normal(mean=0.0, std=sd_out, size=tuple(diff.shape)).to(device=out.device, dtype=torch.float32)
            pad_n = torch.zeros_like(out.detach())
            pad_n[..., r0:r1, c0:c1] = n_out
            out = out + pad_n
        return out

    def forward_many(self, requests):
        """[(plane_name, roi | None), ...] -> the super-resolved planes, like one forward() call per request (models.py:884-926).  In training,
        when gradients are wanted and the planes are equally sized, all requests go through the network TOGETHER (ops.PlanesSRBatchFn: one
        launch per layer convolves every plane's region of interest, one weight-gradient pass per layer in the backward); anything else --
        evaluation, the training noises of models.py:896-897,920-921, more than four planes -- is one forward() per request."""
        reqs = [(r, None) if isinstance(r, str) else (r[0], r[1]) for r in requests]
        lrs = [self.LR_planes[n] for n, _ in reqs]
        net = self.inner_model
        noisy = self.training and (self.input_noise > 0 or self.output_noise > 0)
        batched = (len(reqs) >= 2 and len(reqs) <= capi.SR_BATCH_MAX and self.training and net.wants_grad(*lrs) and not noisy
                   and len({tuple(t.shape[-3:]) for t in lrs}) == 1 and all(t.dtype == torch.float32 for t in lrs)
                   and all((roi is None) == (reqs[0][1] is None) for _, roi in reqs))
        if not batched:
            return [self.forward(n if roi is None else (n, roi)) for n, roi in reqs]
        rois = None
        if reqs[0][1] is not None:
            rois = [float(v) for _, roi in reqs for v in (roi if isinstance(roi, (list, tuple)) else torch.as_tensor(roi).detach().cpu().reshape(-1).tolist())]
        mean = std = None
        if hasattr(self, "planes_mean_NON_LEARNED"):
            mean, std = capi.f32c(self.planes_mean_NON_LEARNED.detach().reshape(-1)), capi.f32c(self.planes_std_NON_LEARNED.detach().reshape(-1))
        arith = capi.resolve_conv_arithmetic(net.arithmetic)
        cfg = dict(packed=net.packed_weights(arith), packed_dgrad=net.packed_dgrad_weights(arith), geometry=list(net.geometry), pad=self._kernel_pad,
                   over=self._kernel_over, rois=rois, mean=mean, std=std, arithmetic=arith,
                   align_corners=bool(self.align_corners), bicubic=self.plane_interp == "bicubic",
                   # data-parallel training: the weight-gradient blob all-reduced bucket by bucket inside the backward (distributed.OverlappedSRGradSync.attach)
                   bucket_sync=self.__dict__.get("grad_bucket_sync"))
        return list(ops.PlanesSRBatchFn.apply(cfg, net.natural_blob(differentiable=True), *lrs))

    def forward(self, plane_name):
        if isinstance(plane_name, tuple):
            full_plane, plane_roi, plane_name = False, plane_name[1], plane_name[0]
        else:
            full_plane, plane_roi = True, None
        lr_src = lr_clean = self.LR_planes[plane_name]
        differentiable = self.training and self.inner_model.wants_grad(lr_src)
        if plane_name in self.SR_planes and not differentiable:      # (a cached plane carries no graph: never serve it to a training step)
            return self.SR_planes[plane_name]
        noisy = self.training and (self.input_noise > 0 or self.output_noise > 0)
        noise_in = None
        if noisy and self.input_noise > 0:
            # models.py:896-897: LR_plane + N(0, (sr_input_noise * LR_plane.std())^2), drawn by torch.normal from the CPU generator (the
            # reference's call has no device: a seeded run draws the same numbers here).  Only the NETWORK sees the noisy plane -- the
            # bilinear residual is taken from self.LR_planes (models.py:858-868) -- so the fused operator runs on LR + n and the
            # up-sampled noise is taken out of its (linear) residual term below.
            sd_in = float(self.input_noise * lr_src.detach().float().std())
            noise_in = torch.normal(mean=0.0, std=sd_in, size=tuple(lr_src.shape)).to(device=lr_src.device, dtype=torch.float32)
            lr_src = lr_src + noise_in
        lr = capi.f32c(lr_src.detach())
        Cc, R0, R1 = lr.shape[-3:]
        cin, cout, hid, nb, n_up = self.inner_model.geometry
        assert Cc == cin == cout
        roi = None
        if plane_roi is not None:
            roi = [float(v) for v in torch.as_tensor(plane_roi).detach().cpu().reshape(-1)]
        mean = std = None
        if hasattr(self, "planes_mean_NON_LEARNED"):
            mean, std = capi.f32c(self.planes_mean_NON_LEARNED.detach().reshape(-1)), capi.f32c(self.planes_std_NON_LEARNED.detach().reshape(-1))
        pad, over = self._kernel_pad, self._kernel_over
        geometry = list(self.inner_model.geometry)
        if differentiable:
            # training: gradients for the EDSR weights and the (non-detached) LR plane; the result is never cached
            net = self.inner_model
            arith = capi.resolve_conv_arithmetic(net.arithmetic)
            out, _ = torch.ops.nvsr.planes_sr_train(lr_src if lr_src.dtype == torch.float32 else lr_src.float(), net.natural_blob(differentiable=True),
                                                    net.packed_weights(arith), net.packed_dgrad_weights(arith), geometry, pad, over, roi, mean, std,
                                                    arith, bool(self.align_corners), self.plane_interp == "bicubic")
            return self._apply_training_noise(out, noise_in, lr_clean) if noisy else out
        out = torch.ops.nvsr.planes_sr([lr.reshape(Cc, R0, R1)], self.inner_model.packed_weights(), geometry, pad, over, roi, mean, std,
                                       self.inner_model.arith(), bool(self.align_corners), self.plane_interp == "bicubic")[0]
        if noisy:
            return self._apply_training_noise(out, noise_in, lr_clean)          # (like the reference, a noisy plane is never cached: training only)
        if full_plane:
            self.SR_planes[plane_name] = out      # kept on the GPU (the reference parks it on the CPU and re-uploads per call, :893,:925)
        return out


# =======================================================================================================================
# Positional-encoding baseline (models.py:14-108) -- interface completeness, not the tri-plane hot path
# =======================================================================================================================
class FlexibleNeRFModel(nn.Module):
    """models.py:14-108 with use_viewdirs=True, num_layers_dir=1, scalar hidden_size (what train_nerf.py:342-348 builds)."""

    def __init__(self, num_layers=4, num_layers_dir=1, dirs_hidden_width_ratio=2, hidden_size=128, skip_connect_every=4,
                 num_encoding_fn_xyz=6, num_encoding_fn_dir=4, include_input_xyz=True, include_input_dir=True, use_viewdirs=True,
                 input_dim=None, xyz_input_2_dir=False):
        super().__init__()
        if isinstance(hidden_size, list) or not use_viewdirs or num_layers_dir != 1 or dirs_hidden_width_ratio != 2 or xyz_input_2_dir \
                or input_dim is not None:
            raise NotImplementedError("only the default FlexibleNeRFModel head layout is implemented natively")
        self.skip_connect_every = skip_connect_every
        self.dim_xyz = (3 if include_input_xyz else 0) + 2 * 3 * num_encoding_fn_xyz
        self.dim_dir = (3 if include_input_dir else 0) + 2 * 3 * num_encoding_fn_dir
        self.hidden_size, self.num_layers = hidden_size, num_layers
        self.layer1 = nn.Linear(self.dim_xyz, hidden_size)
        self.layers_xyz = nn.ModuleList()
        for i in range(num_layers - 1):
            if i % self.skip_connect_every == 0 and i > 0 and i != num_layers - 1:
                self.layers_xyz.append(nn.Linear(self.dim_xyz + hidden_size, hidden_size))
            else:
                self.layers_xyz.append(nn.Linear(hidden_size, hidden_size))
        self.use_viewdirs = True
        self.layers_dir = nn.ModuleList([nn.Linear(self.dim_dir + hidden_size, hidden_size // 2)])
        self.fc_alpha = nn.Linear(hidden_size, 1)
        self.fc_rgb = nn.Linear(hidden_size // 2, 3)
        self.fc_feat = nn.Linear(hidden_size, hidden_size)
        for i, l in enumerate(self.layers_xyz):      # the reference's forward concatenates whenever i % skip == 0 and i > 0 (:90-95)
            expect = hidden_size + (self.dim_xyz if (i % skip_connect_every == 0 and i > 0) else 0)
            if l.in_features != expect:
                raise NotImplementedError("this num_layers / skip_connect_every combination is inconsistent in the reference as well")

    # of the fused paths (mip_forward, pe_forward): 'f32' | 'bf16x3' | 'f16x2' (2 f16 limbs, NaN and the range flag beyond their range:
    # evaluation falls back to 'bf16x3' by itself, training raises -- train_utils._run_nerf_baseline, training.StepMetrics) | None (the process
    # default, with 'f16x2' read as 'bf16x3': capi.resolve_nerf_arithmetic)
    arithmetic = "bf16x3"

    def _layers(self):
        return [self.layer1] + list(self.layers_xyz) + [self.layers_dir[0], self.fc_alpha, self.fc_rgb, self.fc_feat]

    def natural_blob(self, differentiable=False):
        """parameters in state-dict order, one flat f32 tensor; differentiable=True keeps the graph to every nn.Linear, otherwise the blob is
        cached against the parameters' versions"""
        params = [t for m in self._layers() for t in (m.weight, m.bias)]
        if differentiable:
            return torch.cat([t.reshape(-1).float() for t in params])
        key = tuple((p.data_ptr(), p._version) for p in params)
        cache = self.__dict__.get("_natural_cache")
        if cache is None or cache[0] != key:
            cache = self.__dict__["_natural_cache"] = (key, torch.cat([t.detach().reshape(-1).float() for t in params]))
        return cache[1]

    def is_mip_baseline(self):
        """the geometry the Mip-NeRF kernels are built for: FlexibleNeRFModel(include_input_xyz=False), the constructor defaults otherwise"""
        return self._is_baseline(36)

    def is_pe_baseline(self):
        """the geometry the positional-encoding kernels are built for: num_encoding_fn_xyz=6, num_encoding_fn_dir=4, include_input_xyz and
        include_input_dir, the constructor defaults otherwise (dim_xyz 39 and dim_dir 27 admit no other encoding counts)"""
        return self._is_baseline(39)

    def _is_baseline(self, dim_xyz):
        return (self.dim_xyz == dim_xyz and self.dim_dir == 27 and self.hidden_size == 128 and self.num_layers == 4
                and all(l.in_features == 128 for l in self.layers_xyz))

    def mip_forward(self, rays, edges, radius, arithmetic=None):
        """The Mip-NeRF baseline's model call (train_utils.py:19-64 with mip_nerf=True, then forward): packed rays [N,11], interval edges
        [N,S+1], the cone radius -> raw [N,S,4].  The integrated positional encoding happens inside the kernel; with gradients enabled,
        loss.backward() reaches every nn.Linear of the model.  arithmetic: this call's, instead of self.arithmetic."""
        if not self.is_mip_baseline():
            raise NotImplementedError("the Mip-NeRF kernels are built for FlexibleNeRFModel(include_input_xyz=False) with the constructor defaults")
        return self._fused_forward(torch.ops.nvsr.mip_nerf, rays, edges, float(radius), arithmetic=arithmetic)

    def pe_forward(self, rays, z, arithmetic=None):
        """The positional-encoding baseline's model call (train_utils.py:15-64 with mip_nerf=False, then forward): packed rays [N,11], sample
        depths z [N,S] -> raw [N,S,4].  The points ro + rd z and their positional encoding happen inside the kernel; with gradients enabled,
        loss.backward() reaches every nn.Linear of the model.  arithmetic: this call's, instead of self.arithmetic."""
        if not self.is_pe_baseline():
            raise NotImplementedError("the positional-encoding kernels are built for FlexibleNeRFModel(num_encoding_fn_xyz=6, num_encoding_fn_dir=4, "
                                      "include_input_xyz=True, include_input_dir=True) with the constructor defaults")
        return self._fused_forward(torch.ops.nvsr.pe_nerf, rays, z, arithmetic=arithmetic)

    def _fused_forward(self, op, *inputs, arithmetic=None):
        """op(*inputs, natural, want_record, arithmetic) -> raw, recording for the backward when a parameter wants a gradient"""
        grad = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        nat = self.natural_blob(differentiable=grad)
        capi.require_cuda(nat)
        raw, _ = op(*inputs, nat, grad, capi.arith_code(self.arithmetic if arithmetic is None else arithmetic))
        return raw

    def forward(self, x):
        x = capi.f32c(x)
        assert x.shape[-1] == self.dim_xyz + self.dim_dir
        P = x.numel() // x.shape[-1]
        blob = self.natural_blob()
        capi.require_cuda(blob)
        out = torch.empty((P, 4), dtype=torch.float32, device=x.device)
        capi.call("nvsr_flexible_nerf_forward", P, capi.ptr(x), self.dim_xyz, self.dim_dir, self.hidden_size, self.num_layers,
                  self.skip_connect_every, capi.ptr(blob), capi.ptr(out), capi.stream())
        return out.reshape(list(x.shape[:-1]) + [4])
