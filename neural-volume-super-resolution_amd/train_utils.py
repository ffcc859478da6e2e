"""Render orchestration -- mirror of the reference's train_utils.py (a3, a4, a5).

Same call surface as the reference (`run_one_iter_of_nerf` returns the 9-tuple, `eval_nerf` the 9-tuple of images); the
ray-chunk and point-chunk Python loops of the reference collapse into one `nvsr_render_rays` call per ray block: coarse
depths -> fused coarse pass -> inverse-CDF resampling + sort -> fused fine pass, all on the current stream."""
import ctypes as C
import os
from typing import Callable, NamedTuple, Optional, Sequence

import torch

from . import capi
from . import models
from . import ops


def identity_encoding(x):
    return x


def _cfg(node, name, default=None):
    """attribute- or key-style access (CfgNode, SimpleNamespace, dict)"""
    if isinstance(node, dict):
        return node.get(name, default)
    return getattr(node, name, default)


MAX_RAYS_PER_LAUNCH = 1 << 22   # bounds the [N, 3*Nc+Nf] depth/weight workspace (5.4 GB at 64+128 samples)
MAX_RAYS_PER_LAUNCH_GENERIC = 1 << 17   # generic geometries materialise [N*S,6] points and [N*S,4] outputs per pass (0.25 GB at 192 samples)


def run_network(network_fn, pts, ray_batch, chunksize, embed_fn, embeddirs_fn, scene_id=None, **kw):
    """train_utils.py:15-64 for the planes model: points [..., 3] + the batch's view directions -> radiance field [..., 4].
    (chunksize is accepted for signature parity; the decode kernel walks the whole point list in one launch.)"""
    pts_shape = list(pts.shape)
    flat = embed_fn(pts.reshape((-1, pts_shape[-1])))
    if embeddirs_fn is not None:
        viewdirs = ray_batch[..., None, -3:]
        flat = torch.cat((flat, embeddirs_fn(viewdirs.expand(pts_shape).reshape((-1, 3)))), dim=-1)
    out = network_fn(flat)
    return out.reshape(pts_shape[:-1] + [out.shape[-1]])


def _draw_point_jitter(model, n_rays, S, chunksize):
    """The point_coords_noise draws of one pass over a ray chunk, in the reference's order: run_network cuts the chunk's n_rays * S points
    into network batches of `chunksize` points (train_utils.py:47-58) and every model call draws torch.normal of its batch's shape from the
    CPU generator (models.py:291-293).  -> [n_rays, S, 3] or None when the model does not jitter right now."""
    std = model.jitter_std()
    if not std:
        return None
    n = n_rays * S
    step = max(1, n if chunksize is None else int(chunksize))
    parts = [torch.normal(mean=0, std=std, size=[min(step, n - i), 3]) for i in range(0, n, step)]
    return torch.cat(parts, 0).reshape(n_rays, S, 3) if parts else torch.empty(0, S, 3)


def _reference_chunks(n_rays, options, mode, model_coarse, model_fine):
    """Ray-chunk partition of the reference (train_utils.py:228-235); only used to draw random numbers in its order."""
    chunk = _cfg(_cfg(options.nerf, mode), "chunksize")
    chunk = int(chunk / (model_coarse.num_density_planes / 3))
    if hasattr(model_fine, "SR_model"):
        chunk //= 10
    return [(i, min(i + chunk, n_rays)) for i in range(0, n_rays, chunk)]


from .ops import RECORD_RAYS, RECORD_FORWARD_MAX_POINTS  # noqa: E402,F401  (tests and tools tune them through this module)


def _record_limits():
    """(RECORD_RAYS, RECORD_FORWARD_MAX_POINTS) as currently set on THIS module (tests lower them to force the recomputing path)"""
    import sys
    me = sys.modules[__name__]
    ops.RECORD_RAYS = me.RECORD_RAYS
    return me.RECORD_RAYS, me.RECORD_FORWARD_MAX_POINTS


def _NV():
    """the operator namespace _RenderRaysFn calls: the operators' bodies (ops.direct: no dispatcher round trip inside the Function);
    NVSR_OPS_DISPATCH=1 routes the calls through torch.ops.nvsr instead (host-time A/B)"""
    return torch.ops.nvsr if os.environ.get("NVSR_OPS_DISPATCH") == "1" else ops.direct


class _Pass(NamedTuple):
    """One pass (coarse or fine) of a training render, built once in predict_and_render_radiance: data only.  The host facts come first
    (_pass_facts: known, and checked by _refuse_untrainable, before anything is launched); the tensors follow."""
    S: int                          # samples per ray
    arith: int                      # the arithmetic of its forward, handed to every backward operator
    noise: Optional[torch.Tensor]
    dec_grad: bool                  # its decoder takes a gradient
    records: bool                   # ... and its forward records the layer inputs (9.2 KB per point): N * S <= RECORD_FORWARD_MAX_POINTS.
    #                                 A pass with dec_grad that does not record publishes no gates: its backward recomputes the forward.
    planes: Sequence = ()           # channel-last, detached
    packed: Optional[torch.Tensor] = None
    packed_bwd: Optional[torch.Tensor] = None
    leaves: Sequence = ()           # the plane leaves its gradient planes go back to, and the planes' shapes
    shapes: Sequence = ()


def _pass_facts(N, S, arith, noise, dec_grad, fwd_max):
    """the host facts of a pass; the ONE place that asks whether a pass of N x S points fits a forward record"""
    return _Pass(S, arith, noise, dec_grad, dec_grad and N * S <= fwd_max)


def _refuse_untrainable(models, N, passes, rays_grad, det, fwd_max):
    """what a training render does not cover, refused before anything is launched: the 'f16' arithmetic; rays that need a gradient, or the
    deterministic mode, with a pass whose backward would recompute the forward (it leaves no rows behind, and adds with float atomics); the
    deterministic mode in 'f32'"""
    capi.refuse_f16_training(*models)
    recomputing = [p.S for p in passes if p.dec_grad and not p.records]
    if rays_grad and recomputing:
        raise NotImplementedError("rays that require a gradient need the recorded forward: a pass of %d rays x %d samples with decoder gradients "
                                  "exceeds RECORD_FORWARD_MAX_POINTS = %d; at most %d rays per call fit"
                                  % (N, recomputing[-1], fwd_max, fwd_max // recomputing[-1]))
    if det and capi.ARITHMETIC["f32"] in [p.arith for p in passes]:
        capi.refuse_deterministic("a training step in the 'f32' arithmetic")
    if det and recomputing:
        capi.refuse_deterministic("a pass of more than RECORD_FORWARD_MAX_POINTS points with decoder gradients (its backward recomputes the "
                                  "forward: decode_rays_backward_recompute)")


class _RenderRaysFn(torch.autograd.Function):
    """Differentiable predict_and_render_radiance, written against torch.ops.nvsr.*.  Inputs: cfg (what the passes share), passes ([coarse] or
    [coarse, fine], _Pass), then the leaves: the four planes the last pass samples, the decoder parameters of the coarse / fine model as flat
    blobs in state-dict order (`TwoDimPlanesModel.natural_blob(differentiable=True)`; torch's own cat/reshape backward hands the slices to the
    parameters), the four planes of the coarse pass where they are other tensors (passes[0].leaves is not passes[-1].leaves: the reference's
    default SR training, train_nerf.py:554-561 with apply_2_coarse False -- only the fine model super-resolves, the coarse model samples the LR
    planes) and, with cfg["rays_grad"], the packed rays (camera-pose refinement; the kernels read cfg["rays"], the same values
    detached).

    forward  = coarse_z, then per pass: [importance_resample (no gradient, train_utils.py:153) ->] decode_rays -> composite_rays;
    backward = per pass: composite_backward (wave per ray) -> the gate-driven backward on the step's route (ops.gate_backward_: atomic,
               ordered in deterministic mode, ordered with points when the rays need their gradient -> rays_grad, coarse first, fine
               accumulating) [-> decoder_weight_grad on the forward's record]; a pass that published no gates recomputes its forward
               (decode_rays_backward_recompute).  All passes over one set of plane leaves add into ONE set of zero-filled gradient planes."""

    @staticmethod
    def forward(ctx, cfg, passes, p0, p1, p2, pv, nat_c, nat_f, *more_leaves):
        rays, white = cfg["rays"], bool(cfg["white"])
        nv = _NV()
        # an output the loss does not use hands None to backward() instead of a zero tensor: the disparity / opacity chain rules are
        # skipped for them (a dozen per-ray kernels per pass otherwise)
        ctx.set_materialize_grads(False)
        # training batches are a few thousand rays: the sample-parallel decoder + the wave-per-ray compositor fill the chip, the fused
        # per-ray kernel would run 32 workgroups; raw is needed by the backward anyway.  The forward publishes its ReLU gates (128 B per
        # point) so that the backward does not recompute it; when decoder gradients are wanted it also records every layer's input
        # (9.2 KB per point) unless the pass is too large for that (_Pass.records)
        z = nv.coarse_z(rays, passes[0].S, bool(cfg["lindisp"]), cfg["t_rand"])
        outs, saved, guarded = [], {}, [rays]
        for k, p in zip("cf", passes):
            if k == "f":
                z = nv.importance_resample(z, w, p.S - passes[0].S, cfg["u"])
            raw, gates, rec = nv.decode_rays(p.planes, cfg["consts"], p.packed, rays, z, p.records or not p.dec_grad, p.records, p.arith)
            rgb, disp, acc, w = nv.composite_rays(raw, z, rays, p.noise, white, k == "c")
            outs += [rgb, disp, acc]
            # disp_map is differentiable like the reference's (volume_rendering_utils.py:46): its gradient is folded into those of depth / acc
            # (detached views: the outputs themselves would close a reference cycle ctx -> saved -> output -> grad_fn -> ctx, and every step's
            #  7 GB of forward record would wait for the cyclic garbage collector)
            saved.update({"z_" + k: z, "raw_" + k: raw, "gates_" + k: gates if gates.numel() else None, "rec_" + k: rec if rec.numel() else None,
                          "disp_" + k: disp.detach(), "acc_" + k: acc.detach()})
            guarded += [*p.planes, p.packed]
        ctx.cfg, ctx.passes, ctx.saved = cfg, passes, saved          # (ctx.saved is also what the parity tests read the fine depths from)
        # autograd's version check: everything the backward reads -- the forward's intermediates and the channel-last planes (views of the
        # plane parameters, sharing their version counters) -- also goes through save_for_backward, so an in-place update of a plane or of a
        # saved tensor between forward and backward raises instead of producing the gradient of another function
        ctx.save_for_backward(*[t for t in guarded + list(saved.values()) if isinstance(t, torch.Tensor)])
        if not cfg["coarse_grad"] and len(passes) > 1:
            ctx.mark_non_differentiable(*outs[:3])     # the coarse pass ran under the model's optional_no_grad (train_nerf.py:560)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        ctx.saved_tensors          # (raises if a tensor saved by the forward was modified in place since)
        cfg, passes, sv = ctx.cfg, ctx.passes, ctx.saved
        N, rays, consts, white = cfg["N"], cfg["rays"], cfg["consts"], bool(cfg["white"])
        nv = _NV()
        dev = rays.device
        need = ctx.needs_input_grad          # of: cfg, passes, p0..pv (2..5), nat_c, nat_f (6, 7), the coarse pass's own planes (8..11), the rays (last)
        top = passes[-1]
        # per set of plane leaves: which planes need a gradient, and their gradient planes (channel-last; every pass over the set ADDS into them)
        sets = {id(top.leaves): ([bool(n) for n in need[2:6]], [None] * 4)}
        sets.setdefault(id(passes[0].leaves), ([bool(n) for n in need[8:12]], [None] * 4))
        need_rays = bool(cfg["rays_grad"]) and bool(need[-1])
        # rays that need their gradient: ONE rows launch per pass feeds the ordered scatter into the planes, the record and
        # triplane_points_grad, then rays_grad reduces the points' gradient per ray -- coarse writes d_rays, fine adds, on one stream
        route = ops.gate_route(cfg["det"], need_rays)
        d_rays = []                                              # [d_rays] once a pass has written it

        def zero_planes(p):
            """the gradient planes of pass p's leaves, zero-filled in one allocation by the first pass that scatters into them"""
            need_planes, gplanes = sets[id(p.leaves)]
            if any(need_planes) and all(gplanes[d] is None for d in range(4) if need_planes[d]):
                gplanes[:] = [g if need_planes[d] else None for d, g in enumerate(ops.zero_planes_like(p.planes, need_planes, rays))]

        def backward_pass(k, p, g_rgb, g_disp, g_acc):
            """-> decoder gradient of pass p (state-dict order) or None; plane gradients are added into its leaves' gradient planes"""
            need_planes, gplanes = sets[id(p.leaves)]
            if (g_rgb is None and g_acc is None and g_disp is None) or (not any(need_planes) and not p.dec_grad and not need_rays):
                return None
            z, raw = sv["z_" + k], sv["raw_" + k]
            g_rgb = torch.zeros((N, 3), dtype=torch.float32, device=dev) if g_rgb is None else capi.f32c(g_rgb)
            g_acc = None if g_acc is None else capi.f32c(g_acc)
            g_depth = None
            if g_disp is not None:
                q = 1.0 / sv["disp_" + k]           # disp = 1 / max(1e-10, q): q itself wherever the gradient is not zero (NaN stays NaN)
                g_acc, g_depth = ops.fold_disp_grad(g_disp, q, sv["acc_" + k], q * sv["acc_" + k], g_acc, None)
            g_raw = nv.composite_backward_rays(raw, z, rays, p.noise, white, False, g_rgb, g_acc, g_depth)     # (directions read from the packed rays)
            if p.dec_grad and not p.records:
                # no gates published (pass too large for a forward record): recompute the forward in the backward, RECORD_RAYS rays at a time
                _record_limits()
                out = nv.decode_rays_backward_recompute(p.planes, consts, p.packed, p.packed_bwd, rays, z, g_raw, need_planes, True, p.arith)
                for d in range(4):
                    if need_planes[d]:
                        gplanes[d] = out[d] if gplanes[d] is None else gplanes[d].add_(out[d])
                return out[4]
            # gate-driven backward (no recomputation); with the forward's record it adds the gradient half, then ONE contraction
            zero_planes(p)
            rec = sv["rec_" + k]
            inputs = ops.gate_backward_(nv, route, p.planes, consts, p.packed, p.packed_bwd, rays, z, g_raw, sv["gates_" + k], rec, need_planes, p.arith,
                                        [g if g is not None else rays.new_empty((0,)) for g in gplanes])
            if inputs is not None:
                first = not d_rays                               # the first pass writes d_rays, a later one adds onto it
                if first:
                    d_rays.append(torch.empty((N, 11), dtype=torch.float32, device=dev))
                nv.rays_grad(rays, z, inputs[0], inputs[1], raw, p.noise, g_raw, d_rays[0], not first)
            if not p.dec_grad:
                return None
            return nv.decoder_weight_grad(rec, N, p.S, p.arith) if route == ops.ATOMIC else nv.decoder_weight_grad_det(rec, N, p.S, p.arith, None)

        # The two passes' backward kernels are independent (both ADD into the gradient planes with float atomics): the coarse pass runs on a
        # second stream, so that its workgroups fill the fine pass's partly empty rounds (same-box A/B of the planes-only iteration: eager
        # 1.683 -> 1.631 ms, replayed from a graph 1.728 -> 1.709 ms; NVSR_BWD_STREAMS=0 keeps one stream).  Planes-only passes: nothing
        # allocated on the second stream outlives the join.  Deterministic mode: ONE stream, coarse then fine -- the fine pass adds onto the
        # coarse pass's sums, and that order is part of the result's bits.
        two = (route == ops.ATOMIC and os.environ.get("NVSR_BWD_STREAMS", "1") == "1" and len(sets) == 1 and cfg["coarse_grad"] and len(passes) > 1
               and dev.type == "cuda" and any(sets[id(top.leaves)][0]) and not need[6] and not need[7]
               and all(a.shape == b.shape and a.stride() == b.stride() for a, b in zip(passes[0].planes, top.planes)))
        gdec = [None, None]
        if two:
            zero_planes(top)                                     # zero-filled before the fork
            cur, side = torch.cuda.current_stream(dev), _side_stream(dev)
            side.wait_stream(cur)
            with torch.cuda.stream(side):
                gdec[0] = backward_pass("c", passes[0], *grads[0:3])
            gdec[1] = backward_pass("f", top, *grads[3:6])
            cur.wait_stream(side)
        else:
            for i, p in enumerate(passes):
                if i or cfg["coarse_grad"]:
                    gdec[i] = backward_pass("cf"[i], p, *grads[3 * i: 3 * i + 3])

        def to_leaves(p):
            """the gradient planes of p's leaves back in the reference's [1,C,H,W]"""
            out = []
            for d, (wanted, g) in enumerate(zip(*sets[id(p.leaves)])):
                if wanted and g is None:
                    g = torch.zeros(p.shapes[d], dtype=torch.float32, device=dev)
                out.append(None if g is None else models.from_channel_last(g, like=p.leaves[d]))
            return out

        for i in range(len(passes)):
            if need[6 + i] and gdec[i] is None:
                gdec[i] = torch.zeros(capi.DECODER_NATURAL_FLOATS, dtype=torch.float32, device=dev)
        out = [None, None] + to_leaves(top) + gdec + (to_leaves(passes[0]) if len(sets) > 1 else [])
        if cfg["rays_grad"]:
            out.append(None if not need_rays else d_rays[0] if d_rays else torch.zeros((N, 11), dtype=torch.float32, device=dev))
        return tuple(out)


_SIDE_STREAMS = {}


def _side_stream(dev):
    k = (dev.type, dev.index)
    if k not in _SIDE_STREAMS:
        _SIDE_STREAMS[k] = torch.cuda.Stream(device=dev)
    return _SIDE_STREAMS[k]


def _planes_need_grad(model):
    """does a plane of the current scene train?  (asked of the stored tensor: of a low-rank plane's factors, models.gen_plane)"""
    if not torch.is_grad_enabled() or getattr(model, "planes_", None) is None:
        return False
    names = [models.get_plane_name(model.cur_id, d) for d in range(model.num_density_planes + 1)]
    return any(n in model.planes_ and model.planes_[n].requires_grad for n in names)


def _decoder_needs_grad(model):
    return torch.is_grad_enabled() and any(p.requires_grad for p in model.decoder_parameters())


def _warn_no_rays_grad(model, why):
    """once per model: rays that require a gradient met a route that returns none for them (the precedent of models._warn_no_points_grad)"""
    if not model.__dict__.get("_rays_grad_warned"):
        import warnings
        warnings.warn("the rays require a gradient, but a render with %s returns none for them (their .grad stays None); a training render of "
                      "the shipped tri-plane geometry in 'f16x2' / 'bf16x3' does" % why)
        model.__dict__["_rays_grad_warned"] = True


def predict_and_render_radiance(ray_batch, model_coarse, model_fine, options, scene_id, mode="train", encode_position_fn=None,
                                encode_direction_fn=None, randoms=None, force_arith=None):
    """train_utils.py:71-182 on packed rays [N,11].  `randoms` (extension) = dict(t_rand, u, noise_coarse, noise_fine) of
    explicit random inputs; when absent they are drawn on the CPU generator in the reference's order."""
    if _cfg(options.nerf, "encode_position_fn", None) == "mip":
        raise NotImplementedError("Mip-NeRF baseline is outside the tri-plane hot path (SURVEY.md 2)")
    m = _cfg(options.nerf, mode)
    Nc, Nf = int(m.num_coarse), int(m.num_fine)
    rays_leaf = capi.f32c(ray_batch)
    # rays that require a gradient: the training path of the shipped geometry in a limb arithmetic returns one; every other
    # route warns once per model and leaves it None.  The kernels always read the detached values.
    rays_ask = torch.is_grad_enabled() and rays_leaf.requires_grad
    rays = rays_leaf.detach()
    N = rays.shape[0]
    dev = rays.device
    std = float(m.radiance_field_noise_std)
    r = dict(randoms or {})
    if randoms is None:
        # same draws, same order as the reference: t_rand (train_utils.py:108), coarse noise (volume_rendering_utils.py:32),
        # u (nerf_helpers.py:683; only when perturb != 0), fine noise
        for mdl in (model_coarse, model_fine):
            mdl.set_cur_scene_id(scene_id)
        if m.perturb:
            r["t_rand"] = torch.rand([N, Nc])
        r["jitter_coarse"] = _draw_point_jitter(model_coarse, N, Nc, m.chunksize)
        if std > 0.0:
            r["noise_coarse"] = torch.randn([N, Nc]) * std
        if Nf > 0:
            if m.perturb != 0.0:
                r["u"] = torch.rand([N, Nf])
            r["jitter_fine"] = _draw_point_jitter(model_fine, N, Nc + Nf, m.chunksize)
            if std > 0.0:
                r["noise_fine"] = torch.randn([N, Nc + Nf]) * std
    t_rand, u, n_c, n_f = (None if r.get(k) is None else capi.f32c(r[k].to(dev)) for k in ("t_rand", "u", "noise_coarse", "noise_fine"))
    jit_c, jit_f = (None if r.get(k) is None else capi.f32c(r[k].to(dev)).reshape(-1, 3) for k in ("jitter_coarse", "jitter_fine"))
    if not m.perturb:
        t_rand = None

    for mdl in (model_coarse, model_fine):
        mdl.set_cur_scene_id(scene_id)
    if not (model_coarse.is_native_geometry() and (Nf <= 0 or model_fine.is_native_geometry())):
        if mode == "train" and torch.is_grad_enabled() and capi.deterministic() and any(
                _planes_need_grad(mdl) or _decoder_needs_grad(mdl) for mdl in (model_coarse, model_fine)):
            capi.refuse_deterministic("training a generic decoder geometry (generic.hip)")
        if rays_ask:
            _warn_no_rays_grad(model_fine if Nf > 0 else model_coarse, "a generic decoder geometry")
        return _render_generic(rays, model_coarse, model_fine, m, Nc, Nf, t_rand, u, n_c, n_f, jit_c, jit_f)
    top = model_fine if Nf > 0 else model_coarse
    dec_c_grad = _decoder_needs_grad(model_coarse)
    dec_f_grad = Nf > 0 and _decoder_needs_grad(model_fine)
    sr_on = hasattr(top, "SR_model") and not top.skip_SR_
    sr_grad = sr_on and torch.is_grad_enabled() and top.SR_model.training and \
        top.SR_model.inner_model.wants_grad(*top.SR_model.LR_planes.values())
    train_path = mode == "train" and N > 0 and (_planes_need_grad(top) or dec_c_grad or dec_f_grad or sr_grad)
    # (an evaluation render whose operands leave the f16 limbs' range is found by the library's range flag and rendered again with
    #  force_arith = bf16x3: run_one_iter_of_nerf; a training step raises: training.TrainStep)
    # ('f16', one f16 limb: evaluation renders only -- the fused passes of the two-decoder frame; no occupancy grid, no shared decoder)
    arith_c = capi.resolve_render_arithmetic(model_coarse.arithmetic if force_arith is None else force_arith)
    arith_f = capi.resolve_render_arithmetic(model_fine.arithmetic if force_arith is None else force_arith) if Nf > 0 else arith_c
    rays_grad = False
    if rays_ask:
        if mode != "train":
            _warn_no_rays_grad(top, "evaluation mode")
        elif capi.ARITHMETIC["f32"] in (arith_c, arith_f):
            _warn_no_rays_grad(top, "the 'f32' arithmetic")
        elif N > 0:
            rays_grad = train_path = True
    det = train_path and capi.deterministic()
    if mode == "train":
        # the host facts of the passes, and what a training render does not cover -- before anything is launched
        coarse_grad = not isinstance(model_coarse.optional_no_grad(), torch.no_grad) if hasattr(model_coarse, "optional_no_grad") else True
        _, fwd_max = _record_limits()
        passes = [_pass_facts(N, Nc, arith_c, n_c, dec_c_grad and coarse_grad, fwd_max)]
        if Nf > 0:
            passes.append(_pass_facts(N, Nc + Nf, arith_f, n_f, dec_f_grad, fwd_max))
        _refuse_untrainable((model_coarse, model_fine), N, passes, rays_grad, det, fwd_max)
    packed_c = model_coarse.packed_decoder()
    packed_f = model_fine.packed_decoder() if Nf > 0 else None
    if not (train_path and sr_on):       # (the SR training path builds its scene from the ROI planes below)
        planes_c, consts = model_coarse.scene_args()
        if Nf > 0:
            # both passes sample the same planes in the reference unless only the fine model super-resolves
            planes_f, consts_f = model_fine.scene_args()
            same = all(a.data_ptr() == b.data_ptr() for a, b in zip(planes_c, planes_f))
        else:
            planes_f, same = planes_c, True
    white, lindisp = bool(m.white_background), bool(m.lindisp)

    if train_path:
        # training path (mode == "train" only; evaluation never builds a graph): gradients flow to whatever requires grad among the
        # planes of the current scene, the decoder parameters of the two models and -- through the super-resolved planes -- the SR
        # network and its LR planes
        leaves_c = []
        if sr_on:
            leaves = top.training_planes(rays)
            planes_f, consts = top.scene_args(planes=[models.to_channel_last(p.detach()) for p in leaves])
            planes_c = planes_f
            if Nf > 0 and not (hasattr(model_coarse, "SR_model") and not model_coarse.skip_SR_):
                # the reference's default (train_nerf.py:554-561, super_resolution.apply_2_coarse False): only the fine model super-resolves; the
                # coarse pass samples the LR planes -- plane leaves of its own
                leaves_c = model_coarse.training_planes(rays)
                planes_c, _ = model_coarse.scene_args(planes=[models.to_channel_last(p.detach()) for p in leaves_c])
        else:
            names = [models.get_plane_name(scene_id, d) for d in range(4)]
            leaves = [top.raw_plane(n) for n in names]          # (a low-rank plane: generated once, shared by both passes; models.gen_plane)
        plane_leaves = leaves[:4]
        leaves += [model_coarse.natural_blob(differentiable=True) if dec_c_grad else None,
                   model_fine.natural_blob(differentiable=True) if dec_f_grad else None]
        leaves += leaves_c
        # 'f16x2': the library runs the forward of a pass whose decoder is not trained (no weight-gradient record) and every gate-driven
        # backward on 2 f16 limbs, the recording forward and the weight-gradient contraction on 3 bf16 limbs (include/nvsr.h); the gates a
        # forward publishes are signs, valid for either backward
        passes[0] = passes[0]._replace(planes=planes_c, packed=packed_c, packed_bwd=model_coarse.packed_decoder_bwd(),
                                       leaves=leaves_c or plane_leaves, shapes=[tuple(k.shape) for k in planes_c])
        if Nf > 0:
            passes[1] = passes[1]._replace(planes=planes_f, packed=packed_f, packed_bwd=model_fine.packed_decoder_bwd(),
                                           leaves=plane_leaves, shapes=[tuple(k.shape) for k in planes_f])
        cfg = dict(N=N, rays=rays, consts=consts, lindisp=lindisp, white=white, t_rand=t_rand, u=u, det=det, rays_grad=rays_grad, coarse_grad=coarse_grad)
        if rays_grad:
            leaves = leaves + [rays_leaf]
        outs = _RenderRaysFn.apply(cfg, passes, *leaves)
        if Nf > 0:
            return outs[0], outs[1], outs[2], outs[3], outs[4], outs[5], None, None, None
        return outs[0], outs[1], outs[2], None, None, None, None, None, None

    nv = torch.ops.nvsr
    if N == 0:
        e = lambda *sh: torch.empty(sh, dtype=torch.float32, device=dev)
        return (e(0, 3), e(0), e(0)) + ((e(0, 3), e(0), e(0)) if Nf > 0 else (None, None, None)) + (None, None, None)
    # occupancy grids (models.build_occupancy): evaluation without noise only, each model its own grid; (grid, resolution) or None.  The frame
    # of one shared decoder has no occupancy route and keeps the plain one.
    occ_c = occ_f = None
    limb = (capi.ARITHMETIC["f16x2"], capi.ARITHMETIC["bf16x3"])
    if mode != "train" and std == 0.0 and n_c is None and n_f is None and not (Nf > 0 and packed_f.data_ptr() == packed_c.data_ptr()):
        occ_c = model_coarse.occupancy_entry(scene_id) if arith_c in limb else None
        occ_f = model_fine.occupancy_entry(scene_id) if Nf > 0 and arith_f in limb else None
    if same and arith_c == arith_f:
        if occ_c is not None or occ_f is not None:
            (g_c, G_c), (g_f, G_f) = occ_c or (None, 1), occ_f or (None, 1)
            rgb_c, disp_c, acc_c, rgb_f, disp_f, acc_f = nv.render_rays_occupancy(planes_c, consts, packed_c, packed_f, rays, Nc, Nf, lindisp, white, t_rand,
                                                                                 u, g_c, G_c, g_f, G_f, arith_c)
        else:
            rgb_c, disp_c, acc_c, rgb_f, disp_f, acc_f = nv.render_rays(planes_c, consts, packed_c, packed_f, rays, Nc, Nf, lindisp, white, t_rand, u,
                                                                       n_c, n_f, arith_c)
        if Nf <= 0:
            rgb_f = disp_f = acc_f = None
    else:
        # the two passes sample different planes (only the fine model super-resolves) or run in different arithmetic: pass by pass
        fused = N >= capi.fused_min_rays()     # below it the sample-parallel decoder + the wave-per-ray compositor fill the chip

        def one_pass(planes, packed, z, noise, want_w, arith, occ=None):
            if fused and occ is not None:
                return nv.render_pass_occupancy(planes, consts, packed, rays, z, z.shape[1], lindisp, white, want_w, occ[0], occ[1], arith)
            if fused:
                return nv.render_pass(planes, consts, packed, rays, z, noise, white, want_w, arith)
            if arith == capi.RENDER_ARITHMETIC["f16"]:      # (the decode kernels have no one-limb mode: an un-fused pass runs in 'f16x2')
                arith = capi.ARITHMETIC["f16x2"]
            raw, _, _ = nv.decode_rays(planes, consts, packed, rays, z, False, False, arith)
            return nv.composite_rays(raw, z, rays, noise, white, want_w)

        z_c = nv.coarse_z(rays, Nc, lindisp, t_rand)
        rgb_c, disp_c, acc_c, w_c = one_pass(planes_c, packed_c, z_c, n_c, Nf > 0, arith_c, occ_c)
        rgb_f = disp_f = acc_f = None
        if Nf > 0:
            z_f = nv.importance_resample(z_c, w_c, Nf, u)
            rgb_f, disp_f, acc_f, _ = one_pass(planes_f, packed_f, z_f, n_f, False, arith_f, occ_f)
    return rgb_c, disp_c, acc_c, rgb_f, disp_f, acc_f, None, None, None


def _generic_occupancy(model, noise, jit):
    """(grid, resolution) if a pass of `model` through _render_generic takes the occupancy route now, else None: a generic geometry, no
    gradients, no density noise and no jitter of the sample positions, generic_route() == 'fused', NVSR_GENERIC_TWO_PHASE not 0, and a grid of
    the current scene that is not stale (model.occupancy_entry).  A model for which nobody built a grid is asked nothing else."""
    if torch.is_grad_enabled() or noise is not None or jit is not None or not model.__dict__.get("_occupancy"):
        return None
    if not model.generic_phases_allowed():
        return None
    return model.occupancy_entry(model.cur_id)


def _render_generic(rays, model_coarse, model_fine, m, Nc, Nf, t_rand, u, n_c, n_f, jit_c=None, jit_f=None):
    """predict_and_render_radiance for decoder geometries other than the shipped one, pass by pass like the reference (train_utils.py:95-180):
    depths -> run_network (the model's generic kernels on the [N*S,6] point list) -> compositing -> importance resampling -> again.
    With gradients enabled the model call and the compositing are the differentiable operators (the importance samples are detached,
    train_utils.py:153)."""
    nv = torch.ops.nvsr
    N = rays.shape[0]
    white, lindisp = bool(m.white_background), bool(m.lindisp)
    if N == 0:
        e = lambda *sh: torch.empty(sh, dtype=torch.float32, device=rays.device)
        return (e(0, 3), e(0), e(0)) + ((e(0, 3), e(0), e(0)) if Nf > 0 else (None, None, None)) + (None, None, None)
    def composite(raw, z, noise, want_weights):
        if raw.requires_grad:
            rgb, disp, acc, w, _ = nv.composite(raw, z, rays[:, 3:6].contiguous(), noise, white, False)
            return rgb, disp, acc, w.detach()
        return nv.composite_rays(raw, z, rays, noise, white, want_weights)

    def decode(model, z, noise, jit):
        """raw [N,S,4] of a pass.  Without gradients, a model whose generic_frame_route() is 'two_phase' runs its colour decoder on the samples
        of nonzero weight only: density phase, the compositor's weights on [+0, +0, +0, sigma] (the same `noise` as the final call), their
        live list, colour phase -- all enqueued, no host round trip.  A sample it leaves out keeps colour logits +0 under a weight of 0:
        the one-phase frame's bits (include/nvsr.h has the contract and its one exception, NaN logits under a zero weight)."""
        pts = nv.ray_points(rays, z)
        occ = _generic_occupancy(model, noise, jit)
        if occ is not None:
            # the model's occupancy grid (models.build_occupancy: the user opted in, whatever generic_frame_route() says): the density decoder on the
            # kept samples only, a culled one being [+0, +0, +0, capi.CULLED_SIGMA] -- weight +0.0, absent from the live list; then as below
            raw, _, _ = model.density_field_kept(pts, occ[0], occ[1])
            w = nv.composite_rays(raw.reshape(N, z.shape[1], 4), z, rays, None, white, True)[3]
            index, count = nv.generic_live_list(w)
            return model.colour_field_(raw, pts, index, count).reshape(N, z.shape[1], 4)
        if torch.is_grad_enabled() or not hasattr(model, "generic_frame_route") or model.generic_frame_route() != "two_phase":
            return model(pts, coord_noise=jit).reshape(N, z.shape[1], 4)
        raw = model.density_field(pts, coord_noise=jit)
        w = nv.composite_rays(raw.reshape(N, z.shape[1], 4), z, rays, noise, white, True)[3]
        index, count = nv.generic_live_list(w)
        return model.colour_field_(raw, pts, index, count, coord_noise=jit).reshape(N, z.shape[1], 4)

    z_c = nv.coarse_z(rays, Nc, lindisp, t_rand)
    raw = decode(model_coarse, z_c, n_c, jit_c)
    rgb_c, disp_c, acc_c, w_c = composite(raw, z_c, n_c, Nf > 0)
    rgb_f = disp_f = acc_f = None
    if Nf > 0:
        z_f = nv.importance_resample(z_c, w_c, Nf, u)
        raw_f = decode(model_fine, z_f, n_f, jit_f)
        rgb_f, disp_f, acc_f, _ = composite(raw_f, z_f, n_f, False)
    return rgb_c, disp_c, acc_c, rgb_f, disp_f, acc_f, None, None, None


def _sr_of(model):
    return model.SR_model if hasattr(model, "SR_model") and not model.skip_SR_ else None


# the arithmetics of the SR convolutions that have f16's ranges and raise bit 2 of the range flag
_SR_RANGED = (capi.CONV_ARITHMETIC["f16x2"], capi.CONV_ARITHMETIC["f16"])


def _f16_in_play(*ms):
    """does an evaluation of these models launch anything in NVSR_ARITH_F16X2 -- or in the one-limb 'f16' (render passes, SR network), which has the same ranges?"""
    f16 = (capi.RENDER_ARITHMETIC["f16x2"], capi.RENDER_ARITHMETIC["f16"])
    for m in ms:
        if capi.resolve_render_arithmetic(m.arithmetic) in f16:
            return True
        sr = _sr_of(m)
        if sr is not None and capi.resolve_conv_arithmetic(sr.inner_model.arithmetic) in _SR_RANGED:
            return True
    return False


def _range_key(*ms):
    """(storage, version) of everything an evaluation reads: decoder parameters, planes, SR weights"""
    key = []
    for m in ms:
        ts = list(m.decoder_parameters()) + list((getattr(m, "planes_", None) or {}).values())
        sr = _sr_of(m)
        if sr is not None:
            ts += list(sr.inner_model.parameters())
        key += [(t.data_ptr(), t._version) for t in ts]
    return tuple(key)


def _generic_limb_frame(launch_all, limb_models, model_coarse, model_fine, device):
    """an evaluation frame of generic geometries of which `limb_models` evaluate in 'f16x2' (csrc/generic_fused_limb.hip), range-checked like
    a native frame (run_one_iter_of_nerf): operands beyond the limbs' range -- found beforehand (f16_operands_in_range) or by the range flag
    after the frame -- send this frame and the later ones of the same parameter versions through the exact-f32 generic route, warned once.
    model.arithmetic stays as it is."""
    key = _range_key(model_coarse, model_fine)

    def f32_frame():
        for mdl in limb_models:
            mdl.__dict__["_generic_limb_off"] = True
        try:
            return launch_all()
        finally:
            for mdl in limb_models:
                mdl.__dict__.pop("_generic_limb_off", None)

    if model_fine.__dict__.get("_f16_unfit") == key:
        return f32_frame()
    fit = all(mdl.f16_operands_in_range(mdl.scene_args(check_native=False)[0]) for mdl in limb_models)
    if fit:
        flag = capi.range_flag(device)
        flag.reset()
        out = launch_all()
        if not capi.RangeFlag.raised(flag.read_async()):
            return out
        flag.reset()
    if not model_fine.__dict__.get("_f16_unfit_warned"):
        import warnings
        warnings.warn("weights, plane values or activations beyond NVSR_ARITH_F16X2's range (|W| < 255, |feature / activation| < 4094): this generic "
                      "decoder geometry renders in 'f32' while its parameters stay as they are (set model.arithmetic = None to render there in the "
                      "first place)")
        model_fine.__dict__["_f16_unfit_warned"] = True
    model_fine.__dict__["_f16_unfit"] = key
    return f32_frame()


def _sr_fallback(*ms, redo=False):
    """the SR networks of these models super-resolve in 'bf16x3' for the evaluation frame being rendered.  Cached SR planes are dropped when `redo`
    says so (they come from an F16X2 or F16 pass that raised the range flag: NaN inside) or when they were NOT made in 'bf16x3' (`_planes_arith`, set by
    _sr_restore behind a fallback frame, forgotten by clear_SR_planes): planes a fallback frame has super-resolved stay cached for the next frames of
    the same parameters (the arithmetic was put back after every frame, so every later frame found 'f16x2', dropped the planes and ran the
    SR stage again, ~80 ms per scene and frame).  -> [(PlanesSR, its network's arithmetic before)]: the caller puts it back after the frame
    (_sr_restore, in a `finally`), so that a later training iteration of the same SR model runs in the arithmetic it was configured with"""
    changed, seen = [], set()
    for m in ms:
        sr = _sr_of(m)
        if sr is None or id(sr) in seen:
            continue
        seen.add(id(sr))
        if capi.resolve_conv_arithmetic(sr.inner_model.arithmetic) in _SR_RANGED:
            changed.append((sr, sr.inner_model.arithmetic))
            sr.inner_model.arithmetic = "bf16x3"
            if redo or sr.__dict__.get("_planes_arith") != "bf16x3":
                sr.clear_SR_planes()
        elif redo:
            sr.clear_SR_planes()
    return changed


def _sr_restore(changed, rendered=True):
    """puts the SR networks' arithmetic back; rendered: the frame completed, the planes now cached were made in 'bf16x3'"""
    for sr, before in changed:
        sr.inner_model.arithmetic = before
        if rendered:
            sr.__dict__["_planes_arith"] = "bf16x3"


def pack_rays(ray_origins, ray_directions, near, far, H=None, W=None, focal=None, no_ndc=True):
    """run_one_iter_of_nerf's ray packing (train_utils.py:207-226): rays [N,11] = [ro, rd, near, far, viewdir]."""
    ro, rd = capi.f32c(ray_origins).reshape(-1, 3), capi.f32c(ray_directions).reshape(-1, 3)
    N = ro.shape[0]
    view_src = rd
    if no_ndc is False:
        from .nerf_helpers import ndc_rays
        ro, rd = ndc_rays(H, W, focal, 1.0, ro, rd)
    if torch.is_grad_enabled() and (ro.requires_grad or rd.requires_grad or view_src.requires_grad):
        # origins or directions that require a gradient (camera-pose refinement): the same entry as a differentiable operator
        return torch.ops.nvsr.pack_rays(ro, rd, None if view_src is rd else view_src, float(near), float(far))
    rays = torch.empty((N, 11), dtype=torch.float32, device=ro.device)
    if N == 0:
        return rays
    capi.call("nvsr_pack_rays", N, capi.ptr(ro), capi.ptr(rd), capi.ptr(view_src), float(near), float(far), capi.ptr(rays), capi.stream())
    return rays


_PATCH_ORDER = {}
PATCH_W, PATCH_H = 16, 2                 # 32 rays = one wave tile of the fused pass
SUPER_W, SUPER_H = 8, 16                 # patches per super-block: 128 x 32 pixels, visited block by block


def __getattr__(name):
    # PATCH_ORDER_MIN_RAYS = the library's fused-path threshold (the fused passes tile by ray; below it the sample-parallel kernels do not),
    # read from the library when first used so that the two can never disagree
    if name == "PATCH_ORDER_MIN_RAYS":
        return capi.fused_min_rays()
    raise AttributeError("module %r has no attribute %r" % (__name__, name))



def patch_order(n_rays, grid_width, device):
    """(perm, inv) that reorder the rays of a row-major pixel grid [n_rays / grid_width, grid_width] into 16 x 2 pixel patches (row-major
    inside a patch), the patches visited super-block by super-block (8 x 16 patches = 128 x 32 pixels, row-major inside and between
    blocks).  A wave tile of the fused render pass is 32 consecutive rays: as a patch they are half as far apart as 32 pixels of a row,
    their samples share more texels (fewer distinct cache lines per gather instruction, more L1 / L2 hits), and the workgroups that run
    side by side stay inside one compact block; the frame renders 3-4 % faster than in row order -- the pixels are the same bits, every
    ray is independent of its neighbours (tools/ray_order_time.py: 8 x 4 and 16 x 2 patches are within 1 % of each other, the blocks add
    0.5 %).  Ragged edges are fine: any permutation is valid."""
    key = (int(n_rays), int(grid_width), str(device))
    hit = _PATCH_ORDER.get(key)
    if hit is None:
        rows = n_rays // grid_width
        ys = torch.arange(rows, device=device)[:, None]
        xs = torch.arange(grid_width, device=device)[None, :]
        bw, bh = PATCH_W * SUPER_W, PATCH_H * SUPER_H
        k = ((((ys // bh) * ((grid_width + bw - 1) // bw) + xs // bw) * SUPER_H + (ys // PATCH_H) % SUPER_H) * SUPER_W + (xs // PATCH_W) % SUPER_W) \
            * (PATCH_W * PATCH_H) + (ys % PATCH_H) * PATCH_W + xs % PATCH_W
        perm = torch.argsort(k.reshape(-1))
        inv = torch.empty_like(perm)
        inv[perm] = torch.arange(perm.numel(), device=device)
        if len(_PATCH_ORDER) > 16:
            _PATCH_ORDER.clear()
        hit = _PATCH_ORDER[key] = (perm, inv)
    return hit


def run_one_iter_of_nerf(H, W, focal, model_coarse, model_fine, batch_rays, options, scene_id, mode="train",
                         encode_position_fn=None, encode_direction_fn=None, scene_config={}, randoms=None, ray_grid_width=None):
    """train_utils.py:185-282 -> (rgb_coarse, disp_coarse, acc_coarse, rgb_fine, disp_fine, acc_fine, None, None, None)
    ray_grid_width (not in the reference): the rays are whole rows of a row-major pixel grid of this width (eval_nerf, the row-sharded
    renders) -- an evaluation pass then renders them in patch order (patch_order) and returns the results in the caller's order."""
    if isinstance(model_coarse, models.FlexibleNeRFModel):
        encode = _cfg(options.nerf, "encode_position_fn", None)
        b = _NERF_BASELINES.get(encode)
        if b is None or not all(b.fits(mdl) for mdl in (model_coarse, model_fine)):
            raise NotImplementedError("FlexibleNeRFModel runs as the Mip-NeRF baseline (nerf.encode_position_fn: mip) with include_input_xyz=False, or "
                                      "as the positional-encoding NeRF (nerf.encode_position_fn: positional_encoding) with num_encoding_fn_xyz=6, "
                                      "num_encoding_fn_dir=4, include_input_xyz=True, include_input_dir=True; both with the constructor defaults "
                                      "otherwise; got %r with dim_xyz %d / %d" % (encode, model_coarse.dim_xyz, model_fine.dim_xyz))
        return _run_nerf_baseline(b, H, W, focal, model_coarse, model_fine, batch_rays, options, scene_id, mode, scene_config, randoms)
    if not isinstance(model_coarse, models.TwoDimPlanesModel):
        raise NotImplementedError("only the tri-plane model is on the accelerated path")
    if mode == "train":
        capi.refuse_f16_training(model_coarse, model_fine)      # (before the first launch: pack_rays below)
    if not options.nerf.use_viewdirs:
        raise NotImplementedError("the decoder kernel expects use_viewdirs=True (all shipped configs)")
    rays = pack_rays(batch_rays[0], batch_rays[1], _cfg(scene_config, "near"), _cfg(scene_config, "far"), H, W, focal,
                     no_ndc=_cfg(scene_config, "no_ndc"))
    N = rays.shape[0]
    m = _cfg(options.nerf, mode)
    for mdl in (model_coarse, model_fine):
        mdl.set_cur_scene_id(scene_id)
    jitters = bool(model_coarse.jitter_std() or (int(m.num_fine) > 0 and model_fine.jitter_std()))
    if randoms is None and (m.perturb or float(m.radiance_field_noise_std) > 0.0 or jitters):
        # draw per reference ray chunk so that the CPU generator is consumed in the reference's order
        parts = []
        Nc, Nf, std = int(m.num_coarse), int(m.num_fine), float(m.radiance_field_noise_std)
        for a, b in _reference_chunks(N, options, mode, model_coarse, model_fine):
            n = b - a
            p = {}
            if m.perturb:
                p["t_rand"] = torch.rand([n, Nc])
            if model_coarse.jitter_std():
                p["jitter_coarse"] = _draw_point_jitter(model_coarse, n, Nc, m.chunksize)
            if std > 0.0:
                p["noise_coarse"] = torch.randn([n, Nc]) * std
            if Nf > 0 and m.perturb != 0.0:
                p["u"] = torch.rand([n, Nf])
            if Nf > 0 and model_fine.jitter_std():
                p["jitter_fine"] = _draw_point_jitter(model_fine, n, Nc + Nf, m.chunksize)
            if Nf > 0 and std > 0.0:
                p["noise_fine"] = torch.randn([n, Nc + Nf]) * std
            parts.append(p)
        randoms = {k: torch.cat([p[k] for p in parts], 0) for k in parts[0]} if parts else {}
    outs = []
    native = model_coarse.is_native_geometry() and model_fine.is_native_geometry()
    inv = None
    if (ray_grid_width and native and mode != "train" and not randoms and N >= capi.fused_min_rays()
            and N % int(ray_grid_width) == 0 and PATCH_H * SUPER_H * int(ray_grid_width) <= MAX_RAYS_PER_LAUNCH and not os.environ.get("NVSR_ROW_ORDER")):
        perm, inv = patch_order(N, ray_grid_width, rays.device)
        rays = rays.index_select(0, perm)
    step = MAX_RAYS_PER_LAUNCH if native else MAX_RAYS_PER_LAUNCH_GENERIC
    if inv is not None:
        step -= step % (PATCH_H * SUPER_H * int(ray_grid_width))       # launches split between rows of super-blocks
    def launch_all(force_arith=None):
        outs = []
        for a in range(0, max(N, 1), step):
            b = min(a + step, N)
            sub = None if randoms is None else {k: v[a:b] for k, v in randoms.items()}
            outs.append(predict_and_render_radiance(rays[a:b], model_coarse, model_fine, options, scene_id, mode=mode, randoms=sub if sub is not None else {},
                                                    force_arith=force_arith))
        return outs[0] if len(outs) == 1 else tuple(None if outs[0][i] is None else torch.cat([o[i] for o in outs], 0) for i in range(9))

    # Evaluation in NVSR_ARITH_F16X2 heals itself: the reference renders finite pixels for any f32 model (models.py:395-421); the f16 limbs
    # have ranges (|W| < 255, |feature / activation| < 4094), beyond which the kernels write NaN and raise the library's range flag.  One
    # device word, zeroed before the frame and read back after it (the only host wait of an evaluation frame; a frame is >= 100 ms of
    # kernels at 800 x 800): raised -> the frame is rendered again in the 3-bf16-limb arithmetic (warned once), and later frames of the same
    # parameters go there directly.  Covers hidden activations, which no check of the operands could see beforehand.
    # Generic geometries: the same healing for a frame of which a model evaluates in 'f16x2' (models.generic_arithmetic: by name only), except
    # that the frame is rendered again through the exact-f32 generic route -- the bits of arithmetic=None.
    limb_models = [] if (mode == "train" or native or N == 0) else [
        mdl for mdl in {id(x_): x_ for x_ in (model_coarse, model_fine)}.values() if not mdl.is_native_geometry() and mdl.generic_arithmetic() == "f16x2"]
    if limb_models:
        return _generic_limb_frame(launch_all, limb_models, model_coarse, model_fine, rays.device)      # (no patch order: that is a native frame's)
    range_checked = mode != "train" and native and N > 0 and _f16_in_play(model_coarse, model_fine)
    force, sr_changed = None, []
    if range_checked:
        key = _range_key(model_coarse, model_fine)
        if model_fine.__dict__.get("_f16_unfit") == key:
            force = "bf16x3"
            # (only when it was the SR stage that left the range -- bit 2: a decoder out of range says nothing about planes super-resolved in f16x2)
            if model_fine.__dict__.get("_f16_unfit_bits", 3) & 2:
                sr_changed = _sr_fallback(model_coarse, model_fine)
        else:
            flag = capi.range_flag(rays.device)
            flag.reset()
    rendered = False
    try:
        out = launch_all(force)
        if range_checked and force is None:
            bits = capi.RangeFlag.raised(flag.read_async())
            if bits:
                import warnings
                if not model_fine.__dict__.get("_f16_unfit_warned"):
                    warnings.warn("weights, plane values or activations beyond NVSR_ARITH_F16X2's range (|W| < 255, |feature / activation| < 4094; 'f16' has the same): this "
                                  "model renders in 'bf16x3' while its parameters stay as they are (set model.arithmetic = 'bf16x3' to render there in "
                                  "the first place)")
                    model_fine.__dict__["_f16_unfit_warned"] = True
                model_fine.__dict__["_f16_unfit"] = key
                model_fine.__dict__["_f16_unfit_bits"] = int(bits)
                if bits & 2:
                    sr_changed = _sr_fallback(model_coarse, model_fine, redo=True)
                out = launch_all("bf16x3")
                flag.reset()
        rendered = True
    finally:
        _sr_restore(sr_changed, rendered)          # (also when a launch raised: the model must not stay in 'bf16x3')
    if inv is not None:
        out = tuple(None if t is None else t.index_select(0, inv) for t in out)
    return out


def mip_radius(scene_id):
    """the cone radius of the Mip-NeRF baseline (train_utils.py:19-27): ds 0.00135 2 / sqrt(12), ds = the scene id's trailing _DS<d>"""
    import re
    import numpy as np
    m = re.search(r"(?<=_DS)(\d)+(?=$)", str(scene_id))
    if m is None:
        raise ValueError("Mip-NeRF needs the downsampling factor at the end of the scene id (e.g. 'lego_DS8'); got %r" % (scene_id,))
    return int(m.group(0)) * 0.00135 * 2 / np.sqrt(12.0)


class _NerfBaseline(NamedTuple):
    """what differs between the two FlexibleNeRFModel baselines on the host (the reference's predict_and_render_radiance with mip_nerf=True /
    False, train_utils.py:71-282)"""
    name: str
    fits: Callable          # FlexibleNeRFModel -> bool: the geometry its kernels are built for
    extra: int              # Mip samples Nc + 1 interval edges and Nf + 1 samples (its noise_fine is Nc + Nf + 1 wide); PE Nc and Nf depths
    chunk_div: int          # the reference draws its random numbers per chunksize // chunk_div rays (train_utils.py:228-235)
    bins: Callable          # depths [N,S] -> the bins of sample_pdf_2
    mip: bool               # the compositor's interval branch
    model_call: Callable    # scene_id -> (model, packed rays, depths, arithmetic or None) -> raw


def _mid(z):
    return 0.5 * (z[..., 1:] + z[..., :-1])


def _mip_call(scene_id):
    radius = mip_radius(scene_id)
    return lambda model, rays, edges, arith: model.mip_forward(rays, edges, radius, arithmetic=arith)


_NERF_BASELINES = {
    "mip": _NerfBaseline("Mip-NeRF", models.FlexibleNeRFModel.is_mip_baseline, 1, 4, lambda z: _mid(_mid(z)), True, _mip_call),
    "positional_encoding": _NerfBaseline("positional-encoding", models.FlexibleNeRFModel.is_pe_baseline, 0, 1, _mid, False,
                                         lambda scene_id: lambda model, rays, z, arith: model.pe_forward(rays, z, arithmetic=arith)),
}


def _run_nerf_baseline(b, H, W, focal, model_coarse, model_fine, batch_rays, options, scene_id, mode, scene_config, randoms):
    """run_one_iter_of_nerf + predict_and_render_radiance (train_utils.py:71-282) for the baseline b: Nc + b.extra coarse depths (Mip: the
    interval edges), the fused encoding + model kernel per pass, the compositor, sample_pdf_2 on b.bins(depths) with weights[..., 1:-1],
    Nf + b.extra samples, sort(cat(depths, samples)).  Gradients reach both models (the coarse pass's optional_no_grad is a null context
    upstream); the depths are detached."""
    if not options.nerf.use_viewdirs:
        raise NotImplementedError("the %s kernels expect use_viewdirs=True (MipNeRF_baseline.yml)" % b.name)
    from . import nerf_helpers
    model_call = b.model_call(scene_id)
    rays = pack_rays(batch_rays[0], batch_rays[1], _cfg(scene_config, "near"), _cfg(scene_config, "far"), H, W, focal,
                     no_ndc=_cfg(scene_config, "no_ndc"))
    if torch.is_grad_enabled() and rays.requires_grad:
        _warn_no_rays_grad(model_fine, "the %s baseline" % b.name)
    rays = rays.detach()
    N = rays.shape[0]
    m = _cfg(options.nerf, mode)
    Nc, Nf, std, x = int(m.num_coarse), int(m.num_fine), float(m.radiance_field_noise_std), b.extra
    if randoms is None and (m.perturb or std > 0.0):
        # per reference ray chunk, in the reference's order: t_rand, coarse noise, u, fine noise
        parts = []
        chunk = max(1, int(m.chunksize) // b.chunk_div)
        for a in range(0, N, chunk):
            n = min(a + chunk, N) - a
            p = {}
            if m.perturb:
                p["t_rand"] = torch.rand([n, Nc + x])
            if std > 0.0:
                p["noise_coarse"] = torch.randn([n, Nc]) * std
            if Nf > 0 and m.perturb != 0.0:
                p["u"] = torch.rand([n, Nf + x])
            if Nf > 0 and std > 0.0:
                p["noise_fine"] = torch.randn([n, Nc + Nf + x]) * std
            parts.append(p)
        randoms = {k: torch.cat([p[k] for p in parts], 0) for k in parts[0]} if parts else {}
    r = randoms or {}
    dev = rays.device
    t_rand, u, n_c, n_f = (None if r.get(k) is None else capi.f32c(r[k].to(dev)) for k in ("t_rand", "u", "noise_coarse", "noise_fine"))
    if not m.perturb:
        t_rand = None
    white, lindisp = bool(m.white_background), bool(m.lindisp)
    nv = torch.ops.nvsr
    if N == 0:
        e = lambda *sh: torch.empty(sh, dtype=torch.float32, device=dev)
        return (e(0, 3), e(0), e(0)) + ((e(0, 3), e(0), e(0)) if Nf > 0 else (None, None, None)) + (None, None, None)
    rd = rays[:, 3:6].contiguous()

    def render(force):
        # force: the arithmetic of the models that would run 'f16x2' (None: as configured)
        call = lambda mdl, z: model_call(mdl, rays, z, force if force and capi.resolve_nerf_arithmetic(mdl.arithmetic) == f16 else None)
        z_c = nv.coarse_z(rays, Nc + x, lindisp, t_rand)
        raw_c = call(model_coarse, z_c)
        rgb_c, disp_c, acc_c, w_c, _ = nv.composite(raw_c, z_c, rd, n_c, white, b.mip)
        rgb_f = disp_f = acc_f = None
        if Nf > 0:
            samples = nerf_helpers.sample_pdf_2(b.bins(z_c), w_c.detach()[..., 1:-1].contiguous(), Nf + x, det=(m.perturb == 0.0), u=u)
            z_f = nerf_helpers.sort_depths(torch.cat((z_c, samples), dim=-1))
            raw_f = call(model_fine, z_f)
            rgb_f, disp_f, acc_f, _, _ = nv.composite(raw_f, z_f, rd, n_f, white, b.mip)
        return rgb_c, disp_c, acc_c, rgb_f, disp_f, acc_f, None, None, None

    # An evaluation in 'f16x2' heals itself, as run_one_iter_of_nerf's does for the tri-plane model: the f16 limbs have ranges (|W| < 255,
    # |activation| < 4094) beyond which the kernels write NaN and raise the range flag.  The flag is zeroed before the frame and read once after
    # it; raised -> warned once, the frame is rendered again in 'bf16x3', and later frames of the same parameters (storage, version of both
    # models') go there directly.  Training does not come here: its metrics raise (training.StepMetrics).
    f16 = capi.ARITHMETIC["f16x2"]
    ms = [mdl for mdl in (model_coarse, model_fine) if mdl is not None]
    if mode == "train" or not any(capi.resolve_nerf_arithmetic(mdl.arithmetic) == f16 for mdl in ms):
        return render(None)
    key = tuple((p.data_ptr(), p._version) for mdl in ms for p in mdl.parameters())
    owner = ms[-1]
    if owner.__dict__.get("_nerf_f16_unfit") == key:
        return render("bf16x3")
    flag = capi.range_flag(dev)
    flag.reset()
    out = render(None)
    if capi.RangeFlag.raised(flag.read_async()):
        if not owner.__dict__.get("_nerf_f16_unfit_warned"):
            import warnings
            warnings.warn("weights or activations beyond NVSR_ARITH_F16X2's range (|W| < 255, |activation| < 4094): this %s model renders in "
                          "'bf16x3' while its parameters stay as they are (set model.arithmetic = 'bf16x3' to render there in the first place)" % b.name)
            owner.__dict__["_nerf_f16_unfit_warned"] = True
        owner.__dict__["_nerf_f16_unfit"] = key
        out = render("bf16x3")
        flag.reset()
    return out


def eval_nerf(height, width, focal_length, model_coarse, model_fine, ray_origins, ray_directions, options, scene_id,
              mode="validation", encode_position_fn=None, encode_direction_fn=None, scene_config={}):
    """train_utils.py:285-331 -> (rgb_coarse[H,W,3], None, None, rgb_fine[H,W,3] | None, None, None, None, None, None)"""
    ray_origins = ray_origins.reshape((1, -1, 3))
    ray_directions = ray_directions.reshape((1, -1, 3))
    batch_rays = torch.cat((ray_origins, ray_directions), dim=0)
    rgb_coarse, _, _, rgb_fine, _, _, rgb_SR, _, _ = run_one_iter_of_nerf(
        height, width, focal_length, model_coarse, model_fine, batch_rays, options, mode="validation",
        encode_position_fn=encode_position_fn, encode_direction_fn=encode_direction_fn, scene_id=scene_id, scene_config=scene_config,
        ray_grid_width=width)
    rgb_coarse = rgb_coarse.reshape([height, width, -1])
    if rgb_fine is not None:
        rgb_fine = rgb_fine.reshape([height, width, -1])
    return rgb_coarse, None, None, rgb_fine, None, None, rgb_SR, None, None


def _geometry_chunk(rays, model_coarse, model_fine, m, force_arith):
    """depth [n], acc [n], normal [n,3] of the top pass of a ray chunk: coarse depths, the coarse pass with weights and depth, the importance
    resampling, the fine pass likewise, then the normals of the top pass's live samples (ops.normals_of_pass)"""
    nv = torch.ops.nvsr
    Nc, Nf = int(m.num_coarse), int(m.num_fine)
    white, lindisp = bool(m.white_background), bool(m.lindisp)
    arith = lambda mdl: capi.resolve_render_arithmetic(mdl.arithmetic if force_arith is None else force_arith)
    top = model_coarse
    planes, consts = top.scene_args()            # (a model with SR planes renders its super-resolved planes)
    z = nv.coarse_z(rays, Nc, lindisp, None)
    _, _, acc, w, depth = nv.render_pass_geometry(planes, consts, top.packed_decoder(), rays, z, None, white, arith(top))
    if Nf > 0:
        z = nv.importance_resample(z, w, Nf, None)
        top = model_fine
        planes, consts = top.scene_args()
        _, _, acc, w, depth = nv.render_pass_geometry(planes, consts, top.packed_decoder(), rays, z, None, white, arith(top))
    normal = ops.normals_of_pass(planes, consts, top.packed_decoder(), top.packed_decoder_bwd(), rays, z, w, arith(top))
    return depth, acc, normal


def eval_geometry(height, width, focal_length, model_coarse, model_fine, ray_origins, ray_directions, options, scene_id,
                  mode="validation", scene_config={}):
    """Depth and surface-normal maps of a view (not in the reference) -> dict(depth [H,W], acc [H,W], normal [H,W,3]) of the
    fine pass, of the coarse pass when num_fine == 0, rendered as an evaluation frame: no perturbation, no density noise.
    depth = sum_s w_s z_s, acc = sum_s w_s, normal = sum_s w_s n_s with n_s = -normalize(d sigma / d p) on the samples of nonzero weight
    (include/nvsr.h, "surface normals").  The normal is NOT renormalised: its length is at most about acc, so background pixels go to 0;
    normalise it for unit vectors.  It lives in the coordinate system of the rays the passes march: NDC space for a scene with no_ndc False.
    The shipped decoder geometry in 'f16x2' or 'bf16x3' only; an 'f16x2' chunk that leaves the limbs' range is rendered again in 'bf16x3'
    like an evaluation render."""
    m = _cfg(options.nerf, mode)
    Nf = int(m.num_fine)
    used = (model_coarse, model_fine) if Nf > 0 else (model_coarse,)
    limb = (capi.ARITHMETIC["f16x2"], capi.ARITHMETIC["bf16x3"])
    for mdl in used:
        if not isinstance(mdl, models.TwoDimPlanesModel):
            raise NotImplementedError("eval_geometry: the tri-plane model only (got a %s: the NeRF baselines have no density-gradient route)"
                                      % type(mdl).__name__)
        if not mdl.is_native_geometry():
            raise NotImplementedError("eval_geometry: the shipped decoder geometry only (this model runs a generic one)")
        code = capi.resolve_render_arithmetic(mdl.arithmetic)
        if code not in limb:
            name = {v: k for k, v in capi.RENDER_ARITHMETIC.items()}.get(code, code)
            raise NotImplementedError("eval_geometry: the limb arithmetics 'f16x2' / 'bf16x3' only (this model resolves to %r)" % name)
    if not options.nerf.use_viewdirs:
        raise NotImplementedError("the decoder kernel expects use_viewdirs=True (all shipped configs)")
    rays = pack_rays(ray_origins.reshape(-1, 3), ray_directions.reshape(-1, 3), _cfg(scene_config, "near"), _cfg(scene_config, "far"), height, width,
                     focal_length, no_ndc=_cfg(scene_config, "no_ndc"))
    N = rays.shape[0]
    for mdl in used:
        mdl.set_cur_scene_id(scene_id)
    top = used[-1]
    range_checked = N > 0 and _f16_in_play(*used)
    key = _range_key(*used) if range_checked else None
    flag = capi.range_flag(rays.device) if range_checked else None
    outs, sr_changed, rendered = [], [], False
    try:
        with torch.no_grad():
            for a in range(0, max(N, 1), MAX_RAYS_PER_LAUNCH):
                sub = rays[a: min(a + MAX_RAYS_PER_LAUNCH, N)]
                if range_checked and top.__dict__.get("_f16_unfit") == key:
                    if not sr_changed and top.__dict__.get("_f16_unfit_bits", 3) & 2:
                        sr_changed = _sr_fallback(*used)
                    outs.append(_geometry_chunk(sub, model_coarse, model_fine, m, "bf16x3"))
                    continue
                if range_checked:
                    flag.reset()
                out = _geometry_chunk(sub, model_coarse, model_fine, m, None)
                bits = capi.RangeFlag.raised(flag.read_async()) if range_checked else 0
                if bits:
                    if not top.__dict__.get("_f16_unfit_warned"):
                        import warnings
                        warnings.warn("weights, plane values or activations beyond NVSR_ARITH_F16X2's range (|W| < 255, |feature / activation| < 4094): "
                                      "this model renders in 'bf16x3' while its parameters stay as they are (set model.arithmetic = 'bf16x3' to "
                                      "render there in the first place)")
                        top.__dict__["_f16_unfit_warned"] = True
                    top.__dict__["_f16_unfit"] = key
                    top.__dict__["_f16_unfit_bits"] = int(bits)
                    if bits & 2:
                        sr_changed = _sr_fallback(*used, redo=True)
                    out = _geometry_chunk(sub, model_coarse, model_fine, m, "bf16x3")
                    flag.reset()
                outs.append(out)
        rendered = True
    finally:
        _sr_restore(sr_changed, rendered)
    depth, acc, normal = (torch.cat([o[i] for o in outs], 0) for i in range(3))
    return dict(depth=depth.reshape(height, width), acc=acc.reshape(height, width), normal=normal.reshape(height, width, 3))


def find_latest_checkpoint(ckpt_path, sr, find_best=False):
    """train_utils.py:333-345 (implemented with the rest of the store protocol in plane_store.py)"""
    from .plane_store import find_latest_checkpoint as impl
    return impl(ckpt_path, sr, find_best)
