"""GPU tests of the tri-plane training kernels -- the recording and the gates-only forward (nvsr_decode_rays_arith: decode_core.h,
decode_limb.hip, decode_pair.hip), the gate-driven backward (nvsr_render_pass_backward_gates_arith: render_bwd.hip, render_bwd_limb.hip), the
recomputing f32 backward (nvsr_render_pass_backward_ex) and view_reduce_scatter_kernel -- per layer and per texel against float64, through the
C ABI on buffers the test owns (tests/triplane_checks.py holds the references and the derivations of the bounds).

Every layer is checked from the kernel's OWN record of its input, so a ReLU gate that differs between f32 and float64 cannot blur the
comparison: each element has a bound that follows from the arithmetic, each texel of a gradient plane one that follows from its contributions.
The position taps of the inputs are exact in f32 (triplane_checks' docstring); the view plane's carry the counted term e_v.

  gates ........... the words of a recording forward are [H > 0] of its own record, all eight layers and every bit; the gates-only forward
                    gives the same words and raw bits (the tile-pair kernel -- f16x2, no record, S >= 128 -- up to activations below 2^-29 and
                    2e-6 of raw's range, as test_pair_forward_matches_the_one_tile_forward states)
  forward ......... Xr, Xd, Hd[l], Hr[l] and raw, each from the recorded input (check_forward)
  backward ........ g4, Gd[l], Gr[l], each from the recorded gradient above and the gates (check_backward_layers)
  view rows ....... view_ws against Gr[0] W_r0[:, 144:192]: one row per point (f32) or one pre-summed row per (ray, 32-sample chunk) (limbs);
                    the other rows keep the sentinel
  planes .......... per texel: initial + sum w gF with gamma_(n + 2) (scatter_reference); texels outside the footprint keep their bits; a NULL
                    entry of grad_planes is skipped and changes nothing else; with and without view_ws
  no record ....... the gates-only backward and the recomputing backward without a record: the float64 chain from dL/draw and the gates with
                    the bound propagated layer by layer (chain_from_gates)
  padding ......... raw, gates, the record, view_ws and the four gradient planes end in NaN-sentinel words that every call leaves alone;
                    record rows >= P in front of the dump rows are unwritten; N = 0 writes nothing
Shapes (triplane_checks.cases): below one tile and one tile, partial last chunks with 1, 2, 3 and 0 (mod 4) wave tiles, f32 ray blocks of 128
and 256 at S = 3, the tile-pair forward, launches past the grid caps (without a record), ordinary coordinates on 200 x 200 planes.

Measured on an MI355X, worst err / bound over all cases (f32 / bf16x3 / f16x2; every test prints its own): features Xr, Xd 0.79 in each; hidden
layers forward 0.12 / 0.22 / 0.19, heads 0.02; backward heads 1.00 (one rounding against a one-rounding bound) and 0.84, transposed layers
0.04 / 0.16 / 0.14; view_ws rows 0.04 / 0.08 / 0.09; planes from the record 0.47 / 0.47 / 0.44, from the gates alone 0.33 / 0.36 / 0.37, past
the grid caps <= 0.06.  On the view plane's 4 x 4 blocks the counted tap term e_v is up to the whole bound (a block texel without contributions
has no other term); the plane's worst err / bound is 0.32.

What these tests found: scatter_plane_cached_v (bwd_core.h) read the previous point's texels with __shfl inside the `pt != 0` arm of a select;
point 0's lanes were inactive there and ds_bpermute returned 0 for them, so a slot that moved onto the plane's FIRST texel at the second sample
of a tile was not flushed and its sum landed on that texel (record-127x3 .. 257x3 in the limb arithmetics failed per texel by the size of
one contribution).
"""
import ctypes as C
from types import SimpleNamespace as NS

import pytest
import torch

import triplane_checks as tc
from nerf_baseline_checks import DEV, T, assert_within, bits
from triplane_checks import gamma

pytestmark = pytest.mark.gpu

ARITHS = ["f32", "bf16x3", "f16x2"]
SENTINEL = 0x7FC0FFEE           # a quiet-NaN bit pattern no kernel computes
PAD = 256                       # sentinel words behind every buffer
CH = tc.C


def padded(n, fill=None):
    """n float32 words for a kernel, then PAD words of the sentinel (a float32 view of one int32 allocation); fill: the first n words"""
    b = torch.full((n + PAD,), SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)
    if fill is not None:
        b[:n] = fill
    return b


def pad_intact(buf, n):
    return bool((buf.view(torch.int32)[n:] == SENTINEL).all())


def untouched(buf):
    return bool((buf.view(torch.int32) == SENTINEL).all())


class Setup:
    """one case on the device: scene, planes, packed weights, rays, depths, dL/draw, float64 taps"""

    def __init__(self, hip, c):
        self.capi, self.c, self.N, self.S, self.P = hip.capi, c, c.N, c.S, c.N * c.S
        capi = hip.capi
        scene, planes, rays, z, g = tc.case_inputs(c)
        self.scene_np = scene
        self.planes = [T(p) for p in planes]
        self.rays, self.z, self.g_raw = T(rays), T(z), T(g)
        self.nat = T(tc.make_decoder(7))
        self.dec = tc.unpack(self.nat, DEV)
        self.packed = torch.zeros(capi.DECODER_PACKED_FLOATS, device=DEV)
        self.packed_bwd = torch.zeros(capi.DECODER_PACKED_BWD_FLOATS, device=DEV)
        capi.call("nvsr_pack_decoder", capi.ptr(self.nat), capi.ptr(self.packed), capi.stream())
        capi.call("nvsr_pack_decoder_bwd", capi.ptr(self.nat), capi.ptr(self.packed_bwd), capi.stream())
        sc = capi.Scene()
        for d in range(4):
            sc.planes[d] = self.planes[d].data_ptr()
            sc.ph[d], sc.pw[d] = scene.ph[d], scene.pw[d]
        for i in range(5):
            sc.lo[i], sc.range[i] = float(scene.lo[i]), float(scene.range[i])
        for d in range(3):
            for j in range(6):
                sc.proj[d][j] = float(scene.proj[d][j])
        self.sc = sc
        self.taps = tc.taps_to(tc.all_taps(rays, z, scene, c.exact), DEV)
        self.rec_floats = int(capi.lib().nvsr_decoder_record_floats(c.N, c.S)) if c.record else 0
        self.ws_floats = int(capi.lib().nvsr_view_grad_workspace_floats(c.N, c.S))
        assert self.ws_floats == self.P * CH
        gen = torch.Generator(device=DEV).manual_seed(c.seed)
        self.initial = [torch.randn(p.numel(), device=DEV, generator=gen) for p in self.planes]     # the kernels accumulate: not zeros

    def forward(self, arith, record):
        capi, p = self.capi, self.capi.ptr
        raw, gates = padded(self.P * 4), padded(self.P * 32)
        rec = padded(self.rec_floats) if record else None
        capi.call("nvsr_decode_rays_arith", C.byref(self.sc), p(self.packed), self.N, self.S, p(self.rays), p(self.z), p(raw), p(gates), p(rec),
                  capi.ARITHMETIC[arith], capi.stream())
        return NS(raw=raw, gates=gates, rec=rec)

    def grad_planes(self, null=None):
        bufs = [None if d == null else padded(i.numel(), i) for d, i in enumerate(self.initial)]
        arr = (C.c_void_p * 4)(*[None if b is None else b.data_ptr() for b in bufs])
        return bufs, arr

    def backward(self, arith, gates, rec=None, view_ws=False, null=None, recompute=False):
        """the gate-driven backward (recompute: nvsr_render_pass_backward_ex) -> planes, view_ws; rec: a record buffer to complete, or True
        for a fresh one (the recomputing kernel writes both halves)"""
        capi, p = self.capi, self.capi.ptr
        bufs, arr = self.grad_planes(null)
        ws = padded(self.ws_floats) if view_ws else None
        if rec is True:
            rec = padded(self.rec_floats)
        if recompute:
            capi.call("nvsr_render_pass_backward_ex", C.byref(self.sc), p(self.packed), p(self.packed_bwd), self.N, self.S, p(self.rays), p(self.z),
                      p(self.g_raw), arr, p(rec), p(ws), capi.stream())
        else:
            capi.call("nvsr_render_pass_backward_gates_arith", C.byref(self.sc), p(self.packed), p(self.packed_bwd), self.N, self.S, p(self.rays),
                      p(self.z), p(self.g_raw), p(gates), arr, p(ws), p(rec), capi.ARITHMETIC[arith], capi.stream())
        return NS(planes=bufs, ws=ws, rec=rec, null=null)

    def views(self, rec):
        return tc.record_views(rec[:self.rec_floats], self.N, self.S)

    def plane_pads_intact(self, out):
        return all(b is None or pad_intact(b, i.numel()) for b, i in zip(out.planes, self.initial))


def _tag(s, arith):
    return "%s %s" % (tc.case_id(s.c), arith)


def _report(s, arith, what, rep):
    print("%s %s, worst err / bound: %s" % (_tag(s, arith), what, ", ".join("%s %.3f" % kv for kv in rep.items())))


def check_planes(s, arith, name, out, gF, E):
    """the planes of one backward call per texel (tc.check_plane); a NULL entry has no buffer"""
    rep = {}
    for d in range(4):
        if out.planes[d] is None:
            continue
        n = s.initial[d].numel()
        rep["plane %d" % d], share = tc.check_plane("%s %s plane %d" % (_tag(s, arith), name, d), out.planes[d][:n], s.initial[d], s.taps[d], gF[d],
                                                    E[d])
        if s.taps[d].inexact:
            rep["tap share %d" % d] = share
    _report(s, arith, name, rep)


def check_view_rows(s, arith, ws, gF3, E3, per_point):
    """view_ws: one row per point (the f32 kernels: store_view_rows) or one pre-summed row per (ray, 32-sample chunk) (the limb kernel: 8 adds in
    each of four partial sums and two more, gamma_10 sum |gF|); every other row keeps the sentinel"""
    N, S = s.N, s.S
    if per_point:
        rows, ref, bound = s.P, gF3, E3
    else:
        nsc = (S + 31) // 32
        rows = N * nsc
        pad = lambda a: torch.nn.functional.pad(a.view(N, S, CH), (0, 0, 0, nsc * 32 - S)).view(N * nsc, 32, CH)
        ref, bound = pad(gF3).sum(1), pad(E3).sum(1) + gamma(10) * pad(gF3.abs() + E3).sum(1)
    got = ws[:rows * CH].view(rows, CH)
    worst = assert_within("%s view_ws" % _tag(s, arith), got.double(), ref, bound)
    assert untouched(ws[rows * CH:]), "%s: view_ws rows that belong to no point were written" % _tag(s, arith)
    return worst


# ---- cases with a record ----------------------------------------------------------------------------------------------------------------

RECORD_CASES = [c for c in tc.cases() if c.record]
CAP_CASES = [c for c in tc.cases() if not c.record]


@pytest.fixture(scope="module", params=[(c, a) for c in RECORD_CASES for a in ARITHS], ids=lambda p: "%s-%s" % (tc.case_id(p[0]), p[1]))
def run(request, hip):
    """one (case, arithmetic): recording forward, gates-only forward, the backward with record and view_ws, with neither, with a NULL plane
    entry, with a record and no view_ws; f32: the recomputing backward with a record and without"""
    c, arith = request.param
    s = Setup(hip, c)
    flag = hip.capi.range_flag(torch.device(DEV))
    flag.reset()
    f_rec, f_gates = s.forward(arith, True), s.forward(arith, False)
    b_full = s.backward(arith, f_rec.gates, rec=f_rec.rec, view_ws=True)
    b_bare = s.backward(arith, f_rec.gates)
    b_null = s.backward(arith, f_rec.gates, view_ws=True, null=c.null)
    rec2 = f_rec.rec.clone()
    b_rec = s.backward(arith, f_rec.gates, rec=rec2)
    x_rec = x_bare = None
    if arith == "f32":
        x_rec = s.backward(arith, None, rec=True, view_ws=True, recompute=True)
        x_bare = s.backward(arith, None, recompute=True)
    torch.cuda.synchronize()
    P = s.P
    r = NS(s=s, arith=arith, f_rec=f_rec, f_gates=f_gates, b_full=b_full, b_bare=b_bare, b_null=b_null, b_rec=b_rec, x_rec=x_rec, x_bare=x_bare,
           flag=int(flag.word[0]), rec=s.views(f_rec.rec), raw=f_rec.raw[:P * 4].view(P, 4), gates=f_rec.gates[:P * 32].view(torch.int32).view(P, 2, 16),
           g=s.g_raw.view(P, 4))
    r.un = tc.undo_factors(s.g_raw) if arith == "f16x2" else (None, None)
    r.gF, r.E = tc.feature_gradients(arith, s.dec, r.rec.Gd[0].double(), r.rec.Gr[0].double(), un_d=r.un[0], un_r=r.un[1])
    return r


def test_gates_are_the_signs_of_the_record(run):
    r, s = run, run.s
    want = tc.gate_words(r.rec.Hd, r.rec.Hr)
    diff = want != r.gates
    assert not bool(diff.any()), "%s: %d gate words differ from [H > 0], the first at point %d" % (_tag(s, r.arith), int(diff.sum()),
                                                                                                   int(diff.nonzero()[0, 0]))
    open_ = float(tc.gates_to_masks(r.gates, s.P).mean())
    assert 0.2 < open_ < 0.8, open_
    # the gates-only forward
    P = s.P
    raw2, gates2 = r.f_gates.raw[:P * 4].view(P, 4), r.f_gates.gates[:P * 32].view(torch.int32).view(P, 2, 16)
    if r.arith == "f16x2" and s.S >= 128:
        # the tile-pair kernel: a gate may read closed where the recorded activation is positive and below 2^-29; raw within 2e-6 of its range
        H = torch.cat([r.rec.Hd, r.rec.Hr])
        H = torch.where((H > 0) & (H < tc.PAIR_GATE_FLOOR), torch.zeros_like(H), H)
        may_differ = r.gates ^ tc.gate_words(H[:4], H[4:])                # the bits of such activations
        ok = ((gates2 ^ r.gates) & ~may_differ) == 0
        assert bool(ok.all()), "%s: the pair forward's gates differ beyond activations below 2^-29" % _tag(s, r.arith)
        scale = float(r.raw.abs().max())
        err = float((raw2 - r.raw).abs().max())
        assert err <= 2e-6 * scale, (err, scale)
        print("%s pair forward: raw max|err| %.2e of the range, %d gate words differ" % (_tag(s, r.arith), err / scale, int((gates2 != r.gates).sum())))
    else:
        assert torch.equal(gates2, r.gates), "%s: the gates-only forward's words differ" % _tag(s, r.arith)
        assert torch.equal(bits(raw2), bits(r.raw)), "%s: the gates-only forward's raw differs" % _tag(s, r.arith)


def test_forward_layer_by_layer(run):
    r, s = run, run.s
    _report(s, r.arith, "forward", tc.check_forward(r.arith, s.dec, s.planes, s.taps, r.rec, r.raw))
    if r.x_rec is not None:          # the recomputing backward writes the layer-input half itself (raw: the forward's, same code)
        _report(s, r.arith, "recomputed forward", tc.check_forward(r.arith, s.dec, s.planes, s.taps, s.views(r.x_rec.rec), r.raw))


def test_backward_layer_by_layer(run):
    r, s = run, run.s
    _report(s, r.arith, "backward", tc.check_backward_layers(r.arith, s.dec, r.rec, r.g, r.gates))
    _report(s, r.arith, "backward (no view_ws)", tc.check_backward_layers(r.arith, s.dec, s.views(r.b_rec.rec), r.g, r.gates))
    if r.x_rec is not None:
        v = s.views(r.x_rec.rec)
        _report(s, r.arith, "recomputing backward", tc.check_backward_layers(r.arith, s.dec, v, r.g, tc.gate_words(v.Hd, v.Hr)))


def test_view_rows(run):
    r, s = run, run.s
    rep = {"gate backward": check_view_rows(s, r.arith, r.b_full.ws, r.gF[3], r.E[3], r.arith == "f32")}
    if r.b_null.null != 3:
        rep["NULL entry"] = check_view_rows(s, r.arith, r.b_null.ws, r.gF[3], r.E[3], r.arith == "f32")
    else:
        assert untouched(r.b_null.ws), "view_ws was written although the view plane is frozen"      # (nothing reads it then; the kernel skips it)
    if r.x_rec is not None:
        v = s.views(r.x_rec.rec)
        gF, E = tc.feature_gradients(r.arith, s.dec, v.Gd[0].double(), v.Gr[0].double())
        rep["recomputing"] = check_view_rows(s, r.arith, r.x_rec.ws, gF[3], E[3], True)
    _report(s, r.arith, "view_ws", rep)


def test_planes_per_texel(run):
    r, s = run, run.s
    check_planes(s, r.arith, "record + view_ws", r.b_full, r.gF, r.E)
    v = s.views(r.b_rec.rec)
    gF, E = tc.feature_gradients(r.arith, s.dec, v.Gd[0].double(), v.Gr[0].double(), un_d=r.un[0], un_r=r.un[1])
    check_planes(s, r.arith, "record", r.b_rec, gF, E)
    check_planes(s, r.arith, "NULL entry %d + view_ws" % r.b_null.null, r.b_null, r.gF, r.E)
    if r.x_rec is not None:
        v = s.views(r.x_rec.rec)
        gF, E = tc.feature_gradients(r.arith, s.dec, v.Gd[0].double(), v.Gr[0].double())
        check_planes(s, r.arith, "recomputing, record + view_ws", r.x_rec, gF, E)


def test_planes_without_a_record(run):
    r, s = run, run.s
    Gd0, Ed0, Gr0, Er0, un_d, un_r = tc.chain_from_gates(r.arith, s.dec, r.g, r.gates)
    gF, E = tc.feature_gradients(r.arith, s.dec, Gd0, Gr0, Ed0, Er0, un_d, un_r)
    check_planes(s, r.arith, "gates only", r.b_bare, gF, E)
    if r.x_bare is not None:          # the gates of its recording twin
        v = s.views(r.x_rec.rec)
        Gd0, Ed0, Gr0, Er0, _, _ = tc.chain_from_gates(r.arith, s.dec, r.g, tc.gate_words(v.Hd, v.Hr))
        gF, E = tc.feature_gradients(r.arith, s.dec, Gd0, Gr0, Ed0, Er0)
        check_planes(s, r.arith, "recomputing, no record", r.x_bare, gF, E)


def test_padding_and_range_flag(run):
    r, s = run, run.s
    P, tag = s.P, _tag(s, r.arith)
    assert r.flag == 0, "%s: range flag %d" % (tag, r.flag)
    for name, f in (("recording", r.f_rec), ("gates-only", r.f_gates)):
        assert pad_intact(f.raw, P * 4) and pad_intact(f.gates, P * 32), "%s: %s forward wrote behind raw / gates" % (tag, name)
    for name, rec in (("forward + backward", r.f_rec.rec), ("backward", r.b_rec.rec)) + ((("recomputing", r.x_rec.rec),) if r.x_rec else ()):
        assert pad_intact(rec, s.rec_floats), "%s: %s wrote behind the record" % (tag, name)
        v = s.views(rec)
        assert v.floats == s.rec_floats
        assert untouched(v.tail), "%s: %s wrote record rows >= P in front of the dump rows" % (tag, name)
    for name, out in (("full", r.b_full), ("bare", r.b_bare), ("null", r.b_null), ("rec", r.b_rec), ("recompute", r.x_rec), ("recompute bare", r.x_bare)):
        if out is None:
            continue
        assert s.plane_pads_intact(out), "%s: backward (%s) wrote behind a gradient plane" % (tag, name)
        assert out.ws is None or pad_intact(out.ws, s.ws_floats), "%s: backward (%s) wrote behind view_ws" % (tag, name)


# ---- past the grid caps, without a record -----------------------------------------------------------------------------------------------

def _cap_params():
    out = []
    for c in CAP_CASES:
        for a in (["bf16x3", "f16x2"] if c.kind == "limb" else ["f32"]):
            out.append((c, a))
    return out


@pytest.mark.parametrize("c,arith", _cap_params(), ids=lambda v: tc.case_id(v) if hasattr(v, "kind") else v)
def test_past_the_grid_caps(hip, c, arith):
    """More tiles than workgroups (2 048 for the limb launches of 4 wave tiles, 1 024 for the f32 backward kernels): the gates-only forward
    and backward, per texel against the float64 chain from dL/draw and the gates (chain_from_gates).  The recomputing kernel (f32_recompute)
    has no recording twin at this size (9.2 KB per point): its gates are the f32 gates-only forward's, the same layer code."""
    s = Setup(hip, c)
    flag = hip.capi.range_flag(torch.device(DEV))
    flag.reset()
    f = s.forward(arith, False)
    outs = [("view_ws", s.backward(arith, f.gates, view_ws=True, recompute=c.kind == "f32_recompute")),
            ("bare", s.backward(arith, f.gates, recompute=c.kind == "f32_recompute"))]
    torch.cuda.synchronize()
    P = s.P
    assert int(flag.word[0]) == 0
    assert pad_intact(f.raw, P * 4) and pad_intact(f.gates, P * 32)
    gates = f.gates[:P * 32].view(torch.int32).view(P, 2, 16)
    Gd0, Ed0, Gr0, Er0, un_d, un_r = tc.chain_from_gates(arith, s.dec, s.g_raw.view(P, 4), gates)
    gF, E = tc.feature_gradients(arith, s.dec, Gd0, Gr0, Ed0, Er0, un_d, un_r)
    # raw against the float64 forward on the same gates is not a per-element check (no record): the heads' inputs are unknown; finite is all
    assert bool(torch.isfinite(f.raw[:P * 4]).all())
    for name, out in outs:
        check_planes(s, arith, name, out, gF, E)
        assert s.plane_pads_intact(out) and (out.ws is None or pad_intact(out.ws, s.ws_floats))
    _report(s, arith, "view_ws", {"rows": check_view_rows(s, arith, outs[0][1].ws, gF[3], E[3], arith == "f32")})


# ---- N = 0 ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("arith", ARITHS)
def test_zero_rays_write_nothing(hip, arith):
    c = NS(N=1, S=4, sizes=tc.SIZES[0], seed=1, exact=True, sort=True, record=True, kind="zero", null=None)
    s = Setup(hip, c)
    capi, p = hip.capi, hip.capi.ptr
    raw, gates, rec, ws = padded(0), padded(0), padded(0), padded(0)
    bufs, arr = s.grad_planes()
    capi.call("nvsr_decode_rays_arith", C.byref(s.sc), p(s.packed), 0, 4, p(s.rays), p(s.z), p(raw), p(gates), p(rec), capi.ARITHMETIC[arith], capi.stream())
    capi.call("nvsr_render_pass_backward_gates_arith", C.byref(s.sc), p(s.packed), p(s.packed_bwd), 0, 4, p(s.rays), p(s.z), p(s.g_raw), p(gates), arr,
              p(ws), p(rec), capi.ARITHMETIC[arith], capi.stream())
    capi.call("nvsr_render_pass_backward_ex", C.byref(s.sc), p(s.packed), p(s.packed_bwd), 0, 4, p(s.rays), p(s.z), p(s.g_raw), arr, p(rec), p(ws),
              capi.stream())
    torch.cuda.synchronize()
    for b in (raw, gates, rec, ws):
        assert untouched(b)
    for b, i in zip(bufs, s.initial):
        assert torch.equal(bits(b[:i.numel()]), bits(i)) and pad_intact(b, i.numel())
