// Backward of TwoDimPlanesModel.forward for ANY decoder geometry, PLANE gradients only, in ONE launch: the fused twin of generic.hip's layered
// backward for iterations in which the decoder's parameters take no gradient (planes-only training, refinement under a frozen decoder).
//
// Reference: torch.autograd through models.py:381-421 (see generic.hip for the layer lists and the combination rules).
//
// The contract is the layered route's BITS up to the scatter.  There (generic_dgrad_kernel) every dX[p][k] is one v_mfma_f32_32x32x2_f32 chain
// from +0.0 over the pairs (2s, 2s + 1) of the output index m in ascending order, up to M rounded up to 32 with zero operands, on dZ = dY zeroed
// where the layer's output is not > 0; the gradients of a decoder's input start at +0.0 and take, layers descending, a skip layer's K2 part
// and last layer 0's part with __fadd_rn.  gf_layer_t below is that chain, NT 32-column output tiles at once.  The scatter multiplies by the
// tap weights as gen_scatter (generic.hip) does and adds the density decoder's and the colour decoder's product of a (texel, channel) with one
// __fadd_rn in front of ONE atomic: with at most these two addends on a zeroed texel, 0 + a + b in either order -- the layered route's bits.
//
// generic_backward_fused_kernel: the forward kernel's layout -- 1 .. 4 waves, 32 points per wave, a wave only touches its own 32 rows.
//   row of a point (GenFusedBwdPlan::ld floats, 2 x an odd number: the bank rule of generic_fused.hip):
//     [0, Kr)            Xr (or the raw sums under 'sum' / 'avg' / 'mult' view features), later dXr
//     [xd_off, + Kd)     Xd where it is not a prefix of Xr (always its own columns here), later dXd
//     [h_off, + hidden)  the current layer's input / output, later the current dZ
//     [dout_off, + 4)    the point's cotangent d_out[p][0:4] (+0 past P)
//     [gate_off, ..)     (nd + nr) x ceil(hidden / 32) words: bit m & 31 of word m >> 5 of a layer = its output m is > 0 (NaN and 0: closed)
//   forward     stage 0 and both decoders' hidden layers exactly as generic_decode_fused_kernel (gf_stage0, gf_layer); only the gate bits stay
//   colour      head from d_out[:, 0:3], the layers descending; dXr replaces Xr
//   view plane  two points at a time, 32 lanes over the channels of one texel: the view plane's atomics; under 'avg' / 'mult' dXr becomes
//               the gradient of the combined position feature in place ('mult': v (1 + vv) and v pp from the forward's own pp, vv)
//   density     head from d_out[:, 3], the layers descending; dXd replaces Xd
//   planes      two points at a time, 32 lanes over the channels: one atomic per (tap, channel) of every wanted position plane
// Capacity (gen_fused_bwd_plan, documented in include/nvsr.h): the forward kernel's, with the longer row in 160 KB.
//
// The kernel's text is generic_fused_bwd_kernel.h.  It is compiled a second time as generic_backward_fused_record_kernel, which also stores what
// the decoder's WEIGHT gradients contract -- Xd, Xr, every hidden activation and every gated dZ, the layered workspace's arrays with the layered
// route's bits -- as it forms them in LDS; nvsr_generic_decode_backward_fused_record_ext runs it per chunk of GEN_BWD_CHUNK points and then the
// layered route's own generic_wgrad_kernel launches (gen_wgrad_launch, generic.hip) on that record.  A training iteration WITH decoder gradients
// thereby keeps the layered route's values up to the order of the float atomics, without the recomputed layered forward and data gradients.
#include "generic_fused_bwd_core.h"

namespace nvsr {

// 1 = the fused backward holds this geometry, 0 = it does not (never 1 where gen_fused_plan answers 0)
static inline int gen_fused_bwd_plan(const GenGeom& g, GenFusedBwdPlan* pl) {
    GenFusedPlan f;
    if (!gen_fused_plan(g, &f)) return 0;
    pl->nt = f.nt;
    pl->gw = (g.hidden + 31) / 32;
    pl->xd_off = g.Kr;
    pl->h_off = g.Kr + g.Kd;
    pl->dout_off = pl->h_off + g.hidden;
    pl->gate_off = pl->dout_off + 4;
    long ld = pl->gate_off + (long)(g.nd + g.nr) * pl->gw;
    ld += ld & 1;
    if ((ld / 2) % 2 == 0) ld += 2;
    if (32 * ld > GF_LDS_FLOATS[GF_CLASSES - 1]) return 0;
    pl->ld = (int)ld;
    int best = 0;
    for (int c = 0; c < GF_CLASSES; ++c) {
        int w = GF_LDS_FLOATS[c] / (32 * pl->ld);
        if (w > GF_MAX_WAVES) w = GF_MAX_WAVES;
        const int per_cu = w * (4 >> c);
        if (per_cu > best) { best = per_cu; pl->cls = c; pl->waves = w; }
    }
    return best ? 1 : 0;
}

// ---- the record of a launch that also serves the decoder's weight gradients (generic_backward_fused_record_kernel) ----
// The operands of generic_wgrad_kernel for the P points of the launch (a chunk), in the layered workspace's shapes, with the layered route's
// bits: what generic_inputs_kernel and the kept forward would have left there, and every hidden layer's dZ already gated.
struct GenRecord {
    float* Xd;       // [P][Kd]
    float* Xr;       // [P][Kr]
    float* H;        // [nd + nr][P][hidden]: every hidden layer's output, the density layers first
    float* dZ;       // [nd + nr][P][hidden]: the gradient of every hidden layer's output, zeroed where the output is not > 0
    int planes;      // 0: no plane gradient is wanted -- the gradients of the decoder inputs and both scatters are left out
};
// columns [col, col + K) of the wave's 32 rows -> dst[(base + pt) * K + c] for the points base + pt < P: one contiguous block of global memory,
// read back from LDS behind a barrier.  K % 4 == 0: whole 16-byte stores (every array starts at a multiple of 16 bytes, so does a point's row);
// else dword stores.  The lanes walk the block 64 vectors at a time: (pt, c) advance by the quotient and remainder of 64, no division per step.
__device__ __forceinline__ void gfr_store_rows(const float* rows, int ld, int col, int K, float* __restrict__ dst, long base, long P, int lane) {
    if (base >= P) return;
    const int live = P - base < 32 ? (int)(P - base) : 32;
    float* __restrict__ out = dst + base * K;
    const bool vec = (K & 3) == 0;
    const int per = vec ? K >> 2 : K, total = live * per, dq = 64 / per, dr = 64 % per;
    int pt = lane / per, c = lane % per;
    for (int e = lane; e < total; e += 64) {
        if (vec) {
            const float* r = rows + pt * ld + col + 4 * c;
            *reinterpret_cast<float4*>(out + 4L * e) = make_float4(r[0], r[1], r[2], r[3]);
        } else {
            out[e] = rows[pt * ld + col + c];
        }
        pt += dq; c += dr;
        if (c >= per) { c -= per; ++pt; }
    }
}

// generic_backward_fused_kernel<NT, LDS floats> and generic_backward_fused_record_kernel<NT, LDS floats>: one text, compiled twice
#define GFB_KERNEL_NAME generic_backward_fused_kernel
#define GFB_RECORD 0
#include "generic_fused_bwd_kernel.h"
#undef GFB_KERNEL_NAME
#undef GFB_RECORD
#define GFB_KERNEL_NAME generic_backward_fused_record_kernel
#define GFB_RECORD 1
#include "generic_fused_bwd_kernel.h"
#undef GFB_KERNEL_NAME
#undef GFB_RECORD

// the launches of either kernel over the P points at x: rec == nullptr: generic_backward_fused_kernel; else the recording kernel
static int gfb_launch(const SceneDevN& sc, const GenGeom& g, const GenFusedBwdPlan& pl, long P, const float* x, const float* noise,
                      const float* natural, const float* d_out, const GradPlanesN& gp, const GenRecord* rec, hipStream_t stream) {
    return gf_for_plan(pl.nt, pl.cls, [&](auto nt, auto cls) {
        constexpr int NT = decltype(nt)::value, LDSF = GF_LDS_FLOATS[decltype(cls)::value];
        return gf_launch_pieces(P, pl.waves, [&](long b0, unsigned nb) {
            if (rec)
                hipLaunchKernelGGL((generic_backward_fused_record_kernel<NT, LDSF>), dim3(nb), dim3(64 * pl.waves), 0, stream, sc, g, pl, P, b0, x, noise,
                                   natural, d_out, gp, *rec);
            else
                hipLaunchKernelGGL((generic_backward_fused_kernel<NT, LDSF>), dim3(nb), dim3(64 * pl.waves), 0, stream, sc, g, pl, P, b0, x, noise,
                                   natural, d_out, gp);
        });
    });
}

// floats of a point in the record, and the room that lets its four arrays start at multiples of 16 bytes in any workspace
static inline int64_t gfr_floats_per_point(const GenGeom& g) { return (int64_t)g.Kd + g.Kr + 2 * (int64_t)(g.nd + g.nr) * g.hidden; }
constexpr int GFR_ALIGN_FLOATS = 16;
// the record of a chunk of n points in the workspace: Xd, Xr, H, dZ, each from the next multiple of 16 bytes on
static inline GenRecord gfr_carve(float* workspace, const GenGeom& g, long n, bool planes) {
    auto up4 = [](long v) { return (v + 3) & ~3L; };
    GenRecord r;
    r.Xd = reinterpret_cast<float*>((reinterpret_cast<uintptr_t>(workspace) + 15) & ~(uintptr_t)15);
    r.Xr = r.Xd + up4(n * g.Kd);
    r.H = r.Xr + up4(n * g.Kr);
    r.dZ = r.H + up4((long)(g.nd + g.nr) * n * g.hidden);
    r.planes = planes ? 1 : 0;
    return r;
}

}  // namespace nvsr

using namespace nvsr;

extern "C" {

int nvsr_generic_backward_fused_supported(const nvsr_decoder_geometry* geometry, int num_position_planes) {
    return gf_supported(geometry, num_position_planes, [](const GenGeom& g) {
        GenFusedBwdPlan pl;
        return gen_fused_bwd_plan(g, &pl);
    });
}

int nvsr_generic_decode_backward_fused_ext(const nvsr_scene_ext* scene, const nvsr_decoder_geometry* geometry, const float* natural, int64_t P,
                                           const float* x, const float* coord_noise, const float* d_out, float* const* d_planes,
                                           nvsr_stream_t stream) {
    GenGeom g;
    GenFusedBwdPlan pl;
    SceneDevN sc;
    const int e = gf_check_entry(scene, geometry, [&](const GenGeom& gg) { return gen_fused_bwd_plan(gg, &pl); }, natural && x && d_out, GF_FULL,
                                 GenFusedList{nullptr, nullptr, 0}, P, &g, &sc);
    if (e != GF_LAUNCH) return e;
    GradPlanesN gp = {};
    if (!gfb_wanted(d_planes, g.np, &gp)) return NVSR_OK;
    return gfb_launch(sc, g, pl, (long)P, x, coord_noise, natural, d_out, gp, nullptr, (hipStream_t)stream);
}

int64_t nvsr_generic_backward_chunk(void) { return GEN_BWD_CHUNK; }

int64_t nvsr_generic_backward_fused_record_workspace_floats_ext(const nvsr_decoder_geometry* geometry, int num_position_planes, int64_t P) {
    GenGeom g;
    if (gen_resolve(geometry, &g, num_position_planes) || P < 0) return -1;
    return (P < GEN_BWD_CHUNK ? P : GEN_BWD_CHUNK) * gfr_floats_per_point(g) + GFR_ALIGN_FLOATS;
}

int nvsr_generic_decode_backward_fused_record_ext(const nvsr_scene_ext* scene, const nvsr_decoder_geometry* geometry, const float* natural, int64_t P,
                                                  const float* x, const float* coord_noise, const float* d_out, float* d_natural,
                                                  float* const* d_planes, float* workspace, nvsr_stream_t stream) {
    GenGeom g;
    GenFusedBwdPlan pl;
    SceneDevN sc;
    const int e = gf_check_entry(scene, geometry, [&](const GenGeom& gg) { return gen_fused_bwd_plan(gg, &pl); },
                                 natural && x && d_out && (workspace || !d_natural), GF_FULL, GenFusedList{nullptr, nullptr, 0}, P, &g, &sc);
    if (e != GF_LAUNCH) return e;
    GradPlanesN gp = {};
    const bool planes = gfb_wanted(d_planes, g.np, &gp);
    if (!d_natural)       // nvsr_generic_decode_backward_fused_ext: nothing is recorded
        return planes ? gfb_launch(sc, g, pl, (long)P, x, coord_noise, natural, d_out, gp, nullptr, (hipStream_t)stream) : NVSR_OK;
    long woff[2][65];
    gen_blob_offsets(g, woff);
    hipStream_t s = (hipStream_t)stream;
    for (int64_t a = 0; a < P; a += GEN_BWD_CHUNK) {
        const long n = (long)((P - a) < GEN_BWD_CHUNK ? (P - a) : GEN_BWD_CHUNK);
        const GenRecord rec = gfr_carve(workspace, g, n, planes);
        const float* da = d_out + a * 4;
        if (int err = gfb_launch(sc, g, pl, n, x + a * 6, coord_noise ? coord_noise + a * 3 : nullptr, natural, da, gp, &rec, s)) return err;
        // the layered route's contractions (gen_decode_backward) on the record: the same slabs, the same operands' bits, dZ already gated
        for (int dec = 0; dec < 2; ++dec) {
            const int k0 = dec ? g.Kr : g.Kd, nl = dec ? g.nr : g.nd, Mh = dec ? 3 : 1, hoff = dec ? 0 : 3;
            const float* in0 = dec ? rec.Xr : rec.Xd;
            const float* Hs = rec.H + (dec ? (long)g.nd * n * g.hidden : 0);
            const float* dZs = rec.dZ + (dec ? (long)g.nd * n * g.hidden : 0);
            const float* last = Hs + (long)(nl - 1) * n * g.hidden;
            float* gh = d_natural + woff[dec][nl];
            if (int err = gen_wgrad_launch(n, Mh, g.hidden, 0, da, 4, hoff, nullptr, last, last, gh, gh + (long)Mh * g.hidden, s)) return err;
            for (int l = nl - 1; l >= 0; --l) {
                const bool skip = l > 0 && gen_skip_layer(l - 1, g.skip);
                const int K1 = l == 0 ? k0 : g.hidden, K2 = skip ? k0 : 0;
                const float* X1 = l == 0 ? in0 : Hs + (long)(l - 1) * n * g.hidden;
                float* gw = d_natural + woff[dec][l];
                if (int err = gen_wgrad_launch(n, g.hidden, K1, K2, dZs + (long)l * n * g.hidden, g.hidden, 0, nullptr, X1, in0, gw,
                                               gw + (long)g.hidden * (K1 + K2), s))
                    return err;
            }
        }
    }
    return NVSR_OK;
}

}  // extern "C"
