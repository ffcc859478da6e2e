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

template <int NT, int LDSF>
__global__ __launch_bounds__(64 * GF_MAX_WAVES) void generic_backward_fused_kernel(SceneDevN sc, GenGeom g, GenFusedBwdPlan L, long P, long block0,
                                                                                    const float* __restrict__ x, const float* __restrict__ noise,
                                                                                    const float* __restrict__ natural,
                                                                                    const float* __restrict__ d_out, GradPlanesN gp) {
    __shared__ __attribute__((aligned(16))) float lds[LDSF];
    NVSR_RACE_PROBE_DELAY(lds);      // (probe builds only, nvsr_common.h)
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, n = lane & 31, h = lane >> 5;
    const long slot0 = (block0 + blockIdx.x) * (long)(blockDim.x >> 6) * 32;
    const long p = slot0 + wave * 32 + n;
    const bool live = p < P;
    float* rows = lds + wave * 32 * L.ld;
    float* row = rows + n * L.ld;
    unsigned* gate = reinterpret_cast<unsigned*>(row + L.gate_off);

    // ---- forward: stage 0 and the hidden layers of both decoders; the gate bits stay ----
    const GenFusedRows R = {rows, row, L.ld, L.xd_off};
    float vgx, vgy;
    gf_stage0<GF_FULL>(sc, g, R, n, h, live, p, x, noise, vgx, vgy);
    const bool raw = g.proj == 2 || g.view == 4;
    const int xd_in = g.proj == 2 ? 0 : L.xd_off;       // 'concat': Xd is the head of Xr
    if (h == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) row[L.dout_off + r] = live ? d_out[p * 4 + r] : 0.0f;
    }
    const float* const wcolour = natural + gf_density_floats(g);
    for (int dec = 0; dec < 2; ++dec) {
        const bool rgb = dec == 1;
        if (rgb && !raw) {                                // Xd -> Xr: the combined position features, then combine_all_planes in place
            for (int c = h; c < g.C; c += 2) row[c] = row[L.xd_off + c];
            __syncthreads();
            gf_plane_features(sc, g, R, n, h, g.np, g.Cv, vgx, vgy, 0, 2);
            __syncthreads();
        }
        const int k0 = rgb ? g.Kr : g.Kd, nl = rgb ? g.nr : g.nd, in0 = rgb ? 0 : xd_in;
        const float* w = rgb ? wcolour : natural;
        int cur = in0, cur_k = k0;
        for (int l = 0; l < nl; ++l) {
            const bool skip = l > 0 && gen_skip_layer(l - 1, g.skip);
            const int K1 = cur_k, K2 = skip ? k0 : 0;
            f32x16 acc[NT];
            gf_zero<NT>(acc);
            gf_layer<NT>(acc, row, K1, cur, K2, in0, w, g.hidden, n, h);
            const float* b = w + (long)g.hidden * (K1 + K2);
            __syncthreads();
            unsigned* gl = gate + (rgb ? g.nd + l : l) * L.gw;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                unsigned bits = 0;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int j = (r & 3) + 8 * (r >> 2) + 4 * h, m = 32 * t + j;
                    if (m < g.hidden) {
                        const float v = fmaxf(__fadd_rn(acc[t][r], b[m]), 0.0f);
                        row[L.h_off + m] = v;
                        if (v > 0.0f) bits |= 1u << j;
                    }
                }
                bits |= (unsigned)__shfl_xor((int)bits, 32);
                if (h == 0 && t < L.gw) gl[t] = bits;
            }
            __syncthreads();
            w += (long)g.hidden * (K1 + K2) + g.hidden;
            cur = L.h_off; cur_k = g.hidden;
        }
    }

    // ---- the transposed chains: the colour decoder first (its inputs' room is free), the view plane, then the density decoder ----
    float n0 = 0.0f, n1 = 0.0f, n2 = 0.0f;
    if (live) gen_position(sc, x + p * 6, noise, p, n0, n1, n2);
    for (int dec = 1; dec >= 0; --dec) {
        const bool rgb = dec == 1;
        const int k0 = rgb ? g.Kr : g.Kd, nl = rgb ? g.nr : g.nd, Mh = rgb ? 3 : 1, dx = rgb ? 0 : L.xd_off;
        // the layers' offsets: the head follows the last layer
        const float* wh = rgb ? wcolour : natural;
        for (int l = 0; l < nl; ++l) wh += (long)g.hidden * ((l == 0 ? k0 : g.hidden + (gen_skip_layer(l - 1, g.skip) ? k0 : 0)) + 1);
        for (int c = h; c < k0; c += 2) row[dx + c] = 0.0f;       // the gradient of the decoder's input starts at +0.0
        // the head: d_out -> the gradient of the last layer's output, gated by that layer
        {
            f32x16 acc[NT];
            gf_zero<NT>(acc);
            gf_layer_t<NT>(acc, row, L.dout_off + (rgb ? 0 : 3), Mh, wh, g.hidden, 0, g.hidden, n, h);
            __syncthreads();
            gf_store_gated<NT>(acc, row + L.h_off, g.hidden, gate + (rgb ? g.nd + nl - 1 : nl - 1) * L.gw, L.gw, h);
            __syncthreads();
        }
        const float* w = wh;
        for (int l = nl - 1; l >= 0; --l) {
            const bool skip = l > 0 && gen_skip_layer(l - 1, g.skip);
            const int K1 = l == 0 ? k0 : g.hidden, K2 = skip ? k0 : 0, K = K1 + K2;
            w -= (long)g.hidden * (K + 1);
            if (l == 0) {
                gf_input_grad<NT>(row, L.h_off, g.hidden, w, K, 0, K1, dx, n, h);
                __syncthreads();
                break;
            }
            if (skip) gf_input_grad<NT>(row, L.h_off, g.hidden, w, K, K1, K2, dx, n, h);
            f32x16 acc[NT];
            gf_zero<NT>(acc);
            gf_layer_t<NT>(acc, row, L.h_off, g.hidden, w, K, 0, K1, n, h);
            __syncthreads();                              // the layer's last read is done: its input gradient takes dZ's place, gated
            gf_store_gated<NT>(acc, row + L.h_off, g.hidden, gate + (rgb ? g.nd + l - 1 : l - 1) * L.gw, L.gw, h);
            __syncthreads();
        }

        if (rgb) {
            gfb_view_scatter(sc, g, rows, L.ld, L.xd_off, gp, vgx, vgy, slot0 + wave * 32, P, n, h);
        }
    }

    gfb_plane_scatter(sc, g, rows, L.ld, L.xd_off, gp, n0, n1, n2, slot0 + wave * 32, P, n, h);
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
    return gf_for_plan(pl.nt, pl.cls, [&](auto nt, auto cls) {
        constexpr int NT = decltype(nt)::value, LDSF = GF_LDS_FLOATS[decltype(cls)::value];
        return gf_launch_pieces((long)P, pl.waves, [&](long b0, unsigned nb) {
            hipLaunchKernelGGL((generic_backward_fused_kernel<NT, LDSF>), dim3(nb), dim3(64 * pl.waves), 0, (hipStream_t)stream, sc, g, pl, (long)P, b0, x,
                               coord_noise, natural, d_out, gp);
        });
    });
}

}  // extern "C"
