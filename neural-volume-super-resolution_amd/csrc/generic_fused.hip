// TwoDimPlanesModel.forward for ANY decoder geometry, evaluation only, in ONE launch: the fused twin of generic.hip's layer-by-layer forward.
//
// Reference: models.py:381-421 (see generic.hip for the layer lists and the combination rules; both files compile them out of generic_core.h).
//
// The contract is the layered route's BITS.  There, every output of a layer is one v_mfma_f32_32x32x2_f32 chain from +0.0 over the k pairs
// (2s, 2s + 1) of the concatenated input [X1 | X2] in ascending order, up to K rounded up to 32 with zero operands, followed by
// __fadd_rn(acc, b[m]) and fmaxf(., 0).  An MFMA output depends on its own row of A and its own column of B only, so the same instruction on
// the same operand pairs in the same order gives the same bits wherever the tile sits: gf_layer (generic_fused_core.h) is that chain, and the only place it is
// written.  generic_fused_limb.hip is this kernel with the hidden layers' product swapped for two f16 limbs; stage 0 and the heads are shared.
//
// generic_decode_fused_kernel: a workgroup of 1 .. 4 waves, 32 points per wave; a wave only ever touches its own 32 rows of LDS.
//   row of a point (GenFusedPlan::ld floats, 2 x an odd number: the 64 lanes (point n, k half h) of a B-operand read hit 64 different banks):
//     [0, Kr)           the colour decoder's input Xr -- of which the density decoder's input Xd is the first Kd columns whenever the position
//                       features are concatenated ('concat'); under 'sum' / 'avg' / 'mult' view features Xd (= Kr columns) stands here first
//                       and becomes Xr in place once the density decoder is done
//     [xd_off, + Kd)    Xd under 'sum' / 'avg' position features with 'concat_pos': made from the raw per-plane features of Xr
//     [h_off, + hidden) the current layer's input / output
//   stage 0   per (point, plane): position, projection (atan2f for the view plane) once per point, the taps once per (point, plane) -- two
//             points at a time, 32 lanes each over the channels, so a tap's channels are one contiguous read
//   layers    k outer, the layer's NT 32-row output tiles inner: one LDS read feeds NT independent MFMA chains, the whole layer's
//             accumulators are held, and the output replaces the input in place behind the last read.  Weights and biases come straight
//             from the natural blob (L2 / L1 resident: a few MB at most).
//   heads     out[p][3] behind the density decoder, out[p][0:3] behind the colour decoder
// Capacity (gen_fused_plan, documented in include/nvsr.h): hidden <= 256 (NT <= 8: 128 accumulator registers), max(Kd, Kr) <= 512, 32 rows in
// 160 KB.  The LDS array is static (40 / 80 / 160 KB instantiations, so that small geometries keep several workgroups per CU); the plan takes
// the size class that puts the most waves on a CU.
#include "generic_fused_core.h"

namespace nvsr {

// PHASE (generic_fused_core.h): GF_FULL is the kernel above; GF_DENSITY / GF_COLOUR are its two halves for a frame in two phases -- the density
// decoder on every point, then the colour decoder on the listed points (`list`, not read by the other phases) -- out of the same code: the same
// rows, the same chains, the same bits.  GF_DENSITY_LIST is GF_DENSITY on the listed points: the kept samples of an occupancy grid.
template <int NT, int LDSF, int PHASE>
__global__ __launch_bounds__(64 * GF_MAX_WAVES) void generic_decode_fused_kernel(SceneDevN sc, GenGeom g, GenFusedPlan L, long P, long block0,
                                                                                  const float* __restrict__ x, const float* __restrict__ noise,
                                                                                  const float* __restrict__ natural, float* __restrict__ out,
                                                                                  GenFusedList list) {
    __shared__ __attribute__((aligned(16))) float lds[LDSF];
    NVSR_RACE_PROBE_DELAY(lds);      // (probe builds only, nvsr_common.h)
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, n = lane & 31, h = lane >> 5;
    const long slot0 = (block0 + blockIdx.x) * (long)(blockDim.x >> 6) * 32;
    long p;
    bool live;
    if (!gf_point<PHASE>(list, P, slot0, slot0 + wave * 32 + n, p, live)) return;
    float* rows = lds + wave * 32 * L.ld;       // this wave's 32 points
    float* row = rows + n * L.ld;               // this lane's point (shared by the lane's two halves)

    // ---- stage 0: the decoder inputs (generic_fused_core.h) ----
    const GenFusedRows R = {rows, row, L.ld, L.xd_off};
    float vgx, vgy;
    gf_stage0<PHASE>(sc, g, R, n, h, live, p, x, noise, vgx, vgy);
    const bool raw = g.proj == 2 || g.view == 4;

    // ---- the two decoders (one of them in a phase) ----
    const float* w = natural;
    if (PHASE == GF_COLOUR) w += gf_density_floats(g);
    for (int dec = PHASE == GF_COLOUR ? 1 : 0; dec < (gf_density_only(PHASE) ? 1 : 2); ++dec) {
        const bool rgb = dec == 1;
        if (rgb && !raw) {                                // Xd -> Xr in place: combine_all_planes 'sum' / 'avg' / 'mult'
            gf_plane_features(sc, g, R, n, h, g.np, g.Cv, vgx, vgy, 0, 2);
            __syncthreads();
        }
        const int k0 = rgb ? g.Kr : g.Kd, nl = rgb ? g.nr : g.nd, in0 = rgb ? 0 : L.xd_off;
        int cur = in0, cur_k = k0;
        for (int l = 0; l < nl; ++l) {
            const bool skip = l > 0 && gen_skip_layer(l - 1, g.skip);       // x = cat(x, input) in front of this layer (models.py:397-399)
            const int K1 = cur_k, K2 = skip ? k0 : 0;
            f32x16 acc[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
            gf_layer<NT>(acc, row, K1, cur, K2, in0, w, g.hidden, n, h);
            const float* b = w + (long)g.hidden * (K1 + K2);
            __syncthreads();                              // the layer's last read is done: its output takes the input's place
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int m = 32 * t + (r & 3) + 8 * (r >> 2) + 4 * h;
                    if (m < g.hidden) row[L.h_off + m] = fmaxf(__fadd_rn(acc[t][r], b[m]), 0.0f);
                }
            __syncthreads();
            w += (long)g.hidden * (K1 + K2) + g.hidden;
            cur = L.h_off; cur_k = g.hidden;
        }
        const int M = rgb ? 3 : 1;                        // fc_rgb -> out[:, 0:3], fc_alpha -> out[:, 3]
        f32x16 acc[1];
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[0][r] = 0.0f;
        gf_layer<1>(acc, row, cur_k, cur, 0, cur, w, M, n, h);
        const float* b = w + (long)M * g.hidden;
        if (live && h == 0) {
            if (gf_density_only(PHASE)) {                 // the whole row: the colour logits of a sample the colour phase leaves out are +0
                f32x4 o = {0.0f, 0.0f, 0.0f, __fadd_rn(acc[0][0], b[0])};
                *reinterpret_cast<f32x4*>(out + p * 4) = o;
            } else {
#pragma unroll
                for (int r = 0; r < 3; ++r)
                    if (r < M) out[p * 4 + (rgb ? 0 : 3) + r] = __fadd_rn(acc[0][r], b[r]);
            }
        }
        w += (long)M * g.hidden + M;
    }
}

// a phase's launch: it covers P points (GF_FULL, GF_DENSITY) or list.max_count slots of the list (GF_COLOUR, GF_DENSITY_LIST: workgroups beyond
// the count return at once)
int gen_fused_f32_phase(int phase, const SceneDevN& sc, const GenGeom& g, const GenFusedPlan& pl, long P, const float* x, const float* noise,
                        const float* natural, float* out, const GenFusedList& list, hipStream_t stream) {
    return gf_for_phase(phase, [&](auto ph) {
        return gf_for_plan(pl.nt, pl.cls, [&](auto nt, auto cls) {
            constexpr int PHASE = decltype(ph)::value, NT = decltype(nt)::value, LDSF = GF_LDS_FLOATS[decltype(cls)::value];
            return gf_launch_pieces(gf_listed(PHASE) ? list.max_count : P, pl.waves, [&](long b0, unsigned nb) {
                hipLaunchKernelGGL((generic_decode_fused_kernel<NT, LDSF, PHASE>), dim3(nb), dim3(64 * pl.waves), 0, stream, sc, g, pl, P, b0, x, noise,
                                   natural, out, list);
            });
        });
    });
}

}  // namespace nvsr

using namespace nvsr;

extern "C" {

int nvsr_generic_fused_supported(const nvsr_decoder_geometry* geometry, int num_position_planes) {
    return nvsr_generic_fused_supported_arith(geometry, num_position_planes, NVSR_ARITH_F32);
}

int nvsr_generic_decode_fused_ext(const nvsr_scene_ext* scene, const nvsr_decoder_geometry* geometry, const float* natural, int64_t P, const float* x,
                                  const float* coord_noise, float* out, nvsr_stream_t stream) {
    return gen_fused_arith_phase(GF_FULL, scene, geometry, natural, nullptr, P, x, coord_noise, out, GenFusedList{nullptr, nullptr, 0}, NVSR_ARITH_F32, stream);
}

}  // extern "C"
