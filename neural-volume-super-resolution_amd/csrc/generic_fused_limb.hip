// generic_fused.hip's one-launch evaluation of ANY decoder geometry with the hidden layers in NVSR_ARITH_F16X2: two round-to-nearest f16 limbs per
// operand under the static scales 2^8 (weights) / 2^4 (activations), three v_mfma_f32_32x32x16_f16 per product block (limb_core.h), f32
// accumulation.  Stage 0 (position, projections, taps, combination rules) and the heads are the f32 kernel's, compiled out of
// generic_fused_core.h: inputs, biases, heads and outputs are f32 as in every arithmetic of the library.
//
// Weights: the packed blob of nvsr_pack_generic_decoder_ext (include/nvsr.h has the layout).  Per hidden layer, in state-dict order,
// fragments [kb][t][limb] of 256 words: word 4 lane + j of lane (m = lane & 31, h = lane >> 5) = {f16 W~[32 t + m][16 kb + 8 h + 2 j] (low half),
// f16 W~[..][.. + 1] (high half)}, W~ = 2^8 W, +0 beyond the matrix, limb 0 = RN(W~), limb 1 = RN(W~ - limb 0): the A operand of one MFMA is one
// global_load_dwordx4 per lane.  Heads and biases are read from the natural blob.
//
// A hidden layer (gfl_layer): k outer over the 16-column K-blocks of [X1 | X2], the layer's output tiles inner.  Lane (n, h) takes the 8 values
// k = 16 kb + 8 h .. + 7 of its point's row (two 16-byte LDS reads wherever the 8 columns lie within one operand and 16-byte aligned; value by
// value across the X1 | X2 seam and in the padded last block), scales them by 2^4 and splits them: xh = RN_f16(16 x), xl = RN_f16(16 x - xh).
// Per tile: Wh xl, Wh xh, Wl xh (limb_w / limb_x) into the tile's accumulator.  The next K-block's fragments and values are fetched in front of
// the current block's MFMAs.  Output: row[h_off + m] = relu(fmaf(acc, 2^-12, b[m])) with a ReLU that KEEPS NaN (y < 0 ? 0 : y).
//
// Rows in LDS (gen_fused_plan(limb = true)): xd_off, h_off and the stride ld are multiples of 4 floats, the hidden activation is padded to a
// multiple of 4 columns (written as zeros), and ld = 4 x an odd number.  Banks: a 16-byte read takes the lanes in four groups of 16, each within one
// half h, whose point indices n cover every residue mod 16 ({0-3, 12-15, 20-27} and {4-11, 16-19, 28-31}).  Lane n reads the 16-byte slot
// (n ld / 4 + c) mod 16 of the 256-byte bank row (c: the group's common column); ld / 4 is odd, hence invertible mod 16: 16 lanes, 16 slots, no
// conflict.  The activations are written 16 bytes per lane as well (registers 4 q .. 4 q + 3 of an accumulator are the consecutive outputs
// m = 8 q + 4 h + 0 .. 3 of point n).
//
// Range: beyond |W| < 255 / |x| < 4094 a high limb is inf and its low limb -inf (or NaN): inf meets -inf, or inf meets 0, and the output is NaN --
// never a finite wrong number; NaN inputs stay NaN.  The heads multiply NaN activations in f32: a NaN row.  A wave that writes a non-finite out
// row ORs 1 into the registered range flag (nvsr_get_range_flag, read when the launch is enqueued) -- whether the NaN was made here or came in
// with the planes, the weights or the points.
#include "generic_fused_limb_core.h"

namespace nvsr {

// packed blob: words of all hidden layers, density decoder first
static int64_t gfl_packed_words(const GenGeom& g) {
    int64_t words = 0;
    for (int dec = 0; dec < 2; ++dec)
        for (int l = 0; l < (dec ? g.nr : g.nd); ++l) words += (int64_t)gfl_kb(gfl_layer_in(g, dec == 1, l)) * gfl_tt(g.hidden) * 2 * 256;
    return words;
}

// one thread per packed word
__global__ __launch_bounds__(256) void generic_pack_limb_kernel(GenGeom g, long words, const float* __restrict__ natural, unsigned* __restrict__ packed) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= words) return;
    const int TT = gfl_tt(g.hidden);
    long w0 = 0, nat = 0;             // first packed word / first natural float of the layer that holds idx
    int K = 0;
    bool found = false;
    for (int dec = 0; dec < 2 && !found; ++dec) {
        const int nl = dec ? g.nr : g.nd;
        for (int l = 0; l < nl; ++l) {
            K = gfl_layer_in(g, dec == 1, l);
            const long lw = (long)gfl_kb(K) * TT * 512;
            if (idx < w0 + lw) { found = true; break; }
            w0 += lw;
            nat += (long)g.hidden * K + g.hidden;
        }
        if (!found) nat += (dec ? 3 : 1) * (long)g.hidden + (dec ? 3 : 1);      // the head between the decoders
    }
    const long r = idx - w0;
    const int frag = (int)(r >> 8), word = (int)(r & 255), lane = word >> 2, j = word & 3;
    const int limb = frag & 1, t = (frag >> 1) % TT, kb = (frag >> 1) / TT;
    const int m = 32 * t + (lane & 31), k = 16 * kb + 8 * (lane >> 5) + 2 * j;
    const float* W = natural + nat;
    float v[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const float ws = (m < g.hidden && k + e < K) ? __fmul_rn(W[(long)m * K + k + e], F16_W_SCALE) : 0.0f;
        const float hi = (float)(_Float16)ws;
        v[e] = limb ? __fsub_rn(ws, hi) : ws;
    }
    packed[idx] = f16_pair(v[1], v[0]);
}

// PHASE (generic_fused_core.h): GF_FULL, or one decoder of a frame in two phases -- GF_DENSITY on every point, GF_COLOUR on the listed points --
// from the same packed blob (the colour decoder's fragments start behind the density layers').  The range flag: GF_DENSITY raises it for a
// non-finite sigma, GF_COLOUR for non-finite colour logits of the listed points only.  GF_DENSITY_LIST: GF_DENSITY on the listed points (the kept
// samples of an occupancy grid); the flag is raised for a non-finite sigma of a listed point only.
template <int NT, int LDSF, int PHASE>
__global__ __launch_bounds__(64 * GF_MAX_WAVES) void generic_decode_fused_limb_kernel(SceneDevN sc, GenGeom g, GenFusedPlan L, long P, long block0,
                                                                                       const float* __restrict__ x, const float* __restrict__ noise,
                                                                                       const float* __restrict__ natural,
                                                                                       const unsigned* __restrict__ packed, float* __restrict__ out,
                                                                                       unsigned* flag, GenFusedList list) {
    __shared__ __attribute__((aligned(16))) float lds[LDSF];
    NVSR_RACE_PROBE_DELAY(lds);      // (probe builds only, nvsr_common.h)
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, n = lane & 31, h = lane >> 5;
    const long slot0 = (block0 + blockIdx.x) * (long)(blockDim.x >> 6) * 32;
    long p;
    bool live;
    if (!gf_point<PHASE>(list, P, slot0, slot0 + wave * 32 + n, p, live)) return;
    float* rows = lds + wave * 32 * L.ld;
    float* row = rows + n * L.ld;

    // ---- stage 0: the decoder inputs, the f32 kernel's (generic_fused_core.h) ----
    const GenFusedRows R = {rows, row, L.ld, L.xd_off};
    float vgx, vgy;
    gf_stage0<PHASE>(sc, g, R, n, h, live, p, x, noise, vgx, vgy);
    const bool raw = g.proj == 2 || g.view == 4;

    // ---- the two decoders ----
    const int TT = gfl_tt(g.hidden), hid4 = (g.hidden + 3) & ~3;
    const float* w = natural;
    const u32x4* wp = reinterpret_cast<const u32x4*>(packed);
    bool bad = false;
    if (PHASE == GF_COLOUR) {
        w += gf_density_floats(g);
        for (int l = 0; l < g.nd; ++l) wp += (long)gfl_kb(gfl_layer_in(g, false, l)) * TT * 128;
    }
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
            gfl_layer<NT>(acc, row, K1, cur, K2, in0, wp, TT, lane, h);
            const float* b = w + (long)g.hidden * (K1 + K2);
            __syncthreads();                              // the layer's last read is done: its output takes the input's place
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int m0 = 32 * t + 8 * q + 4 * h;
                    if (t < TT && m0 < hid4) {
                        f32x4 y;
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const float s = m0 + i < g.hidden ? fmaf(acc[t][4 * q + i], GFL_UNSCALE, b[m0 + i]) : 0.0f;
                            y[i] = s < 0.0f ? 0.0f : s;   // (keeps NaN: fmaxf would answer 0, a finite wrong number, to an operand beyond the range)
                        }
                        *reinterpret_cast<f32x4*>(row + L.h_off + m0) = y;
                    }
                }
            __syncthreads();
            w += (long)g.hidden * (K1 + K2) + g.hidden;
            wp += (long)gfl_kb(K1 + K2) * TT * 128;
            cur = L.h_off; cur_k = g.hidden;
        }
        const int M = rgb ? 3 : 1;                        // fc_rgb -> out[:, 0:3], fc_alpha -> out[:, 3]: f32 on the f32 activations
        float o[3];
        gf_head(row, cur_k, cur, w, rgb, n, h, o);
        if (live && h == 0) {
            if (gf_density_only(PHASE)) {                 // the whole row: the colour logits of a sample the colour phase leaves out are +0
                f32x4 row4 = {0.0f, 0.0f, 0.0f, o[0]};
                *reinterpret_cast<f32x4*>(out + p * 4) = row4;
                bad = bad || !(fabsf(o[0]) <= 3.0e38f);
            } else {
#pragma unroll
                for (int r = 0; r < 3; ++r)
                    if (r < M) {
                        out[p * 4 + (rgb ? 0 : 3) + r] = o[r];
                        bad = bad || !(fabsf(o[r]) <= 3.0e38f);
                    }
            }
        }
        w += (long)M * g.hidden + M;
    }
    // range flag of the f16 limbs (nvsr.h: nvsr_set_range_flag): one atomic per wave that wrote a non-finite row
    if (flag && __any(bad) && lane == 0) __hip_atomic_fetch_or(flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// one entry for the four phases, in either arithmetic: the checks (gf_check_entry), then the phase's launch -- over P points or over
// list.max_count slots of the list, whose workgroups beyond the count return at once
int gen_fused_arith_phase(int phase, const nvsr_scene_ext* scene, const nvsr_decoder_geometry* geometry, const float* natural, const float* packed,
                          int64_t P, const float* x, const float* coord_noise, float* out, const GenFusedList& list, int arith, nvsr_stream_t stream) {
    if (arith != NVSR_ARITH_F32 && arith != NVSR_ARITH_F16X2) return NVSR_ERR_SHAPE;      // by name only: no process default, no one-limb or bf16 mode here
    const bool limb = arith == NVSR_ARITH_F16X2;
    GenGeom g;
    GenFusedPlan pl;
    SceneDevN sc;
    const int e = gf_check_entry(scene, geometry, [&](const GenGeom& gg) { return gen_fused_plan(gg, &pl, limb); },
                                 natural && (!limb || packed) && x && out, phase, list, P, &g, &sc);
    if (e != GF_LAUNCH) return e;
    hipStream_t s = (hipStream_t)stream;
    if (!limb) return gen_fused_f32_phase(phase, sc, g, pl, (long)P, x, coord_noise, natural, out, list, s);
    unsigned* flag = nvsr_get_range_flag();
    return gf_for_phase(phase, [&](auto ph) {
        return gf_for_plan(pl.nt, pl.cls, [&](auto nt, auto cls) {
            constexpr int PHASE = decltype(ph)::value, NT = decltype(nt)::value, LDSF = GF_LDS_FLOATS[decltype(cls)::value];
            return gf_launch_pieces(gf_listed(PHASE) ? list.max_count : (long)P, pl.waves, [&](long b0, unsigned nb) {
                hipLaunchKernelGGL((generic_decode_fused_limb_kernel<NT, LDSF, PHASE>), dim3(nb), dim3(64 * pl.waves), 0, s, sc, g, pl, (long)P, b0, x,
                                   coord_noise, natural, reinterpret_cast<const unsigned*>(packed), out, flag, list);
            });
        });
    });
}

}  // namespace nvsr

using namespace nvsr;

extern "C" {

int64_t nvsr_generic_packed_floats_ext(const nvsr_decoder_geometry* geometry, int num_position_planes) {
    GenGeom g;
    if (int e = gen_resolve(geometry, &g, num_position_planes)) return -e;
    return gfl_packed_words(g);
}

int nvsr_pack_generic_decoder_ext(const nvsr_decoder_geometry* geometry, int num_position_planes, const float* natural, float* packed,
                                  nvsr_stream_t stream) {
    GenGeom g;
    if (int e = gen_resolve(geometry, &g, num_position_planes)) return e;
    if (!natural || !packed) return NVSR_ERR_NULL;
    const int64_t words = gfl_packed_words(g);
    hipLaunchKernelGGL(generic_pack_limb_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, (hipStream_t)stream, g, (long)words, natural,
                       reinterpret_cast<unsigned*>(packed));
    return NVSR_CHECK_LAUNCH();
}

int nvsr_generic_fused_supported_arith(const nvsr_decoder_geometry* geometry, int num_position_planes, int arith) {
    return gf_supported(geometry, num_position_planes, [&](const GenGeom& g) {
        GenFusedPlan pl;
        return gen_fused_plan_arith(g, &pl, arith);
    });
}

int nvsr_generic_decode_fused_arith_ext(const nvsr_scene_ext* scene, const nvsr_decoder_geometry* geometry, const float* natural, const float* packed,
                                        int64_t P, const float* x, const float* coord_noise, float* out, int arith, nvsr_stream_t stream) {
    return gen_fused_arith_phase(GF_FULL, scene, geometry, natural, packed, P, x, coord_noise, out, GenFusedList{nullptr, nullptr, 0}, arith, stream);
}

int nvsr_generic_decode_fused_density_arith_ext(const nvsr_scene_ext* scene, const nvsr_decoder_geometry* geometry, const float* natural,
                                                const float* packed, int64_t P, const float* x, const float* coord_noise, float* raw_out, int arith,
                                                nvsr_stream_t stream) {
    return gen_fused_arith_phase(GF_DENSITY, scene, geometry, natural, packed, P, x, coord_noise, raw_out, GenFusedList{nullptr, nullptr, 0}, arith,
                                 stream);
}

int nvsr_generic_decode_fused_colour_arith_ext(const nvsr_scene_ext* scene, const nvsr_decoder_geometry* geometry, const float* natural,
                                               const float* packed, int64_t P, const float* x, const float* coord_noise, const int32_t* index,
                                               const int32_t* count_dev, int64_t max_count, float* raw_inout, int arith, nvsr_stream_t stream) {
    return gen_fused_arith_phase(GF_COLOUR, scene, geometry, natural, packed, P, x, coord_noise, raw_inout, GenFusedList{index, count_dev, (long)max_count},
                                 arith, stream);
}

int nvsr_generic_decode_fused_density_list_arith_ext(const nvsr_scene_ext* scene, const nvsr_decoder_geometry* geometry, const float* natural,
                                                     const float* packed, int64_t P, const float* x, const float* coord_noise, const int32_t* index,
                                                     const int32_t* count_dev, int64_t max_count, float* raw_inout, int arith, nvsr_stream_t stream) {
    return gen_fused_arith_phase(GF_DENSITY_LIST, scene, geometry, natural, packed, P, x, coord_noise, raw_inout,
                                 GenFusedList{index, count_dev, (long)max_count}, arith, stream);
}

}  // extern "C"
