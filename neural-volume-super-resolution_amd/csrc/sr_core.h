// Host-side helpers shared by sr.hip (forward) and sr_bwd.hip (backward) -- not part of the public ABI.
#pragma once
#include <math.h>
#include <stdlib.h>

#include <initializer_list>

#include "nvsr_common.h"

namespace nvsr {

// Source position of output index `o` of F.interpolate(mode='bilinear', scale_factor=sf) along an axis of `in` texels (ATen UpSample.h:
// area_pixel_compute_source_index + guard_index_and_lambda): align_corners=True maps the first / last output onto the first / last input,
// src = o (in - 1) / (out - 1); False maps pixel centres, src = (o + 0.5) / sf - 0.5, clamped at 0.  -> first tap i0, offset of the second
// tap (0 at the last texel), weight of the second tap.
struct BilinearTap { int i0, step; float w1; };
__device__ __forceinline__ BilinearTap bilinear_tap(int o, int in, int out, int sf, int align) {
    float src;
    if (align) src = (out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.0f) * (float)o;
    else {
        src = __fsub_rn(__fmul_rn((float)(1.0 / (double)sf), (float)o + 0.5f), 0.5f);
        if (src < 0.0f) src = 0.0f;
    }
    BilinearTap t;
    t.i0 = min((int)src, in - 1);
    t.step = t.i0 < in - 1 ? 1 : 0;
    t.w1 = fminf(fmaxf(src - (float)t.i0, 0.0f), 1.0f);
    return t;
}
// The same for mode='bicubic' (UpSample.h: area_pixel_compute_source_index with cubic = true -- no clamp at 0 --, the four taps floor - 1 ..
// floor + 2 clamped to the axis, cubic convolution weights with A = -0.75)
struct CubicTap { int i[4]; float w[4]; };
__device__ __forceinline__ CubicTap cubic_tap(int o, int in, int out, int sf, int align) {
    float src;
    if (align) src = (out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.0f) * (float)o;
    else src = __fsub_rn(__fmul_rn((float)(1.0 / (double)sf), (float)o + 0.5f), 0.5f);
    const float fl = floorf(src);
    const float t = fminf(fmaxf(src - fl, 0.0f), 1.0f);
    const float A = -0.75f;
    const float x0 = t + 1.0f, x1 = t, x2 = 1.0f - t, x3 = x2 + 1.0f;
    CubicTap c;
    c.w[0] = ((A * x0 - 5.0f * A) * x0 + 8.0f * A) * x0 - 4.0f * A;
    c.w[1] = ((A + 2.0f) * x1 - (A + 3.0f)) * x1 * x1 + 1.0f;
    c.w[2] = ((A + 2.0f) * x2 - (A + 3.0f)) * x2 * x2 + 1.0f;
    c.w[3] = ((A * x3 - 5.0f * A) * x3 + 8.0f * A) * x3 - 4.0f * A;
    const int i0 = (int)fl;
#pragma unroll
    for (int k = 0; k < 4; ++k) c.i[k] = min(max(i0 - 1 + k, 0), in - 1);
    return c;
}
// process-wide: align_corners and mode of PlanesSR's residual up-sampling (sr.hip: nvsr_set_sr_align_corners, nvsr_set_sr_plane_interp)
int sr_align_corners();
int sr_bicubic();


// f16-limb data / weight gradients of the SR network: the power of two that puts the largest |dy| of a gradient tensor (its bits in
// `absmax_bits`, absmax_kernel) into [2^12, 2^13).  Exponent field clamped to 254 (a tensor whose largest magnitude is below 2^-115 would
// otherwise ask for a scale beyond the largest finite power of two); an all-zero or non-finite tensor is not scaled.
__host__ __device__ inline float f16_gradient_scale(unsigned absmax_bits) {
    const int e = (int)((absmax_bits >> 23) & 0xffu);
    if (e == 0 || e == 255) return 1.0f;
    const int s = 254 + 12 - e;
    const unsigned bits = (unsigned)(s > 254 ? 254 : s) << 23;
#if defined(__HIP_DEVICE_COMPILE__)
    return __uint_as_float(bits);
#else
    float f; __builtin_memcpy(&f, &bits, 4); return f;
#endif
}


constexpr int K_PER_CHUNK = 18;                 // MFMA k-steps per 4-channel chunk (36 k / 2)
constexpr int FRAG_FLOATS = K_PER_CHUNK * 64;   // 1152 floats per (chunk, co-block)

// EPI_MASK_SCALE / EPI_ADD_CENTER are the two fused epilogues of a residual block's backward (sr_bwd.hip)
enum ConvEpilogue { EPI_NONE = 0, EPI_RELU = 1, EPI_RESIDUAL = 2, EPI_PIXEL_SHUFFLE = 3, EPI_MASK_SCALE = 4, EPI_ADD_CENTER = 5 };

struct ConvLayer { int Cin, Cout; };

inline int conv_ncb(int Cout) { return (Cout + 63) / 64 * 2; }
inline int conv_nchunks(int Cin) { return (Cin + 3) / 4; }
inline int64_t conv_packed_f32_floats(int Cin, int Cout) { return (int64_t)conv_nchunks(Cin) * conv_ncb(Cout) * FRAG_FLOATS; }
// bf16-limb fragments (sr.hip, conv3x3_limb_kernel): layers with Cin % 16 == 0 and a multiple of 256 (or at most 64) output channels carry, behind the f32
// fragments, [chunk of 16 input channels][co-block][tap 0..8][limb 0..2][lane][4 words] = 6912 words per (chunk, co-block)
constexpr int CL_FRAG_WORDS = 9 * 3 * 256;
inline bool conv_limb_eligible(int Cin, int Cout) { return Cin % 16 == 0 && (conv_ncb(Cout) % 8 == 0 || conv_ncb(Cout) == 2); }
inline int64_t conv_packed_limb_words(int Cin, int Cout) {
    return conv_limb_eligible(Cin, Cout) ? (int64_t)(Cin / 16) * conv_ncb(Cout) * CL_FRAG_WORDS : 0;
}
// bf16-limb fragments for v_mfma_f32_16x16x32_bf16 (sr.hip, conv3x3_limb16_kernel; round 3): layers with Cin % 32 == 0 and Cout % 128 == 0 carry a
// third region, [chunk of 32 input channels][16-channel co-block][tap 0..8][limb 0..2][lane][4 words]; lane (co = 16 cb + (l & 15),
// g = l >> 4) holds input channels 32 chunk + 8 g + 0..7 as bf16 pairs
inline bool conv_limb16_eligible(int Cin, int Cout) { return Cin % 32 == 0 && Cout % 128 == 0; }
inline int64_t conv_packed_limb16_words(int Cin, int Cout) {
    return conv_limb16_eligible(Cin, Cout) ? (int64_t)(Cin / 32) * (Cout / 16) * CL_FRAG_WORDS : 0;
}
// the same fragments in the 2-f16-limb arithmetic (limb_core.h: W 2^8 as hi + lo, round to nearest), a fourth region: [..][limb 0..1][lane][4 words]
inline int64_t conv_packed_f16_words(int Cin, int Cout) {
    return conv_limb16_eligible(Cin, Cout) ? (int64_t)(Cin / 32) * (Cout / 16) * (9 * 2 * 256) : 0;
}
inline int64_t conv_packed_floats(int Cin, int Cout) {
    return conv_packed_f32_floats(Cin, Cout) + conv_packed_limb_words(Cin, Cout) + conv_packed_limb16_words(Cin, Cout) + conv_packed_f16_words(Cin, Cout);
}
// the arithmetics of the convolutions: the decoder's three and NVSR_ARITH_F16 (one f16 limb; nvsr.h)
inline bool conv_arith_ok(int arith) { return arith == NVSR_ARITH_F32 || arith == NVSR_ARITH_F16 || arith == NVSR_ARITH_F16X2 || arith == NVSR_ARITH_BF16X3; }
// f16 limbs, one or two: the scaled operands, the gradient tensors' magnitude words, the range flag
inline bool conv_arith_f16(int arith) { return arith == NVSR_ARITH_F16X2 || arith == NVSR_ARITH_F16; }

// ---- the route of one convolution launch: which kernel, on which grid, reading which region of the packed blob ---------------------------------
// Compile-time defaults of the route (the kernels themselves are in sr.hip)
#ifndef CV16_WAVES
#define CV16_WAVES 4
#endif
#ifndef CV16_ROWCOST3
#define CV16_ROWCOST3 1.05   // cost of an output row in a 3-row / 2-row tile of conv3x3_limb16_kernel relative to a 4-row tile (measured: 4.68 / 4.47 ms, 4.93 / 4.47 ms)
#define CV16_ROWCOST2 1.10
#endif
#ifndef CV16_ROWCOST6
#define CV16_ROWCOST6 0.97   // f16 limbs: cost of an output row in a 6-row tile relative to a 4-row tile (measured on a 1024^2 layer: 2.547 / 2.636 ms)
#endif
#ifndef CV_USE_16X16X32
#define CV_USE_16X16X32 1   // limb layers with Cin % 32 == 0 and Cout % 128 == 0 (all of EDSR's trunk and up-sampling convolutions): 1 = conv3x3_limb16_kernel
#endif
#ifndef CV_WIDE_ROWS8
#define CV_WIDE_ROWS8 0     // wide layers: 1 = one output block x 8 rows per wave, 0 = two output blocks x 2..4 rows (equally fast; see conv3x3_limb_kernel)
#endif
constexpr int CONV_RAGGED_MAX = 4;      // planes of a ragged batch (ConvRagged below)
enum ConvFamily {
    CONV_LIMB_NARROW,      // conv3x3_limb_kernel<2, 1>: 64 output channels, 4 waves x 2 rows
    CONV_LIMB16,           // conv3x3_limb16_kernel<pb, CV16_WAVES, limbs>: v_mfma 16x16x32, 2 / 3 / 4 (/ 6, f16 limbs) rows
    CONV_LIMB_WIDE8,       // conv3x3_limb_kernel<8, 4, 1>: 128 output channels x 8 rows
    CONV_LIMB_WIDE,        // conv3x3_limb_kernel<pb>: 256 output channels x 2..4 rows
    CONV_F32_WIDE,         // conv3x3_kernel<4, 1, pb>: exact f32, 256 output channels x 2..4 rows
    CONV_F32_NARROW,       // conv3x3_kernel<1, 8>: exact f32, 64 output channels x 32 rows
    CONV_PLANEWISE         // a ragged batch of a layer no limb kernel is eligible for: plane after plane on the exact-f32 kernels
};
// sizes of a launch as the kernels see them (the virtual border included): `batch` planes of H x W, or n > 0 planes of rH[b] x rW[b]
struct ConvShape { int H = 0, W = 0, batch = 1, n = 0; int rH[CONV_RAGGED_MAX] = {0, 0, 0, 0}, rW[CONV_RAGGED_MAX] = {0, 0, 0, 0}; };
struct ConvRoute {
    int family = CONV_F32_NARROW;
    int limbs = 0;             // 3 bf16, 2 / 1 f16, 0 exact f32
    int pb = 0;                // the kernel's PB (rows per wave or tile, see the family)
    int tile_rows = 0;         // output rows per workgroup tile
    int ncg = 0;               // groups of output channels in the grid
    int region = 0;            // region of the packed blob the kernel reads: 0 f32, 1 bf16 limbs 32x32x16, 2 bf16 limbs 16x16x32, 3 f16 limbs 16x16x32
    bool in_scale = false;     // f16 data gradient: the kernel scales its input by the tensor's magnitude word (ConvExec::in_absmax)
    unsigned grid[3] = {1, 1, 1}, block = 256;
    unsigned tile0[CONV_RAGGED_MAX + 1] = {0, 0, 0, 0, 0};       // ConvRagged::tile0 of a ragged launch
    long tiles = 0;            // workgroup tiles the cost model priced for tile_rows (= the grid's)
};
// Rows per tile with the cheapest launch: rounds of the chip's `slots` workgroup slots x rows x the measured cost of a row in such a tile
// (row_cost, relative to a 4-row tile); a last round of at most half the slots has every CU to itself and costs `half_round` of a full one.
// Candidates are tried in the order given, the first of equal costs wins.
template <class RowCost, class TilesOf>
inline int choose_rows(std::initializer_list<int> candidates, RowCost row_cost, long slots, double half_round, TilesOf tiles_of) {
    int best = 0;
    double best_cost = 1e300;
    for (int pb : candidates) {
        const long tiles = tiles_of(pb), full = tiles / slots, rest = tiles % slots;
        const double rounds = (double)full + (rest == 0 ? 0.0 : rest <= slots / 2 ? half_round : 1.0);
        const double cost = rounds * pb * row_cost(pb);
        if (cost < best_cost) { best_cost = cost; best = pb; }
    }
    return best;
}
// NVSR_CV16_ROWS=2|3|4|6 (environment, read once): force the row count of every 16x16x32 launch (tools: per-layer comparison of the variants)
inline int conv_cv16_rows_env() {
    static const int forced = [] { const char* e = getenv("NVSR_CV16_ROWS"); return e ? atoi(e) : 0; }();
    return forced;
}
// arith: resolved (conv_resolve_arith).  rows = ConvExec::rows: 0 = the cost model; 2 / 3 / 4 = rows per tile of the wide kernels; 8 = the 8-row wide
// limb kernel; 16 = the 16x16x32 kernel with its own choice, 18 / 19 / 20 / 22 = that kernel with 2 / 3 / 4 / 6 rows.
// NVSR_ARITH_F16X2: the 16x16x32 kernel on 2 f16 limbs -- forward convolutions and data gradients (pad != 0 or a backward epilogue: the input
// scaled by its tensor's magnitude) of the wide layers; the narrow input / output layers stay on 3 bf16 limbs.  NVSR_ARITH_F16: the same launches
// with the high limb alone.
inline int conv_route(int Cin, int Cout, const ConvShape& s, int pad, int epilogue, int arith, int rows, ConvRoute* r) {
    if (!conv_arith_ok(arith)) return NVSR_ERR_SHAPE;
    if (rows != 0 && (rows < 2 || rows > 4) && rows != 8 && rows != 16 && !(rows >= 18 && rows <= 20) && rows != 22) return NVSR_ERR_SHAPE;
    if (s.n < 0 || s.n > CONV_RAGGED_MAX || (s.n && arith == NVSR_ARITH_F32)) return NVSR_ERR_SHAPE;
    for (int b = 0; b < s.n; ++b)
        if (s.rH[b] < 3 || s.rW[b] < 3) return NVSR_ERR_SHAPE;
    if (!s.n && (s.H < 3 || s.W < 3 || s.batch < 1 || s.batch > 1024)) return NVSR_ERR_SHAPE;
    const bool limbs = arith != NVSR_ARITH_F32, f16 = conv_arith_f16(arith);
    const bool wl = limbs && conv_limb_eligible(Cin, Cout), w16 = limbs && conv_limb16_eligible(Cin, Cout);
    const int ncb = conv_ncb(Cout);
    *r = ConvRoute{};
    // tiles of a launch with `tr` output rows per tile and 32-pixel column chunks: all planes of a ragged batch, or batch x the one size
    auto tiles_of = [&](int tr) -> long {
        if (!s.n) return (long)((s.W - 2 + 31) / 32) * ((s.H - 2 + tr - 1) / tr) * r->ncg * s.batch;
        long t = 0;
        for (int b = 0; b < s.n; ++b) t += (long)((s.rW[b] - 2 + 31) / 32) * ((s.rH[b] - 2 + tr - 1) / tr) * r->ncg;
        return t;
    };
    if (wl && ncb == 2) {
        r->family = CONV_LIMB_NARROW; r->limbs = 3; r->region = 1; r->ncg = 1; r->pb = 2; r->tile_rows = 8;
    } else if (rows >= 16 && !w16) {
        return NVSR_ERR_SHAPE;                                          // (eligible limb layers only)
    } else if (w16 && (rows >= 16 || (rows == 0 && CV_USE_16X16X32))) {
        r->family = CONV_LIMB16; r->limbs = arith == NVSR_ARITH_F16 ? 1 : f16 ? 2 : 3; r->region = f16 ? 3 : 2;       // (F16 reads limb 0 of F16X2's region)
        r->ncg = Cout / (32 * CV16_WAVES); r->block = 64 * CV16_WAVES;
        r->in_scale = f16 && (pad != 0 || epilogue == EPI_MASK_SCALE || epilogue == EPI_ADD_CENTER);
        // f16 limbs: a 6-row tile too (96 accumulator registers, 2 x 35 KB of LDS: still two workgroups per CU) -- with half the MFMAs per weight
        // fragment the stream of fragments out of L2 (4 KB per wave and tap) is what a row costs, and 6 rows amortise it over 1.5 x the MFMAs.
        // Row costs: tools/conv_time.py rows 18 / 19 / 20 on a layer of full rounds; a last round of at most 256 tiles: ~0.62 of a round's time
        auto row_cost = [](int pb) { return pb == 6 ? CV16_ROWCOST6 : pb == 4 ? 1.0 : pb == 3 ? CV16_ROWCOST3 : CV16_ROWCOST2; };
        constexpr long slots = CV16_WAVES == 4 ? 512 : 256;
        constexpr double half_round = CV16_WAVES == 4 ? 0.62 : 1.0;
        r->pb = f16 ? choose_rows({6, 4, 3, 2}, row_cost, slots, half_round, tiles_of) : choose_rows({4, 3, 2}, row_cost, slots, half_round, tiles_of);
        if (rows >= 18) r->pb = rows - 16;
        if (r->pb == 6 && !f16) return NVSR_ERR_SHAPE;
        const int forced = conv_cv16_rows_env();
        if (((forced >= 2 && forced <= 4) || (forced == 6 && f16)) && rows < 18) r->pb = forced;
        r->tile_rows = r->pb;
    } else if (rows == 8 && !wl) {
        return NVSR_ERR_SHAPE;                                          // (only the wide limb kernel has it)
    } else if (wl && (rows == 8 || (rows == 0 && CV_WIDE_ROWS8))) {
        r->family = CONV_LIMB_WIDE8; r->limbs = 3; r->region = 1; r->ncg = ncb / 4; r->pb = r->tile_rows = 8;
    } else if (wl) {
        // 512 workgroup slots; per row of a tile, 3-row tiles cost 1.13 x and 2-row tiles 1.39 x a 4-row tile's (their weight stream per MFMA is 4/3, 2 x)
        r->family = CONV_LIMB_WIDE; r->limbs = 3; r->region = 1; r->ncg = ncb / 8;
        r->pb = rows ? rows : choose_rows({4, 3, 2}, [](int pb) { return pb == 4 ? 1.0 : pb == 3 ? 1.13 : 1.39; }, 512, 0.62, tiles_of);
        r->tile_rows = r->pb;
    } else if (s.n) {
        r->family = CONV_PLANEWISE;
        return NVSR_OK;
    } else if (ncb >= 8 && ncb % 8 == 0) {
        // two independent 4-wave workgroups per CU (2 x 80 KB of LDS): one's chunk barrier is covered by the other's MFMAs.  All tiles of a launch take
        // the same time: whole rounds of the 512 slots; fewer rows amortise the weight reads a little worse, +3 % per row dropped
        r->family = CONV_F32_WIDE; r->ncg = ncb / 8;
        r->pb = rows ? rows : choose_rows({4, 3, 2}, [](int pb) { return 1.0 + 0.03 * (4 - pb); }, 512, 1.0, tiles_of);
        r->tile_rows = r->pb;
    } else {
        r->family = CONV_F32_NARROW; r->ncg = ncb / 2; r->tile_rows = 32; r->block = 512;
    }
    r->tiles = tiles_of(r->tile_rows);
    if (!s.n) {
        r->grid[0] = (unsigned)((s.W - 2 + 31) / 32); r->grid[1] = (unsigned)((s.H - 2 + r->tile_rows - 1) / r->tile_rows); r->grid[2] = (unsigned)(r->ncg * s.batch);
        return NVSR_OK;
    }
    // ragged launch: a one-dimensional grid over the planes' tiles, plane after plane (no empty tiles); planes that do not exist start at the
    // end of the 32-bit range (tile0[n] included unless all CONV_RAGGED_MAX planes exist)
    unsigned t = 0;
    for (int b = 0; b <= CONV_RAGGED_MAX; ++b) {
        r->tile0[b] = b < s.n || (b == s.n && b == CONV_RAGGED_MAX) ? t : 0xffffffffu;
        if (b < s.n) t += (unsigned)((s.rW[b] - 2 + 31) / 32) * (unsigned)((s.rH[b] - 2 + r->tile_rows - 1) / r->tile_rows) * (unsigned)r->ncg;
    }
    r->grid[0] = t;
    return NVSR_OK;
}
// Fragment kinds of a packed layer (bit k = region k of the blob) that launch_conv (sr.hip) READS for a launch in `arith` with the library's own
// choice of rows per tile (rows_per_tile 0: what every EDSR / PlanesSR entry point passes): the route's own answer.  A training iteration re-packs
// both blobs of the network (the weights change every iteration): packing only these regions writes a fifth of the bytes (nvsr_pack_edsr_arith).
// arith == NVSR_PACK_ALL_ARITHMETICS: every region.
constexpr unsigned CONV_KINDS_ALL = 15u;
inline unsigned conv_kinds_for(int Cin, int Cout, int arith) {
    if (arith == NVSR_PACK_ALL_ARITHMETICS) return CONV_KINDS_ALL;
    ConvShape s;
    s.H = s.W = 3;                                 // (the family, and with it the region, does not depend on the sizes)
    ConvRoute r;
    return conv_route(Cin, Cout, s, 0, EPI_NONE, arith, 0, &r) ? 0u : 1u << r.region;
}

// conv_input, (conv1, conv2) x nblocks, conv_mid, n_up x up-conv, conv_output  (state-dict order, models.py:802-816)
inline void edsr_layers(int Cin, int Cout, int hid, int nblocks, int n_up, ConvLayer* L, int* n) {
    int k = 0;
    L[k++] = {Cin, hid};
    for (int b = 0; b < 2 * nblocks; ++b) L[k++] = {hid, hid};
    L[k++] = {hid, hid};
    for (int u = 0; u < n_up; ++u) L[k++] = {hid, 4 * hid};
    L[k++] = {hid, Cout};
    *n = k;
}
constexpr int EDSR_MAX_LAYERS = 600;
inline bool edsr_geometry_ok(int nblocks, int n_up) { return nblocks >= 0 && nblocks <= 290 && n_up >= 0 && n_up <= 8; }

// Geometry of one EDSR application to an [Cin][H][W] input: per layer the input size, the epilogue, and where the layer's input lives
// in the activation record kept for the backward pass (layer 0 reads the caller's x).
struct EdsrPlan {
    int n;
    ConvLayer L[EDSR_MAX_LAYERS];
    int ih[EDSR_MAX_LAYERS], iw[EDSR_MAX_LAYERS];
    int epi[EDSR_MAX_LAYERS];          // forward epilogue of layer l
    int64_t act_off[EDSR_MAX_LAYERS];  // floats; input of layer l >= 1 inside the record
    int64_t acts_floats;               // size of the record
    int64_t max_tensor;                // largest activation (= largest gradient tensor) of the net, floats
    int Ho, Wo;                        // output size
};

inline int edsr_plan(int Cin, int Cout, int hid, int nblocks, int n_up, int H, int W, EdsrPlan* P) {
    if (!edsr_geometry_ok(nblocks, n_up) || Cin < 1 || Cout < 1 || hid < 1) return NVSR_ERR_SHAPE;
    edsr_layers(Cin, Cout, hid, nblocks, n_up, P->L, &P->n);
    int64_t h = H, w = W, off = 0, mx = 0;
    for (int l = 0; l < P->n; ++l) {
        if (h < 3 || w < 3 || h > 1 << 20 || w > 1 << 20) return NVSR_ERR_SHAPE;
        P->ih[l] = (int)h; P->iw[l] = (int)w;
        const bool in_blocks = l >= 1 && l <= 2 * nblocks;
        const bool up = l > 2 * nblocks + 1 && l < P->n - 1;
        P->epi[l] = in_blocks ? ((l & 1) ? EPI_RELU : EPI_RESIDUAL) : (up ? EPI_PIXEL_SHUFFLE : EPI_NONE);
        int64_t oh = h - 2, ow = w - 2, oc = P->L[l].Cout;
        if (up) { oh *= 2; ow *= 2; oc /= 4; }
        const int64_t out_floats = oc * oh * ow;
        if (out_floats > mx) mx = out_floats;
        if (l + 1 < P->n) { P->act_off[l + 1] = off; off += (out_floats + 3) / 4 * 4; }
        h = oh; w = ow;
    }
    P->act_off[0] = -1;
    P->acts_floats = off;
    P->max_tensor = mx;
    P->Ho = (int)h; P->Wo = (int)w;
    return NVSR_OK;
}
// The plan's sizes in closed form, for the sizing functions that have no channel counts and answer for ANY nblocks / n_up (nvsr_edsr_out_size,
// nvsr_edsr_workspace_floats): the output size (< 1: the input is too small) and the largest tensor that lives in the inference forward's
// rotating buffers -- conv_input's output or an up-conv's; the final Cout tensor goes to the caller's `out`, so this is not EdsrPlan::max_tensor
struct EdsrExtent { int64_t Ho, Wo, max_rotating; };
inline EdsrExtent edsr_extent(int H, int W, int hid, int nblocks, int n_up) {
    int64_t h = (int64_t)H - 2, w = (int64_t)W - 2, mx = (int64_t)hid * h * w;      // conv_input
    h -= 4 * nblocks + 2; w -= 4 * nblocks + 2;                                     // the blocks, conv_mid
    for (int u = 0; u < n_up; ++u) {
        h = (h - 2) * 2; w = (w - 2) * 2;
        if ((int64_t)hid * h * w > mx) mx = (int64_t)hid * h * w;
    }
    return {h - 2, w - 2, mx};
}
// Where the input of layer l lives (l = P.n: the network's output) is the policy of the forward walk (sr.hip: edsr_forward_walk): the activation
// record of a training forward (act_off), or the inference path's three rotating buffers.  Either way a layer's output never aliases its input or
// the input of the layer before it, which a residual block's second conv still reads.
// Inference: three rotating buffers, the output of layer l - 1 in buffer (l - 1) % 3
inline int edsr_rotating_slot(int l) { return (l - 1) % 3; }

// PlanesSR's ROI arithmetic (models.py:902-905): roi = NULL (full plane) or [[ymin,xmin],[ymax,xmax]] in [-1,1] -> LR pixel bounds
inline void sr_roi(int R0, int R1, const float* roi, int* lo, int* hi) {
    lo[0] = lo[1] = 0; hi[0] = R0; hi[1] = R1;
    if (!roi) return;
    const int shape[2] = {R0, R1};
    for (int a = 0; a < 2; ++a) {
        const float mn = (float)shape[a] * (1.0f + roi[a]) / 2.0f, mx = (float)shape[a] * (1.0f + roi[2 + a]) / 2.0f;
        int l = (int)floorf(mn), hh = (int)ceilf(mx);
        l = l - 1 > 0 ? l - 1 : 0;
        hh = hh + 1 < shape[a] ? hh + 1 : shape[a];
        lo[a] = l; hi[a] = hh;
    }
}

// Region setup of a PlanesSR call on B regions of interest: per plane the LR bounds, the network's input and output sizes, and where the plane's
// tensors lie inside `keep` and inside the workspaces.  Every entry point carves its buffers with these offsets and every *_floats function
// returns these totals.
struct SrPlane {
    int lo[2], hi[2], Hp, Wp, Ho, Wo;
    int64_t n_in, n_diff;          // floats of the prepared input [Cc][Hp][Wp] and of the network's output [Cc][Ho][Wo]
    int64_t keep_xin, keep_acts;   // keep: plane after plane, the prepared input + the activation record (plans only)
    int64_t fwd_diff;              // workspace of the batched training forward: the network's outputs, plane after plane
    int64_t bwd_diff, bwd_dxin;    // workspace of a backward: per plane d_diff + the prepared input's gradient, then the EDSR backward's own
    // workspace of the inference (and one-plane training) forward on B planes of this size: [B] inputs, [B] outputs, the rotating buffers
    int64_t inf_diff(int B) const { return B * n_in; }
    int64_t inf_ews(int B) const { return B * (n_in + n_diff); }
};
struct SrRegions {
    int ok = 0;                    // planes set up (< B: plane `ok` was refused)
    SrPlane p[CONV_RAGGED_MAX];
    int64_t keep_floats = 0, fwd_floats = 0, bwd_floats = 0;      // totals of the three carve-ups
};
// P: B plans to fill, or NULL -- sizes from edsr_extent alone, for the sizing functions of the inference path, which have always answered for any
// nblocks / n_up; over < 0: no check of pad / over against the net (the sizing functions take no `over`)
inline int sr_regions(int B, int Cc, int R0, int R1, int hid, int nblocks, int n_up, int pad, int over, const float* rois, EdsrPlan* P, SrRegions* g) {
    *g = SrRegions{};
    if (B < 1 || B > CONV_RAGGED_MAX) return NVSR_ERR_SHAPE;
    const int sf = 1 << n_up;
    for (int b = 0; b < B; ++b) {
        SrPlane& s = g->p[b];
        sr_roi(R0, R1, rois ? rois + 4 * b : nullptr, s.lo, s.hi);
        const int ch = s.hi[0] - s.lo[0], cw = s.hi[1] - s.lo[1];
        s.Hp = ch + 2 * pad; s.Wp = cw + 2 * pad;
        if (P) {
            if (int e = edsr_plan(Cc, Cc, hid, nblocks, n_up, s.Hp, s.Wp, &P[b])) return e;
            s.Ho = P[b].Ho; s.Wo = P[b].Wo;
        } else {
            const EdsrExtent x = edsr_extent(s.Hp, s.Wp, hid, nblocks, n_up);
            if (x.Ho < 1 || x.Wo < 1) return NVSR_ERR_SHAPE;
            s.Ho = (int)x.Ho; s.Wo = (int)x.Wo;
        }
        if (over >= 0 && (s.Ho != ch * sf + 2 * over || s.Wo != cw * sf + 2 * over)) return NVSR_ERR_SHAPE;      // pad / over inconsistent with the net
        s.n_in = (int64_t)Cc * s.Hp * s.Wp; s.n_diff = (int64_t)Cc * s.Ho * s.Wo;
        s.keep_xin = g->keep_floats; s.keep_acts = s.keep_xin + round4(s.n_in);
        g->keep_floats = s.keep_acts + (P ? P[b].acts_floats : 0);
        s.fwd_diff = g->fwd_floats; g->fwd_floats += round4(s.n_diff);
        s.bwd_diff = g->bwd_floats; s.bwd_dxin = s.bwd_diff + round4(s.n_diff);
        g->bwd_floats = s.bwd_dxin + round4(s.n_in);
        g->ok = b + 1;
    }
    return NVSR_OK;
}

// H, W: size of the tensor in memory; pad: virtual zero border (the kernel sees (H+2pad) x (W+2pad)).  Defined in sr.hip.
// batch: consecutive [C][H][W] planes in `in` / `skip` / `out`, all convolved with the same weights in one launch.
// ConvExec: per-call execution options of the convolutions (include/nvsr.h, the *_arith entry points).  arith = NVSR_ARITH_* or
// NVSR_ARITH_INHERIT (the process default of nvsr_set_conv_arithmetic); rows = 0 (cost model) or 2 / 3 / 4 rows per workgroup tile of the wide
// kernels (the parity tests force every instantiation).
struct ConvExec { int arith = -1; int rows = 0; const unsigned* in_absmax = nullptr; unsigned* out_absmax = nullptr; };      // out_absmax: ZEROED word that receives the bits of max |out| (the epilogues' atomicMax)
//      // in_absmax: launch_absmax of the input, if the caller has it already (f16 data gradients)
int conv_resolve_arith(int arith);      // INHERIT -> process default; sr.hip
// bits of max |x| over a tensor, in a device word that stays valid for the launches queued behind it (sr.hip): the power-of-two scale of an
// f16-limb gradient operand; NULL on a launch error
const unsigned* launch_absmax(const float* x, long n, hipStream_t stream, unsigned* owned = nullptr);
// A RAGGED batch: up to CONV_RAGGED_MAX planes of DIFFERENT sizes through one launch with the same weights -- the regions of interest of a
// scene's position planes in an SR training iteration (models.py:270-284: every plane has its own crop).  One 256-channel layer of one crop is
// 2-3 workgroup rounds with a last round a fifth full; the three crops together are 6-7 rounds.  The launch is a linear list of the planes'
// tiles, plane after plane (ConvRagged::tile0).  H, W: logical input size per plane INCLUDING the virtual border.
struct ConvRagged {
    int n = 0;                                   // 0: not ragged (ConvParams' own tensors and batch strides apply)
    int H[CONV_RAGGED_MAX] = {0, 0, 0, 0}, W[CONV_RAGGED_MAX] = {0, 0, 0, 0};
    const float* in[CONV_RAGGED_MAX] = {nullptr, nullptr, nullptr, nullptr};
    float* out[CONV_RAGGED_MAX] = {nullptr, nullptr, nullptr, nullptr};
    const float* skip[CONV_RAGGED_MAX] = {nullptr, nullptr, nullptr, nullptr};
    // (filled by launch_conv) first workgroup of every plane in the launch's linear tile list -- the list has no empty tiles: a grid sized for the
    // largest plane would leave the smaller planes' unused tiles in a few XCDs' contiguous shares of the list (measured: two XCDs 28 % idle)
    unsigned tile0[CONV_RAGGED_MAX + 1] = {0, 0, 0, 0, 0};
};
// the convolution kernels' first argument (sr.hip); filled by launch_conv
struct ConvParams {
    const float* in;      // [Cin][H-2pad][W-2pad]
    const float* wpk;     // packed weights [chunk][cb][t][lane]
    const unsigned* wpk_limb;   // bf16-limb fragments behind them (conv_limb_eligible layers), else NULL
    const unsigned* wpk_limb16; // 16x16x32 fragments behind those (conv_limb16_eligible layers), else NULL
    const unsigned* wpk_f16;    // 16x16x32 fragments of the 2-f16-limb arithmetic behind those (same layers), else NULL
    const unsigned* absmax;     // f16 limbs, data gradient: bits of max |in| over the whole input (absmax_kernel) -> the input's power-of-two scale; else NULL
    float* out;           // [Cout][H-2][W-2]  (pixel shuffle: [Cout/4][2(H-2)][2(W-2)])
    const float* skip;    // EPI_RESIDUAL: identity [Cout][H+2][W+2] (block input); EPI_MASK_SCALE: forward activation
                          // [Cout][H-2][W-2] whose sign gates the result; EPI_ADD_CENTER: [Cout][H-6][W-6] added to the centre
    int Cin, Cout, H, W;  // H, W = logical input size, INCLUDING the virtual zero border of `pad` pixels
    int ncb_total;        // padded co-blocks in wpk (multiple of 2)
    int nchunks;          // ceil(Cin/4)
    int epilogue;
    int pad;              // 0, or 2 for the data gradient of a valid conv ("full" correlation with the flipped kernel)
    int ncg;              // co-groups of the grid; blockIdx.z = batch * ncg + co-group
    long in_bs, out_bs, skip_bs;   // floats between consecutive planes of a batch (the 3 planes of a scene share the weights)
    unsigned* out_absmax;          // NULL, or a word that receives (atomicMax) the bits of max |out| over everything this launch writes: the
                                   // power-of-two scale of the NEXT f16-limb gradient launches that read `out` (no separate reduction pass)
};
// rag != NULL: in / skip / out / H / W / batch are ignored (rag->H, rag->W = sizes of the tensors in memory, the virtual border is added here);
// limb arithmetics only, and an f16 data gradient needs cx.in_absmax (one word for all planes: launch_absmax_ragged)
int launch_conv(const float* in, int Cin, int H, int W, const float* wpk, int Cout, int epilogue, const float* skip, float* out,
                hipStream_t stream, int pad = 0, int batch = 1, ConvExec cx = ConvExec{}, const ConvRagged* rag = nullptr);
// fragment blobs of nl consecutive layers (natural: their [Cout][Cin][3][3] weights one after the other) in 4 launches per 36 layers; transposed: the
// data gradients' fragments (nvsr_pack_conv3x3_dgrad per layer).  sr.hip
int pack_layers(const float* natural, const ConvLayer* layers, int nl, float* packed, int transposed, hipStream_t stream, int arith = NVSR_PACK_ALL_ARITHMETICS);
// max |x| over up to CONV_RAGGED_MAX tensors in one launch, into the caller's word
const unsigned* launch_absmax_ragged(int n, const float* const* x, const long* count, hipStream_t stream, unsigned* owned);

}  // namespace nvsr
