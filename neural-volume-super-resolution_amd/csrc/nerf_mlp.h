// The layer engine of the two FlexibleNeRFModel baselines (models.py:14-108 with the constructor defaults, train_nerf.py:342-348): the
// Mip-NeRF one (mip.hip, 36 IPE columns into layer1) and the positional-encoding one (pe.hip, 39 columns: xyz and 36 sin / cos).  Both run
// layer1 K->128 (linear), 3 x ReLU(128->128), ReLU(fc_feat) 128->128, fc_alpha 128->1, ReLU(layers_dir(cat(feat, dir 27))) 155->64,
// fc_rgb 64->3; they differ only in the width K of layer1's input and in the encoder that computes a point's row.
//
// Kernels (templates on the encoder / the layer-1 width, instantiated by mip.hip and pe.hip)
//   nerf_encode_kernel         one thread per (point, column): rows [P][K + 27] = [encoding | direction] (tests, tools)
//   nerf_forward_kernel        one wave per tile of 32 consecutive points: the encoding is computed straight into the wave's LDS rows (never
//                              to HBM), then the 8 layers on the matrix pipe with the activations kept in two LDS row buffers of the wave;
//                              optional record of every layer input and ReLU output for the training backward (Layout::REC floats per point)
//   nerf_backward_kernel       the same tiling: dL/draw through the transposed layers, ReLU gates read from the record -> the pre-activation
//                              gradient of every layer (NERF_GREC floats per point)
//   nerf_wgrad_kernel          dW = sum_points G^T X, db = sum_points G per layer: one (32 x 32) tile x one slab of points per workgroup, the
//                              4 waves' partial sums added in a fixed order, one partial blob per slab; nerf_wgrad_reduce_kernel adds the
//                              slabs in order.  No float atomics: the same inputs give the same bits.
// Weights are read from the natural (state-dict order) blob through L2: every wave multiplies its tile by the whole model (324 KB for Mip).
// DESIGN.md 3.7 has the traffic this costs.
//
// Arithmetic: NVSR_ARITH_F32 = v_mfma_f32_32x32x2_f32 (exact products); NVSR_ARITH_BF16X3 = v_mfma_f32_32x32x16_bf16 on 3 truncation limbs of
// both operands, 6 products; NVSR_ARITH_F16X2 = v_mfma_f32_32x32x16_f16 on 2 round-to-nearest f16 limbs, 3 products, with the static scales
// of limb_core.h (weights x 2^F16_SW, activations x 2^F16_SX; the backward's gradient operand carries one power of two per point instead).
// Every operand is split where it is multiplied, the weights included: the weight stream stays the natural f32 blob.  An
// F16X2 request that INHERITS the process default runs BF16X3 (include/nvsr.h).  The weight gradients are exact-f32 MFMAs in every case.
#pragma once
#include "limb_core.h"

namespace nvsr {

constexpr int NERF_DIR = 27;                       // positional_encoding(viewdir, 4, include_input=True)
constexpr int MH = 128, MHD = 64;                  // hidden width, direction-layer width
constexpr int MIP_LD = 161;                        // LDS row stride of the activation buffers (160 columns + 1: odd, few bank conflicts)

// Offsets of the model with a layer-1 input of ENC columns.
template <int ENC_>
struct NerfLayout {
    static constexpr int ENC = ENC_, IN = ENC + NERF_DIR;
    static_assert(ENC <= 48, "the encoding block of the LDS rows is 48 columns wide");
    // natural blob (state-dict order: layer1, layers_xyz.0-2, layers_dir.0, fc_alpha, fc_rgb, fc_feat; weight [out][in] then bias)
    static constexpr int W_L1 = 0, B_L1 = W_L1 + MH * ENC;
    static constexpr int W_X0 = B_L1 + MH, B_X0 = W_X0 + MH * MH;
    static constexpr int W_X1 = B_X0 + MH, B_X1 = W_X1 + MH * MH;
    static constexpr int W_X2 = B_X1 + MH, B_X2 = W_X2 + MH * MH;
    static constexpr int W_DIR = B_X2 + MH, B_DIR = W_DIR + MHD * (MH + NERF_DIR);
    static constexpr int W_A = B_DIR + MHD, B_A = W_A + MH;
    static constexpr int W_RGB = B_A + 1, B_RGB = W_RGB + 3 * MHD;
    static constexpr int W_F = B_RGB + 3, B_F = W_F + MH * MH;
    static constexpr int NAT = B_F + MH;
    // record of the recording forward, per point: [enc ENC | dir 27 | h1 | h2 | h3 | h4 | feat (128 each) | hd 64]
    static constexpr int R_ENC = 0, R_DIR = ENC, R_H1 = IN, R_H2 = R_H1 + MH, R_H3 = R_H2 + MH, R_H4 = R_H3 + MH, R_FEAT = R_H4 + MH,
                         R_HD = R_FEAT + MH;
    static constexpr int REC = R_HD + MHD;
};

// pre-activation gradients, per point (the same for every layer-1 width): [layer1 | x0 | x1 | x2 | feat (128 each) | alpha 1 | dir 64 | rgb 3]
constexpr int G_L1 = 0, G_X0 = 128, G_X1 = 256, G_X2 = 384, G_FEAT = 512, G_A = 640, G_DIR = 641, G_RGB = 705;
constexpr int NERF_GREC = G_RGB + 3;

__device__ __forceinline__ void wave_sync() {      // this wave's LDS stores before its later LDS reads (the rows are per wave)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// direction column q (0 .. 26) of a packed ray r [11]: positional_encoding(viewdir, 4, include_input=True) (nerf_helpers.py:552-575)
__device__ __forceinline__ float dir_column(const float* __restrict__ r, int q) {
    if (q < 3) return r[8 + q];
    q -= 3;
    const int l = q / 6, s = q % 6;
    const float v = __fmul_rn(ldexpf(1.0f, l), r[8 + s % 3]);
    return s < 3 ? sinf(v) : cosf(v);
}

// One dense layer of a 32-point tile: for every block of 32 outputs o, acc = W'[o][0..K) . X[point][0..K) on the matrix pipe, then
// put(point n, output m, acc) for m < M.  W'[o][k] = W[o * ldw + k] (forward) or W[k * ldw + o] (TRANS: the transposed layer of the backward),
// 0 outside o < M, k < K.  X: the wave's LDS rows (stride MIP_LD); its columns [K, K rounded up to the K-step) must hold zeros.
// F16X2: the weights go in as W 2^F16_SW and the activations as x 2^F16_SX (GRAD: as they are -- the backward's rows carry a power of two per
// point), put() receives the unscaled sum.  Forward (not GRAD): a weight |W| >= 255 or an activation |x| >= 4094 enters the products as NaN.
// Backward (GRAD): no compare per weight and use.  A weight whose W 2^8 rounds beyond the f16 range (|W| >= 255.97; up to there both limbs
// are exact) has hi = inf and lo = RN(W 2^8 - inf) = -inf, so Wh x + Wl x = inf - inf = NaN for x != 0 and inf 0 = NaN for x = 0: the
// overflow is its own poison, as in the tri-plane kernels (and a weight in [255, 255.97) has already made its forward NaN).  A gradient
// operand beyond the f16 range overflows to inf the same way: the outputs it reaches are NaN, never a finite wrong number.
// (Measured, profiles/nerf_baseline_time.txt: the backward without the weight compare is 4 % faster than the one with it, the forward 7 %
// slower -- its schedule around the weight loads changes; each keeps its faster form.)
constexpr float NERF_F16_W_MAX = 255.0f, NERF_F16_X_MAX = 4094.0f;
template <int ARITH, bool TRANS, bool GRAD = false, class Put>
__device__ __forceinline__ void tile_layer(const float* __restrict__ W, int ldw, int M, int K, const float* X, int lane, Put put) {
    const int n = lane & 31, h = lane >> 5;
#pragma nounroll
    for (int o0 = 0; o0 < M; o0 += 32) {
        const int o = o0 + n;
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
        if constexpr (ARITH == NVSR_ARITH_F32) {
#pragma unroll 8
            for (int k0 = 0; k0 < K; k0 += 2) {            // (K odd: column K of X is a zero)
                const int k = k0 + h;
                const float a = (o < M && k < K) ? (TRANS ? W[(long)k * ldw + o] : W[(long)o * ldw + k]) : 0.0f;
                acc = mfma32(a, X[n * MIP_LD + k], acc);
            }
        } else if constexpr (ARITH == NVSR_ARITH_F16X2) {
#pragma unroll 2
            for (int k0 = 0; k0 < K; k0 += 16) {
                float a[8], b[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int k = k0 + 8 * h + j;
                    const float wv = (o < M && k < K) ? (TRANS ? W[(long)k * ldw + o] : W[(long)o * ldw + k]) : 0.0f;
                    const float xv = X[n * MIP_LD + k];
                    a[j] = GRAD ? wv * F16_W_SCALE : (fabsf(wv) < NERF_F16_W_MAX ? wv * F16_W_SCALE : __builtin_nanf(""));
                    b[j] = GRAD ? xv : (fabsf(xv) < NERF_F16_X_MAX ? xv * F16_X_SCALE : __builtin_nanf(""));
                }
                Limbs<2> wa, xb;
                split_all<2>([&](int i) { return a[i]; }, wa);
                split_all<2>([&](int i) { return b[i]; }, xb);
#pragma unroll
                for (int p = 0; p < 3; ++p) acc = mfma_limb<2>(wa.v[limb_w(2, p)], xb.v[limb_x(2, p)], acc);
            }
            constexpr float un = GRAD ? F16_ACC_UNSCALE : F16_ACC_UNSCALE * F16_HEAD_SCALE;      // 2^-SW, 2^-(SW + SX)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] *= un;
        } else {
#pragma unroll 2
            for (int k0 = 0; k0 < K; k0 += 16) {
                float a[8], b[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int k = k0 + 8 * h + j;
                    a[j] = (o < M && k < K) ? (TRANS ? W[(long)k * ldw + o] : W[(long)o * ldw + k]) : 0.0f;
                    b[j] = X[n * MIP_LD + k];
                }
                Limbs<3> wa, xb;
                split8(a, wa);
                split8(b, xb);
#pragma unroll
                for (int p = 0; p < 6; ++p) acc = mfma_bf16(wa.v[limb_w(3, p)], xb.v[limb_x(3, p)], acc);
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = o0 + (r & 3) + 8 * (r >> 2) + 4 * h;
            if (m < M) put(n, m, acc[r]);
        }
    }
    wave_sync();
}

// rows [0, 32) x columns [c0, c0 + nc) of the wave's LDS buffer -> rec[point][off + c] (stride ld), points < P only
__device__ __forceinline__ void store_rows(const float* X, int c0, int nc, float* __restrict__ rec, int ld, int off, long p0, long P, int lane) {
    for (int e = lane; e < 32 * nc; e += 64) {
        const int pt = e / nc, c = e - pt * nc;
        if (p0 + pt < P) rec[(p0 + pt) * ld + off + c] = X[pt * MIP_LD + c0 + c];
    }
    wave_sync();
}

constexpr int MIP_WAVES = 1;     // waves per workgroup, one 32-point tile each: 41 KB of LDS per wave, 3 workgroups per CU

// An encoder E: E::ENC (the layer-1 width) and `float operator()(long p, int c) const`, column c (0 .. ENC + 26) of point p's row.
template <class E>
__global__ void nerf_encode_kernel(long P, E enc, float* __restrict__ out) {
    constexpr int IN = E::ENC + NERF_DIR;
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= P * IN) return;
    const long p = e / IN;
    out[e] = enc(p, (int)(e - p * IN));
}

// The LDS rows of a tile through the forward (xa / xb: [32][MIP_LD] each):
//   enc -> xa[0,48) (ENC..47 zero), dir -> xb[128,160) (155..159 zero)
//   layer1: xa -> xb[0,128) h1;  x0: xb -> xa h2;  x1: xa -> xb h3;  x2: xb -> xa[0,128) h4
//   fc_alpha: xa -> xa[131];  fc_feat: xa -> xb[0,128) feat (next to dir);  layers_dir: xb[0,160) -> xa[0,64) hd;  fc_rgb: xa -> xa[128,131)
//   F16X2: a ReLU that keeps NaN (fmaxf(NaN, 0) is 0: an out-of-range hidden activation would vanish), and a lane that writes a non-finite raw
//   row ORs 1 into the range flag (include/nvsr.h: nvsr_set_range_flag)
template <class E, int ARITH>
__global__ __launch_bounds__(64 * MIP_WAVES) void nerf_forward_kernel(long P, E enc, const float* __restrict__ w, float* __restrict__ raw,
                                                                     float* __restrict__ rec, unsigned* __restrict__ flag) {
    using L = NerfLayout<E::ENC>;
    __shared__ float lds[MIP_WAVES * 2 * 32 * MIP_LD];
    NVSR_RACE_PROBE_DELAY(lds);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, n = lane & 31, h = lane >> 5;
    float* xa = lds + wave * 2 * 32 * MIP_LD;
    float* xb = xa + 32 * MIP_LD;
    const long p0 = ((long)blockIdx.x * MIP_WAVES + wave) * 32;
    if (p0 >= P) return;
    const long p = p0 + n;
    const bool live = p < P;
    for (int c = h; c < L::IN; c += 2) {                 // the lane pair (n, 0), (n, 1) encodes point n
        const float v = live ? enc(p, c) : 0.0f;
        if (c < L::ENC) xa[n * MIP_LD + c] = v;
        else xb[n * MIP_LD + MH + c - L::ENC] = v;
    }
    for (int c = L::ENC + h; c < 48; c += 2) xa[n * MIP_LD + c] = 0.0f;
    for (int c = MH + NERF_DIR + h; c < 160; c += 2) xb[n * MIP_LD + c] = 0.0f;
    wave_sync();
    if (rec) { store_rows(xa, 0, L::ENC, rec, L::REC, L::R_ENC, p0, P, lane); store_rows(xb, MH, NERF_DIR, rec, L::REC, L::R_DIR, p0, P, lane); }
    auto dense = [&](int wo, int bo, int M, int K, const float* X, float* Y, int yoff, bool relu) {
        tile_layer<ARITH, false>(w + wo, K, M, K, X, lane, [&](int pt, int m, float a) {
            const float v = __fadd_rn(a, w[bo + m]);
            if constexpr (ARITH == NVSR_ARITH_F16X2) Y[pt * MIP_LD + yoff + m] = (relu && !(v != v)) ? fmaxf(v, 0.0f) : v;
            else Y[pt * MIP_LD + yoff + m] = relu ? fmaxf(v, 0.0f) : v;
        });
    };
    dense(L::W_L1, L::B_L1, MH, L::ENC, xa, xb, 0, false);
    if (rec) store_rows(xb, 0, MH, rec, L::REC, L::R_H1, p0, P, lane);
    dense(L::W_X0, L::B_X0, MH, MH, xb, xa, 0, true);
    if (rec) store_rows(xa, 0, MH, rec, L::REC, L::R_H2, p0, P, lane);
    dense(L::W_X1, L::B_X1, MH, MH, xa, xb, 0, true);
    if (rec) store_rows(xb, 0, MH, rec, L::REC, L::R_H3, p0, P, lane);
    dense(L::W_X2, L::B_X2, MH, MH, xb, xa, 0, true);
    if (rec) store_rows(xa, 0, MH, rec, L::REC, L::R_H4, p0, P, lane);
    dense(L::W_A, L::B_A, 1, MH, xa, xa, 131, false);
    dense(L::W_F, L::B_F, MH, MH, xa, xb, 0, true);
    if (rec) store_rows(xb, 0, MH, rec, L::REC, L::R_FEAT, p0, P, lane);
    dense(L::W_DIR, L::B_DIR, MHD, MH + NERF_DIR, xb, xa, 0, true);
    if (rec) store_rows(xa, 0, MHD, rec, L::REC, L::R_HD, p0, P, lane);
    dense(L::W_RGB, L::B_RGB, 3, MHD, xa, xa, 128, false);
    if (live && h == 0) {
        float4 o = {xa[n * MIP_LD + 128], xa[n * MIP_LD + 129], xa[n * MIP_LD + 130], xa[n * MIP_LD + 131]};
        reinterpret_cast<float4*>(raw)[p] = o;
        if constexpr (ARITH == NVSR_ARITH_F16X2) {
            if (flag && !(fabsf(o.x + o.y + o.z + o.w) <= 3.0e38f)) __hip_atomic_fetch_or(flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// dL/draw [P][4] -> the pre-activation gradients of every layer (grec, NERF_GREC per point).  LDS rows:
//   G_rgb -> xa[0,3) (3..15 zero);  fc_rgb's input gradient gated by hd > 0 = G_dir -> xb[0,64)
//   (G_dir W_dir)[0,128) gated by feat > 0 = G_feat -> xa[0,128);  G_feat W_feat + G_alpha W_alpha gated by h4 > 0 = G_x2 -> xb
//   G_x2 W_x2 gated by h3 = G_x1 -> xa;  G_x1 W_x1 gated by h2 = G_x0 -> xb;  G_x0 W_x0 = G_1 (layer1 is linear) -> xa
// F16X2: gradients span far more binades than f16's 5 exponent bits, but one chain of one point does not -- every layer of the backward is
// linear in that point's dL/draw (the ReLU gates come from the record).  As in render_bwd_limb.hip (pow2_scales), a point carries two powers
// of two: the rgb chain (G_rgb -> G_dir -> G_feat) is scaled by the one that puts max |dL/drgb| into [2^NERF_F16_UP, 2^(NERF_F16_UP+1)), and
// from fc_feat's transposed product on (G_x2 .. G_1, where dL/dalpha joins) the chain runs at the scale of max |dL/draw|; the rgb part enters
// there through an exact multiply by the ratio of the two (<= 1: what it shrinks below an f32 subnormal is below 2^-126 of the joint chain).
// Behind a surface dL/dalpha and dL/drgb of one sample differ by many binades: one scale for both would leave the rgb chain in subnormal f16.
// The rows are written unscaled (lane pt holds point pt's two undos; a row's is read with v_readlane).  Exact: a point is a column of every
// product, and a loss scaled by 2^k gives the same bits times 2^k.  A lane that writes a non-finite gradient ORs 1 into the range flag (the
// stored values are accumulated as v 0: NaN iff one of them is inf or NaN -- one FMA per value).
constexpr int NERF_F16_UP = 3;
__device__ __forceinline__ void nerf_pow2_scale(float m, float& sc, float& un) {
    const int e = (int)((__float_as_uint(m) >> 23) & 0xffu);              // biased exponent of the largest magnitude (0: zero or subnormal)
    // (clamped to [1 + UP, 253]: both factors stay normal numbers; a non-finite dL/draw keeps a scale of 1 and comes out non-finite)
    const int eu = (e == 255 ? 127 + NERF_F16_UP : (e > 253 ? 253 : (e < 1 + NERF_F16_UP ? 1 + NERF_F16_UP : e))) - NERF_F16_UP;
    sc = __uint_as_float((unsigned)(254 - eu) << 23);
    un = __uint_as_float((unsigned)eu << 23);
}
template <int ENC, int ARITH>
__global__ __launch_bounds__(64 * MIP_WAVES) void nerf_backward_kernel(long P, const float* __restrict__ w, const float* __restrict__ rec,
                                                                      const float* __restrict__ g_raw, float* __restrict__ grec,
                                                                      unsigned* __restrict__ flag) {
    using L = NerfLayout<ENC>;
    constexpr bool F16 = ARITH == NVSR_ARITH_F16X2;
    __shared__ float lds[MIP_WAVES * 2 * 32 * MIP_LD];
    NVSR_RACE_PROBE_DELAY(lds);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, n = lane & 31, h = lane >> 5;
    float* xa = lds + wave * 2 * 32 * MIP_LD;
    float* xb = xa + 32 * MIP_LD;
    const long p0 = ((long)blockIdx.x * MIP_WAVES + wave) * 32;
    if (p0 >= P) return;
    const long p = p0 + n;
    const bool live = p < P;
    const float g_alpha_in = live ? g_raw[p * 4 + 3] : 0.0f;
    float sc_r = 1.0f, un_r = 1.0f, sc_m = 1.0f, un_m = 1.0f, join = 1.0f, chk = 0.0f;
    if constexpr (F16) {
        const float mr = live ? fmaxf(fmaxf(fabsf(g_raw[p * 4]), fabsf(g_raw[p * 4 + 1])), fabsf(g_raw[p * 4 + 2])) : 0.0f;
        nerf_pow2_scale(mr, sc_r, un_r);
        nerf_pow2_scale(fmaxf(mr, fabsf(g_alpha_in)), sc_m, un_m);
        join = sc_m * un_r;                                                 // rgb chain -> joint chain, a power of two <= 1
    }
    const float g_alpha = F16 ? g_alpha_in * sc_m : g_alpha_in;
    for (int c = h; c < 16; c += 2) xa[n * MIP_LD + c] = (live && c < 3) ? (F16 ? g_raw[p * 4 + c] * sc_r : g_raw[p * 4 + c]) : 0.0f;
    wave_sync();
    auto store = [&](const float* X, int nc, int off, float un) {
        if constexpr (F16) {
            for (int pt = 0; pt < 32 && p0 + pt < P; ++pt) {
                const float u = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(un), pt));
                for (int c = lane; c < nc; c += 64) {
                    const float v = X[pt * MIP_LD + c] * u;
                    chk = fmaf(v, 0.0f, chk);
                    grec[(p0 + pt) * NERF_GREC + off + c] = v;
                }
            }
            wave_sync();
        } else {
            store_rows(X, 0, nc, grec, NERF_GREC, off, p0, P, lane);
        }
    };
    store(xa, 3, G_RGB, un_r);
    if (live && h == 0) grec[p * NERF_GREC + G_A] = g_alpha_in;
    if constexpr (F16) { if (live && h == 0) chk = fmaf(g_alpha_in, 0.0f, chk); }
    // (a dead point's record row does not exist: its gate reads are skipped and its gradient rows are zeros)
    auto gate = [&](int off, int pt, int m) { return p0 + pt < P && rec[(p0 + pt) * L::REC + off + m] > 0.0f; };
    tile_layer<ARITH, true, true>(w + L::W_RGB, MHD, MHD, 3, xa, lane, [&](int pt, int m, float a) {
        xb[pt * MIP_LD + m] = gate(L::R_HD, pt, m) ? a : 0.0f;
    });
    store(xb, MHD, G_DIR, un_r);
    tile_layer<ARITH, true, true>(w + L::W_DIR, MH + NERF_DIR, MH, MHD, xb, lane, [&](int pt, int m, float a) {
        xa[pt * MIP_LD + m] = gate(L::R_FEAT, pt, m) ? a : 0.0f;
    });
    store(xa, MH, G_FEAT, un_r);
    // (lane (pt, h) holds point pt's g_alpha and join)
    tile_layer<ARITH, true, true>(w + L::W_F, MH, MH, MH, xa, lane, [&](int pt, int m, float a) {
        if constexpr (F16) a *= join;
        xb[pt * MIP_LD + m] = gate(L::R_H4, pt, m) ? __fadd_rn(a, __fmul_rn(g_alpha, w[L::W_A + m])) : 0.0f;
    });
    store(xb, MH, G_X2, un_m);
    tile_layer<ARITH, true, true>(w + L::W_X2, MH, MH, MH, xb, lane, [&](int pt, int m, float a) { xa[pt * MIP_LD + m] = gate(L::R_H3, pt, m) ? a : 0.0f; });
    store(xa, MH, G_X1, un_m);
    tile_layer<ARITH, true, true>(w + L::W_X1, MH, MH, MH, xa, lane, [&](int pt, int m, float a) { xb[pt * MIP_LD + m] = gate(L::R_H2, pt, m) ? a : 0.0f; });
    store(xb, MH, G_X0, un_m);
    tile_layer<ARITH, true, true>(w + L::W_X0, MH, MH, MH, xb, lane, [&](int pt, int m, float a) { xa[pt * MIP_LD + m] = a; });
    store(xa, MH, G_L1, un_m);
    if constexpr (F16) {
        if (chk != 0.0f && flag) __hip_atomic_fetch_or(flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// partial[slab][wo + m * K + k] = sum over the slab's points of G[p][m] X[p][k] (X = [X1 (K1 columns) | X2 (K - K1 columns)]),
// partial[slab][bo + m] = sum G[p][m] (the tile column k == K, whose operand is 1).  Every (m, k) of a slab is written by exactly one workgroup.
constexpr int MW_SLAB = 8192;
template <int ENC>
__global__ __launch_bounds__(256) void nerf_wgrad_kernel(long P, int M, int K, int K1, const float* __restrict__ G, int goff,
                                                         const float* __restrict__ rec, int x1off, int x2off, int wo, int bo, float* __restrict__ partial) {
    using L = NerfLayout<ENC>;
    __shared__ float red[3 * 64 * 16];
    NVSR_RACE_PROBE_DELAY(red);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, n = lane & 31, h = lane >> 5;
    const int m0 = blockIdx.x * 32, k0 = blockIdx.y * 32;
    const long pa = (long)blockIdx.z * MW_SLAB + wave * (MW_SLAB / 4), pb = min(pa + MW_SLAB / 4, P);
    const int m = m0 + n, k = k0 + n;
    const int xo = k < K1 ? x1off + k : x2off + (k - K1);
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    for (long ps = pa; ps < pb; ps += 2) {                   // (uniform trip count: every lane takes part in every MFMA)
        const long q = ps + h;
        float a = 0.0f, b = 0.0f;
        if (q < pb) {
            if (m < M) a = G[q * NERF_GREC + goff + m];
            if (k < K) b = rec[q * L::REC + xo];
            else if (k == K) b = 1.0f;
        }
        acc = mfma32(a, b, acc);
    }
    if (wave) {
#pragma unroll
        for (int r = 0; r < 16; ++r) red[((wave - 1) * 64 + lane) * 16 + r] = acc[r];
    }
    __syncthreads();
    if (wave || k > K) return;
    float* out = partial + (long)blockIdx.z * L::NAT;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const float v = __fadd_rn(__fadd_rn(__fadd_rn(acc[r], red[lane * 16 + r]), red[(64 + lane) * 16 + r]), red[(128 + lane) * 16 + r]);
        const int mr = m0 + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (mr < M) out[k < K ? wo + mr * K + k : bo + mr] = v;
    }
}

template <int NAT>
__global__ void nerf_wgrad_reduce_kernel(int slabs, const float* __restrict__ partial, float* __restrict__ grad) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= NAT) return;
    float s = partial[i];
    for (int z = 1; z < slabs; ++z) s = __fadd_rn(s, partial[(long)z * NAT + i]);
    grad[i] = s;
}

// ---- host side: the launches behind the C entry points of mip.hip and pe.hip ----------------------------------------------------------

// the arithmetic a call runs: an explicit F16X2 runs F16X2; NVSR_ARITH_INHERIT resolves to the decoder default with F16X2 read as BF16X3 (the
// meaning these entry points had before they had an f16 path: a caller who never names F16X2 sees no change -- include/nvsr.h)
static inline int nerf_arith(int arithmetic, int* out) {
    const bool inherit = arithmetic == NVSR_ARITH_INHERIT;
    if (inherit) arithmetic = nvsr_get_decoder_arithmetic();
    if (arithmetic == NVSR_ARITH_F32) *out = NVSR_ARITH_F32;
    else if (arithmetic == NVSR_ARITH_BF16X3) *out = NVSR_ARITH_BF16X3;
    else if (arithmetic == NVSR_ARITH_F16X2) *out = inherit ? NVSR_ARITH_BF16X3 : NVSR_ARITH_F16X2;
    else return NVSR_ERR_SHAPE;
    return NVSR_OK;
}

// The bodies of nvsr_{mip,pe}_encode and nvsr_{mip,pe}_nerf_forward_arith: argument checks, then the launch.  `depths` is the encoder's
// per-ray array (Mip: the S + 1 interval edges; PE: the S sample depths), checked for null beside the rays.
template <class E>
static int nerf_encode_launch(int64_t N, int S, const float* rays, const float* depths, const E& enc, float* out, hipStream_t stream) {
    if (N < 0 || S < 1) return NVSR_ERR_SHAPE;
    if (N == 0) return NVSR_OK;
    if (!rays || !depths || !out) return NVSR_ERR_NULL;
    const long n = (long)(N * S) * (E::ENC + NERF_DIR);
    hipLaunchKernelGGL(nerf_encode_kernel<E>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, (long)(N * S), enc, out);
    return NVSR_CHECK_LAUNCH();
}

template <class E>
static int nerf_forward_launch(int64_t N, int S, const float* rays, const float* depths, const E& enc, const float* natural, float* raw,
                               float* record, int arithmetic, hipStream_t stream) {
    int arith;
    if (N < 0 || S < 1 || nerf_arith(arithmetic, &arith)) return NVSR_ERR_SHAPE;
    if (N == 0) return NVSR_OK;
    if (!rays || !depths || !natural || !raw) return NVSR_ERR_NULL;
    if (reinterpret_cast<uintptr_t>(raw) % 16) return NVSR_ERR_ALIGN;
    const long P = (long)(N * S);
    const dim3 grid((unsigned)((P + 32 * MIP_WAVES - 1) / (32 * MIP_WAVES)));
    unsigned* flag = nullptr;
    if (arith == NVSR_ARITH_F32)
        hipLaunchKernelGGL((nerf_forward_kernel<E, NVSR_ARITH_F32>), grid, dim3(64 * MIP_WAVES), 0, stream, P, enc, natural, raw, record, flag);
    else if (arith == NVSR_ARITH_BF16X3)
        hipLaunchKernelGGL((nerf_forward_kernel<E, NVSR_ARITH_BF16X3>), grid, dim3(64 * MIP_WAVES), 0, stream, P, enc, natural, raw, record, flag);
    else
        hipLaunchKernelGGL((nerf_forward_kernel<E, NVSR_ARITH_F16X2>), grid, dim3(64 * MIP_WAVES), 0, stream, P, enc, natural, raw, record,
                           nvsr_get_range_flag());
    return NVSR_CHECK_LAUNCH();
}

template <int ENC>
static int nerf_backward_launch(int64_t P, const float* natural, const float* record, const float* g_raw, float* grad_record, int arithmetic,
                                hipStream_t stream) {
    int arith;
    if (P < 0 || nerf_arith(arithmetic, &arith)) return NVSR_ERR_SHAPE;
    if (P == 0) return NVSR_OK;
    if (!natural || !record || !g_raw || !grad_record) return NVSR_ERR_NULL;
    const dim3 grid((unsigned)((P + 32 * MIP_WAVES - 1) / (32 * MIP_WAVES)));
    unsigned* flag = nullptr;
    if (arith == NVSR_ARITH_F32)
        hipLaunchKernelGGL((nerf_backward_kernel<ENC, NVSR_ARITH_F32>), grid, dim3(64 * MIP_WAVES), 0, stream, (long)P, natural, record, g_raw,
                           grad_record, flag);
    else if (arith == NVSR_ARITH_BF16X3)
        hipLaunchKernelGGL((nerf_backward_kernel<ENC, NVSR_ARITH_BF16X3>), grid, dim3(64 * MIP_WAVES), 0, stream, (long)P, natural, record, g_raw,
                           grad_record, flag);
    else
        hipLaunchKernelGGL((nerf_backward_kernel<ENC, NVSR_ARITH_F16X2>), grid, dim3(64 * MIP_WAVES), 0, stream, (long)P, natural, record, g_raw,
                           grad_record, nvsr_get_range_flag());
    return NVSR_CHECK_LAUNCH();
}

template <int ENC>
static int64_t nerf_wgrad_workspace_floats(int64_t P) {
    return P <= 0 ? 0 : ((P + MW_SLAB - 1) / MW_SLAB) * (int64_t)NerfLayout<ENC>::NAT;
}

template <int ENC>
static int nerf_weight_grad_launch(int64_t P, const float* record, const float* grad_record, float* workspace, float* grad_natural,
                                   hipStream_t stream) {
    using L = NerfLayout<ENC>;
    if (P < 0) return NVSR_ERR_SHAPE;
    if (!grad_natural) return NVSR_ERR_NULL;
    if (P == 0) return hipMemsetAsync(grad_natural, 0, L::NAT * sizeof(float), stream) == hipSuccess ? NVSR_OK : NVSR_ERR_LAUNCH;
    if (!record || !grad_record || !workspace) return NVSR_ERR_NULL;
    const int slabs = (int)((P + MW_SLAB - 1) / MW_SLAB);
    struct Lay { int M, K, K1, goff, x1, x2, wo, bo; };
    const Lay layers[8] = {{MH, ENC, ENC, G_L1, L::R_ENC, 0, L::W_L1, L::B_L1},     {MH, MH, MH, G_X0, L::R_H1, 0, L::W_X0, L::B_X0},
                           {MH, MH, MH, G_X1, L::R_H2, 0, L::W_X1, L::B_X1},        {MH, MH, MH, G_X2, L::R_H3, 0, L::W_X2, L::B_X2},
                           {MHD, MH + NERF_DIR, MH, G_DIR, L::R_FEAT, L::R_DIR, L::W_DIR, L::B_DIR}, {1, MH, MH, G_A, L::R_H4, 0, L::W_A, L::B_A},
                           {3, MHD, MHD, G_RGB, L::R_HD, 0, L::W_RGB, L::B_RGB},    {MH, MH, MH, G_FEAT, L::R_H4, 0, L::W_F, L::B_F}};
    for (const Lay& l : layers) {
        const dim3 grid((unsigned)((l.M + 31) / 32), (unsigned)(l.K / 32 + 1), (unsigned)slabs);     // (k tiles up to and including k == K)
        hipLaunchKernelGGL(nerf_wgrad_kernel<ENC>, grid, dim3(256), 0, stream, (long)P, l.M, l.K, l.K1, grad_record, l.goff, record, l.x1, l.x2,
                           l.wo, l.bo, workspace);
        if (hipGetLastError() != hipSuccess) return NVSR_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(nerf_wgrad_reduce_kernel<L::NAT>, dim3((L::NAT + 255) / 256), dim3(256), 0, stream, slabs, workspace, grad_natural);
    return NVSR_CHECK_LAUNCH();
}

}  // namespace nvsr
