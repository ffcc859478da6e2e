// The Mip-NeRF baseline (config/MipNeRF_baseline.yml): integrated positional encoding of conical frustums and the FlexibleNeRFModel it feeds,
// forward and training.
//
// Reference: mip.py:9-44 (cast_rays -> conical_frustum_to_gaussian -> lift_gaussian), mip.py:154-199 (IntegratedPositionalEncoding with
// multires 7: degrees 2^0 .. 2^5, a sin block of 18 columns ordered (l, d) then the cos block as sin(y + pi/2), both damped by
// exp(-0.5 var 4^l)), nerf_helpers.py positional_encoding(viewdir, 4, include_input) for the 27 direction columns, train_utils.py:19-27
// (radius = ds 0.00135 2 / sqrt(12)), models.py:14-108 (FlexibleNeRFModel with the constructor defaults, train_nerf.py:342-348).
//
// Kernels
//   mip_encode_kernel          one thread per (interval, column): rows [N*S][63] = [36 IPE | 27 direction] (tests, tools)
//   mip_nerf_forward_kernel    one wave per tile of 32 consecutive intervals: the encoding is computed straight into the wave's LDS rows
//                              (never to HBM), then the 8 layers on the matrix pipe with the activations kept in two LDS row buffers of
//                              the wave; optional record of every layer input for the training backward (MIP_REC floats per point)
//   mip_nerf_backward_kernel   the same tiling: dL/draw through the transposed layers, ReLU gates read from the record -> the pre-activation
//                              gradient of every layer (MIP_GREC floats per point)
//   mip_wgrad_kernel           dW = sum_points G^T X, db = sum_points G per layer: one (32 x 32) tile x one slab of points per workgroup, the
//                              4 waves' partial sums added in a fixed order, one partial blob per slab; mip_wgrad_reduce_kernel adds the
//                              slabs in order.  No float atomics: the same inputs give the same bits.
// Weights are read from the natural (state-dict order) blob through L2: every wave multiplies its tile by the whole 324 KB of the model.
// DESIGN.md 3.7 has the traffic this costs.
//
// Arithmetic: NVSR_ARITH_F32 = v_mfma_f32_32x32x2_f32 (exact products); NVSR_ARITH_BF16X3 = v_mfma_f32_32x32x16_bf16 on 3 truncation limbs of
// both operands, 6 products (limb_core.h).  NVSR_ARITH_F16X2 runs BF16X3 (include/nvsr.h).  The weight gradients are exact-f32 MFMAs in
// either case.
#include "limb_core.h"

namespace nvsr {

constexpr int MIP_ENC = 36, MIP_DIR = 27, MIP_IN = MIP_ENC + MIP_DIR;
constexpr int MH = 128, MHD = 64;                  // hidden width, direction-layer width
constexpr int MIP_LD = 161;                        // LDS row stride of the activation buffers (160 columns + 1: odd, few bank conflicts)

// natural blob (state-dict order: layer1, layers_xyz.0-2, layers_dir.0, fc_alpha, fc_rgb, fc_feat; weight [out][in] then bias)
constexpr int MW_L1 = 0, MB_L1 = MW_L1 + MH * MIP_ENC;
constexpr int MW_X0 = MB_L1 + MH, MB_X0 = MW_X0 + MH * MH;
constexpr int MW_X1 = MB_X0 + MH, MB_X1 = MW_X1 + MH * MH;
constexpr int MW_X2 = MB_X1 + MH, MB_X2 = MW_X2 + MH * MH;
constexpr int MW_DIR = MB_X2 + MH, MB_DIR = MW_DIR + MHD * (MH + MIP_DIR);
constexpr int MW_A = MB_DIR + MHD, MB_A = MW_A + MH;
constexpr int MW_RGB = MB_A + 1, MB_RGB = MW_RGB + 3 * MHD;
constexpr int MW_F = MB_RGB + 3, MB_F = MW_F + MH * MH;
constexpr int MIP_NAT = MB_F + MH;
static_assert(MIP_NAT == NVSR_MIP_NERF_NATURAL_FLOATS, "natural blob size");

// record of the recording forward, per point: [enc 36 | dir 27 | h1 | h2 | h3 | h4 | feat (128 each) | hd 64]
constexpr int R_ENC = 0, R_DIR = 36, R_H1 = 63, R_H2 = R_H1 + MH, R_H3 = R_H2 + MH, R_H4 = R_H3 + MH, R_FEAT = R_H4 + MH, R_HD = R_FEAT + MH;
constexpr int MIP_REC = R_HD + MHD;
// pre-activation gradients, per point: [layer1 | x0 | x1 | x2 | feat (128 each) | alpha 1 | dir 64 | rgb 3]
constexpr int G_L1 = 0, G_X0 = 128, G_X1 = 256, G_X2 = 384, G_FEAT = 512, G_A = 640, G_DIR = 641, G_RGB = 705;
constexpr int MIP_GREC = G_RGB + 3;
static_assert(MIP_REC == NVSR_MIP_NERF_RECORD_FLOATS && MIP_GREC == NVSR_MIP_NERF_GRAD_RECORD_FLOATS, "record sizes");

__device__ __forceinline__ void wave_sync() {      // this wave's LDS stores before its later LDS reads (the rows are per wave)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// column c (0 .. 62) of the encoded row of interval j of ray i; every operation rounded like the reference's f32 tensor expressions
__device__ float mip_column(const float* __restrict__ rays, const float* __restrict__ edges, int S, float r2, long p, int c) {
    const long i = p / S;
    const int j = (int)(p - i * S);
    const float* r = rays + i * 11;
    if (c >= MIP_ENC) {                                   // positional_encoding(viewdir, 4, include_input=True)
        int q = c - MIP_ENC;
        if (q < 3) return r[8 + q];
        q -= 3;
        const int l = q / 6, s = q % 6;
        const float v = __fmul_rn(ldexpf(1.0f, l), r[8 + s % 3]);
        return s < 3 ? sinf(v) : cosf(v);
    }
    const int blk = c / 18, rr = c % 18, l = rr / 3, d = rr % 3;
    const float t0 = edges[i * (S + 1) + j], t1 = edges[i * (S + 1) + j + 1];
    const float mu = __fdiv_rn(__fadd_rn(t0, t1), 2.0f), hw = __fdiv_rn(__fsub_rn(t1, t0), 2.0f);
    const float mu2 = __fmul_rn(mu, mu), hw2 = __fmul_rn(hw, hw), hw4 = __fmul_rn(hw2, hw2);
    const float den = __fadd_rn(__fmul_rn(3.0f, mu2), hw2);
    const float t_mean = __fadd_rn(mu, __fdiv_rn(__fmul_rn(__fmul_rn(2.0f, mu), hw2), den));
    const float t_var = __fsub_rn(__fdiv_rn(hw2, 3.0f),
                                  __fmul_rn(4.0f / 15.0f, __fdiv_rn(__fmul_rn(hw4, __fsub_rn(__fmul_rn(12.0f, mu2), hw2)), __fmul_rn(den, den))));
    const float r_var = __fmul_rn(r2, __fsub_rn(__fadd_rn(__fdiv_rn(mu2, 4.0f), __fmul_rn(5.0f / 12.0f, hw2)),
                                                __fdiv_rn(__fmul_rn(4.0f / 15.0f, hw4), den)));
    const float dx = r[3], dy = r[4], dz = r[5], dd = r[3 + d];
    const float mag = fmaxf(1e-10f, __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz)));
    const float dd2 = __fmul_rn(dd, dd);
    const float mean = __fadd_rn(__fmul_rn(dd, t_mean), r[d]);
    const float cov = __fadd_rn(__fmul_rn(t_var, dd2), __fmul_rn(r_var, __fsub_rn(1.0f, __fdiv_rn(dd2, mag))));
    float y = __fmul_rn(mean, ldexpf(1.0f, l));
    const float var = __fmul_rn(cov, ldexpf(1.0f, 2 * l));
    if (blk) y = __fadd_rn(y, 1.57079637f);               // y + 0.5 pi (the f32 rounding of the double constant)
    return __fmul_rn(expf(__fmul_rn(-0.5f, var)), sinf(y));
}

__global__ void mip_encode_kernel(long P, int S, const float* __restrict__ rays, const float* __restrict__ edges, float r2, float* __restrict__ out) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= P * MIP_IN) return;
    const long p = e / MIP_IN;
    out[e] = mip_column(rays, edges, S, r2, p, (int)(e - p * MIP_IN));
}

// One dense layer of a 32-point tile: for every block of 32 outputs o, acc = W'[o][0..K) . X[point][0..K) on the matrix pipe, then
// put(point n, output m, acc) for m < M.  W'[o][k] = W[o * ldw + k] (forward) or W[k * ldw + o] (TRANS: the transposed layer of the backward),
// 0 outside o < M, k < K.  X: the wave's LDS rows (stride MIP_LD); its columns [K, K rounded up to the K-step) must hold zeros.
template <int ARITH, bool TRANS, class Put>
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

// The LDS rows of a tile through the forward (xa / xb: [32][MIP_LD] each):
//   enc -> xa[0,48) (36..47 zero), dir -> xb[128,160) (155..159 zero)
//   layer1: xa -> xb[0,128) h1;  x0: xb -> xa h2;  x1: xa -> xb h3;  x2: xb -> xa[0,128) h4
//   fc_alpha: xa -> xa[131];  fc_feat: xa -> xb[0,128) feat (next to dir);  layers_dir: xb[0,160) -> xa[0,64) hd;  fc_rgb: xa -> xa[128,131)
template <int ARITH>
__global__ __launch_bounds__(64 * MIP_WAVES) void mip_nerf_forward_kernel(long P, int S, const float* __restrict__ rays, const float* __restrict__ edges,
                                                                         float r2, const float* __restrict__ w, float* __restrict__ raw,
                                                                         float* __restrict__ rec) {
    __shared__ float lds[MIP_WAVES * 2 * 32 * MIP_LD];
    NVSR_RACE_PROBE_DELAY(lds);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, n = lane & 31, h = lane >> 5;
    float* xa = lds + wave * 2 * 32 * MIP_LD;
    float* xb = xa + 32 * MIP_LD;
    const long p0 = ((long)blockIdx.x * MIP_WAVES + wave) * 32;
    if (p0 >= P) return;
    const long p = p0 + n;
    const bool live = p < P;
    for (int c = h; c < 64; c += 2) {                    // the lane pair (n, 0), (n, 1) encodes point n
        const float v = (live && c < MIP_IN) ? mip_column(rays, edges, S, r2, p, c) : 0.0f;
        if (c < MIP_ENC) xa[n * MIP_LD + c] = v;
        else xb[n * MIP_LD + MH + c - MIP_ENC] = v;      // (c == 63: the zero of column 155)
    }
    for (int c = MIP_ENC + h; c < 48; c += 2) xa[n * MIP_LD + c] = 0.0f;
    for (int c = MH + 28 + h; c < 160; c += 2) xb[n * MIP_LD + c] = 0.0f;
    wave_sync();
    if (rec) { store_rows(xa, 0, MIP_ENC, rec, MIP_REC, R_ENC, p0, P, lane); store_rows(xb, MH, MIP_DIR, rec, MIP_REC, R_DIR, p0, P, lane); }
    auto dense = [&](int wo, int bo, int M, int K, const float* X, float* Y, int yoff, bool relu) {
        tile_layer<ARITH, false>(w + wo, K, M, K, X, lane, [&](int pt, int m, float a) {
            const float v = __fadd_rn(a, w[bo + m]);
            Y[pt * MIP_LD + yoff + m] = relu ? fmaxf(v, 0.0f) : v;
        });
    };
    dense(MW_L1, MB_L1, MH, MIP_ENC, xa, xb, 0, false);
    if (rec) store_rows(xb, 0, MH, rec, MIP_REC, R_H1, p0, P, lane);
    dense(MW_X0, MB_X0, MH, MH, xb, xa, 0, true);
    if (rec) store_rows(xa, 0, MH, rec, MIP_REC, R_H2, p0, P, lane);
    dense(MW_X1, MB_X1, MH, MH, xa, xb, 0, true);
    if (rec) store_rows(xb, 0, MH, rec, MIP_REC, R_H3, p0, P, lane);
    dense(MW_X2, MB_X2, MH, MH, xb, xa, 0, true);
    if (rec) store_rows(xa, 0, MH, rec, MIP_REC, R_H4, p0, P, lane);
    dense(MW_A, MB_A, 1, MH, xa, xa, 131, false);
    dense(MW_F, MB_F, MH, MH, xa, xb, 0, true);
    if (rec) store_rows(xb, 0, MH, rec, MIP_REC, R_FEAT, p0, P, lane);
    dense(MW_DIR, MB_DIR, MHD, MH + MIP_DIR, xb, xa, 0, true);
    if (rec) store_rows(xa, 0, MHD, rec, MIP_REC, R_HD, p0, P, lane);
    dense(MW_RGB, MB_RGB, 3, MHD, xa, xa, 128, false);
    if (live && h == 0) {
        float4 o = {xa[n * MIP_LD + 128], xa[n * MIP_LD + 129], xa[n * MIP_LD + 130], xa[n * MIP_LD + 131]};
        reinterpret_cast<float4*>(raw)[p] = o;
    }
}

// dL/draw [P][4] -> the pre-activation gradients of every layer (grec, MIP_GREC per point).  LDS rows:
//   G_rgb -> xa[0,3) (3..15 zero);  fc_rgb's input gradient gated by hd > 0 = G_dir -> xb[0,64)
//   (G_dir W_dir)[0,128) gated by feat > 0 = G_feat -> xa[0,128);  G_feat W_feat + G_alpha W_alpha gated by h4 > 0 = G_x2 -> xb
//   G_x2 W_x2 gated by h3 = G_x1 -> xa;  G_x1 W_x1 gated by h2 = G_x0 -> xb;  G_x0 W_x0 = G_1 (layer1 is linear) -> xa
template <int ARITH>
__global__ __launch_bounds__(64 * MIP_WAVES) void mip_nerf_backward_kernel(long P, const float* __restrict__ w, const float* __restrict__ rec,
                                                                          const float* __restrict__ g_raw, float* __restrict__ grec) {
    __shared__ float lds[MIP_WAVES * 2 * 32 * MIP_LD];
    NVSR_RACE_PROBE_DELAY(lds);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, n = lane & 31, h = lane >> 5;
    float* xa = lds + wave * 2 * 32 * MIP_LD;
    float* xb = xa + 32 * MIP_LD;
    const long p0 = ((long)blockIdx.x * MIP_WAVES + wave) * 32;
    if (p0 >= P) return;
    const long p = p0 + n;
    const bool live = p < P;
    const float g_alpha = live ? g_raw[p * 4 + 3] : 0.0f;
    for (int c = h; c < 16; c += 2) xa[n * MIP_LD + c] = (live && c < 3) ? g_raw[p * 4 + c] : 0.0f;
    wave_sync();
    store_rows(xa, 0, 3, grec, MIP_GREC, G_RGB, p0, P, lane);
    if (live && h == 0) grec[p * MIP_GREC + G_A] = g_alpha;
    // (a dead point's record row does not exist: its gate reads are skipped and its gradient rows are zeros)
    auto gate = [&](int off, int pt, int m) { return p0 + pt < P && rec[(p0 + pt) * MIP_REC + off + m] > 0.0f; };
    tile_layer<ARITH, true>(w + MW_RGB, MHD, MHD, 3, xa, lane, [&](int pt, int m, float a) {
        xb[pt * MIP_LD + m] = gate(R_HD, pt, m) ? a : 0.0f;
    });
    store_rows(xb, 0, MHD, grec, MIP_GREC, G_DIR, p0, P, lane);
    tile_layer<ARITH, true>(w + MW_DIR, MH + MIP_DIR, MH, MHD, xb, lane, [&](int pt, int m, float a) {
        xa[pt * MIP_LD + m] = gate(R_FEAT, pt, m) ? a : 0.0f;
    });
    store_rows(xa, 0, MH, grec, MIP_GREC, G_FEAT, p0, P, lane);
    tile_layer<ARITH, true>(w + MW_F, MH, MH, MH, xa, lane, [&](int pt, int m, float a) {
        xb[pt * MIP_LD + m] = gate(R_H4, pt, m) ? __fadd_rn(a, __fmul_rn(g_alpha, w[MW_A + m])) : 0.0f;   // (lane (pt, h) holds point pt's g_alpha)
    });
    store_rows(xb, 0, MH, grec, MIP_GREC, G_X2, p0, P, lane);
    tile_layer<ARITH, true>(w + MW_X2, MH, MH, MH, xb, lane, [&](int pt, int m, float a) { xa[pt * MIP_LD + m] = gate(R_H3, pt, m) ? a : 0.0f; });
    store_rows(xa, 0, MH, grec, MIP_GREC, G_X1, p0, P, lane);
    tile_layer<ARITH, true>(w + MW_X1, MH, MH, MH, xa, lane, [&](int pt, int m, float a) { xb[pt * MIP_LD + m] = gate(R_H2, pt, m) ? a : 0.0f; });
    store_rows(xb, 0, MH, grec, MIP_GREC, G_X0, p0, P, lane);
    tile_layer<ARITH, true>(w + MW_X0, MH, MH, MH, xb, lane, [&](int pt, int m, float a) { xa[pt * MIP_LD + m] = a; });
    store_rows(xa, 0, MH, grec, MIP_GREC, G_L1, p0, P, lane);
}

// partial[slab][wo + m * K + k] = sum over the slab's points of G[p][m] X[p][k] (X = [X1 (K1 columns) | X2 (K - K1 columns)]),
// partial[slab][bo + m] = sum G[p][m] (the tile column k == K, whose operand is 1).  Every (m, k) of a slab is written by exactly one workgroup.
constexpr int MW_SLAB = 8192;
__global__ __launch_bounds__(256) void mip_wgrad_kernel(long P, int M, int K, int K1, const float* __restrict__ G, int goff,
                                                        const float* __restrict__ rec, int x1off, int x2off, int wo, int bo, float* __restrict__ partial) {
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
            if (m < M) a = G[q * MIP_GREC + goff + m];
            if (k < K) b = rec[q * MIP_REC + xo];
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
    float* out = partial + (long)blockIdx.z * MIP_NAT;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const float v = __fadd_rn(__fadd_rn(__fadd_rn(acc[r], red[lane * 16 + r]), red[(64 + lane) * 16 + r]), red[(128 + lane) * 16 + r]);
        const int mr = m0 + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (mr < M) out[k < K ? wo + mr * K + k : bo + mr] = v;
    }
}

__global__ void mip_wgrad_reduce_kernel(int slabs, const float* __restrict__ partial, float* __restrict__ grad) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= MIP_NAT) return;
    float s = partial[i];
    for (int z = 1; z < slabs; ++z) s = __fadd_rn(s, partial[(long)z * MIP_NAT + i]);
    grad[i] = s;
}

static int mip_arith(int arithmetic, int* out) {
    if (arithmetic == NVSR_ARITH_INHERIT) arithmetic = nvsr_get_decoder_arithmetic();
    if (arithmetic == NVSR_ARITH_F32) *out = NVSR_ARITH_F32;
    else if (arithmetic == NVSR_ARITH_BF16X3 || arithmetic == NVSR_ARITH_F16X2) *out = NVSR_ARITH_BF16X3;   // (include/nvsr.h)
    else return NVSR_ERR_SHAPE;
    return NVSR_OK;
}

}  // namespace nvsr

using namespace nvsr;

extern "C" {

int nvsr_mip_encode(int64_t N, int S, const float* rays, const float* edges, double radius, float* out, nvsr_stream_t stream) {
    if (N < 0 || S < 1) return NVSR_ERR_SHAPE;
    if (N == 0) return NVSR_OK;
    if (!rays || !edges || !out) return NVSR_ERR_NULL;
    const int64_t n = N * S * MIP_IN;
    hipLaunchKernelGGL(mip_encode_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (long)(N * S), S, rays, edges,
                       (float)(radius * radius), out);
    return NVSR_CHECK_LAUNCH();
}

int nvsr_mip_nerf_forward_arith(int64_t N, int S, const float* rays, const float* edges, double radius, const float* natural, float* raw,
                                float* record, int arithmetic, nvsr_stream_t stream) {
    int arith;
    if (N < 0 || S < 1 || mip_arith(arithmetic, &arith)) return NVSR_ERR_SHAPE;
    if (N == 0) return NVSR_OK;
    if (!rays || !edges || !natural || !raw) return NVSR_ERR_NULL;
    if (reinterpret_cast<uintptr_t>(raw) % 16) return NVSR_ERR_ALIGN;
    const long P = (long)(N * S);
    const dim3 grid((unsigned)((P + 32 * MIP_WAVES - 1) / (32 * MIP_WAVES)));
    if (arith == NVSR_ARITH_F32)
        hipLaunchKernelGGL(mip_nerf_forward_kernel<NVSR_ARITH_F32>, grid, dim3(64 * MIP_WAVES), 0, (hipStream_t)stream, P, S, rays, edges,
                           (float)(radius * radius), natural, raw, record);
    else
        hipLaunchKernelGGL(mip_nerf_forward_kernel<NVSR_ARITH_BF16X3>, grid, dim3(64 * MIP_WAVES), 0, (hipStream_t)stream, P, S, rays, edges,
                           (float)(radius * radius), natural, raw, record);
    return NVSR_CHECK_LAUNCH();
}

int nvsr_mip_nerf_backward_arith(int64_t P, const float* natural, const float* record, const float* g_raw, float* grad_record, int arithmetic,
                                 nvsr_stream_t stream) {
    int arith;
    if (P < 0 || mip_arith(arithmetic, &arith)) return NVSR_ERR_SHAPE;
    if (P == 0) return NVSR_OK;
    if (!natural || !record || !g_raw || !grad_record) return NVSR_ERR_NULL;
    const dim3 grid((unsigned)((P + 32 * MIP_WAVES - 1) / (32 * MIP_WAVES)));
    if (arith == NVSR_ARITH_F32)
        hipLaunchKernelGGL(mip_nerf_backward_kernel<NVSR_ARITH_F32>, grid, dim3(64 * MIP_WAVES), 0, (hipStream_t)stream, (long)P, natural, record,
                           g_raw, grad_record);
    else
        hipLaunchKernelGGL(mip_nerf_backward_kernel<NVSR_ARITH_BF16X3>, grid, dim3(64 * MIP_WAVES), 0, (hipStream_t)stream, (long)P, natural,
                           record, g_raw, grad_record);
    return NVSR_CHECK_LAUNCH();
}

int64_t nvsr_mip_nerf_wgrad_workspace_floats(int64_t P) {
    return P <= 0 ? 0 : ((P + MW_SLAB - 1) / MW_SLAB) * (int64_t)MIP_NAT;
}

int nvsr_mip_nerf_weight_grad(int64_t P, const float* record, const float* grad_record, float* workspace, float* grad_natural, nvsr_stream_t stream) {
    if (P < 0) return NVSR_ERR_SHAPE;
    if (!grad_natural) return NVSR_ERR_NULL;
    if (P == 0) return hipMemsetAsync(grad_natural, 0, MIP_NAT * sizeof(float), (hipStream_t)stream) == hipSuccess ? NVSR_OK : NVSR_ERR_LAUNCH;
    if (!record || !grad_record || !workspace) return NVSR_ERR_NULL;
    const int slabs = (int)((P + MW_SLAB - 1) / MW_SLAB);
    struct L { int M, K, K1, goff, x1, x2, wo, bo; };
    const L layers[8] = {{MH, MIP_ENC, MIP_ENC, G_L1, R_ENC, 0, MW_L1, MB_L1},  {MH, MH, MH, G_X0, R_H1, 0, MW_X0, MB_X0},
                         {MH, MH, MH, G_X1, R_H2, 0, MW_X1, MB_X1},             {MH, MH, MH, G_X2, R_H3, 0, MW_X2, MB_X2},
                         {MHD, MH + MIP_DIR, MH, G_DIR, R_FEAT, R_DIR, MW_DIR, MB_DIR}, {1, MH, MH, G_A, R_H4, 0, MW_A, MB_A},
                         {3, MHD, MHD, G_RGB, R_HD, 0, MW_RGB, MB_RGB},          {MH, MH, MH, G_FEAT, R_H4, 0, MW_F, MB_F}};
    for (const L& l : layers) {
        const dim3 grid((unsigned)((l.M + 31) / 32), (unsigned)(l.K / 32 + 1), (unsigned)slabs);     // (k tiles up to and including k == K)
        hipLaunchKernelGGL(mip_wgrad_kernel, grid, dim3(256), 0, (hipStream_t)stream, (long)P, l.M, l.K, l.K1, grad_record, l.goff, record, l.x1, l.x2,
                           l.wo, l.bo, workspace);
        if (hipGetLastError() != hipSuccess) return NVSR_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(mip_wgrad_reduce_kernel, dim3((MIP_NAT + 255) / 256), dim3(256), 0, (hipStream_t)stream, slabs, workspace, grad_natural);
    return NVSR_CHECK_LAUNCH();
}

}  // extern "C"
