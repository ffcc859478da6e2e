// What the kernels of the generic decoder geometries in NVSR_ARITH_F16X2 share (generic_fused_limb.hip: the evaluation; generic_fused_bwd_limb.hip:
// the plane gradients, which recompute the forward): the split of a K-block into two f16 limbs and the hidden layer on the packed fragments.
// Both compile the SAME layer out of this header, so the backward's recomputed activations -- and its gate bits -- are the forward launch's.
#pragma once
#include "generic_fused_core.h"
#include "limb_core.h"

namespace nvsr {

constexpr float GFL_UNSCALE = 1.0f / 4096.0f;         // 2^-(F16_SW + F16_SX)
static_assert(F16_SW + F16_SX == 12, "the accumulator of a limb layer holds 2^12 W x");

// K-blocks and output tiles of a hidden layer with K input columns
NVSR_CX int gfl_kb(int K) { return (K + 15) >> 4; }
NVSR_CX int gfl_tt(int hidden) { return (hidden + 31) >> 5; }
// gen_layer_in (generic_core.h) for host and device: in_features of decoder layer l
__host__ __device__ inline int gfl_layer_in(const GenGeom& g, bool rgb, int l) {
    const int k0 = rgb ? g.Kr : g.Kd;
    return l == 0 ? k0 : g.hidden + (gen_skip_layer(l - 1, g.skip) ? k0 : 0);
}
// 8 values, already scaled, in two f16 limbs: hi = RN(e), lo = RN(e - hi) (split_all<2>'s arithmetic, straight-line)
__device__ __forceinline__ void gfl_split_scaled(const float (&e)[8], Limbs<2>& out) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        out.v[0][j] = f16_pair(e[2 * j + 1], e[2 * j]);
        out.v[1][j] = f16_pair(f16_rest<1>(e[2 * j + 1], out.v[0][j]), f16_rest<0>(e[2 * j], out.v[0][j]));
    }
}
// the 8 values of a lane's K-block, scaled by 2^4, in two f16 limbs: hi = RN(16 x), lo = RN(16 x - hi)
__device__ __forceinline__ void gfl_split(const float (&v)[8], Limbs<2>& out) {
    float e[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) e[i] = __fmul_rn(v[i], F16_X_SCALE);
    gfl_split_scaled(e, out);
}

// acc[t] (+)= 2^12 W[32 t + m][k] . [X1 | X2][point][k] in two f16 limbs.  wp: the layer's fragments, 16 bytes per lane: [kb][t][limb][64];
// row: this lane's point's row; X1 = row[x1 .. x1 + K1), X2 = row[x2 .. x2 + K2), x1 and x2 multiples of 4.
template <int NT>
__device__ __forceinline__ void gfl_layer(f32x16 (&acc)[NT], const float* row, int K1, int x1, int K2, int x2, const u32x4* __restrict__ wp, int TT,
                                          int lane, int h) {
    const int K = K1 + K2, KB = gfl_kb(K);
    const bool x2_aligned = (K1 & 3) == 0;
    auto fetch_a = [&](int kb, u32x4 (&fa)[NT][2]) GEN_INL {
        const u32x4* f = wp + (long)kb * TT * 128 + lane;
#pragma unroll
        for (int t = 0; t < NT; ++t)
            if (t < TT) { fa[t][0] = f[t * 128]; fa[t][1] = f[t * 128 + 64]; }
    };
    auto fetch_b = [&](int kb, float (&v)[8]) GEN_INL {
        const int k8 = 16 * kb + 8 * h;
        const float* src = nullptr;
        if (k8 + 8 <= K1) src = row + x1 + k8;
        else if (k8 >= K1 && k8 + 8 <= K && x2_aligned) src = row + x2 + (k8 - K1);
        if (src) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(src), b = *reinterpret_cast<const f32x4*>(src + 4);
#pragma unroll
            for (int i = 0; i < 4; ++i) { v[i] = a[i]; v[4 + i] = b[i]; }
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int kk = k8 + i, kc = kk < K ? kk : K - 1;
                const float xv = row[kc < K1 ? x1 + kc : x2 + (kc - K1)];
                v[i] = kk < K ? xv : 0.0f;
            }
        }
    };
    u32x4 fa[NT][2];
    float v[8];
    Limbs<2> xb;
    fetch_a(0, fa);
    fetch_b(0, v);
    gfl_split(v, xb);
    for (int kb = 0; kb < KB; ++kb) {
        u32x4 fn[NT][2];
        float vn[8];
        const int kn = kb + 1 < KB ? kb + 1 : kb;
        fetch_a(kn, fn);
        fetch_b(kn, vn);
#pragma unroll
        for (int t = 0; t < NT; ++t)
            if (t < TT) {
#pragma unroll
                for (int p = 0; p < 3; ++p) acc[t] = mfma_limb<2>(fa[t][limb_w(2, p)], xb.v[limb_x(2, p)], acc[t]);
            }
        gfl_split(vn, xb);
#pragma unroll
        for (int t = 0; t < NT; ++t)
            if (t < TT) { fa[t][0] = fn[t][0]; fa[t][1] = fn[t][1]; }
    }
}

}  // namespace nvsr
