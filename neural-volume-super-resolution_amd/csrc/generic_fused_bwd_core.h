// What the two fused backward kernels of the generic decoder geometries share (generic_fused_bwd.hip: exact f32; generic_fused_bwd_limb.hip:
// the transposed hidden layers in two f16 limbs): the exact-f32 transposed chain, which both run for the heads, and everything behind the chain
// -- the view plane's and the position planes' scatter through the combination rules and the taps.  Both compile the SAME scatter out of this
// header: the limb kernel differs from the f32 one in the hidden layers only.
#pragma once
#include "generic_fused_core.h"

namespace nvsr {

struct GradPlanesN { float* g[NVSR_MAX_POSITION_PLANES + 1]; };
// the caller's array of plane gradients -> gp; false: no plane is wanted (a NULL array, or NULL entries only) and nothing is launched
static inline bool gfb_wanted(float* const* d_planes, int np, GradPlanesN* gp) {
    bool want = false;
    if (d_planes)
        for (int d = 0; d <= np; ++d) { gp->g[d] = d_planes[d]; want = want || d_planes[d] != nullptr; }
    return want;
}

// the row plan of a backward kernel (gen_fused_bwd_plan: f32; gen_fused_bwd_limb_plan: two f16 limbs)
struct GenFusedBwdPlan {
    int nt, cls, waves;
    int ld, xd_off, h_off, dout_off, gate_off, gw;      // gw: gate words per layer
};

// acc[t] (+)= sum_m dZ[point][m] . W[m][kbase + 32 t + k] over the layered route's m pairs: the chain of generic_dgrad_kernel, NT tiles at once.
// dZ = row[dz .. dz + M) (already gated); W row-major [M][K] in global memory; kn: how many columns from kbase on exist.
// A: lane (k, h) = W[m0 + 2s + h][k] -- the lanes of a half read 32 consecutive floats of one row;  B: lane (n, h) = dZ[point n][m0 + 2s + h]
template <int NT>
__device__ __forceinline__ void gf_layer_t(f32x16 (&acc)[NT], const float* row, int dz, int M, const float* __restrict__ W, int K, int kbase, int kn,
                                           int n, int h) {
    const int Mp = (M + 31) & ~31;
    int col[NT];
    bool cok[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        cok[t] = 32 * t + n < kn;
        col[t] = kbase + (cok[t] ? 32 * t + n : 0);
    }
    float a[GF_U][NT], bv[GF_U];
    auto fetch = [&](int m0, float (&fa)[GF_U][NT], float (&fb)[GF_U]) GEN_INL {
#pragma unroll
        for (int u = 0; u < GF_U; ++u) {
            const int mm = m0 + 2 * u + h, mc = mm < M ? mm : M - 1;
            const bool mok = mm < M;
            const float zv = row[dz + mc];
            fb[u] = mok ? zv : 0.0f;
            const float* wr = W + (long)mc * K;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const float wv = wr[col[t]];
                fa[u][t] = (mok && cok[t]) ? wv : 0.0f;
            }
        }
    };
    fetch(0, a, bv);
    for (int m0 = 0; m0 < Mp; m0 += 2 * GF_U) {
        float an[GF_U][NT], bn[GF_U];
        fetch(m0 + 2 * GF_U, an, bn);
#pragma unroll
        for (int u = 0; u < GF_U; ++u)
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] = mfma32(a[u][t], bv[u], acc[t]);
#pragma unroll
        for (int u = 0; u < GF_U; ++u) {
            bv[u] = bn[u];
#pragma unroll
            for (int t = 0; t < NT; ++t) a[u][t] = an[u][t];
        }
    }
}

template <int NT>
__device__ __forceinline__ void gf_zero(f32x16 (&acc)[NT]) {
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
}

// row[dx + k] = row[dx + k] + sum_m dZ[m] W[m][koff + k], k < Kn, in groups of NT tiles (the ACCUM launches of the layered route)
template <int NT>
__device__ __forceinline__ void gf_input_grad(float* row, int dz, int M, const float* __restrict__ W, int K, int koff, int Kn, int dx, int n, int h) {
    for (int k0 = 0; k0 < Kn; k0 += 32 * NT) {
        f32x16 acc[NT];
        gf_zero<NT>(acc);
        gf_layer_t<NT>(acc, row, dz, M, W, K, koff + k0, Kn - k0, n, h);
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int k = k0 + 32 * t + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (k < Kn) row[dx + k] = __fadd_rn(row[dx + k], acc[t][r]);
            }
    }
}

// dz[m] = acc's value of output m where the gate bit of m is set, +0.0 where it is not: the gradient of a hidden layer's output becomes its dZ
template <int NT>
__device__ __forceinline__ void gf_store_gated(const f32x16 (&acc)[NT], float* dz, int hidden, const unsigned* words, int gw, int h) {
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const unsigned bits = t < gw ? words[t] : 0u;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int j = (r & 3) + 8 * (r >> 2) + 4 * h, m = 32 * t + j;
            if (m < hidden) dz[m] = (bits >> j) & 1u ? acc[t][r] : 0.0f;
        }
    }
}

// a decoder's share of one atomic: v times the tap weight under gen_scatter's rule (generic.hip: nothing is added for v == 0)
__device__ __forceinline__ float gf_tap_term(float v, float w) { return v == 0.0f ? 0.0f : v * w; }

// ---- the view plane: the transpose of combine_all_planes; 'avg' / 'mult' leave the combined position feature's gradient in dXr ----
// rows: the wave's 32 rows of stride ld, dXr in columns [0, Kr), Xd (the forward's own pp under 'mult') at xd_off; base: the wave's first slot
__device__ __forceinline__ void gfb_view_scatter(const SceneDevN& sc, const GenGeom& g, float* rows, int ld, int xd_off, const GradPlanesN& gp, float vgx,
                                                 float vgy, long base, long P, int n, int h) {
    float* __restrict__ gv = gp.g[g.np];
    if (gv || g.view == 1 || g.view == 2) {
        const float* __restrict__ plv = sc.plane[g.np];
        const int H = sc.ph[g.np], W = sc.pw[g.np], Cv = g.Cv, c0 = g.view >= 3 ? g.np * g.C : 0;
        for (int i = 0; i < 16; ++i) {
            const int pt = 2 * i + h;
            const float px = __shfl(vgx, pt), py = __shfl(vgy, pt);
            const bool plive = base + pt < P;
            float* r = rows + pt * ld;
            if (sc.bicubic) {
                const CubicTaps t = gen_cubic_taps(H, W, px, py, sc.align);
                for (int c = n; c < Cv; c += 32) {
                    const float v = r[c0 + c];
                    float val = v;
                    if (g.view == 1) { val = v * 0.5f; r[c] = val; }
                    if (g.view == 2) { val = v * r[xd_off + c]; r[c] = v * __fadd_rn(1.0f, gen_cubic_blend(plv, W, Cv, t, c)); }
                    if (!plive || !gv || val == 0.0f) continue;
#pragma unroll
                    for (int a = 0; a < 4; ++a)
#pragma unroll
                        for (int b = 0; b < 4; ++b) {
                            const float wt = t.cx[b] * t.cy[a];
                            if (wt != 0.0f) unsafeAtomicAdd(gv + ((long)t.iy[a] * W + t.ix[b]) * Cv + c, val * wt);
                        }
                }
            } else {
                const GenTaps t = gen_taps(H, W, Cv, px, py, sc.align);
                for (int c = n; c < Cv; c += 32) {
                    const float v = r[c0 + c];
                    float val = v;
                    if (g.view == 1) { val = v * 0.5f; r[c] = val; }
                    if (g.view == 2) { val = v * r[xd_off + c]; r[c] = v * __fadd_rn(1.0f, gen_blend(plv, t, c)); }
                    if (!plive || !gv || val == 0.0f) continue;
#pragma unroll
                    for (int a = 0; a < 4; ++a)
                        if (t.w[a] != 0.0f) unsafeAtomicAdd(gv + t.o[a] + c, val * t.w[a]);
                }
            }
        }
        __syncthreads();
    }
}

// ---- the position planes: combine_pos_planes transposed; the two decoders' products of a (tap, channel) in one atomic ----
// dXd at xd_off, dXr in columns [0, Kr) of every row; (n0, n1, n2): the lane's point's normalised position
__device__ __forceinline__ void gfb_plane_scatter(const SceneDevN& sc, const GenGeom& g, const float* rows, int ld, int xd_off, const GradPlanesN& gp,
                                                  float n0, float n1, float n2, long base, long P, int n, int h) {
    const bool xr_split = g.proj == 2 || g.view == 4;       // dXr holds a column per (plane, channel)
    for (int d = 0; d < g.np; ++d) {
        float* __restrict__ gd = gp.g[d];
        if (!gd) continue;
        float gx, gy;
        gen_pos_grid(sc, d, n0, n1, n2, gx, gy);
        const int H = sc.ph[d], W = sc.pw[d], C = g.C;
        for (int i = 0; i < 16; ++i) {
            const int pt = 2 * i + h;
            const float px = __shfl(gx, pt), py = __shfl(gy, pt);
            const bool plive = base + pt < P;
            const float* r = rows + pt * ld;
            auto value = [&](int c, float& va, float& vb) GEN_INL {
                va = g.proj == 2 ? r[xd_off + d * C + c] : r[xd_off + c];
                vb = xr_split ? r[d * C + c] : r[c];
                if (g.proj == 1) {
                    va = va / (float)g.np;
                    if (!xr_split) vb = vb / (float)g.np;
                }
            };
            if (sc.bicubic) {
                const CubicTaps t = gen_cubic_taps(H, W, px, py, sc.align);
                for (int c = n; c < C; c += 32) {
                    float va, vb;
                    value(c, va, vb);
                    if (!plive || (va == 0.0f && vb == 0.0f)) continue;
#pragma unroll
                    for (int a = 0; a < 4; ++a)
#pragma unroll
                        for (int b = 0; b < 4; ++b) {
                            const float wt = t.cx[b] * t.cy[a];
                            if (wt != 0.0f) unsafeAtomicAdd(gd + ((long)t.iy[a] * W + t.ix[b]) * C + c, __fadd_rn(gf_tap_term(va, wt), gf_tap_term(vb, wt)));
                        }
                }
            } else {
                const GenTaps t = gen_taps(H, W, C, px, py, sc.align);
                for (int c = n; c < C; c += 32) {
                    float va, vb;
                    value(c, va, vb);
                    if (!plive || (va == 0.0f && vb == 0.0f)) continue;
#pragma unroll
                    for (int a = 0; a < 4; ++a)
                        if (t.w[a] != 0.0f) unsafeAtomicAdd(gd + t.o[a] + c, __fadd_rn(gf_tap_term(va, t.w[a]), gf_tap_term(vb, t.w[a])));
                }
            }
        }
    }
}

}  // namespace nvsr
