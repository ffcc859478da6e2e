// TwoDimPlanesModel.forward for ANY decoder geometry (inference): the fallback behind the MFMA kernels that are compiled for the shipped
// one (3 + 1 planes x 48 channels, 'avg' / 'concat_pos', 4 + 4 layers x 128).
//
// Reference: models.py:381-421 with the layer lists of the constructor :169-195, is_skip_layer :203-207, combine_pos_planes :355-361,
// combine_all_planes :363-379; the shipped YAMLs list dec_channels 256, proj_combination sum / concat, 24-channel planes and skip layers as
// alternatives (config/TrainModels.yml:78,82,92).
//
// Forward: three plain kernels, activations through HBM (this is the compatibility path, not the hot one):
//   generic_inputs_kernel   one thread per (point, input column): normalise, project, 4 bilinear taps per plane, combine -> the density
//                           decoder's input Xd [P][Kd] and the colour decoder's input Xr [P][Kr]
//   generic_linear_kernel   Y[P][M] = act(b + W[M][K1 + K2] . [X1[P][K1] | X2[P][K2]])  (X2 = the skip connection's second operand) on
//                           v_mfma_f32_32x32x2_f32 (exact f32 products, k in order), one 32 x 32 tile per wave, operands staged through LDS
//   ray_points_kernel       x[N*S][6] = [ro + rd * z, viewdir]  (run_network's input, train_utils.py:15-64,111)
// Backward (the reference differentiates the same forward with torch.autograd): the forward of a chunk is recomputed with every layer's
// output kept, then per layer, top down,
//   generic_wgrad_kernel    dW[M][K] += dZ^T . [X1 | X2],  db += column sums of dZ   (dZ = dY where the layer's output is > 0; the points
//                           are the contraction index: MFMA operands straight from memory, partial tiles added with float atomics)
//   generic_dgrad_kernel    dX[P][columns of W] (+)= dZ . W   (the forward's tiling with W read transposed)
// and generic_inputs_backward_kernel scatters the gradients of the two decoder inputs through the combination rule and the four
// bilinear taps into the channel-last gradient planes (float atomics, like grid_sampler_2d_backward).
// Evaluation has a second route, generic_fused.hip (one launch, activations in LDS, the same bits); what the two share is generic_core.h.
#include "generic_core.h"

namespace nvsr {

struct GradPlanesN { float* g[NVSR_MAX_POSITION_PLANES + 1]; };
// gen_sample's transpose: v times the tap weights, added into the gradient plane
__device__ __forceinline__ void gen_scatter(const SceneDevN& sc, int d, int Cc, float gx, float gy, int c, float v, float* __restrict__ g) {
    if (!g || v == 0.0f) return;
    if (sc.bicubic) {
        const CubicTaps t = gen_cubic_taps(sc.ph[d], sc.pw[d], gx, gy, sc.align);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float w = t.cx[j] * t.cy[i];
                if (w != 0.0f) unsafeAtomicAdd(g + ((long)t.iy[i] * sc.pw[d] + t.ix[j]) * Cc + c, v * w);
            }
        return;
    }
    const GenTaps t = gen_taps(sc.ph[d], sc.pw[d], Cc, gx, gy, sc.align);
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (t.w[i] != 0.0f) unsafeAtomicAdd(g + t.o[i] + c, v * t.w[i]);
}

__global__ void generic_inputs_kernel(SceneDevN sc, GenGeom g, long P, const float* __restrict__ x, const float* __restrict__ noise,
                                      float* __restrict__ Xd, float* __restrict__ Xr) {
    const int K = g.Kd + g.Kr;
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= P * K) return;
    const long p = idx / K;
    const int j = (int)(idx - p * K);
    const float* q = x + p * 6;
    // (cart2az_el nerf_helpers.py:492-496)
    float n0, n1, n2;
    gen_position(sc, q, noise, p, n0, n1, n2);
    auto pos_feat = [&](int d, int c) GEN_INL {
        float gx, gy;
        gen_pos_grid(sc, d, n0, n1, n2, gx, gy);
        return gen_sample(sc, d, g.C, gx, gy, c);
    };
    auto view_feat = [&](int c) GEN_INL {
        float gx, gy;
        gen_view_grid(sc, q, gx, gy);
        return gen_sample(sc, g.np, g.Cv, gx, gy, c);
    };
    auto combined_pos = [&](int c) GEN_INL {                       // combine_pos_planes, column c of its result (stack(...).sum(0) / .mean(0): plane by plane)
        if (g.proj == 2) return pos_feat(c / g.C, c % g.C);
        float s = pos_feat(0, c);
        for (int d = 1; d < g.np; ++d) s = __fadd_rn(s, pos_feat(d, c));
        return gen_combine_pos(g.proj, s, g.np);
    };
    if (j < g.Kd) { Xd[p * g.Kd + j] = combined_pos(j); return; }
    const int c = j - g.Kd;
    float v;
    if (g.view == 4) v = c < g.np * g.C ? pos_feat(c / g.C, c % g.C) : view_feat(c - g.np * g.C);       // cat(pos_planes + [viewdir])
    else if (g.view == 3) v = c < g.Kd ? combined_pos(c) : view_feat(c - g.Kd);                        // cat([combined, viewdir])
    else {
        const float pp = combined_pos(c), vv = view_feat(c);
        v = gen_combine_view(g.view, pp, vv);
    }
    Xr[p * g.Kr + c] = v;
}

// Y[p][yoff + m] (row stride ldy) = act(b[m] + sum_k W[m][k] X[p][k]),  X = [X1 | X2] with K1 + K2 columns, W row-major [M][K1 + K2]
constexpr int GL_PTS = 128, GL_OUT = 32, GL_K = 32, GL_LD = GL_K + 1;
template <bool RELU>
__global__ __launch_bounds__(256) void generic_linear_kernel(long P, int M, int K1, int K2, const float* __restrict__ X1, const float* __restrict__ X2,
                                                            const float* __restrict__ Wt, const float* __restrict__ b, float* __restrict__ Y, int ldy,
                                                            int yoff) {
    __shared__ float xs[GL_PTS * GL_LD], ws[GL_OUT * GL_LD];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, n = lane & 31, h = lane >> 5;
    const long p0 = (long)blockIdx.x * GL_PTS;
    const int o0 = blockIdx.y * GL_OUT, K = K1 + K2;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    for (int k0 = 0; k0 < K; k0 += GL_K) {
        __syncthreads();
        for (int e = tid; e < GL_PTS * GL_K; e += 256) {
            const int pt = e / GL_K, k = e % GL_K;
            const long p = p0 + pt;
            const int kk = k0 + k;
            float v = 0.0f;
            if (p < P && kk < K) v = kk < K1 ? X1[p * K1 + kk] : X2[p * K2 + (kk - K1)];
            xs[pt * GL_LD + k] = v;
        }
        for (int e = tid; e < GL_OUT * GL_K; e += 256) {
            const int o = e / GL_K, k = e % GL_K;
            ws[o * GL_LD + k] = (o0 + o < M && k0 + k < K) ? Wt[(long)(o0 + o) * K + k0 + k] : 0.0f;
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < GL_K / 2; ++s)      // A: lane (m, h) = W[o0 + m][2s + h];  B: lane (n, h) = X[point n of this wave][2s + h]
            acc = mfma32(ws[n * GL_LD + 2 * s + h], xs[(wave * 32 + n) * GL_LD + 2 * s + h], acc);
    }
    const long p = p0 + wave * 32 + n;
    if (p >= P) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = o0 + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (m < M) {
            float v = __fadd_rn(acc[r], b[m]);
            if (RELU) v = fmaxf(v, 0.0f);
            Y[p * ldy + yoff + m] = v;
        }
    }
}

__global__ void ray_points_kernel(long N, int S, const float* __restrict__ rays, const float* __restrict__ z, float* __restrict__ x) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N * S) return;
    const float* r = rays + (i / S) * 11;
    const float zc = z[i];
    float* o = x + i * 6;
    o[0] = __fadd_rn(r[0], __fmul_rn(r[3], zc));
    o[1] = __fadd_rn(r[1], __fmul_rn(r[4], zc));
    o[2] = __fadd_rn(r[2], __fmul_rn(r[5], zc));
    o[3] = r[8]; o[4] = r[9]; o[5] = r[10];
}

// dX[p][xoff + k] (row stride ldx; ACCUM: +=) = sum_m dZ[p][m] W[m][koff + k], k < Kn;  dZ[p][m] = dY[p * ldd + doff + m], zeroed where
// Hmask[p][m] <= 0 (Hmask = the layer's post-ReLU output, NULL for the linear heads);  W row-major [M][K]
template <bool ACCUM>
__global__ __launch_bounds__(256) void generic_dgrad_kernel(long P, int M, int K, int koff, int Kn, const float* __restrict__ dY, int ldd, int doff,
                                                           const float* __restrict__ Hmask, const float* __restrict__ Wt, float* __restrict__ dX,
                                                           int ldx, int xoff) {
    __shared__ float xs[GL_PTS * GL_LD], ws[GL_OUT * GL_LD];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, n = lane & 31, h = lane >> 5;
    const long p0 = (long)blockIdx.x * GL_PTS;
    const int o0 = blockIdx.y * GL_OUT;                    // first output column (k) of this tile
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    for (int m0 = 0; m0 < M; m0 += GL_K) {
        __syncthreads();
        for (int e = tid; e < GL_PTS * GL_K; e += 256) {
            const int pt = e / GL_K, mm = m0 + e % GL_K;
            const long p = p0 + pt;
            float v = 0.0f;
            if (p < P && mm < M) {
                v = dY[p * ldd + doff + mm];
                if (Hmask && !(Hmask[p * M + mm] > 0.0f)) v = 0.0f;
            }
            xs[pt * GL_LD + e % GL_K] = v;
        }
        for (int e = tid; e < GL_OUT * GL_K; e += 256) {
            const int o = e % GL_OUT, mm = m0 + e / GL_OUT;      // consecutive threads -> consecutive k of one row of W
            ws[o * GL_LD + e / GL_OUT] = (o0 + o < Kn && mm < M) ? Wt[(long)mm * K + koff + o0 + o] : 0.0f;
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < GL_K / 2; ++s)      // A: lane (k, h) = W[m0 + 2s + h][k];  B: lane (n, h) = dZ[point n of this wave][m0 + 2s + h]
            acc = mfma32(ws[n * GL_LD + 2 * s + h], xs[(wave * 32 + n) * GL_LD + 2 * s + h], acc);
    }
    const long p = p0 + wave * 32 + n;
    if (p >= P) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int k = o0 + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (k < Kn) {
            float* q = dX + p * ldx + xoff + k;
            *q = ACCUM ? __fadd_rn(*q, acc[r]) : acc[r];
        }
    }
}

// dW[m][k] += sum_p dZ[p][m] Xc[p][k] for k < K = K1 + K2 (Xc = [X1 | X2]),  db[m] += sum_p dZ[p][m] (the column k == K of the tile grid,
// whose operand is 1).  Workgroup = one 32 x 32 tile of (m, k) x a slab of GW_PTS points (generic_core.h), a quarter of the slab per wave.
__global__ __launch_bounds__(256) void generic_wgrad_kernel(long P, int M, int K1, int K2, const float* __restrict__ dY, int ldd, int doff,
                                                           const float* __restrict__ Hmask, const float* __restrict__ X1, const float* __restrict__ X2,
                                                           float* __restrict__ dW, float* __restrict__ db) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, n = lane & 31, h = lane >> 5;
    const int m0 = blockIdx.x * 32, k0 = blockIdx.y * 32, K = K1 + K2;
    const long pa = (long)blockIdx.z * GW_PTS + wave * (GW_PTS / 4), pb = min(pa + GW_PTS / 4, P);
    const int m = m0 + n, k = k0 + n;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    for (long ps = pa; ps < pb; ps += 2) {                   // (uniform trip count: every lane takes part in every MFMA)
        const long p = ps + h;
        float a = 0.0f, b = 0.0f;
        if (p < pb) {
            if (m < M) {
                a = dY[p * ldd + doff + m];
                if (Hmask && !(Hmask[p * M + m] > 0.0f)) a = 0.0f;
            }
            if (k < K1) b = X1[p * K1 + k];
            else if (k < K) b = X2[p * K2 + (k - K1)];
            else if (k == K) b = 1.0f;
        }
        acc = mfma32(a, b, acc);                              // A: lane (m, h) = dZ[p][m];  B: lane (k, h) = Xc[p][k]
    }
    if (k > K) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int mr = m0 + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (mr < M) unsafeAtomicAdd(k < K ? dW + (long)mr * K + k : db + mr, acc[r]);
    }
}

// gradients of the decoder inputs -> gradient planes: the transpose of generic_inputs_kernel, one thread per (point, input column)
__global__ void generic_inputs_backward_kernel(SceneDevN sc, GenGeom g, long P, const float* __restrict__ x, const float* __restrict__ noise,
                                               const float* __restrict__ dXd, const float* __restrict__ dXr, GradPlanesN gp) {
    const int K = g.Kd + g.Kr;
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= P * K) return;
    const long p = idx / K;
    const int j = (int)(idx - p * K);
    const float* q = x + p * 6;
    float n0, n1, n2;
    gen_position(sc, q, noise, p, n0, n1, n2);
    auto pos_grid = [&](int d, float& gx, float& gy) GEN_INL { gen_pos_grid(sc, d, n0, n1, n2, gx, gy); };
    auto view_grid = [&](float& gx, float& gy) GEN_INL { gen_view_grid(sc, q, gx, gy); };
    auto scatter_plane = [&](int d, int c, float v) GEN_INL {         // position plane d, channel c
        float gx, gy;
        pos_grid(d, gx, gy);
        gen_scatter(sc, d, g.C, gx, gy, c, v, gp.g[d]);
    };
    auto scatter_view = [&](int c, float v) GEN_INL {
        float gx, gy;
        view_grid(gx, gy);
        gen_scatter(sc, g.np, g.Cv, gx, gy, c, v, gp.g[g.np]);
    };
    auto pos_value = [&](int d, int c) GEN_INL { float gx, gy; pos_grid(d, gx, gy); return gen_sample(sc, d, g.C, gx, gy, c); };
    auto scatter_pos = [&](int c, float v) GEN_INL {                 // combine_pos_planes transposed, column c of its result
        if (g.proj == 2) { scatter_plane(c / g.C, c % g.C, v); return; }
        const float f = g.proj == 1 ? v / (float)g.np : v;
        for (int d = 0; d < g.np; ++d) scatter_plane(d, c, f);
    };
    auto combined_pos = [&](int c) GEN_INL {
        if (g.proj == 2) return pos_value(c / g.C, c % g.C);
        float s = pos_value(0, c);
        for (int d = 1; d < g.np; ++d) s = __fadd_rn(s, pos_value(d, c));
        return g.proj == 1 ? __fdiv_rn(s, (float)g.np) : s;
    };
    if (j < g.Kd) { scatter_pos(j, dXd[p * g.Kd + j]); return; }
    const int c = j - g.Kd;
    const float v = dXr[p * g.Kr + c];
    if (g.view == 4) {
        if (c < g.np * g.C) scatter_plane(c / g.C, c % g.C, v);
        else scatter_view(c - g.np * g.C, v);
    } else if (g.view == 3) {
        if (c < g.Kd) scatter_pos(c, v);
        else scatter_view(c - g.Kd, v);
    } else if (g.view == 0) {
        scatter_pos(c, v);
        scatter_view(c, v);
    } else if (g.view == 1) {
        scatter_pos(c, v * 0.5f);
        scatter_view(c, v * 0.5f);
    } else {                                                 // mult: pp * (1 + vv)
        float gx, gy;
        view_grid(gx, gy);
        const float pp = combined_pos(c), vv = gen_sample(sc, g.np, g.Cv, gx, gy, c);
        scatter_pos(c, v * __fadd_rn(1.0f, vv));
        scatter_view(c, v * pp);
    }
}

constexpr long GEN_CHUNK = 1L << 20;       // points per pass of the layer stack (bounds the activation workspace)
// (the backward keeps every layer's output of a chunk of GEN_BWD_CHUNK points: generic_core.h)

int gen_wgrad_launch(long n, int M, int K1, int K2, const float* dY, int ldd, int doff, const float* Hmask, const float* X1, const float* X2,
                     float* dW, float* db, hipStream_t stream) {
    const unsigned slabs = (unsigned)((n + GW_PTS - 1) / GW_PTS);
    hipLaunchKernelGGL(generic_wgrad_kernel, dim3((M + 31) / 32, (K1 + K2 + 1 + 31) / 32, slabs), dim3(256), 0, stream, n, M, K1, K2, dY, ldd, doff, Hmask,
                       X1, X2, dW, db);
    return NVSR_CHECK_LAUNCH();
}

}  // namespace nvsr

using namespace nvsr;

extern "C" {

static int64_t gen_natural_floats(const nvsr_decoder_geometry* geom, int np) {
    GenGeom g;
    if (gen_resolve(geom, &g, np)) return -1;
    int64_t n = 0;
    for (int l = 0; l < g.nd; ++l) n += (int64_t)g.hidden * gen_layer_in(g, false, l) + g.hidden;
    n += g.hidden + 1;
    for (int l = 0; l < g.nr; ++l) n += (int64_t)g.hidden * gen_layer_in(g, true, l) + g.hidden;
    n += 3 * g.hidden + 3;
    return n;
}
int64_t nvsr_generic_decoder_natural_floats(const nvsr_decoder_geometry* geom) { return gen_natural_floats(geom, 3); }
int64_t nvsr_generic_decoder_natural_floats_ext(const nvsr_decoder_geometry* geom, int num_position_planes) { return gen_natural_floats(geom, num_position_planes); }

static int64_t gen_workspace_floats(const nvsr_decoder_geometry* geom, int np, int64_t P) {
    GenGeom g;
    if (gen_resolve(geom, &g, np) || P < 0) return -1;
    const int64_t c = P < GEN_CHUNK ? P : GEN_CHUNK;
    return c * (int64_t)(g.Kd + g.Kr + 2 * g.hidden);
}
int64_t nvsr_generic_decode_workspace_floats(const nvsr_decoder_geometry* geom, int64_t P) { return gen_workspace_floats(geom, 3, P); }
int64_t nvsr_generic_decode_workspace_floats_ext(const nvsr_decoder_geometry* geom, int num_position_planes, int64_t P) {
    return gen_workspace_floats(geom, num_position_planes, P);
}

static int gen_decode(const SceneDevN& sc, const GenGeom& g, const float* natural, int64_t P, const float* x, const float* coord_noise, float* out,
                      float* workspace, hipStream_t stream) {
    if (!natural || !x || !out || !workspace) return NVSR_ERR_NULL;
    if (int e = gen_check_scene(sc, g)) return e;
    if (P < 0) return NVSR_ERR_SHAPE;
    for (int64_t a = 0; a < P; a += GEN_CHUNK) {
        const long n = (long)((P - a) < GEN_CHUNK ? (P - a) : GEN_CHUNK);
        float* Xd = workspace;
        float* Xr = Xd + n * g.Kd;
        float* H[2] = {Xr + n * g.Kr, Xr + n * g.Kr + n * g.hidden};
        const long threads = n * (g.Kd + g.Kr);
        hipLaunchKernelGGL(generic_inputs_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream, sc, g, n, x + a * 6,
                           coord_noise ? coord_noise + a * 3 : nullptr, Xd, Xr);
        if (int e = NVSR_CHECK_LAUNCH()) return e;
        const float* w = natural;
        const dim3 pts((unsigned)((n + GL_PTS - 1) / GL_PTS));
        for (int dec = 0; dec < 2; ++dec) {
            const bool rgb = dec == 1;
            const float* in0 = rgb ? Xr : Xd;
            const int k0 = rgb ? g.Kr : g.Kd, nl = rgb ? g.nr : g.nd;
            const float* cur = in0;
            int cur_k = k0;
            for (int l = 0; l < nl; ++l) {
                const bool skip = l > 0 && gen_skip_layer(l - 1, g.skip);       // x = cat(x, input) in front of this layer (models.py:397-399)
                const int K1 = cur_k, K2 = skip ? k0 : 0;
                float* y = H[l & 1];
                hipLaunchKernelGGL(generic_linear_kernel<true>, dim3(pts.x, (g.hidden + GL_OUT - 1) / GL_OUT), dim3(256), 0, stream, n, g.hidden, K1, K2,
                                   cur, in0, w, w + (long)g.hidden * (K1 + K2), y, g.hidden, 0);
                if (int e = NVSR_CHECK_LAUNCH()) return e;
                w += (long)g.hidden * (K1 + K2) + g.hidden;
                cur = y; cur_k = g.hidden;
            }
            const int M = rgb ? 3 : 1;                                          // fc_rgb -> out[:, 0:3], fc_alpha -> out[:, 3]
            hipLaunchKernelGGL(generic_linear_kernel<false>, dim3(pts.x, 1), dim3(256), 0, stream, n, M, g.hidden, 0, cur, cur, w, w + (long)M * g.hidden,
                               out + a * 4, 4, rgb ? 0 : 3);
            if (int e = NVSR_CHECK_LAUNCH()) return e;
            w += (long)M * g.hidden + M;
        }
    }
    return NVSR_OK;
}
int nvsr_generic_decode(const nvsr_scene* scene, const nvsr_decoder_geometry* geom, const float* natural, int64_t P, const float* x, float* out,
                        float* workspace, nvsr_stream_t stream) {
    GenGeom g;
    if (int e = gen_resolve(geom, &g)) return e;
    if (!scene) return NVSR_ERR_NULL;
    return gen_decode(gen_scene(scene), g, natural, P, x, nullptr, out, workspace, (hipStream_t)stream);
}
int nvsr_generic_decode_ext(const nvsr_scene_ext* scene, const nvsr_decoder_geometry* geom, const float* natural, int64_t P, const float* x,
                            const float* coord_noise, float* out, float* workspace, nvsr_stream_t stream) {
    if (int e = gen_check_ext(scene)) return e;
    GenGeom g;
    if (int e = gen_resolve(geom, &g, scene->num_position_planes)) return e;
    return gen_decode(gen_scene(scene), g, natural, P, x, coord_noise, out, workspace, (hipStream_t)stream);
}

static int64_t gen_bwd_floats_per_point(const GenGeom& g) { return 2 * (int64_t)(g.Kd + g.Kr) + (int64_t)(g.nd + g.nr + 2) * g.hidden; }

static int64_t gen_bwd_workspace_floats(const nvsr_decoder_geometry* geom, int np, int64_t P) {
    GenGeom g;
    if (gen_resolve(geom, &g, np) || P < 0) return -1;
    return (P < GEN_BWD_CHUNK ? P : GEN_BWD_CHUNK) * gen_bwd_floats_per_point(g);
}
int64_t nvsr_generic_decode_backward_workspace_floats(const nvsr_decoder_geometry* geom, int64_t P) { return gen_bwd_workspace_floats(geom, 3, P); }
int64_t nvsr_generic_decode_backward_workspace_floats_ext(const nvsr_decoder_geometry* geom, int num_position_planes, int64_t P) {
    return gen_bwd_workspace_floats(geom, num_position_planes, P);
}

static int gen_decode_backward(const SceneDevN& sc, const GenGeom& g, const float* natural, int64_t P, const float* x, const float* coord_noise,
                               const float* d_out, float* d_natural, const GradPlanesN& gp, float* workspace, hipStream_t stream) {
    if (!natural || !x || !d_out || !workspace) return NVSR_ERR_NULL;
    if (int e = gen_check_scene(sc, g)) return e;
    if (P < 0 || g.nd + g.nr > 128) return NVSR_ERR_SHAPE;
    bool want_planes = false;
    for (int d = 0; d <= g.np; ++d) want_planes = want_planes || gp.g[d] != nullptr;
    long woff[2][65];
    gen_blob_offsets(g, woff);
    for (int64_t a = 0; a < P; a += GEN_BWD_CHUNK) {
        const long n = (long)((P - a) < GEN_BWD_CHUNK ? (P - a) : GEN_BWD_CHUNK);
        float* Xin[2] = {workspace, workspace + n * g.Kd};
        float* Hs[2] = {Xin[1] + n * g.Kr, Xin[1] + n * g.Kr + (long)g.nd * n * g.hidden};          // [layer][n][hidden] per decoder
        float* dXin[2] = {Hs[1] + (long)g.nr * n * g.hidden, Hs[1] + (long)g.nr * n * g.hidden + n * g.Kd};
        float* dH[2] = {dXin[1] + n * g.Kr, dXin[1] + n * g.Kr + n * g.hidden};
        const float* xa = x + a * 6;
        const float* da = d_out + a * 4;
        const long threads = n * (g.Kd + g.Kr);
        const float* na = coord_noise ? coord_noise + a * 3 : nullptr;
        hipLaunchKernelGGL(generic_inputs_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream, sc, g, n, xa, na, Xin[0], Xin[1]);
        if (int e = NVSR_CHECK_LAUNCH()) return e;
        const dim3 pts((unsigned)((n + GL_PTS - 1) / GL_PTS));
        if (hipMemsetAsync(dXin[0], 0, sizeof(float) * n * (g.Kd + g.Kr), stream) != hipSuccess) return NVSR_ERR_LAUNCH;
        for (int dec = 0; dec < 2; ++dec) {
            const float* in0 = Xin[dec];
            const int k0 = dec ? g.Kr : g.Kd, nl = dec ? g.nr : g.nd, Mh = dec ? 3 : 1, hoff = dec ? 0 : 3;
            // forward with every layer's output kept
            const float* cur = in0;
            int cur_k = k0;
            for (int l = 0; l < nl; ++l) {
                const bool skip = l > 0 && gen_skip_layer(l - 1, g.skip);
                const int K1 = cur_k, K2 = skip ? k0 : 0;
                const float* w = natural + woff[dec][l];
                float* y = Hs[dec] + (long)l * n * g.hidden;
                hipLaunchKernelGGL(generic_linear_kernel<true>, dim3(pts.x, (g.hidden + GL_OUT - 1) / GL_OUT), dim3(256), 0, stream, n, g.hidden, K1, K2,
                                   cur, in0, w, w + (long)g.hidden * (K1 + K2), y, g.hidden, 0);
                if (int e = NVSR_CHECK_LAUNCH()) return e;
                cur = y; cur_k = g.hidden;
            }
            // head: d_out[:, hoff : hoff + Mh] -> dH[0]; its weight gradient from the last layer's output
            const float* wh = natural + woff[dec][nl];
            if (d_natural) {
                float* gw = d_natural + woff[dec][nl];
                if (int e = gen_wgrad_launch(n, Mh, g.hidden, 0, da, 4, hoff, nullptr, cur, cur, gw, gw + (long)Mh * g.hidden, stream)) return e;
            }
            hipLaunchKernelGGL(generic_dgrad_kernel<false>, dim3(pts.x, (g.hidden + GL_OUT - 1) / GL_OUT), dim3(256), 0, stream, n, Mh, g.hidden, 0, g.hidden,
                               da, 4, hoff, (const float*)nullptr, wh, dH[0], g.hidden, 0);
            if (int e = NVSR_CHECK_LAUNCH()) return e;
            int cb = 0;
            for (int l = nl - 1; l >= 0; --l) {
                const bool skip = l > 0 && gen_skip_layer(l - 1, g.skip);
                const int K1 = l == 0 ? k0 : g.hidden, K2 = skip ? k0 : 0, K = K1 + K2;
                const float* X1 = l == 0 ? in0 : Hs[dec] + (long)(l - 1) * n * g.hidden;
                const float* Hl = Hs[dec] + (long)l * n * g.hidden;
                const float* w = natural + woff[dec][l];
                if (d_natural) {
                    float* gw = d_natural + woff[dec][l];
                    if (int e = gen_wgrad_launch(n, g.hidden, K1, K2, dH[cb], g.hidden, 0, Hl, X1, in0, gw, gw + (long)g.hidden * K, stream)) return e;
                }
                if (l > 0) {
                    hipLaunchKernelGGL(generic_dgrad_kernel<false>, dim3(pts.x, (K1 + GL_OUT - 1) / GL_OUT), dim3(256), 0, stream, n, g.hidden, K, 0, K1,
                                       dH[cb], g.hidden, 0, Hl, w, dH[cb ^ 1], g.hidden, 0);
                    if (int e = NVSR_CHECK_LAUNCH()) return e;
                    if (skip && want_planes) {
                        hipLaunchKernelGGL(generic_dgrad_kernel<true>, dim3(pts.x, (K2 + GL_OUT - 1) / GL_OUT), dim3(256), 0, stream, n, g.hidden, K, K1, K2,
                                           dH[cb], g.hidden, 0, Hl, w, dXin[dec], k0, 0);
                        if (int e = NVSR_CHECK_LAUNCH()) return e;
                    }
                } else if (want_planes) {
                    hipLaunchKernelGGL(generic_dgrad_kernel<true>, dim3(pts.x, (K1 + GL_OUT - 1) / GL_OUT), dim3(256), 0, stream, n, g.hidden, K, 0, K1,
                                       dH[cb], g.hidden, 0, Hl, w, dXin[dec], k0, 0);
                    if (int e = NVSR_CHECK_LAUNCH()) return e;
                }
                cb ^= 1;
            }
        }
        if (want_planes) {
            hipLaunchKernelGGL(generic_inputs_backward_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream, sc, g, n, xa, na, dXin[0],
                               dXin[1], gp);
            if (int e = NVSR_CHECK_LAUNCH()) return e;
        }
    }
    return NVSR_OK;
}
int nvsr_generic_decode_backward(const nvsr_scene* scene, const nvsr_decoder_geometry* geom, const float* natural, int64_t P, const float* x,
                                 const float* d_out, float* d_natural, float* d_plane0, float* d_plane1, float* d_plane2, float* d_plane3,
                                 float* workspace, nvsr_stream_t stream) {
    GenGeom g;
    if (int e = gen_resolve(geom, &g)) return e;
    if (!scene) return NVSR_ERR_NULL;
    GradPlanesN gp = {};
    gp.g[0] = d_plane0; gp.g[1] = d_plane1; gp.g[2] = d_plane2; gp.g[3] = d_plane3;
    return gen_decode_backward(gen_scene(scene), g, natural, P, x, nullptr, d_out, d_natural, gp, workspace, (hipStream_t)stream);
}
int nvsr_generic_decode_backward_ext(const nvsr_scene_ext* scene, const nvsr_decoder_geometry* geom, const float* natural, int64_t P, const float* x,
                                     const float* coord_noise, const float* d_out, float* d_natural, float* const* d_planes, float* workspace,
                                     nvsr_stream_t stream) {
    if (int e = gen_check_ext(scene)) return e;
    GenGeom g;
    if (int e = gen_resolve(geom, &g, scene->num_position_planes)) return e;
    GradPlanesN gp = {};
    if (d_planes)
        for (int d = 0; d <= scene->num_position_planes; ++d) gp.g[d] = d_planes[d];
    return gen_decode_backward(gen_scene(scene), g, natural, P, x, coord_noise, d_out, d_natural, gp, workspace, (hipStream_t)stream);
}

int nvsr_ray_points(int64_t N, int S, const float* rays, const float* z, float* x, nvsr_stream_t stream) {
    if (!rays || !z || !x) return NVSR_ERR_NULL;
    if (N < 0 || S < 1) return NVSR_ERR_SHAPE;
    if (N == 0) return NVSR_OK;
    const long n = (long)N * S;
    hipLaunchKernelGGL(ray_points_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (long)N, S, rays, z, x);
    return NVSR_CHECK_LAUNCH();
}

}  // extern "C"
