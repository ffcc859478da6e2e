// Ray and camera-pose gradients of a training render: from the per-point gradient nvsr_triplane_points_grad leaves behind
// the rows backward to the packed rays (nvsr_rays_grad), through the packer (nvsr_pack_rays_backward) and the NDC warp
// (nvsr_ndc_rays_backward) to ray origins and directions, and through the ray generator to the 3 x 4 camera-to-world matrix
// (nvsr_ray_bundle_backward).
//
// Every sum runs in a fixed order and every operation is a single correctly rounded one (__f*_rn), as include/nvsr.h states per entry: no
// atomics, no allocation, no synchronisation.  The wave-wide sums are balanced trees over neighbouring lanes: the four DPP steps of
// points_grad.hip's row16_sum inside a row of 16 lanes, then two butterfly steps across the rows.
#include "nvsr_common.h"
#include "nvsr_internal.h"

namespace nvsr {

constexpr int RG_WPB = 4;              // rays (waves) per workgroup of rays_grad_kernel
constexpr int RB_SLAB = 256;           // rays per slab (workgroup) of ray_bundle_backward_slab_kernel: one per thread

template <int CTRL>
__device__ __forceinline__ float tree_dpp(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), CTRL, 0xf, 0xf, false));
}
// sum over the 64 lanes as a balanced tree over neighbouring lanes, (((l0 + l1) + (l2 + l3)) + ...) + ..., the same bits in every lane: swap
// inside pairs, swap the pairs of a quad, mirror the half row and the row, then exchange with the lane 16 and 32 away (after each step the
// lanes of a group agree, so the partner holds the neighbouring group's total).  PRECONDITION: all 64 lanes are active.
__device__ __forceinline__ float wave_tree_sum(float v) {
    v = __fadd_rn(v, tree_dpp<0xB1>(v));     // quad_perm [1, 0, 3, 2]
    v = __fadd_rn(v, tree_dpp<0x4E>(v));     // quad_perm [2, 3, 0, 1]
    v = __fadd_rn(v, tree_dpp<0x141>(v));    // row_half_mirror
    v = __fadd_rn(v, tree_dpp<0x140>(v));    // row_mirror
    v = __fadd_rn(v, __shfl_xor(v, 16));
    v = __fadd_rn(v, __shfl_xor(v, 32));
    return v;
}

// one wave per ray; a wave beyond N runs along on ray N - 1 and stores nothing (the tree needs every lane)
__global__ __launch_bounds__(64 * RG_WPB) void rays_grad_kernel(long N, int S, const float* __restrict__ rays, const float* __restrict__ z,
                                                                 const float* __restrict__ d_points, const float* __restrict__ d_viewdir,
                                                                 const float* __restrict__ raw, const float* __restrict__ noise,
                                                                 const float* __restrict__ g_raw, int accumulate, float* __restrict__ d_rays) {
    const int lane = threadIdx.x & 63;
    long ray = (long)blockIdx.x * RG_WPB + (threadIdx.x >> 6);
    const bool live = ray < N;
    if (!live) ray = N - 1;
    const long base = ray * S;
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, b0 = 0.0f, b1 = 0.0f, b2 = 0.0f, t = 0.0f;
    for (int s = lane; s < S; s += 64) {
        const long m = base + s;
        if (d_points) {                                                    // (kernel argument: uniform)
            const float zc = z[m], p0 = d_points[3 * m], p1 = d_points[3 * m + 1], p2 = d_points[3 * m + 2];
            a0 = __fadd_rn(a0, p0); a1 = __fadd_rn(a1, p1); a2 = __fadd_rn(a2, p2);
            b0 = __fadd_rn(b0, __fmul_rn(zc, p0)); b1 = __fadd_rn(b1, __fmul_rn(zc, p1)); b2 = __fadd_rn(b2, __fmul_rn(zc, p2));
        }
        const float sr = raw[4 * m + 3];
        const float sn = noise ? __fadd_rn(sr, noise[m]) : sr;
        const float sig = sn < 0.0f ? 0.0f : sn;                           // the compositor's relu (a NaN density stays a NaN)
        t = __fadd_rn(t, __fmul_rn(g_raw[4 * m + 3], sig));
    }
    a0 = wave_tree_sum(a0); a1 = wave_tree_sum(a1); a2 = wave_tree_sum(a2);
    b0 = wave_tree_sum(b0); b1 = wave_tree_sum(b1); b2 = wave_tree_sum(b2);
    t = wave_tree_sum(t);
    const float* r = rays + ray * 11;
    const float rd0 = r[3], rd1 = r[4], rd2 = r[5];
    const float rr = __fadd_rn(__fadd_rn(__fmul_rn(rd0, rd0), __fmul_rn(rd1, rd1)), __fmul_rn(rd2, rd2));
    bool bad = false;
#pragma unroll
    for (int j = 0; j < 11; ++j) bad = bad || (j != 6 && j != 7 && r[j] != r[j]);
    // lane j < 11 owns column j
    float v = 0.0f;
    if (lane < 3) v = lane == 0 ? a0 : (lane == 1 ? a1 : a2);
    else if (lane < 6) {
        const float b = lane == 3 ? b0 : (lane == 4 ? b1 : b2), d = lane == 3 ? rd0 : (lane == 4 ? rd1 : rd2);
        v = __fadd_rn(b, __fdiv_rn(__fmul_rn(t, d), rr));
    } else if (lane >= 8 && lane < 11 && d_viewdir) v = d_viewdir[ray * 3 + (lane - 8)];
    if (bad && lane != 6 && lane != 7) v = __int_as_float(0x7fc00000);
    if (live && lane < 11) {
        float* o = d_rays + ray * 11 + lane;
        *o = (accumulate && lane != 6 && lane != 7) ? __fadd_rn(*o, v) : (lane == 6 || lane == 7 ? 0.0f : v);
    }
}

__global__ __launch_bounds__(256) void pack_rays_backward_kernel(long N, const float* __restrict__ d_rays, const float* __restrict__ vs,
                                                                  int view_is_rd, float* __restrict__ d_ro, float* __restrict__ d_rd,
                                                                  float* __restrict__ d_vs) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const float* g = d_rays + 11 * i;
    const float v0 = vs[3 * i], v1 = vs[3 * i + 1], v2 = vs[3 * i + 2];
    const float nrm = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(v0, v0), __fmul_rn(v1, v1)), __fmul_rn(v2, v2)));      // as pack_rays_kernel
    const float u0 = __fdiv_rn(v0, nrm), u1 = __fdiv_rn(v1, nrm), u2 = __fdiv_rn(v2, nrm);
    const float dot = __fadd_rn(__fadd_rn(__fmul_rn(u0, g[8]), __fmul_rn(u1, g[9])), __fmul_rn(u2, g[10]));
    const float c0 = __fdiv_rn(__fsub_rn(g[8], __fmul_rn(u0, dot)), nrm);
    const float c1 = __fdiv_rn(__fsub_rn(g[9], __fmul_rn(u1, dot)), nrm);
    const float c2 = __fdiv_rn(__fsub_rn(g[10], __fmul_rn(u2, dot)), nrm);
    d_ro[3 * i] = g[0]; d_ro[3 * i + 1] = g[1]; d_ro[3 * i + 2] = g[2];
    if (view_is_rd) {
        d_rd[3 * i] = __fadd_rn(g[3], c0); d_rd[3 * i + 1] = __fadd_rn(g[4], c1); d_rd[3 * i + 2] = __fadd_rn(g[5], c2);
    } else {
        d_rd[3 * i] = g[3]; d_rd[3 * i + 1] = g[4]; d_rd[3 * i + 2] = g[5];
        if (d_vs) { d_vs[3 * i] = c0; d_vs[3 * i + 1] = c1; d_vs[3 * i + 2] = c2; }
    }
}

// adjoint of ndc_rays_kernel (aux.hip), which it restates operation by operation: go = d loss / d ro_out, gd = d loss / d rd_out
__global__ __launch_bounds__(256) void ndc_rays_backward_kernel(float sx, float sy, float nr, float two_near, long N, const float* __restrict__ ro,
                                                                 const float* __restrict__ rd, const float* __restrict__ go,
                                                                 const float* __restrict__ gd, float* __restrict__ d_ro, float* __restrict__ d_rd) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const float o0 = ro[3 * i], o1 = ro[3 * i + 1], o2 = ro[3 * i + 2];
    const float d0 = rd[3 * i], d1 = rd[3 * i + 1], d2 = rd[3 * i + 2];
    const float t = __fdiv_rn(-__fadd_rn(nr, o2), d2);
    const float ox = __fadd_rn(o0, __fmul_rn(t, d0)), oy = __fadd_rn(o1, __fmul_rn(t, d1)), oz = __fadd_rn(o2, __fmul_rn(t, d2));
    const float h0 = __fmul_rn(sx, __fsub_rn(go[3 * i], gd[3 * i]));              // what ox / oz receives, times its scale
    const float h1 = __fmul_rn(sy, __fsub_rn(go[3 * i + 1], gd[3 * i + 1]));
    const float h2 = __fmul_rn(two_near, __fsub_rn(go[3 * i + 2], gd[3 * i + 2]));    // what 1 / oz receives
    const float g_ox = __fdiv_rn(h0, oz), g_oy = __fdiv_rn(h1, oz);
    const float g_oz = -__fdiv_rn(__fadd_rn(__fadd_rn(__fmul_rn(ox, h0), __fmul_rn(oy, h1)), h2), __fmul_rn(oz, oz));
    const float k0 = __fmul_rn(sx, gd[3 * i]), k1 = __fmul_rn(sy, gd[3 * i + 1]);   // what d0 / d2, d1 / d2 receive
    const float g_t = __fadd_rn(__fadd_rn(__fmul_rn(g_ox, d0), __fmul_rn(g_oy, d1)), __fmul_rn(g_oz, d2));
    const float q = __fdiv_rn(g_t, d2);
    d_ro[3 * i] = g_ox;
    d_ro[3 * i + 1] = g_oy;
    d_ro[3 * i + 2] = __fsub_rn(g_oz, q);
    d_rd[3 * i] = __fadd_rn(__fdiv_rn(k0, d2), __fmul_rn(t, g_ox));
    d_rd[3 * i + 1] = __fadd_rn(__fdiv_rn(k1, d2), __fmul_rn(t, g_oy));
    const float e = __fdiv_rn(__fadd_rn(__fmul_rn(k0, d0), __fmul_rn(k1, d1)), __fmul_rn(d2, d2));
    d_rd[3 * i + 2] = __fsub_rn(__fsub_rn(__fmul_rn(t, g_oz), e), __fmul_rn(t, q));
}

// stage 1: slab w = rays [256 w, 256 w + 256), one per thread (a thread beyond N contributes +0): 12 wave trees, the four waves of the
// workgroup added as (w0 + w1) + (w2 + w3) -> partials[w][12], entry 4 k + j = d_c2w[k][j]
__global__ __launch_bounds__(RB_SLAB) void ray_bundle_backward_slab_kernel(int H, int W, float fx, float fy, int pad, float off, long N,
                                                                           const int* __restrict__ rc, const float* __restrict__ d_ro,
                                                                           const float* __restrict__ d_rd, float* __restrict__ partials) {
    __shared__ float part[4][12];
    const long i = (long)blockIdx.x * RB_SLAB + threadIdx.x;
    float v[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) v[e] = 0.0f;
    if (i < N) {
        int r, c;
        float ii, jj;
        if (rc) {                                                              // ray_bundle_at_kernel's direction
            r = rc[2 * i]; c = rc[2 * i + 1];
            ii = __fadd_rn((float)c, off); jj = __fadd_rn((float)r, off);
        } else {                                                               // ray_bundle_kernel's
            const int Wp = W + 2 * pad;
            r = (int)(i / Wp); c = (int)(i - (long)r * Wp);
            ii = __fadd_rn((float)c, off); jj = __fadd_rn((float)r, off);
            if (pad > 0) { ii = __fsub_rn(ii, (float)pad); jj = __fsub_rn(jj, (float)pad); }
        }
        const float dir[3] = {__fdiv_rn(__fsub_rn(ii, (float)(W * 0.5)), fx), -__fdiv_rn(__fsub_rn(jj, (float)(H * 0.5)), fy), -1.0f};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float g = d_rd[3 * i + k];
#pragma unroll
            for (int j = 0; j < 3; ++j) v[4 * k + j] = __fmul_rn(g, dir[j]);
            v[4 * k + 3] = d_ro[3 * i + k];
        }
    }
#pragma unroll
    for (int e = 0; e < 12; ++e) v[e] = wave_tree_sum(v[e]);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int e = 0; e < 12; ++e) part[wave][e] = v[e];
    }
    __syncthreads();
    if (threadIdx.x < 12) {
        const int e = threadIdx.x;
        partials[(long)blockIdx.x * 12 + e] = __fadd_rn(__fadd_rn(part[0][e], part[1][e]), __fadd_rn(part[2][e], part[3][e]));
    }
}

// stage 2, one wave: per entry, lane l adds slabs l, l + 64, ... in ascending order from +0, then the tree; row 3 of d_c2w is +0
__global__ __launch_bounds__(64) void ray_bundle_backward_reduce_kernel(long slabs, const float* __restrict__ partials, float* __restrict__ d_c2w) {
    const int lane = threadIdx.x;
    float v[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) v[e] = 0.0f;
    for (long w = lane; w < slabs; w += 64) {
#pragma unroll
        for (int e = 0; e < 12; ++e) v[e] = __fadd_rn(v[e], partials[w * 12 + e]);
    }
#pragma unroll
    for (int e = 0; e < 12; ++e) v[e] = wave_tree_sum(v[e]);
    float out = 0.0f;
#pragma unroll
    for (int e = 0; e < 12; ++e) out = lane == e ? v[e] : out;
    if (lane < 16) d_c2w[lane] = lane < 12 ? out : 0.0f;
}

}  // namespace nvsr

using namespace nvsr;

static inline unsigned blocks_of(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

extern "C" int nvsr_rays_grad(int64_t N, int S, const float* rays, const float* z, const float* d_points, const float* d_viewdir, const float* raw,
                              const float* noise, const float* g_raw, int accumulate, float* d_rays, nvsr_stream_t stream) {
    if (!rays || !raw || !g_raw || !d_rays || (d_points && !z)) return NVSR_ERR_NULL;
    if (N < 0 || S < 1 || S > 4096 || N * (int64_t)S >= (int64_t)1 << 29) return NVSR_ERR_SHAPE;
    if (N == 0) return NVSR_OK;
    hipLaunchKernelGGL(rays_grad_kernel, dim3(blocks_of(N, RG_WPB)), dim3(64 * RG_WPB), 0, (hipStream_t)stream, (long)N, S, rays, z, d_points,
                       d_viewdir, raw, noise, g_raw, accumulate, d_rays);
    return NVSR_CHECK_LAUNCH();
}

extern "C" int nvsr_pack_rays_backward(int64_t N, const float* d_rays, const float* view_src, int view_is_rd, float* d_ro, float* d_rd,
                                       float* d_view_src, nvsr_stream_t stream) {
    if (!d_rays || !view_src || !d_ro || !d_rd) return NVSR_ERR_NULL;
    if (N < 0 || N >= (int64_t)1 << 31) return NVSR_ERR_SHAPE;
    if (N == 0) return NVSR_OK;
    hipLaunchKernelGGL(pack_rays_backward_kernel, dim3(blocks_of(N, 256)), dim3(256), 0, (hipStream_t)stream, (long)N, d_rays, view_src,
                       view_is_rd, d_ro, d_rd, d_view_src);
    return NVSR_CHECK_LAUNCH();
}

extern "C" int nvsr_ndc_rays_backward(int H, int W, double focal, double near_, int64_t N, const float* ro, const float* rd, const float* d_ro_out,
                                      const float* d_rd_out, float* d_ro, float* d_rd, nvsr_stream_t stream) {
    if (!ro || !rd || !d_ro_out || !d_rd_out || !d_ro || !d_rd) return NVSR_ERR_NULL;
    if (N < 0 || N >= (int64_t)1 << 31 || H < 1 || W < 1) return NVSR_ERR_SHAPE;
    if (N == 0) return NVSR_OK;
    const float sx = (float)(-1.0 / (W / (2.0 * focal))), sy = (float)(-1.0 / (H / (2.0 * focal)));      // as nvsr_ndc_rays
    hipLaunchKernelGGL(ndc_rays_backward_kernel, dim3(blocks_of(N, 256)), dim3(256), 0, (hipStream_t)stream, sx, sy, (float)near_,
                       (float)(2.0 * near_), (long)N, ro, rd, d_ro_out, d_rd_out, d_ro, d_rd);
    return NVSR_CHECK_LAUNCH();
}

extern "C" int64_t nvsr_ray_bundle_backward_workspace_floats(int64_t N) { return N < 1 ? 0 : 12 * ((N + RB_SLAB - 1) / RB_SLAB); }

extern "C" int nvsr_ray_bundle_backward(int H, int W, double focal_x, double focal_y, double offset, int64_t N, const int32_t* row_col, int padding,
                                        const float* d_ro, const float* d_rd, float* d_c2w, float* workspace, nvsr_stream_t stream) {
    if (!d_ro || !d_rd || !d_c2w || (N > 0 && !workspace)) return NVSR_ERR_NULL;
    if (H < 1 || W < 1 || N < 0 || N >= (int64_t)1 << 31 || padding < 0) return NVSR_ERR_SHAPE;
    if (!row_col && N != (int64_t)(H + 2 * padding) * (W + 2 * padding)) return NVSR_ERR_SHAPE;
    if (!aligned16(d_c2w)) return NVSR_ERR_ALIGN;
    if (N == 0) return NVSR_OK;
    const int64_t slabs = (N + RB_SLAB - 1) / RB_SLAB;
    hipLaunchKernelGGL(ray_bundle_backward_slab_kernel, dim3((unsigned)slabs), dim3(RB_SLAB), 0, (hipStream_t)stream, H, W, (float)focal_x,
                       (float)focal_y, row_col ? 0 : padding, (float)offset, (long)N, row_col, d_ro, d_rd, workspace);
    if (int e = NVSR_CHECK_LAUNCH()) return e;
    hipLaunchKernelGGL(ray_bundle_backward_reduce_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (long)slabs, workspace, d_c2w);
    return NVSR_CHECK_LAUNCH();
}
