// Surface normals of a rendered view: the density gradient on the LIVE samples of a pass, composited per ray.
//
// nvsr_live_ray_points turns the entries of a live list (nvsr_generic_live_list on the compositor's weights) into one-sample rays, the form
// nvsr_decode_rays and the ROWS backward take; nvsr_normals_composite chains the rows of g_raw = (0, 0, 0, 1) to d sigma_raw / d p with the
// device functions of points_grad.hip (points_grad_core.h: the same arithmetic, not a copy), normalises and folds w n into normal[ray].
//
// Shape of the compositor: a point takes one DPP row of 16 lanes (12 of them load a texel / a row slice), a ray is owned by one such lane
// group, four rays per wave, 16 per workgroup.  The group finds its ray's run in the ascending list by two binary searches and walks it in
// order; the wave walks as many steps as its longest run (the DPP sums need every lane), a group past its run rides along on an entry in
// range and adds nothing.  No atomics, no LDS, no barrier: a ray's sum is a left fold in one lane group.
#include "points_grad_core.h"
#include "nvsr_internal.h"

namespace nvsr {

__global__ __launch_bounds__(256) void live_ray_points_kernel(long P, int S, long M, const int* __restrict__ index, const float* __restrict__ rays,
                                                              const float* __restrict__ z, float* __restrict__ live_rays) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    const long p = index[i];
    if (p < 0 || p >= P) return;
    const float* r = rays + (p / S) * 11;
    const float zc = z[p];
    float* o = live_rays + i * 11;
    o[0] = __fadd_rn(r[0], __fmul_rn(r[3], zc));        // nvsr_ray_points' position
    o[1] = __fadd_rn(r[1], __fmul_rn(r[4], zc));
    o[2] = __fadd_rn(r[2], __fmul_rn(r[5], zc));
    o[3] = o[4] = o[5] = o[6] = o[7] = 0.0f;
    o[8] = r[8]; o[9] = r[9]; o[10] = r[10];
}

// first i in [0, M) with index[i] >= key, M if none (index ascending)
__device__ __forceinline__ long lower_bound(const int* __restrict__ index, long M, long key) {
    long lo = 0, hi = M;
    while (lo < hi) {
        const long mid = (lo + hi) >> 1;
        if ((long)index[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// 16 lanes per ray; M >= 1
__global__ __launch_bounds__(256) void normals_composite_kernel(SceneDev sc, long N, int S, long M, const int* __restrict__ index,
                                                                const float* __restrict__ live_rays, const float* __restrict__ rows0,
                                                                const float* __restrict__ rows1, const float* __restrict__ rows2,
                                                                const float* __restrict__ weights, float* __restrict__ normal) {
    const int sub = threadIdx.x & 15;
    const long ray = (long)blockIdx.x * 16 + (threadIdx.x >> 4);
    long i = 0, end = 0;
    if (ray < N) {
        i = lower_bound(index, M, ray * S);
        end = lower_bound(index, M, (ray + 1) * S);
    }
    const bool any = i < end;
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
    if (any) { a0 = normal[ray * 3]; a1 = normal[ray * 3 + 1]; a2 = normal[ray * 3 + 2]; }
    const float* const rows[3] = {rows0, rows1, rows2};
    while (__ballot(i < end) != 0) {                                   // (wave-uniform: every lane stays in the loop)
        const bool live = i < end;
        const long m = live ? i : M - 1;
        const float* r = live_rays + m * 11;
        const float p0 = r[0], p1 = r[1], p2 = r[2];
        float dn0, dn1, dn2;
        point_slope(sc, p0, p1, p2, rows, m, sub, dn0, dn1, dn2);
        if (live) {
            const bool bad = (p0 != p0) || (p1 != p1) || (p2 != p2);
            const float g0 = point_slope_component(dn0, sc.range[0], bad), g1 = point_slope_component(dn1, sc.range[1], bad),
                        g2 = point_slope_component(dn2, sc.range[2], bad);
            const float q = __fadd_rn(__fadd_rn(__fmul_rn(g0, g0), __fmul_rn(g1, g1)), __fmul_rn(g2, g2));
            const float rr = sqrtf(q);
            const bool flat = q == 0.0f;
            const float n0 = flat ? 0.0f : -__fdiv_rn(g0, rr), n1 = flat ? 0.0f : -__fdiv_rn(g1, rr), n2 = flat ? 0.0f : -__fdiv_rn(g2, rr);
            const float w = weights[index[m]];
            a0 = __fadd_rn(a0, __fmul_rn(w, n0));
            a1 = __fadd_rn(a1, __fmul_rn(w, n1));
            a2 = __fadd_rn(a2, __fmul_rn(w, n2));
            ++i;
        }
    }
    if (any && sub < 3) normal[ray * 3 + sub] = sub == 0 ? a0 : (sub == 1 ? a1 : a2);
}

}  // namespace nvsr

using namespace nvsr;

extern "C" int nvsr_live_ray_points(int64_t N, int S, int64_t M, const int32_t* index, const float* rays, const float* z, float* live_rays,
                                    nvsr_stream_t stream) {
    if (N < 0 || M < 0 || S < 1 || S > 4096 || N * (int64_t)S >= (int64_t)1 << 31 || M >= (int64_t)1 << 31) return NVSR_ERR_SHAPE;
    if (M == 0 || N == 0) return NVSR_OK;
    if (!index || !rays || !z || !live_rays) return NVSR_ERR_NULL;
    hipLaunchKernelGGL(live_ray_points_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (long)(N * S), S, (long)M, index,
                       rays, z, live_rays);
    return NVSR_CHECK_LAUNCH();
}

extern "C" int nvsr_normals_composite(const nvsr_scene* scene, int64_t N, int S, int64_t M, const int32_t* index, const float* live_rays,
                                      const float* const* rows, const float* weights, float* normal, nvsr_stream_t stream) {
    if (!scene) return NVSR_ERR_NULL;
    if (int e = check_scene(scene)) return e;
    if (N < 0 || M < 0 || S < 1 || S > 4096 || N * (int64_t)S >= (int64_t)1 << 31 || M >= (int64_t)1 << 29) return NVSR_ERR_SHAPE;
    if (M == 0 || N == 0) return NVSR_OK;
    if (!index || !live_rays || !rows || !rows[0] || !rows[1] || !rows[2] || !weights || !normal) return NVSR_ERR_NULL;
    if (!aligned16(rows[0]) || !aligned16(rows[1]) || !aligned16(rows[2])) return NVSR_ERR_ALIGN;
    hipLaunchKernelGGL(normals_composite_kernel, dim3((unsigned)((N + 15) / 16)), dim3(256), 0, (hipStream_t)stream, to_dev(scene), (long)N, S, (long)M,
                       index, live_rays, rows[0], rows[1], rows[2], weights, normal);
    return NVSR_CHECK_LAUNCH();
}
