// Input gradients of the tri-plane model: d loss / d (sample position) and d loss / d (view direction).
//
// The limb backward's ROWS variant leaves dL/d(feature of plane d) of every point as a plain row rows[d][m][48], nvsr_view_rows_reduce one
// view-plane row per ray.  The last link is the derivative of the four bilinear taps with respect to the grid coordinate, chained through the
// projection, the normalisation and (view plane) cart2az_el: a gather of 4 texels + 1 row per plane and point, no atomics, no plane touched.
//
// Shape: a texel / a row is 12 lanes x 16 bytes; a point (a ray) takes one DPP row of 16 lanes, lanes 12..15 load nothing and contribute +0.0f;
// four points per wave, 16 per workgroup.  The 48 products are summed four per lane, then across the row by four DPP additions.  Every
// operation is a single correctly rounded one (__f*_rn) in the order stated in include/nvsr.h (nvsr_triplane_points_grad).
#include "points_grad_core.h"
#include "nvsr_internal.h"

namespace nvsr {

// 16 lanes per point m = ray * S + s; a group beyond M runs along on point M - 1 and stores nothing (the DPP sums need every lane)
__global__ __launch_bounds__(256) void points_grad_kernel(SceneDev sc, long M, int S, const float* __restrict__ rays, const float* __restrict__ z,
                                                          const float* __restrict__ rows0, const float* __restrict__ rows1,
                                                          const float* __restrict__ rows2, float* __restrict__ d_points) {
    const int sub = threadIdx.x & 15;
    long m = (long)blockIdx.x * 16 + (threadIdx.x >> 4);
    const bool live = m < M;
    if (!live) m = M - 1;
    const float* r = rays + (m / S) * 11;
    const float zc = z[m];
    const float p0 = __fadd_rn(r[0], __fmul_rn(r[3], zc)), p1 = __fadd_rn(r[1], __fmul_rn(r[4], zc)), p2 = __fadd_rn(r[2], __fmul_rn(r[5], zc));
    const float* const rows[3] = {rows0, rows1, rows2};
    float dn0, dn1, dn2;
    point_slope(sc, p0, p1, p2, rows, m, sub, dn0, dn1, dn2);
    const bool bad = (p0 != p0) || (p1 != p1) || (p2 != p2);
    const float dn = sub == 0 ? dn0 : (sub == 1 ? dn1 : dn2);
    const float range = sub == 0 ? sc.range[0] : (sub == 1 ? sc.range[1] : sc.range[2]);
    const float out = point_slope_component(dn, range, bad);
    if (live && sub < 3) d_points[m * 3 + sub] = out;
}

// 16 lanes per ray: the same rule on the view plane, chained through az = atan2(vy, vx), el = atan2(vz, sqrt(vx^2 + vy^2))
__global__ __launch_bounds__(256) void viewdir_grad_kernel(SceneDev sc, long N, const float* __restrict__ rays, const float* __restrict__ view_rows,
                                                           float* __restrict__ d_viewdir) {
    const int sub = threadIdx.x & 15;
    long ray = (long)blockIdx.x * 16 + (threadIdx.x >> 4);
    const bool live = ray < N;
    if (!live) ray = N - 1;
    const float* r = rays + ray * 11;
    const float vx = r[8], vy = r[9], vz = r[10];
    float Gx = 0.0f, Gy = 0.0f;
    const float q = __fadd_rn(__fmul_rn(vx, vx), __fmul_rn(vy, vy));
    const float rr = sqrtf(q);
    if (view_rows) {                                                   // (kernel argument: uniform)
        const float az = atan2f(vy, vx), el = atan2f(vz, rr);          // view_taps (decode_core.h)
        plane_slope(sc, 3, norm_coord(az, sc.lo[3], sc.range[3]), norm_coord(el, sc.lo[4], sc.range[4]), view_rows + ray * C, sub, Gx, Gy);
    }
    const float d_az = __fdiv_rn(__fmul_rn(2.0f, Gx), sc.range[3]), d_el = __fdiv_rn(__fmul_rn(2.0f, Gy), sc.range[4]);
    const float h = __fadd_rn(q, __fmul_rn(vz, vz));
    const float a = __fdiv_rn(d_az, q), b = __fdiv_rn(d_el, h), c = __fdiv_rn(__fmul_rn(b, vz), rr);
    const float o0 = __fsub_rn(__fmul_rn(-vy, a), __fmul_rn(vx, c));
    const float o1 = __fsub_rn(__fmul_rn(vx, a), __fmul_rn(vy, c));
    const float o2 = __fmul_rn(rr, b);
    const bool bad = (vx != vx) || (vy != vy) || (vz != vz);
    const float out = bad ? __int_as_float(0x7fc00000) : (sub == 0 ? o0 : (sub == 1 ? o1 : o2));
    if (live && sub < 3) d_viewdir[ray * 3 + sub] = out;
}

}  // namespace nvsr

using namespace nvsr;

extern "C" int nvsr_triplane_points_grad(const nvsr_scene* scene, int64_t N, int S, const float* rays, const float* z, const float* const* rows,
                                         const float* view_rows, float* d_points, float* d_viewdir, nvsr_stream_t stream) {
    if (!scene || !rays || (d_points && !z)) return NVSR_ERR_NULL;
    if (int e = check_scene(scene)) return e;
    if (N < 0 || S < 1 || S > 4096 || N * (int64_t)S >= (int64_t)1 << 29) return NVSR_ERR_SHAPE;
    const float* r[3] = {rows ? rows[0] : nullptr, rows ? rows[1] : nullptr, rows ? rows[2] : nullptr};
    if (!aligned16(r[0]) || !aligned16(r[1]) || !aligned16(r[2]) || !aligned16(view_rows)) return NVSR_ERR_ALIGN;
    if (N == 0 || (!d_points && !d_viewdir)) return NVSR_OK;
    const SceneDev sc = to_dev(scene);
    if (d_points) {
        const int64_t M = N * (int64_t)S;
        hipLaunchKernelGGL(points_grad_kernel, dim3((unsigned)((M + 15) / 16)), dim3(256), 0, (hipStream_t)stream, sc, (long)M, S, rays, z, r[0], r[1],
                           r[2], d_points);
        if (int e = NVSR_CHECK_LAUNCH()) return e;
    }
    if (d_viewdir) {
        hipLaunchKernelGGL(viewdir_grad_kernel, dim3((unsigned)((N + 15) / 16)), dim3(256), 0, (hipStream_t)stream, sc, (long)N, rays, view_rows,
                           d_viewdir);
        if (int e = NVSR_CHECK_LAUNCH()) return e;
    }
    return NVSR_OK;
}
