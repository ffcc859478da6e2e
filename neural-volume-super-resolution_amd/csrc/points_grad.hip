// Input gradients of the tri-plane model: d loss / d (sample position) and d loss / d (view direction).
//
// The limb backward's ROWS variant leaves dL/d(feature of plane d) of every point as a plain row rows[d][m][48], nvsr_view_rows_reduce one
// view-plane row per ray.  The last link is the derivative of the four bilinear taps with respect to the grid coordinate, chained through the
// projection, the normalisation and (view plane) cart2az_el: a gather of 4 texels + 1 row per plane and point, no atomics, no plane touched.
//
// Shape: a texel / a row is 12 lanes x 16 bytes; a point (a ray) takes one DPP row of 16 lanes, lanes 12..15 load nothing and contribute +0.0f;
// four points per wave, 16 per workgroup.  The 48 products are summed four per lane, then across the row by four DPP additions.  Every
// operation is a single correctly rounded one (__f*_rn) in the order stated in include/nvsr.h (nvsr_triplane_points_grad).
#include "bwd_core.h"
#include "nvsr_internal.h"

namespace nvsr {

template <int CTRL>
__device__ __forceinline__ float row_dpp(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), CTRL, 0xf, 0xf, false));
}
// sum over the 16 lanes of a DPP row as a balanced tree over neighbouring lanes, ((l0 + l1) + (l2 + l3)) + ((l4 + l5) + (l6 + l7)) ..., the same
// bits in every lane: swap inside pairs, swap the pairs of a quad, then mirror the half row and the row (after the first two steps the lanes of a
// quad agree, so a mirror reads the neighbouring quad's / half's total).  PRECONDITION: all 64 lanes are active.
__device__ __forceinline__ float row16_sum(float v) {
    v = __fadd_rn(v, row_dpp<0xB1>(v));     // quad_perm [1, 0, 3, 2]
    v = __fadd_rn(v, row_dpp<0x4E>(v));     // quad_perm [2, 3, 0, 1]
    v = __fadd_rn(v, row_dpp<0x141>(v));    // row_half_mirror
    v = __fadd_rn(v, row_dpp<0x140>(v));    // row_mirror
    return v;
}

// (Gx, Gy) = (hx sum_c row[c] df_c/dx, hy sum_c row[c] df_c/dy) of plane d at the grid coordinate (gx, gy); sub = lane within the row of 16.
// The cell, its clamps and its fractions are make_taps_cell's; a derivative is 0 where the unclamped pixel coordinate is <= 0 or >= W - 1
// (H - 1): torch's clip_coordinates_set_grad.
__device__ __forceinline__ void plane_slope(const SceneDev& sc, int d, float gx, float gy, const float* __restrict__ row, int sub, float& Gx, float& Gy) {
    int ix, iy;
    const Taps t = make_taps_cell(sc, d, gx, gy, ix, iy);
    const float mx = sc.mx[d], my = sc.my[d];
    const float x = (gx + 1.0f) * sc.hx[d], y = (gy + 1.0f) * sc.hy[d];
    const float xc = fminf(mx, fmaxf(x, 0.0f)), yc = fminf(my, fmaxf(y, 0.0f));
    const float w = xc - floorf(xc), e = 1.0f - w, n = yc - floorf(yc), s = 1.0f - n;
    const f32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
    f32x4 r = zero, t00 = zero, t01 = zero, t10 = zero, t11 = zero;
    if (sub < C / 4) {
        const float* p = sc.plane[d] + 4 * sub;
        r = *reinterpret_cast<const f32x4*>(row + 4 * sub);
        t00 = *reinterpret_cast<const f32x4*>(p + t.o00);
        t01 = *reinterpret_cast<const f32x4*>(p + t.o01);
        t10 = *reinterpret_cast<const f32x4*>(p + t.o10);
        t11 = *reinterpret_cast<const f32x4*>(p + t.o11);
    }
    float ax = 0.0f, ay = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float dx = __fadd_rn(__fmul_rn(s, __fsub_rn(t01[j], t00[j])), __fmul_rn(n, __fsub_rn(t11[j], t10[j])));
        const float dy = __fadd_rn(__fmul_rn(e, __fsub_rn(t10[j], t00[j])), __fmul_rn(w, __fsub_rn(t11[j], t01[j])));
        const float px = __fmul_rn(r[j], dx), py = __fmul_rn(r[j], dy);
        ax = j ? __fadd_rn(ax, px) : px;
        ay = j ? __fadd_rn(ay, py) : py;
    }
    ax = row16_sum(ax);
    ay = row16_sum(ay);
    Gx = (x <= 0.0f || x >= mx) ? 0.0f : __fmul_rn(sc.hx[d], ax);
    Gy = (y <= 0.0f || y >= my) ? 0.0f : __fmul_rn(sc.hy[d], ay);
}

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
    const float n0 = norm_coord(p0, sc.lo[0], sc.range[0]), n1 = norm_coord(p1, sc.lo[1], sc.range[1]), n2 = norm_coord(p2, sc.lo[2], sc.range[2]);
    const float* const rows[3] = {rows0, rows1, rows2};
    float dn0 = 0.0f, dn1 = 0.0f, dn2 = 0.0f;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        if (!rows[d]) continue;                                        // (kernel argument: uniform)
        const float* P = sc.proj + 6 * d;
        float Gx, Gy;
        // the projection as ray_pos_taps (bwd_core.h) writes it
        plane_slope(sc, d, n0 * P[0] + n1 * P[2] + n2 * P[4], n0 * P[1] + n1 * P[3] + n2 * P[5], rows[d] + m * C, sub, Gx, Gy);
        dn0 = __fadd_rn(dn0, __fadd_rn(__fmul_rn(P[0], Gx), __fmul_rn(P[1], Gy)));
        dn1 = __fadd_rn(dn1, __fadd_rn(__fmul_rn(P[2], Gx), __fmul_rn(P[3], Gy)));
        dn2 = __fadd_rn(dn2, __fadd_rn(__fmul_rn(P[4], Gx), __fmul_rn(P[5], Gy)));
    }
    const bool bad = (p0 != p0) || (p1 != p1) || (p2 != p2);
    const float dn = sub == 0 ? dn0 : (sub == 1 ? dn1 : dn2);
    const float range = sub == 0 ? sc.range[0] : (sub == 1 ? sc.range[1] : sc.range[2]);
    const float out = bad ? __int_as_float(0x7fc00000) : __fdiv_rn(__fmul_rn(2.0f, dn), range);
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
