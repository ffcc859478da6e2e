// Device functions of the tri-plane model's position gradient, shared by points_grad.hip (nvsr_triplane_points_grad) and normals.hip
// (nvsr_normals_composite): the tap slope of a plane and its chain through the projection and the normalisation.  One arithmetic, stated in
// include/nvsr.h (nvsr_triplane_points_grad): every operation is a single correctly rounded one (__f*_rn).
#pragma once
#include "bwd_core.h"

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

// dn_k = sum over the position planes of (M[k][0] Gx + M[k][1] Gy) for ONE point p = (p0, p1, p2) whose rows are row m of rows[0..2] (a NULL
// plane adds nothing; uniform across the wave): the same three values in every lane of the point's row of 16.  PRECONDITION: all 64 lanes active.
__device__ __forceinline__ void point_slope(const SceneDev& sc, float p0, float p1, float p2, const float* const (&rows)[3], long m, int sub,
                                            float& dn0, float& dn1, float& dn2) {
    const float n0 = norm_coord(p0, sc.lo[0], sc.range[0]), n1 = norm_coord(p1, sc.lo[1], sc.range[1]), n2 = norm_coord(p2, sc.lo[2], sc.range[2]);
    dn0 = dn1 = dn2 = 0.0f;
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
}
// d_points[k] from dn_k: (2 dn_k) / range_k, NaN if a coordinate of the point is NaN
__device__ __forceinline__ float point_slope_component(float dn, float range, bool bad) {
    return bad ? __int_as_float(0x7fc00000) : __fdiv_rn(__fmul_rn(2.0f, dn), range);
}

}  // namespace nvsr
