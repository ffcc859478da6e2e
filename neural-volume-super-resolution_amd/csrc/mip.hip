// The Mip-NeRF baseline (config/MipNeRF_baseline.yml): integrated positional encoding of conical frustums and the FlexibleNeRFModel it feeds,
// forward and training.
//
// Reference: mip.py:9-44 (cast_rays -> conical_frustum_to_gaussian -> lift_gaussian), mip.py:154-199 (IntegratedPositionalEncoding with
// multires 7: degrees 2^0 .. 2^5, a sin block of 18 columns ordered (l, d) then the cos block as sin(y + pi/2), both damped by
// exp(-0.5 var 4^l)), nerf_helpers.py positional_encoding(viewdir, 4, include_input) for the 27 direction columns, train_utils.py:19-27
// (radius = ds 0.00135 2 / sqrt(12)), models.py:14-108 (FlexibleNeRFModel with the constructor defaults, train_nerf.py:342-348).
//
// This file holds the encoder (MipEncoder: one interval's row, computed where the layer engine needs it); the kernels are the templates of
// nerf_mlp.h with a layer-1 input of 36 columns -- nerf_encode_kernel / nerf_forward_kernel<MipEncoder>, nerf_backward_kernel<36>,
// nerf_wgrad_kernel<36>.
#include "nerf_mlp.h"

namespace nvsr {

using MipLayout = NerfLayout<36>;
constexpr int MIP_ENC = MipLayout::ENC;
static_assert(MipLayout::NAT == NVSR_MIP_NERF_NATURAL_FLOATS, "natural blob size");
static_assert(MipLayout::REC == NVSR_MIP_NERF_RECORD_FLOATS && NERF_GREC == NVSR_MIP_NERF_GRAD_RECORD_FLOATS, "record sizes");

// column c (0 .. 62) of the encoded row of interval j of ray i; every operation rounded like the reference's f32 tensor expressions
__device__ float mip_column(const float* __restrict__ rays, const float* __restrict__ edges, int S, float r2, long p, int c) {
    const long i = p / S;
    const int j = (int)(p - i * S);
    const float* r = rays + i * 11;
    if (c >= MIP_ENC) return dir_column(r, c - MIP_ENC);
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

struct MipEncoder {
    static constexpr int ENC = MIP_ENC;
    const float* rays;
    const float* edges;
    int S;
    float r2;
    __device__ float operator()(long p, int c) const { return mip_column(rays, edges, S, r2, p, c); }
};

}  // namespace nvsr

using namespace nvsr;

extern "C" {

int nvsr_mip_encode(int64_t N, int S, const float* rays, const float* edges, double radius, float* out, nvsr_stream_t stream) {
    return nerf_encode_launch(N, S, rays, edges, MipEncoder{rays, edges, S, (float)(radius * radius)}, out, (hipStream_t)stream);
}

int nvsr_mip_nerf_forward_arith(int64_t N, int S, const float* rays, const float* edges, double radius, const float* natural, float* raw,
                                float* record, int arithmetic, nvsr_stream_t stream) {
    return nerf_forward_launch(N, S, rays, edges, MipEncoder{rays, edges, S, (float)(radius * radius)}, natural, raw, record, arithmetic,
                               (hipStream_t)stream);
}

int nvsr_mip_nerf_backward_arith(int64_t P, const float* natural, const float* record, const float* g_raw, float* grad_record, int arithmetic,
                                 nvsr_stream_t stream) {
    return nerf_backward_launch<MIP_ENC>(P, natural, record, g_raw, grad_record, arithmetic, (hipStream_t)stream);
}

int64_t nvsr_mip_nerf_wgrad_workspace_floats(int64_t P) { return nerf_wgrad_workspace_floats<MIP_ENC>(P); }

int nvsr_mip_nerf_weight_grad(int64_t P, const float* record, const float* grad_record, float* workspace, float* grad_natural, nvsr_stream_t stream) {
    return nerf_weight_grad_launch<MIP_ENC>(P, record, grad_record, workspace, grad_natural, (hipStream_t)stream);
}

}  // extern "C"
