// The positional-encoding NeRF baseline (config/MipNeRF_baseline.yml with encode_position_fn: positional_encoding): the points
// ro + rd z of every sample depth, their positional encoding and the FlexibleNeRFModel they feed, forward and training.
//
// Reference: train_utils.py:71-182 with mip_nerf=False (pts = ro[..., None, :] + rd[..., None, :] * z_vals[..., :, None], two f32 roundings),
// nerf_helpers.py:552-575 (positional_encoding(pts, 6, include_input=True): [x | sin(2^0 x) | cos(2^0 x) | .. | sin(2^5 x) | cos(2^5 x)], 3
// columns each, and positional_encoding(viewdir, 4, include_input=True) for the 27 direction columns), models.py:14-108 (FlexibleNeRFModel
// with the constructor defaults, train_nerf.py:338-348).
//
// This file holds the encoder (PeEncoder: one point's row, computed where the layer engine needs it); the kernels are the templates of
// nerf_mlp.h with a layer-1 input of 39 columns -- nerf_encode_kernel / nerf_forward_kernel<PeEncoder>, nerf_backward_kernel<39>,
// nerf_wgrad_kernel<39>.
#include "nerf_mlp.h"

namespace nvsr {

using PeLayout = NerfLayout<39>;
constexpr int PE_ENC = PeLayout::ENC;
static_assert(PeLayout::NAT == NVSR_PE_NERF_NATURAL_FLOATS, "natural blob size");
static_assert(PeLayout::REC == NVSR_PE_NERF_RECORD_FLOATS && NERF_GREC == NVSR_PE_NERF_GRAD_RECORD_FLOATS, "record sizes");

// column c (0 .. 65) of the encoded row of sample j of ray i (p = i S + j); the point is rounded like the reference's two f32 tensor ops, and
// 2^l x is exact
__device__ float pe_column(const float* __restrict__ rays, const float* __restrict__ z, int S, long p, int c) {
    const long i = p / S;
    const float* r = rays + i * 11;
    if (c >= PE_ENC) return dir_column(r, c - PE_ENC);
    const int d = c < 3 ? c : (c - 3) % 3;
    const float x = __fadd_rn(r[d], __fmul_rn(r[3 + d], z[p]));
    if (c < 3) return x;
    const int q = c - 3, l = q / 6, s = q % 6;
    const float v = __fmul_rn(ldexpf(1.0f, l), x);
    return s < 3 ? sinf(v) : cosf(v);
}

struct PeEncoder {
    static constexpr int ENC = PE_ENC;
    const float* rays;
    const float* z;
    int S;
    __device__ float operator()(long p, int c) const { return pe_column(rays, z, S, p, c); }
};

}  // namespace nvsr

using namespace nvsr;

extern "C" {

int nvsr_pe_encode(int64_t N, int S, const float* rays, const float* z, float* out, nvsr_stream_t stream) {
    return nerf_encode_launch(N, S, rays, z, PeEncoder{rays, z, S}, out, (hipStream_t)stream);
}

int nvsr_pe_nerf_forward_arith(int64_t N, int S, const float* rays, const float* z, const float* natural, float* raw, float* record, int arithmetic,
                               nvsr_stream_t stream) {
    return nerf_forward_launch(N, S, rays, z, PeEncoder{rays, z, S}, natural, raw, record, arithmetic, (hipStream_t)stream);
}

int nvsr_pe_nerf_backward_arith(int64_t P, const float* natural, const float* record, const float* g_raw, float* grad_record, int arithmetic,
                                nvsr_stream_t stream) {
    return nerf_backward_launch<PE_ENC>(P, natural, record, g_raw, grad_record, arithmetic, (hipStream_t)stream);
}

int64_t nvsr_pe_nerf_wgrad_workspace_floats(int64_t P) { return nerf_wgrad_workspace_floats<PE_ENC>(P); }

int nvsr_pe_nerf_weight_grad(int64_t P, const float* record, const float* grad_record, float* workspace, float* grad_natural, nvsr_stream_t stream) {
    return nerf_weight_grad_launch<PE_ENC>(P, record, grad_record, workspace, grad_natural, (hipStream_t)stream);
}

}  // extern "C"
