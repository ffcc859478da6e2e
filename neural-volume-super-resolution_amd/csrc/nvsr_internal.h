// Every extern "C" symbol that crosses files inside the library and is not declared in include/nvsr.h, in one place: the file that defines a
// symbol and every file that calls it include this header, so the compiler checks each definition against the prototype its callers see
// (the symbols are extern "C": a prototype that drifted would still link and pass wrong arguments at run time).  Not part of the public ABI;
// tests and tools that call a *_launch symbol directly take its prototype from capi.py.
#pragma once
#include "nvsr_common.h"

extern "C" {
// the fused render pass, second and third generation (render2.hip, render3.hip); coarse_z: the coarse pass with its depths computed in the kernel
int nvsr_render_pass2_launch(const nvsr_scene* scene, const float* packed_decoder, int64_t N, int S, const float* rays, const float* z, const float* noise, int white_bkgd,
                             float* rgb, float* disp, float* acc, float* weights, float* depth, float* raw_out, nvsr_stream_t stream);
int nvsr_render_pass3_launch(int limbs, const nvsr_scene* scene, const float* packed_decoder, int64_t N, int S, const float* rays, const float* z, const float* noise,
                             int white_bkgd, float* rgb, float* disp, float* acc, float* weights, float* depth, float* raw_out, nvsr_stream_t stream);
int nvsr_render_pass3_coarse_z_launch(int limbs, const nvsr_scene* scene, const float* packed_decoder, int64_t N, int S, const float* rays, int lindisp, const float* noise,
                                      int white_bkgd, float* rgb, float* disp, float* acc, float* weights, float* depth, float* raw_out, nvsr_stream_t stream);
// the limb fragments behind the f32 ones of the packed blobs (render3.hip, render_bwd_limb.hip)
int nvsr_pack_decoder_limbs_launch(const float* natural, float* packed, nvsr_stream_t stream);
int nvsr_pack_decoder_bwd_limbs_launch(const float* natural, float* packed_bwd, nvsr_stream_t stream);
// the training forward on the limb matrix pipe (decode_limb.hip, decode_pair.hip) and its gate-driven backward (render_bwd_limb.hip)
int nvsr_decode_rays_limb_launch(int limbs, const nvsr_scene* scene, const float* packed_decoder, int64_t N, int S, const float* rays, const float* z, float* raw,
                                 uint32_t* gates, float* record, nvsr_stream_t stream);
int nvsr_decode_rays_pair_launch(const nvsr_scene* scene, const float* packed_decoder, int64_t N, int S, const float* rays, const float* z, float* raw, uint32_t* gates,
                                 nvsr_stream_t stream);
int nvsr_render_pass_backward_gates_limb_launch(int limbs, const nvsr_scene* scene, const float* packed_decoder, const float* packed_bwd, int64_t N, int S, const float* rays,
                                                const float* z, const float* g_raw, const uint32_t* gates, float* const* grad_planes, float* view_ws, float* record,
                                                nvsr_stream_t stream);
// the ROWS variant of the same kernel (deterministic route): rows[d][N * S][48] instead of gradient planes
int nvsr_render_pass_backward_rows_limb_launch(int limbs, const nvsr_scene* scene, const float* packed_decoder, const float* packed_bwd, int64_t N, int S, const float* rays,
                                               const float* z, const float* g_raw, const uint32_t* gates, float* const* rows, float* view_ws, float* record,
                                               nvsr_stream_t stream);
// density_tile.hip: the density pass of the two-phase route on two f16 limbs, one 32-ray tile per wave, one 8-wave workgroup per CU
// (z = NULL: depths in registers, `lindisp`); writes what render_pass3_density[_z]_kernel<2> writes
int nvsr_density_tile_launch(const nvsr_scene* scene, const float* packed_decoder, int64_t N, int S, const float* rays, const float* z, int lindisp,
                             const float* noise, float* disp, float* acc, float* weights, float* depth, float* live_z, float* live_w, int* live_n,
                             nvsr_stream_t stream);
// render.hip: NVSR_ARITH_INHERIT -> the process default, anything that is not a mode -> -1; the mode named by an environment variable (dflt if unset;
// conv != 0: the variable of the convolutions, which also takes "f16")
int nvsr_internal_resolve_decoder_arith(int arithmetic);
int nvsr_internal_resolve_render_arith(int arithmetic);      // + NVSR_ARITH_F16 by name (the evaluation renders' fused passes)
int nvsr_internal_parse_arith_env(const char* name, int dflt, int conv);
// colour_order.hip: size the two-phase route's scratch for a pass of N rays x S samples before a frame's first launch (acquire_pass_scratch
// of colour_order.h as a reservation: it leaves no launch behind)
void nvsr_internal_reserve_render_scratch(int64_t N, int S, nvsr_stream_t stream);
// sr.hip: the route of one convolution launch of H x W (sr_core.h: conv_route -- kernel family, packed region read; rows_per_tile as the *_arith
// entry points take it) and the regions the packer writes for that arithmetic (conv_kinds_for); NVSR_PACK_ALL_ARITHMETICS: the packer's answer alone
int nvsr_internal_conv_route(int Cin, int Cout, int H, int W, int arithmetic, int rows_per_tile, int* family, int* region, unsigned* packed_kinds);
}  // extern "C"

namespace nvsr {

inline int check_scene(const nvsr_scene* s) {
    if (!s) return NVSR_ERR_NULL;
    for (int d = 0; d < 4; ++d) {
        if (!s->planes[d]) return NVSR_ERR_NULL;
        if (!aligned16(s->planes[d])) return NVSR_ERR_ALIGN;
        if (s->ph[d] < 1 || s->pw[d] < 1 || (int64_t)s->ph[d] * s->pw[d] * NVSR_PLANE_CHANNELS >= (int64_t)1 << 31) return NVSR_ERR_SHAPE;
    }
    return NVSR_OK;
}

}  // namespace nvsr
