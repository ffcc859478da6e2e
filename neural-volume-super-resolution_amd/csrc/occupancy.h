// The occupancy route of the render pass (include/nvsr.h, "Occupancy grid"): what occupancy.hip (the grid's build and the cull kernel)
// and render3.hip (the density pass over the kept lists) share; the kept lists and their scratch: colour_order.h.  Not part of the public ABI.
#pragma once
#include "colour_order.h"

namespace nvsr {

constexpr int OCC_MAX_G = 512, OCC_MAX_K = 4;

// The cell of a normalised point along one axis: clamp((int)floorf(((n + 1) * 0.5) * G), 0, G - 1), every step one correctly rounded f32
// operation; the clamp is done on the float (the same integer wherever the conversion is defined, and defined for +-inf too).
// A NaN coordinate has no cell: the caller keeps such a sample.
__device__ __forceinline__ int occupancy_cell(float n, int G) {
    const float f = floorf(__fmul_rn(__fmul_rn(__fadd_rn(n, 1.0f), 0.5f), (float)G));
    return (int)fminf(fmaxf(f, 0.0f), (float)(G - 1));
}

// occupancy.hip: one wave per ray -> kept[N, S], kept_n[N] (z = NULL: the depths of coarse_depth(near, far, s, S, lindisp))
void launch_occupancy_cull(const SceneDev& sc, int64_t N, int S, const float* rays, const float* z, int lindisp, const uint32_t* grid, int G, int* kept, int* kept_n,
                           hipStream_t stream);

}  // namespace nvsr
