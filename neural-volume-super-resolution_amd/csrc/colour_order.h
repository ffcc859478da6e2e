// The two-phase route's lists and the colour pass's orders (colour_order.hip), as far as the render kernels and their launchers
// (render3.hip) need them.  Not part of the public ABI.
#pragma once
#include "tile_pair.h"

namespace nvsr {

// The colour pass's ray order (live_order_kernel, colour_order.hip): rays are regrouped inside blocks of ORDER_RAYS consecutive rays -- 16 workgroups, the
// 128 x 32-pixel super-block of train_utils.patch_order -- by the bin of their live count, ORDER_BINS bins of equal width over 1..S and one
// for the empty rays.  A packed entry of live_n is (count << ORDER_SHIFT) | index of the ray in its block.
// ORDER_BINS = 32 is measured (profiles/colour_order_ab.txt): 8 and 16 bins leave more padding, an exact sort loses more of the
// lanes' shared texels than its fewer steps win back.
constexpr int ORDER_SHIFT = 12, ORDER_RAYS = 1 << ORDER_SHIFT, ORDER_BINS = 32;
constexpr int ORDER_MAX_S = 1 << (31 - ORDER_SHIFT);      // a count has to fit above the index
static_assert(ORDER_RAYS % RAYS2 == 0, "a block of the ray order is a whole number of workgroups");

// The point-major colour pass (point_order_kernel, colour_order.hip; render3.hip PHASE 3): a group's live points in the order (band, slot, k),
// POINT_BANDS depth bands over a ray's near..far (0: a band per sample), cut into steps of RAYS2 points; an entry is (slot << 24) | k.
// POINT_BANDS = 0 is measured (profiles/colour_points_ab.txt): 4, 8 and 16 bands leave the fine colour kernel 1.2, 0.7 and 0.5 ms
// slower -- the finer the bands, the closer a wave's points lie, and a band per sample also keeps the runs of a step short.
#ifndef NVSR_POINT_BANDS
#define NVSR_POINT_BANDS 0
#endif
constexpr int POINT_BANDS = NVSR_POINT_BANDS, POINT_NONE = -1, POINT_VIEW_FLOATS = 2 * HALF_C;
static_assert(RAYS2 <= 256 && ORDER_MAX_S <= (1 << 24), "a slot and a list index share an entry");

// the lists of one two-phase launch, in the library's scratch: z, w [N, S] rows, n [N]; slot, trip: [G] each, G = ceil(N / RAYS2)
// pts: the point-major route's entries, [G RAYS2 S]; steps [G], then offs [G]; views [G RAYS2, POINT_VIEW_FLOATS] -- all NULL: the lockstep colour kernels
struct LiveLists { float* z; float* w; int* n; int* slot; int* trip; int* pts; int* steps; float* views; };

// the kept lists of one occupancy launch (include/nvsr.h, "Occupancy grid"), in the library's scratch: idx [N, S] rows of sample indices in
// sample order (the first count entries are valid, the others -1), n [N] counts -- rewritten by live_order_kernel into packed entries like
// the live counts --, and the order of dispatch of the density pass over them: slot [G], trip [G]
struct KeptLists { int* idx; int* n; int* slot; int* trip; };

// The scratch of one render pass, asked for once per pass (colour_order.hip owns it, per (device, stream)); the answer is the pass's route:
//   Fused      the fused kernel, no lists: the caller wants the raw decoder outputs, NVSR_RENDER_ONE_PHASE=1 is set (the A/B handle), the stream
//              is being captured (the scratch cannot grow inside a capture), a count would not fit into a packed entry of the ray order
//              (S >= 2^19) or the lists cannot be had -- same pixels
//   TwoPhase   `live` is filled.  Also the answer to want_kept where the kept lists cannot be had: the pass runs the plain route
//   Occupancy  want_kept only: `live` and `kept` are filled
// An occupancy pass that is not answered Occupancy forgets the kept counts of the stream's latest occupancy launch
// (nvsr_internal_copy_kept_counts returns an error).  launch = false sizes the scratch and leaves no launch behind.
enum class PassRoute { Fused, TwoPhase, Occupancy };
PassRoute acquire_pass_scratch(int64_t N, int S, hipStream_t stream, bool raw_out, bool want_kept, bool launch, LiveLists& live, KeptLists& kept);
// a two-phase pass whose density launch was not the tile-pair kernels' says so behind acquire_pass_scratch (1: the one-tile kernels of
// density_tile.hip); nvsr_internal_density_kernel reads it back
void note_density_kernel(hipStream_t stream, int which);
// the ray order, then the order of dispatch: between the density and the colour launch
void launch_colour_order(const LiveLists& ll, int64_t N, int S, hipStream_t stream);
// the same two orders for the density pass over the kept lists (live_order_kernel and group_order_kernel on the kept counts)
void launch_kept_order(const KeptLists& kl, int64_t N, int S, hipStream_t stream);
// the order of points, behind the two orders above (ll.pts != NULL); rays_nf: the packed rays (near, far) when the lists hold depths, NULL when sample indices
void launch_point_order(const LiveLists& ll, const float* rays_nf, int64_t N, int S, hipStream_t stream);

}  // namespace nvsr
