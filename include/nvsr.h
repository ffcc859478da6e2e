/*
 * nvsr.h -- C ABI of the MI355X (gfx950) implementation of the Neural-Volume-Super-Resolution rendering hot path.
 *
 * The reference (pure PyTorch) has no FFI; its boundary for this path is the Python call surface used by
 * train_nerf.py.  Every entry point below replaces the ATen dispatches of one reference
 * function; the citation gives the reference file:line.  The host-side mirror of the reference interface lives in
 * neural-volume-super-resolution_amd/ and binds these symbols with ctypes.
 *
 * Conventions
 *   - all pointers are DEVICE pointers (fp32 unless stated) except `const nvsr_scene*`, a small host struct passed by value
 *     to the kernels; the library never allocates, never synchronises, and launches on `stream` (a hipStream_t);
 *   - tensors are dense row-major with the shapes given; "ray-major" [N,S] means S contiguous per ray;
 *   - return value: 0 = NVSR_OK, otherwise an nvsr_status; nothing is written on a shape error;
 *   - random inputs of the reference (stratified jitter t_rand, importance u, density noise) are explicit tensors so that
 *     train-mode results are reproducible (reference draws them on the CPU generator: train_utils.py:108,
 *     nerf_helpers.py:683, volume_rendering_utils.py:32).
 */
#ifndef NVSR_H
#define NVSR_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* nvsr_stream_t; /* hipStream_t */

typedef enum {
    NVSR_OK = 0,
    NVSR_ERR_SHAPE = 1,   /* argument out of the supported range */
    NVSR_ERR_LAUNCH = 2,  /* hipGetLastError() != hipSuccess after a launch */
    NVSR_ERR_NULL = 3,    /* required pointer is NULL */
    NVSR_ERR_ALIGN = 4    /* pointer not 16-byte aligned */
} nvsr_status;

/* Decoder geometry compiled into the MFMA kernels: TwoDimPlanesModel(dec_density_layers=4, dec_rgb_layers=4,
 * dec_channels=128, num_plane_channels=48, proj_combination='avg', viewdir_proj_combination='concat_pos'), the only
 * configuration the shipped YAMLs instantiate (config/TrainModels.yml, Feature_Planes_Only.yml; models.py:118-197). */
#define NVSR_PLANE_CHANNELS 48
#define NVSR_DEC_CHANNELS 128
#define NVSR_DEC_LAYERS 4
#define NVSR_DECODER_NATURAL_FLOATS 130564 /* state-dict order, see nvsr_pack_decoder */
#define NVSR_DECODER_PACKED_F32_FLOATS 130576 /* f32 MFMA-fragment order + biases/heads */
/* packed blob = [f32 fragments + biases/heads][bf16 fragments, 3 limbs per weight][bf16 fragments, 2 limbs per weight] (32-bit words) */
#define NVSR_DECODER_PACKED_FLOATS 453136
#define NVSR_DECODER_PACKED_BWD_FLOATS 487424 /* transposed layers for the backward pass (f32 fragments + 3-bf16-limb + 2-f16-limb fragments), see nvsr_pack_decoder_bwd */

/* One scene = 3 position planes + 1 view-direction plane, CHANNEL-LAST [H][W][48] (192 B per texel), the per-scene
 * normalisation box (models.py:261-268) and the plane projections rot_mats[d][:,1:] (models.py:471-497). */
typedef struct nvsr_scene {
    const float* planes[4]; /* device, channel-last; [0..2] position planes D0..D2, [3] view-direction plane */
    int32_t ph[4], pw[4];   /* rows (grid y) and columns (grid x) of each plane */
    float lo[5];            /* (float)box[0][i] */
    float range[5];         /* (float)(box[1][i] - box[0][i]), subtraction in double like the reference */
    float proj[3][6];       /* row-major 3x2: grid = n_xyz @ proj[d] */
} nvsr_scene;

int nvsr_version(void);

/* Arithmetic of the decoder GEMMs: the fused render pass (nvsr_render_pass*, N >= 16384 rays) and the training kernels
 * (nvsr_decode_rays*, nvsr_render_pass_backward_gates, nvsr_decoder_weight_grad -- what computes a gradient uses 3 limbs whenever a limb
 * mode is selected; a forward and the backward that consumes its gates / record must both run limb modes or both run f32).
 * Inputs, outputs, accumulation and everything outside the GEMMs are f32 in every mode.
 *   NVSR_ARITH_F32    v_mfma_f32_32x32x2_f32: exact f32 products, f32 accumulation -- the reference's arithmetic
 *   NVSR_ARITH_BF16X3 every f32 operand split exactly into 3 bf16 limbs (8 + 8 + 8 significant bits, by truncation), the products
 *                     Wh(xh + xm + xl) + Wm(xh + xm) + Wl xh on v_mfma_f32_32x32x16_bf16, 2.7x the f32 matrix rate.  Error of a dot
 *                     product of K terms, relative to sum |W_k||x_k|:
 *                       - the three dropped products: |Wm xl| + |Wl xm| + |Wl xl| < (2^-22 + 2^-22 + 2^-30) |W||x| = 2^-21 + 2^-30
 *                         (truncation limbs: |m| < 2^-7 |v|, |l| < 2^-15 |v|) -- about FOUR f32 roundings per product at worst, and
 *                         one-sided: truncated limbs carry the operand's sign, so the dropped part has the sign of W x and adds up
 *                         over K instead of averaging out;
 *                       - plus one f32 rounding of the running sum per MFMA that adds into it: 6 K / 16 of them (K / 2 for the f32
 *                         MFMA), <= 2^-24 each -- the products are exact, the sums are ordinary f32 sums.
 *                     Measured on adversarial operands (every mantissa 0x7FFFFF or 0x00FFFF, equal signs, K = 192; tests/
 *                     test_hip_round2.py::test_limb_error_bound): max error 9.8e-7 (2^-20), mean -1.8e-7, against 5.6e-7 / +1.8e-8 for
 *                     the exact-f32 kernel.  NOT bit-grade f32; every parity tolerance of the path holds in it (2e-5 on decoder outputs;
 *                     PSNR of the 800^2 frame vs the double-precision oracle 89.2 dB against 90.8 dB).  Default of rounds 1-3 for the
 *                     render pass; still what every training kernel runs (no exponent-range limits: gradients span many decades).
 *   NVSR_ARITH_F16X2  every f32 operand split into 2 f16 limbs by ROUNDING TO NEAREST: hi = RN(x) (11 significant bits), lo = RN(x - hi)
 *                     (x - hi is exact in f32); |x - hi - lo| <= 2^-23 |x| (one f32 ulp, and zero for three operands in four).  Products
 *                     Wh xh + Wh xl + Wl xh on v_mfma_f32_32x32x16_f16 (f16 x f16 products are exact in f32, f32 accumulation): 3 MFMAs
 *                     per f32 product block, 5.3x the f32 matrix rate and twice the rate of NVSR_ARITH_BF16X3.  Error per product
 *                     <= (2^-23 + 2^-23 + 2^-22) |W||x| = 2^-21 |W||x| at worst (the same bound as BF16X3), but with limbs of either sign:
 *                     the dropped Wl xl and the representation errors average out over K instead of adding up, and the sum takes half as
 *                     many f32 roundings (3 K / 16).  Measured against float64 it is as close as BF16X3 or closer (tests/
 *                     test_hip_round3.py::test_limb_gemm_error_bounds; frame PSNR and decoder-output errors in bench.py's line).
 *                     RANGE: f16 has 5 exponent bits, so the kernels carry static power-of-two scales (exact): weights are packed as
 *                     W 2^8 and activations / features are held as x 2^4.  Both limbs are normal numbers for 2^-10 <= |W| < 255 and
 *                     2^-6 <= |x| < 4094; below that the low limb is subnormal (honoured by the matrix pipe) and the error is absolute,
 *                     <= 2^-33 per weight and <= 2^-29 per activation; a weight >= 255 or an activation >= 4094 overflows to inf and
 *                     the pixel comes out NaN -- loud, never a wrong number (use BF16X3 or F32 for such a network).
 *                     The fused render pass (inference), the training forward (nvsr_decode_rays*) and the gate-driven backward
 *                     (nvsr_render_pass_backward_gates*), each with or without the weight-gradient record.  Gradients span many decades --
 *                     from ray to ray and, behind a surface, from sample to sample of one ray and between dL/dsigma and dL/drgb of one
 *                     sample -- but the 128 features of one chain of one POINT do not: the backward scales every point's density chain
 *                     and rgb chain by their own powers of two (exact: a point is a column of every product; the largest |dL/draw| of
 *                     the chain goes to [2^3, 2^4), undone when the chains meet and before the feature gradients are scattered) and
 *                     multiplies by UNSCALED transposed weights (low limb subnormal below |w| = 0.125: absolute error <= 2^-25, ~1e-6
 *                     of a typical weight).  Against the exact-f32 backward on the same gates its plane gradients are as close as the
 *                     3-limb backward's -- relative L2 ~1e-6, worst texel 0.1 % on the gradients of an opaque scene (round 3 scaled
 *                     whole wave tiles: 7e-6 / 1.3 % there; tests/test_hip_round4.py::test_f16_backward_with_the_dynamic_range_of_an_
 *                     opaque_ray, tests/test_hip_round3.py::test_f16_backward_matches_the_f32_backward); the
 *                     gradient half of the record is written UNSCALED, and so is the layer-input half by the recording
 *                     forward (round 4: a pass runs ONE arithmetic, forward and backward, with or without a record).  The weight-gradient
 *                     contraction (nvsr_decoder_weight_grad*) reads that f32 record and runs BF16X3 when F16X2 is selected.
 *                     The gates a forward publishes are signs of pre-activations: any limb backward consumes any limb forward's.
 * The mode is a per-call argument of the *_arith entry points below (NVSR_ARITH_INHERIT = the process default); every other entry point
 * uses the process default, whose initial value comes from the environment variable NVSR_DECODER_ARITHMETIC = f32 | bf16x3 | f16x2
 * and which nvsr_set_decoder_arithmetic changes.  Nothing but that default is process-global: calls with explicit modes are re-entrant
 * across threads and streams. */
#define NVSR_ARITH_INHERIT (-1)
#define NVSR_ARITH_INVALID (-2)     /* what nvsr_get_*_arithmetic returns when the environment variable holds an unknown string: every call
                                       that inherits the process default then fails with NVSR_ERR_SHAPE until nvsr_set_*_arithmetic is called */
#define NVSR_ARITH_F32 0
#define NVSR_ARITH_F16 1            /* THE CONVOLUTIONS (below, "NVSR_ARITH_F16") AND THE EVALUATION RENDERS ("NVSR_ARITH_F16 in the render pass",
                                       right below): nvsr_render_pass_arith, nvsr_render_rays_arith and the fused launches behind them.  Every other
                                       decoder, render, NeRF-baseline, low-rank, occupancy, shared-decoder and deterministic-route entry point
                                       refuses it, and so do nvsr_set_decoder_arithmetic and NVSR_DECODER_ARITHMETIC.  The value of a limb mode is
                                       its limb count. */
#define NVSR_ARITH_F16X2 2
#define NVSR_ARITH_BF16X3 3
#define NVSR_ARITH_DEFAULT NVSR_ARITH_F16X2
int nvsr_get_decoder_arithmetic(void);
int nvsr_set_decoder_arithmetic(int mode);
/* NVSR_ARITH_F16 in the render pass -- mixed precision for evaluation frames, opt-in, BY NAME only (never a process default: nvsr_set_decoder_arithmetic(1)
 * and NVSR_DECODER_ARITHMETIC=f16 answer NVSR_ERR_SHAPE / NVSR_ARITH_INVALID as before).
 *   Arithmetic.  Per layer w^ = RN_f16(W 2^8), x^ = RN_f16(x 2^4) -- F16X2's scales, its high limbs alone -- ONE v_mfma_f32_32x32x16_f16 per product
 *   block in F16X2's K-block and output-block order, f32 accumulation; bias, ReLU, heads and compositing are F16X2's, in f32.  Error: 2^-11 per
 *   operand instead of 2^-23; the decoder's outputs sit about 1e-3 (sigma) / 5e-4 (rgb logits) rms of their own rms from float64
 *   (tests/render_f16_ref.py is the arithmetic in numpy; tests/test_render_f16.py holds the kernels to it).  The weights are limb 0 of F16X2's
 *   fragment region: the packed blob and its size functions are unchanged.
 *   Who takes it.  nvsr_render_pass_arith (raw outputs included) from 16 384 rays on -- below that, and under NVSR_RENDER_V1, it runs the exact-f32
 *   kernel like every other mode -- nvsr_render_rays_arith, and the internal launches nvsr_render_pass3_launch / _coarse_z_launch (limbs = 1).  The
 *   fused kernel, the two-phase route (lockstep and point-major colour pass), their orders and the scratch are chosen exactly as for F16X2, and all
 *   routes give the same bits.  A FRAME BELOW nvsr_fused_min_rays() RAYS (nvsr_render_rays_arith) RUNS ITS UN-FUSED PASSES IN NVSR_ARITH_F16X2: the
 *   decode kernels have no one-limb mode.
 *   Who answers NVSR_ERR_SHAPE to it: nvsr_set_decoder_arithmetic, nvsr_triplane_decode_arith, nvsr_decode_rays*, every backward and weight-gradient
 *   entry, nvsr_render_rays_shared_arith, the occupancy entries (nvsr_occupancy_build, nvsr_render_pass_occupancy_arith,
 *   nvsr_render_rays_occupancy_arith), the Mip-NeRF and PE entries, nvsr_generic_* (of which nvsr_generic_decode_fused_arith_ext takes
 *   NVSR_ARITH_F16X2 by name; the others have no arithmetic argument and run exact f32).
 *   Range contract.  F16X2's ranges (|W| < 255, |feature / activation| < 4094), and never a finite wrong number beyond them.  A lone limb has no
 *   -inf low limb to meet its inf, so an out-of-range operand can leave +-inf in an accumulator where F16X2 leaves NaN: every layer's accumulator and
 *   every head turn +-inf into NaN before the ReLU (the integer-max ReLU would make -inf a 0; an all-positive row would carry +inf to alpha = 1).  A
 *   weight beyond the range poisons the head biases as for F16X2.  A NaN pixel raises bit 1 of the range flag (below) as under F16X2. */
/* Range flag of NVSR_ARITH_F16X2 (round 4).  A launch in that mode whose operands leave the ranges above produces NaN -- which the caller
 * would otherwise have to find by reading its outputs.  With a device word registered here, every F16X2 launch that WRITES A NON-FINITE
 * RESULT also ORs a bit into that word (1 -- the fused render passes: a non-finite rgb / opacity of a ray; nvsr_decode_rays*: a non-finite raw
 * row; 2 -- the SR network: a non-finite value of an output plane inside its region of interest): the host mirror zeroes the word before a frame / an iteration, reads it back
 * asynchronously and re-renders in NVSR_ARITH_BF16X3 or raises (train_utils.py, training.py).  The reference renders any f32 model
 * (models.py:395-421); this is what keeps the drop-in's default arithmetic from ever returning NaN where the reference returns a number.
 * NULL (the initial state) disables the reporting.  The pointer is process-global like the default arithmetic and is read when a launch is
 * enqueued; the word must stay allocated until every launch enqueued while it was registered has finished.  Modes other than F16X2 never
 * touch it (they have no range limit; a NaN they return was a NaN in their inputs) -- except NVSR_ARITH_F16, which shares F16X2's ranges: the
 * convolutions raise bit 2 like F16X2's, the render passes bit 1. */
int nvsr_set_range_flag(uint32_t* device_word);
uint32_t* nvsr_get_range_flag(void);
/* The two-phase render pass.  A fused limb pass (NVSR_ARITH_BF16X3 / _F16X2, N >= nvsr_fused_min_rays) whose caller does not ask for the
 * raw decoder outputs runs as two launches: the DENSITY pass (render_pass3_density[_z]_kernel: planes 0..2, the density decoder, the whole
 * compositing recurrence -- disp, acc, depth, the coarse weights) leaves, per ray, the list of its samples with a weight that is not zero
 * (a NaN weight counts) and their number; the COLOUR pass (render_pass3_colour[_z]_kernel) runs the colour decoder on those entries only, as
 * many steps as the longest list among a workgroup's 256 rays, and adds w sigmoid(raw) in sample order.  A sample with weight +0.0 added +0.0
 * to every sum of the fused kernel, so the outputs are the fused kernel's bit for bit; the one difference lies beyond the F16X2 range: a NaN
 * that only the colour decoder of a weightless sample produces no longer reaches the pixel (the pixel is then the correct finite value; a
 * density-side overflow still gives NaN and raises the range flag -- the density pass checks acc, the colour pass rgb).
 * NVSR_RENDER_ONE_PHASE=1 in the environment (read at every launch) keeps the fused kernel; it also runs when raw outputs are requested,
 * while the stream is being captured into a graph, when S >= 2^19 (a count has to fit into a packed entry, below) or when the scratch below
 * cannot be allocated.
 * Ray order of the colour pass (csrc/colour_order.hip, like the order of dispatch and the scratch below).  Between the two launches live_order_kernel rewrites the N counts in place: inside every block of 4096
 * consecutive rays (16 workgroups) the rays are stably sorted by the bin of their count, fullest bin first -- bin = ceil(count * 32 / S): one
 * bin for the empty rays, 32 of equal width over 1..S -- and entry j of the block becomes (count << 12) | index of that ray in the block.
 * The lane of the colour pass that owned ray j of the block owns the ray entry j names, so a workgroup's 256 rays have similar counts and few
 * of its steps are padding; a ray's sums do not depend on the lane that holds them: same bits.  NVSR_COLOUR_ORDER=0 (read at every launch)
 * makes every entry name its own slot: the grouping of the density pass, for an A/B.
 * Scratch: the lists take 2 N S floats + N ints (0.98 GB for the 800 x 800 x 192 fine pass).  They are NOT part of the caller's workspace
 * (nvsr_render_workspace_floats is unchanged): the library owns one buffer per (device, stream), allocated with hipMalloc at the first
 * two-phase launch on that stream and grown (never shrunk) when a larger pass arrives -- growing waits for the device.
 * nvsr_render_rays and nvsr_render_rays_arith size it for the frame's larger pass (N (Nc + Nf) entries) before the coarse launch, so a frame
 * grows it at most once; nvsr_render_rays_shared_arith's own path asks for raw outputs in every pass, runs the fused kernel and reserves nothing.
 * The buffer stays allocated between frames (0.98 GB at the benchmark size that torch's caching allocator does not see) until it is released.
 * nvsr_release_render_scratch frees every such buffer (the caller makes sure no render launch is still running); later launches allocate anew.
 * nvsr_render_scratch_bytes returns what the library holds at the moment, over all devices and streams (0 until a two-phase launch has
 * run: a caller, or a test, can tell that the two-phase route was taken).
 * Contract: the buffers are keyed by the stream handle and never pruned -- the entry of a destroyed stream keeps its memory (torch's
 * allocator does not see it) until nvsr_release_render_scratch; and only one host thread at a time may enqueue render launches on a given
 * (device, stream): a second thread growing that entry would free the buffer under the first one's launch.
 * Order of dispatch of the colour pass.  A colour workgroup runs as many steps as its longest list, between none and S, and workgroups start
 * in blockIdx order, workgroup b on XCD b % 8.  live_order_kernel also writes group_trip[g], the largest count among entries 256 g .. 256 g +
 * 255 (G = ceil(N / 256) groups; a ragged last group counts what it has), and group_order_kernel (one workgroup, a stable counting sort over
 * 0..S) writes group_slot[r] = the group that workgroup r runs: the groups heaviest first, so rank r lands on XCD r % 8.  A run of groups of
 * equal trip is dealt in pieces, not one by one: the ranks of the run that share an XCD take consecutive groups (the contiguous-eighths formula
 * inside the run; neighbouring groups share texels in their XCD's L2), so a frame whose trips are all equal keeps the density kernels' mapping.
 * The density and fused kernels keep their mapping (XCD x runs the x-th contiguous eighth of the ray blocks); group_slot holds that same
 * mapping with NVSR_COLOUR_GROUP_ORDER=0 (read at every launch, for an A/B) and beyond what the one workgroup sorts: G > 4096 or S > 511.
 * A ray's sums do not depend on the workgroup that holds them: same bits.  The 2 G ints are kept in a buffer of their own beside the lists'
 * (same owner, growth and release; 20 KB at the benchmark size); nvsr_render_scratch_bytes counts the lists' buffer alone.
 * Point-major colour pass (the default).  The lockstep kernels above give a lane a ray and walk all 256 rays of a workgroup to their k-th live
 * sample together: the k-th samples of different rays lie at unrelated depths (one gather instruction touches texels all over a plane) and
 * the workgroup runs as many steps as its fullest ray.  Nothing in a pixel depends on the lane that evaluates a point, only on the order of a
 * ray's additions.  So point_order_kernel (behind the two orders above, one workgroup per group) lists the live points of a group's 256 slots
 * in the order (depth band, slot, k) -- k = the index into the ray's list; band = s * B / S of the sample index s (depths in registers), else
 * ((z - near) * B) / (far - near) truncated and clamped, made monotone along the ray; B = S bands, one per sample (measured against 4, 8 and 16) -- cuts the sequence into steps of
 * 256 points, sorts every step by (slot, k) so that a ray's points of a step are one run, and pads the last step.  The kernels
 * render_pass3_points[_z]_kernel run ceil(points / 256) steps, a lane one point per step: the ray's constants come from the workgroup's ray cache
 * by the entry's slot, its view features from a table the kernel's prologue writes (48 floats per slot), and the point's three terms
 * w sigmoid(raw) go through LDS to the first lane of the run, which adds the run's terms in order to the ray's sums in LDS -- the operands and
 * the order of the lockstep kernels: same bits.  Buffers, owned, grown and released like the lists' and not counted by
 * nvsr_render_scratch_bytes: 256 G S + 2 G ints (entries (slot << 24) | k, group g's at 256 g S; step counts; offsets in steps) and 48 * 256 G
 * floats of view features.  NVSR_COLOUR_POINTS=0 (read at every launch) selects the lockstep kernels, as does a buffer that cannot be had or
 * G S >= 2^31; NVSR_COLOUR_ORDER, NVSR_COLOUR_GROUP_ORDER and NVSR_RENDER_ONE_PHASE keep their meaning and the order of dispatch is group_slot. */
int nvsr_release_render_scratch(void);
int64_t nvsr_render_scratch_bytes(void);
/* Internal hooks of that order (tests and tools; not part of the stable interface).  nvsr_internal_group_order: group_order_kernel alone on
 * G trips (device memory, each 0..S) -> out[G], under the product's handle.  nvsr_internal_copy_group_order: what the latest two-phase
 * launch on `stream` left -> dst (device or host memory), 2 G ints: group_slot[G], then group_trip[G]; G must be that launch's. */
int nvsr_internal_group_order(const int* trips, int64_t G, int S, int* out, nvsr_stream_t stream);
int nvsr_internal_copy_group_order(int* dst, int64_t G, nvsr_stream_t stream);
/* Internal hooks of the ray order.  nvsr_internal_live_order: live_order_kernel alone, with the product's bins, on a caller's array of N counts
 * (device memory, each <= S), in place.  nvsr_internal_colour_order_bins: that number of bins.  nvsr_internal_copy_live_counts: the packed
 * entries the latest two-phase launch on `stream` left in the library's scratch -> dst (N ints, device or host memory; N must be that launch's). */
int nvsr_internal_live_order(int* live_n, int64_t N, int S, nvsr_stream_t stream);
int nvsr_internal_colour_order_bins(void);
int nvsr_internal_copy_live_counts(int* dst, int64_t N, nvsr_stream_t stream);
/* Internal hooks of the order of points.  nvsr_internal_point_order: point_order_kernel alone on a caller's N packed entries of the ray order
 * and [N, S] lists (device memory) -- rays = NULL: the lists hold sample indices as int bits; else depths, and rays[ray * 11 + 6 .. 7] the
 * ray's near and far; bands: 1..S, anything else a band per sample -> points[256 G S], steps[G], offsets[G] (in steps of 256 entries),
 * G = ceil(N / 256); behind a group's steps[g] * 256 entries its part of `points` is not written.  nvsr_internal_point_bands: the product's
 * number of bands (0: a band per sample).  nvsr_internal_copy_point_steps: the step counts the latest two-phase launch on `stream` left ->
 * dst (G ints, device or host memory; G must be that launch's); NVSR_ERR_SHAPE when that launch ran the lockstep colour kernels. */
int nvsr_internal_point_order(const int* entries, const float* lists, const float* rays, int64_t N, int S, int bands, int* points, int* steps, int* offsets,
                              nvsr_stream_t stream);
int nvsr_internal_point_bands(void);
int nvsr_internal_copy_point_steps(int* dst, int64_t G, nvsr_stream_t stream);
/* The density pass of the two-phase route on two f16 limbs has two implementations that write the same bits.  The tile-pair kernels
 * render_pass3_density[_z]_kernel<2> (csrc/render3.hip): one 4-wave workgroup of 256 rays per CU, a wave owns two 32-ray tiles and issues one
 * tile's gathers, bias + ReLU and heads in the gaps of the other tile's MFMAs.  The one-tile kernels density_tile[_z]_kernel
 * (csrc/density_tile.hip): one 8-wave workgroup of 256 rays per CU, a wave owns one tile and runs it in program order, and the two waves of a
 * SIMD are staggered -- waves 4..7 gather a sample's features a step ahead, behind the blocks of layers 0 and 1 -- so that one has the matrix
 * pipe while the other waits for texels; 158 KB of LDS (a weight ring of two 32-KB slots, density layers 0 and 1 resident), at most 256
 * registers per wave.  NVSR_DENSITY_ONE_TILE (read at every launch): 1 selects the one-tile kernels, 0 the tile-pair kernels; unset: the
 * one-tile kernels (the measurement is in profiles/density_one_tile_ab.txt).  The kept-list density pass of the occupancy route, one and three limbs and the fused
 * kernel are not affected.  nvsr_internal_density_kernel (test hook): which of the two the latest two-phase launch on `stream` ran -- 0 the
 * tile-pair kernels (every limb count, the kept lists), 1 the one-tile kernels, -1 when no two-phase launch is on record for the stream. */
int nvsr_internal_density_kernel(nvsr_stream_t stream);
/* Occupancy grid (csrc/occupancy.hip; opt-in: a caller who builds no grid gets the launches and the bits described above).  A grid belongs to one
 * (scene planes, decoder) pair: G^3 bits over the scene's normalised box, 1 <= G <= 512.  Cell (ix, iy, iz) is bit i & 31 of 32-bit word
 * i >> 5, i = (iz G + iy) G + ix; nvsr_occupancy_words(G) = ceil(G^3 / 32) words, the unused bits of the last word 0.
 * Cell of a sample, per axis: c = clamp((int)floorf(((n + 1.0f) * 0.5f) * (float)G), 0, G - 1), n the normalised coordinate exactly as the
 * render kernels form it (2 ((o + d z) - lo) / range - 1), every step one correctly rounded f32 operation; the clamp matches
 * padding_mode='border' (a point outside the box has the border's features).  A sample with a NaN coordinate is KEPT.
 * A CULLED sample (cell bit 0) behaves exactly as if the density decoder had answered sigma + noise <= 0: alpha = 0, w = +0.0, T unchanged
 * (T (1 - 0 + 1e-10f) is T in f32), +0.0 added to depth, acc and the colour sums, weight +0.0 in the [N, S] weights, absent from the live list.
 * A KEPT sample is evaluated with the arithmetic of the two-phase pass; its dist comes from its own successor in the full depth row,
 * z[s + 1] - z[s] (1e10 for s = S - 1), not from the next kept sample.  So an occupancy pass equals, bit for bit in rgb, disp, acc, depth,
 * weights and the live entries, the two-phase pass run with noise = 0 on kept samples and noise = -1e30 on culled ones (as long as T stays
 * a number: behind a NaN transmittance the noise route's culled samples carry NaN weights, this route's +0.0).  One difference is
 * documented: a NaN sigma inside a culled cell no longer reaches the pixel (the pixel is then the finite value of the other samples).
 * The grid is APPROXIMATE by nature: no finite set of probes bounds an MLP over a cell, so a built grid may cull a sample of small positive
 * density.  nvsr_occupancy_build probes every cell at K^3 points, K in 1..4 -- along each axis probe j of cell i at u = ((float)(i K + j) +
 * 0.5f) / (float)(G K) of the box, world coordinate lo + u range, view direction (1, 0, 0): sigma does not depend on it -- with
 * nvsr_triplane_decode_arith in `arithmetic`, sets a cell's bit iff any of its probes has sigma_raw > threshold or a NaN sigma_raw, then
 * applies `dilate` rounds of a 3 x 3 x 3 OR (two buffers, no atomics: deterministic).  It works through the grid in slabs of whole words;
 * workspace: nvsr_occupancy_workspace_floats(G, K) floats (at most 80 MB), 16-byte aligned.  K, threshold and dilate are the caller's knobs.
 * nvsr_render_pass_occupancy_arith is nvsr_render_pass_arith without noise and raw outputs, for the limb arithmetics only and without a
 * minimum ray count (like the kernels behind it): occupancy_cull_kernel (one wave per ray, 64 samples per trip) lists every ray's kept
 * sample indices in sample order, live_order_kernel and group_order_kernel order rays and dispatch on the kept counts as they do for the
 * colour pass, and render_pass3_density_kept[_z]_kernel runs the density decoder over the kept lists -- as many steps as the longest list
 * among a workgroup's 256 rays -- and leaves disp, acc, depth, the weights (zero-filled, then written at the kept samples), the range flag and
 * the live lists; the colour pass and its orders follow unchanged.  z == NULL: the depths are those of nvsr_coarse_z without jitter, formed
 * in registers from the rays' near / far (lindisp as there), and `weights` is required; with z, lindisp is ignored.
 * The route DECLINES and runs the plain route -- always legal: the plain route is what the grid approximates -- where the two-phase pass
 * declines (NVSR_RENDER_ONE_PHASE=1, a stream being captured, S >= 2^19, no scratch) or its own scratch cannot be had.  Scratch: N S + N ints
 * and 2 G ints of group table, owned by the library per (device, stream) beside the live lists, grown and released like them
 * (nvsr_release_render_scratch) and NOT counted by nvsr_render_scratch_bytes, whose value a non-occupancy launch leaves as it was.
 * NVSR_ERR_SHAPE with nothing launched: G outside 1..512, K outside 1..4, dilate < 0, an arithmetic that is not a limb mode on the pass entry. */
int64_t nvsr_occupancy_words(int G);
int64_t nvsr_occupancy_workspace_floats(int G, int K);
int nvsr_occupancy_build(const nvsr_scene* scene, const float* packed_decoder, int G, int K, float threshold, int dilate, int arithmetic, uint32_t* grid,
                         float* workspace, nvsr_stream_t stream);
int nvsr_render_pass_occupancy_arith(const nvsr_scene* scene, const float* packed_decoder, int64_t N, int S, const float* rays, const float* z, int lindisp,
                                     int white_bkgd, float* rgb, float* disp, float* acc, float* weights, float* depth, const uint32_t* grid, int G, int arithmetic,
                                     nvsr_stream_t stream);
/* The frame (nvsr_render_rays_arith without the two noise arguments) with a grid per pass: a pass with a grid goes through
 * nvsr_render_pass_occupancy_arith, a pass whose grid is NULL runs the plain route.  Below nvsr_fused_min_rays() rays, in the f32 arithmetic
 * and with both grids NULL the call is nvsr_render_rays_arith's with noise = NULL: the un-fused path runs and the grids are ignored.
 * (One driver serves both entry points -- render_frame, csrc/aux.hip: this one checks its G arguments and calls it without noise.) */
int nvsr_render_rays_occupancy_arith(const nvsr_scene* scene, const float* packed_coarse, const float* packed_fine, int64_t N, int Nc, int Nf,
                                     const float* rays, int lindisp, int white_bkgd, const float* t_rand, const float* u, float* rgb_c, float* disp_c,
                                     float* acc_c, float* rgb_f, float* disp_f, float* acc_f, float* workspace, const uint32_t* grid_coarse, int G_coarse,
                                     const uint32_t* grid_fine, int G_fine, int arithmetic, nvsr_stream_t stream);
/* Internal hooks of the occupancy route (tests and tools; not part of the stable interface).  nvsr_internal_occupancy_probes: the probe
 * kernel alone over the whole grid -> x [G^3 K^3, 6], probe (jz K + jy) K + jx of cell i at row i K^3 + it.  nvsr_internal_occupancy_cull:
 * the cull kernel alone -> kept [N, S] (a row's first kept_n[ray] entries are the kept sample indices, the others -1), kept_n [N].
 * nvsr_internal_copy_kept_counts: the kept counts the latest occupancy launch on `stream` left -> dst (N ints, device or host memory; N must
 * be that launch's), as packed entries of the ray order, (count << 12) | index of the ray in its block of 4096; NVSR_ERR_SHAPE when none ran or
 * the latest one declined. */
int nvsr_internal_occupancy_probes(const nvsr_scene* scene, int G, int K, float* x, nvsr_stream_t stream);
int nvsr_internal_occupancy_cull(const nvsr_scene* scene, int64_t N, int S, const float* rays, const float* z, int lindisp, const uint32_t* grid, int G, int* kept,
                                 int* kept_n, nvsr_stream_t stream);
int nvsr_internal_copy_kept_counts(int* dst, int64_t N, nvsr_stream_t stream);
/* The arithmetic primitive alone (test hook, one wavefront): Y[32][32] = W[32][K] X[K][32] (row-major f32, K a multiple of 16) with the
 * operands split and multiplied exactly as the kernels of `arithmetic` do it (NVSR_ARITH_F32 | _BF16X3 | _F16X2, incl. the static scales of
 * F16X2) -- lets a test put chosen mantissas / magnitudes through the products that replace models.py:381-421's nn.Linear GEMMs. */
int nvsr_limb_gemm_probe(int arithmetic, int K, const float* W, const float* X, float* Y, nvsr_stream_t stream);
/* Same for the 3x3 convolutions of the SR network (process default + *_arith twins): forward and data gradient of the layers with
 * Cin % 16 == 0 and a multiple of 256, or at most 64, output channels (every layer of EDSR(256); other shapes always use the f32 kernel),
 * and every weight gradient: NVSR_ARITH_F32, NVSR_ARITH_BF16X3 (same error bound as above) or NVSR_ARITH_F16X2 -- the FORWARD convolutions
 * of the layers with Cin % 32 == 0 and Cout % 128 == 0 (EDSR's 65 trunk and 2 up-sampling convolutions, 97 % of the FLOPs) on 2 f16 limbs
 * (3 MFMAs per product block instead of 6; weights packed as W 2^8, the input patch held as x 2^4, same ranges and the same NaN-on-overflow
 * rule as above) -- and their data gradients too, with the power of two that puts the largest |dy| of the layer's whole gradient tensor into
 * [2^12, 2^13) in place of the static activation scale (one reduction per layer: gradients span many decades from layer to layer and step to
 * step, a tensor's values a few) and their weight gradients (X with the static scale, dy with its tensor's); the narrow input / output layers run
 * 3 bf16 limbs in that mode.
 *   NVSR_ARITH_F16 -- mixed precision, opt-in, convolutions only: both operands rounded ONCE to f16, f32 accumulation, f32 storage (activations,
 * gradients and master weights stay f32 in memory).  The same layers, launches, scales and order of work as NVSR_ARITH_F16X2 with the high
 * limb alone: one v_mfma_f32_16x16x32_f16 per product block on w^ = RN_f16(w 2^8) -- limb 0 of F16X2's packed fragments: packing "for F16"
 * packs what packing for F16X2 packs, and the packed sizes do not change -- and x^ = RN_f16(x s), s = 2^4 for activations and the
 * [2^12, 2^13) power of two of its tensor for a data-gradient input and for the dy operand of a weight gradient (X at 2^4); the scales are
 * undone where F16X2 undoes them.  The narrow layers (conv_input, conv_output, any shape outside Cin % 32 == 0 and Cout % 128 == 0) run
 * what they run under F16X2, weight gradients included -- inside a network (the EDSR / PlanesSR entry points) and under an inherited
 * default; the single-layer entry points nvsr_conv3x3[_dgrad|_wgrad]_arith given NVSR_ARITH_F16 by name for such a shape return
 * NVSR_ERR_SHAPE (the layer has no one-limb kernel: a missing kernel is an error, not another arithmetic).
 *   Error model: w^ and x^ are exact inputs of the MFMA and their products are exact in f32, so the only further error is the f32 accumulation
 * of n products, in whatever order:
 *       |y - (sum w^ x^) / (2^8 s)|  <=  1.01 n 2^-24 (sum |w^||x^|) / (2^8 s)
 * with n = 9 Cin for a convolution or data gradient and n = the contracted pixels over all planes of the launch for a weight gradient.  Against
 * the true f32 operands the mode adds at most (2^-10 + 2^-22) sum |w||x| while both are in the normal f16 range -- the price of choosing it.
 *   Range contract: exactly F16X2's.  |W| < 255 and |x| < 4094 (a lone limb overflows to inf where F16X2's high limb does); beyond, the
 * outputs the operand reaches are NaN -- never a wrong number: F16X2's inf meets the -inf of its own low limb, a lone inf would give +-inf
 * (and 0 behind a ReLU), so the kernels write an infinite accumulator as NaN (finite operands cannot produce one) -- an out-of-range weight
 * poisons its outputs, and the PlanesSR entry points raise bit 2 of the range flag (nvsr_set_range_flag) as they do under F16X2.
 * Environment: NVSR_CONV_ARITHMETIC = f32 | bf16x3 | f16x2 | f16. */
#define NVSR_CONV_ARITH_DEFAULT NVSR_ARITH_F16X2
int nvsr_get_conv_arithmetic(void);
int nvsr_set_conv_arithmetic(int mode);

/* ---- data layout ------------------------------------------------------------------------------------------------ */
/* [C,H,W] (reference plane layout, models.py:436-439) -> channel-last [H,W,C]; and back. */
int nvsr_plane_to_channel_last(const float* nchw, float* nhwc, int C, int H, int W, nvsr_stream_t stream);
int nvsr_plane_from_channel_last(const float* nhwc, float* nchw, int C, int H, int W, nvsr_stream_t stream);

/* natural blob = state-dict order (models.py:169-195): density_dec.0.{0..3}.{weight[out,in],bias}, fc_alpha.0.{weight,bias},
 * rgb_dec.0.{0..3}.{weight,bias}, fc_rgb.0.{weight,bias}  ->  packed blob consumed by the decode/render kernels. */
int nvsr_pack_decoder(const float* natural, float* packed, nvsr_stream_t stream);

/* ---- rays (nerf_helpers.py) -------------------------------------------------------------------------------------- */
/* get_ray_bundle (nerf_helpers.py:507-549).  c2w: 16 floats row-major (device).  ro, rd: [(H+2p)*(W+2p), 3].
 * focal_x = get_focal(f,'H'), focal_y = get_focal(f,'W') as the reference names them (:539-540). */
int nvsr_get_ray_bundle(int H, int W, double focal_x, double focal_y, const float* c2w, int padding, double offset,
                        float* ro, float* rd, nvsr_stream_t stream);
/* The rays of N selected pixels only: get_ray_bundle(...)[row, col] as train() uses it (train_nerf.py:814,842-844: the reference
 * generates all H*W rays every iteration, then gathers num_random_rays of them).  row_col [N,2] int32 (device); (row, col) may
 * lie outside the image (padding).  Bit-identical to the corresponding rows of nvsr_get_ray_bundle. */
int nvsr_get_ray_bundle_at(int H, int W, double focal_x, double focal_y, const float* c2w, double offset, int64_t N, const int32_t* row_col,
                           float* ro, float* rd, nvsr_stream_t stream);
/* Training pixels drawn on the device: entries [first, first + n) of a keyed pseudo-random PERMUTATION of range(total), total = H*W --
 * n distinct pixels, the first n draws of `np.random.choice(H*W, n, replace=False)` (train_nerf.py:836-838) with the device as the
 * generator (the reference permutes all H*W indices on the host every iteration: 640 000 for an 800x800 view, more than a whole step
 * of this library).  Ranks that pass the same key and disjoint [first, first + n) draw disjoint shares of one global batch.
 *   permutation: x -> F(x) repeated until F(x) < total ("cycle walking"), F = 8-round balanced Feistel network on 2*hb bits,
 *   hb = the smallest integer >= 1 with 2^(2 hb) >= total; halves L = x >> hb, R = x & (2^hb - 1); round r = 0..7:
 *     h = (uint32) R * 0x9E3779B1 + k_r;  h ^= h >> 15;  h *= 0x85EBCA77;  h ^= h >> 13;  h *= 0xC2B2AE3D;  h ^= h >> 16;
 *     (L, R) <- (R, L ^ (h & (2^hb - 1)));      F(x) = L << hb | R after round 7;
 *   k_r = high 32 bits of splitmix64(key + r)  (splitmix64(x): x += 0x9E3779B97F4A7C15; x = (x ^ x >> 30) * 0xBF58476D1CE4E5B9;
 *   x = (x ^ x >> 27) * 0x94D049BB133111EB; x ^ x >> 31).  Integer arithmetic only: bit-exact against the CPU restatement.
 * Index k of the permutation is pixel (row k % H, col k / H) -- the reference's column-by-column `coords` (train_nerf.py:818-828).
 * row_col [n,2] int32 (what nvsr_get_ray_bundle_at takes).  target (or NULL) [n,channels] = image[row, col, :] of image [H,W,channels]
 * (train_nerf.py:845 `target_s = img_target[select_inds...]`). */
int nvsr_sample_pixels(int64_t total, int H, int W, uint64_t key, int64_t first, int64_t n, const float* image, int channels,
                       int32_t* row_col, float* target, nvsr_stream_t stream);
/* The key of draw number `calls` of a sampler seeded with `seed`: splitmix64(splitmix64(seed) ^ calls) (host function, integer only).
 * DevicePixelSampler passes it to nvsr_sample_pixels; nvsr_sample_pixels_seq derives the same key on the device. */
uint64_t nvsr_sample_key(uint64_t seed, uint64_t calls);
/* nvsr_sample_pixels for launches replayed from a HIP graph (training.GraphedTrainStep): the key is nvsr_sample_key(state[0], state[1]) read
 * from DEVICE memory, and the launch advances state[1] by one when all its workgroups have read it -- replay k of one captured launch
 * draws what the k-th eager nvsr_sample_pixels call of a sampler with the same seed draws.  state: 4 x uint64 on the device
 * {seed, calls, 0 (arrival counter, must be 0 between launches), unused}; launches sharing a state must be ordered on one stream.  n >= 1. */
int nvsr_sample_pixels_seq(int64_t total, int H, int W, uint64_t* state, int64_t first, int64_t n, const float* image, int channels,
                           int32_t* row_col, float* target, nvsr_stream_t stream);
/* img2mse of two images against one target in one launch (train_nerf.py:893-905 computes F.mse_loss(rgb_coarse, target) and
 * F.mse_loss(rgb_fine, target) separately): losses[0] = mean((a - t)^2), losses[1] = mean((b - t)^2) (b may be NULL: losses[1] untouched);
 * g_a / g_b (or NULL) [n] = 2 (x - t) / n, the gradient of the loss with respect to its image.  n <= NVSR_MSE_PAIR_MAX_ELEMS elements
 * (one workgroup sums them; a training batch is 3 x 4096). */
#define NVSR_MSE_PAIR_MAX_ELEMS (1 << 22)
int nvsr_mse_pair(int64_t n, const float* a, const float* b, const float* target, float* losses, float* g_a, float* g_b, nvsr_stream_t stream);
/* the same two losses and their sum, losses3 = {mean((a - t)^2), mean((b - t)^2), their f32 sum} (train_nerf.py:905: loss = coarse_loss +
 * fine_loss) -- the three scalars an iteration reports, contiguous for one copy to the host; no gradients (nvsr_mse_pair_backward) */
int nvsr_mse_pair_sum(int64_t n, const float* a, const float* b, const float* target, float* losses3, nvsr_stream_t stream);
/* gradients of the two losses with the incoming gradients folded in: g_a = (2 (a - t) / n) * *scale_a, g_b = (2 (b - t) / n) * *scale_b
 * (device scalars; NULL = 1; g_a / g_b may be NULL) -- one launch where autograd would run two multiplies behind nvsr_mse_pair's gradients */
int nvsr_mse_pair_backward(int64_t n, const float* a, const float* b, const float* target, const float* scale_a, const float* scale_b, float* g_a,
                           float* g_b, nvsr_stream_t stream);
/* ndc_rays (nerf_helpers.py:578-605) */
int nvsr_ndc_rays(int H, int W, double focal, double near_, int64_t N, const float* ro, const float* rd, float* ro_out,
                  float* rd_out, nvsr_stream_t stream);
/* rays [N,11] = [ro, rd, near, far, viewdir = view_src/|view_src|]  (run_one_iter_of_nerf, train_utils.py:213-226) */
int nvsr_pack_rays(int64_t N, const float* ro, const float* rd, const float* view_src, double near_, double far_,
                   float* rays, nvsr_stream_t stream);
/* coarse depths + stratified jitter (predict_and_render_radiance, train_utils.py:95-109); t_rand [N,Nc] or NULL */
int nvsr_coarse_z(int64_t N, int Nc, const float* rays, int lindisp, const float* t_rand, float* z, nvsr_stream_t stream);

/* ---- importance sampling ------------------------------------------------------------------------------------------ */
/* sample_pdf_2 (nerf_helpers.py:668-702): bins [N,nb], weights [N,nb-1], u [N,ns] or NULL (det=True: linspace(0,1,ns))
 * -> samples [N,ns].  nb <= 256. */
int nvsr_sample_pdf(int64_t N, int nb, int ns, const float* bins, const float* weights, const float* u, float* samples,
                    nvsr_stream_t stream);
/* cumprod_exclusive (nerf_helpers.py:409-430): [N,n] rows -> out[:,0] = 1, out[:,i] = in[:,0] * ... * in[:,i-1]; in and out must not alias */
int nvsr_cumprod_exclusive(int64_t N, int n, const float* in, float* out, nvsr_stream_t stream);
/* autograd of cumprod_exclusive (the reference's helper is differentiable torch code, nerf_helpers.py:409-430): in, out = the forward's input
 * and output [N,n], g_out = dL/dout -> g_in = dL/din; exact for zeros in `in` (no division) */
int nvsr_cumprod_exclusive_backward(int64_t N, int n, const float* in, const float* out, const float* g_out, float* g_in,
                                    nvsr_stream_t stream);
/* torch.sort(x, dim=-1) values of [N,n] rows, n <= 512 (train_utils.py:155); in and out may alias */
int nvsr_sort_rows(int64_t N, int n, const float* in, float* out, nvsr_stream_t stream);
/* fused train_utils.py:144-155: z_mid, sample_pdf(z_mid, w[1:-1], Nf, det = (u == NULL)), sort(cat(z, samples)) -> [N,Nc+Nf] */
int nvsr_importance_resample(int64_t N, int Nc, int Nf, const float* z_coarse, const float* weights, const float* u,
                             float* z_fine, nvsr_stream_t stream);

/* the same with the un-jittered coarse depths of train_utils.py:95-100 recomputed from the rays' near / far (packed rays columns 6, 7)
 * instead of read: z_coarse of nvsr_coarse_z(..., t_rand = NULL) never has to exist (nvsr_render_rays does this for inference frames) */
int nvsr_importance_resample_rays(int64_t N, int Nc, int Nf, const float* rays, int lindisp, const float* weights, const float* u,
                                  float* z_fine, nvsr_stream_t stream);

/* ---- tri-plane decoder -------------------------------------------------------------------------------------------- */
/* TwoDimPlanesModel.forward (models.py:381-421): x [P,6] = [xyz, viewdir] -> out [P,4] = [rgb_raw, sigma_raw].  In the process's default
 * arithmetic (round 4: the limb modes run the training forward's kernel on tiles of 32 consecutive points; NVSR_ARITH_F32 the exact-f32
 * MFMA kernel); nvsr_triplane_decode_arith takes the mode per call. */
int nvsr_triplane_decode(const nvsr_scene* scene, const float* packed_decoder, int64_t P, const float* x, float* out,
                         nvsr_stream_t stream);
int nvsr_triplane_decode_arith(const nvsr_scene* scene, const float* packed_decoder, int64_t P, const float* x, float* out, int arithmetic,
                               nvsr_stream_t stream);

/* ---- compositing -------------------------------------------------------------------------------------------------- */
/* volume_render_radiance_field (volume_rendering_utils.py:6-51), mip_nerf=False.  raw [N,S,4], z [N,S], rd [N,3],
 * noise [N,S] or NULL (already scaled by radiance_field_noise_std).  weights/depth may be NULL. */
int nvsr_composite(int64_t N, int S, const float* raw, const float* z, const float* rd, const float* noise, int white_bkgd,
                   float* rgb, float* disp, float* acc, float* weights, float* depth, nvsr_stream_t stream);

/* same with the ray directions taken from packed rays [N,11] (columns 3..5) */
/* volume_render_radiance_field(..., mip_nerf=True) (volume_rendering_utils.py:19-26,41-42): raw [N,S,4] over the S intervals of the
 * edges z [N,S+1] -- every interval finite (no 1e10 tail), depth_map integrates the interval mid-points */
int nvsr_composite_mip(int64_t N, int S, const float* raw, const float* z, const float* rd, const float* noise, int white_bkgd,
                       float* rgb, float* disp, float* acc, float* weights /* [N,S] or NULL */, float* depth /* or NULL */,
                       nvsr_stream_t stream);
int nvsr_composite_rays(int64_t N, int S, const float* raw, const float* z, const float* rays, const float* noise, int white_bkgd,
                        float* rgb, float* disp, float* acc, float* weights, float* depth, nvsr_stream_t stream);

/* ---- fused per-ray render pass --------------------------------------------------------------------------------------
 * run_network + TwoDimPlanesModel.forward + volume_render_radiance_field for one pass (train_utils.py:111-139 or :156-180):
 * points ro + rd*z are generated, decoded and composited inside one kernel; no [N,S,*] intermediate reaches HBM.
 * rays [N,11], z [N,S] -> rgb [N,3], disp [N], acc [N]; weights [N,S] / depth [N] optional (NULL). */
int nvsr_render_pass(const nvsr_scene* scene, const float* packed_decoder, int64_t N, int S, const float* rays, const float* z,
                     const float* noise, int white_bkgd, float* rgb, float* disp, float* acc, float* weights, float* depth,
                     nvsr_stream_t stream);

/* Un-fused variant for small ray counts (training batches): decoder outputs raw [N,S,4] for all samples of all rays, tiled over
 * (ray block, sample) so that N*S/128 workgroup-steps fill the chip; feed raw to nvsr_composite. */
int nvsr_decode_rays(const nvsr_scene* scene, const float* packed_decoder, int64_t N, int S, const float* rays, const float* z,
                     float* raw, nvsr_stream_t stream);

/* predict_and_render_radiance (train_utils.py:71-182) for a ray chunk: coarse z -> coarse pass -> importance resample ->
 * fine pass.  workspace: nvsr_render_workspace_floats(N, Nc, Nf) floats.  Nf == 0: coarse only (fine outputs untouched).
 * Up to NVSR_FUSED_MIN_RAYS rays the passes run un-fused (nvsr_decode_rays + nvsr_composite), above it fused (nvsr_render_pass). */
#define NVSR_FUSED_MIN_RAYS 65536
/* the same threshold as the library was BUILT with (host mirrors that pick kernels per launch must use this, not a copy of the constant) */
int64_t nvsr_fused_min_rays(void);
int64_t nvsr_render_workspace_floats(int64_t N, int Nc, int Nf);
int nvsr_render_rays(const nvsr_scene* scene, const float* packed_coarse, const float* packed_fine, int64_t N, int Nc, int Nf,
                     const float* rays, int lindisp, int white_bkgd, const float* t_rand, const float* u,
                     const float* noise_coarse, const float* noise_fine, float* rgb_c, float* disp_c, float* acc_c,
                     float* rgb_f, float* disp_f, float* acc_f, float* workspace, nvsr_stream_t stream);

/* ---- feature-plane super-resolution (EDSR wrapped by PlanesSR) ------------------------------------------------------
 * All activations are [C][H][W] fp32 (the reference's layout); convolutions are 3x3, stride 1, no padding, no bias. */
/* one nn.Conv2d weight [Cout][Cin][3][3] -> MFMA fragment order; size = nvsr_conv3x3_packed_floats(Cin, Cout) */
int64_t nvsr_conv3x3_packed_floats(int Cin, int Cout);
int nvsr_pack_conv3x3(const float* w, int Cin, int Cout, float* packed, nvsr_stream_t stream);
/* out = epilogue(conv3x3(in)); epilogue 0 none | 1 ReLU | 2 residual: conv*0.1 + skip[..., 2:-2, 2:-2] with skip [Cout][H+2][W+2]
 * (_Residual_Block.forward, models.py:777-786) | 3 nn.PixelShuffle(2) (out [Cout/4][2(H-2)][2(W-2)]) */
int nvsr_conv3x3(const float* in, int Cin, int H, int W, const float* packed, int Cout, int epilogue, const float* skip, float* out,
                 nvsr_stream_t stream);
/* EDSR(in_channels, out_channels, hidden_size, n_blocks, scale_factor = 2^n_up, padding = 0)  (models.py:789-822).
 * natural = state-dict order: conv_input, residual.{b}.conv1, residual.{b}.conv2, conv_mid, upscale.{0,2,..}, conv_output. */
int64_t nvsr_edsr_natural_floats(int Cin, int Cout, int hid, int nblocks, int n_up);
int64_t nvsr_edsr_packed_floats(int Cin, int Cout, int hid, int nblocks, int n_up);
int nvsr_pack_edsr(const float* natural, int Cin, int Cout, int hid, int nblocks, int n_up, float* packed, nvsr_stream_t stream);
/* The same blob with only the fragment regions that a launch in `arithmetic` reads (NVSR_ARITH_INHERIT = the process default) -- for callers whose
 * weights change between launches: a training iteration (train_nerf.py:903-914: optimizer steps between forwards) re-packs both blobs of the network
 * every iteration, and of the four regions of a layer (f32 fragments, bf16 limbs for two MFMA shapes, f16 limbs) an arithmetic reads one.  The other
 * regions keep whatever `packed` held: such a blob serves launches in THAT arithmetic only (the *_arith entry points with the same value).
 * NVSR_PACK_ALL_ARITHMETICS = every region (what nvsr_pack_edsr does). */
#define NVSR_PACK_ALL_ARITHMETICS (-3)
int nvsr_pack_edsr_arith(const float* natural, int Cin, int Cout, int hid, int nblocks, int n_up, float* packed, int arithmetic, nvsr_stream_t stream);
int nvsr_edsr_out_size(int H, int W, int nblocks, int n_up, int* Ho, int* Wo);
int64_t nvsr_edsr_workspace_floats(int hid, int nblocks, int n_up, int H, int W);
int nvsr_edsr_forward(const float* x, int Cin, int H, int W, const float* packed, int Cout, int hid, int nblocks, int n_up, float* out,
                      float* workspace, nvsr_stream_t stream);
/* PlanesSR.forward (models.py:884-926): lr [C][R0][R1] -> out [C][sf*R0][sf*R1] = EDSR(replicate-padded crop)[over:-over] +
 * bilinear_x{sf}(lr) inside the ROI, NaN outside.  roi: NULL = full plane, else 4 HOST floats [[ymin,xmin],[ymax,xmax]] in [-1,1]
 * (models.py:278-279).  pad = EDSR.required_padding, over = HR_overpadding (models.py:836-842).  mean/std: optional [C] device
 * vectors (planes_{mean,std}_NON_LEARNED). */
/* plane_interp of the reference (config/TrainModels.yml:72,172): how a plane is sampled (grid_sample) and up-sampled (F.interpolate) */
#define NVSR_PLANE_INTERP_BILINEAR 0
#define NVSR_PLANE_INTERP_BICUBIC 1
/* align_corners of the bilinear residual F.interpolate(LR, scale_factor, 'bilinear', align_corners) (models.py:858-859; PlanesSR.align_corners
 * is the planes model's, :222): library state like the conv arithmetic, 1 (every shipped config) unless set; read by every nvsr_planes_sr*
 * call (forward and backward) when it is launched.  A binding with models of both kinds sets it before each call (ops.py does). */
int nvsr_set_sr_align_corners(int align_corners);
int nvsr_get_sr_align_corners(void);
/* ... and its mode (PlanesSR.plane_interp, models.py:858-859): NVSR_PLANE_INTERP_BILINEAR (every shipped config) | NVSR_PLANE_INTERP_BICUBIC */
int nvsr_set_sr_plane_interp(int plane_interp);
int nvsr_get_sr_plane_interp(void);
int64_t nvsr_planes_sr_workspace_floats(int C, int R0, int R1, int hid, int nblocks, int n_up, int pad, const float* roi);
int nvsr_planes_sr(const float* lr, int C, int R0, int R1, const float* packed, int hid, int nblocks, int n_up, int pad, int over,
                   const float* roi, const float* mean, const float* std_, float* out, float* workspace, nvsr_stream_t stream);

/* Batched variants: B planes of equal size share every launch (a single 200^2 plane fills the 256 CUs for only 1.2-1.8 workgroup
 * rounds per layer; the 3 position planes of a scene together for 3.6-5.4).  x [B][Cin][H][W] -> out [B][Cout][Ho][Wo];
 * workspace = B * nvsr_edsr_workspace_floats(...).  nvsr_planes_sr_batch: lr / out are HOST arrays of B device pointers,
 * workspace = B * nvsr_planes_sr_workspace_floats(...). */
int nvsr_edsr_forward_batch(const float* x, int B, int Cin, int H, int W, const float* packed, int Cout, int hid, int nblocks, int n_up,
                            float* out, float* workspace, nvsr_stream_t stream);
int nvsr_planes_sr_batch(const float* const* lr, int B, int C, int R0, int R1, const float* packed, int hid, int nblocks, int n_up, int pad,
                         int over, const float* roi, const float* mean, const float* stdv, float* const* out, float* workspace,
                         nvsr_stream_t stream);

/* ---- positional-encoding baseline (MipNeRF_baseline.yml; not on the tri-plane path) ------------------------------------ */
/* positional_encoding (nerf_helpers.py:552-575): x [P,D] -> [P, (include_input ? D : 0) + 2*D*L] = [x, sin(2^0 x), cos(2^0 x), ...] */
int nvsr_positional_encoding(int64_t P, int D, const float* x, int L, int include_input, float* out, nvsr_stream_t stream);
/* FlexibleNeRFModel.forward (models.py:83-108), use_viewdirs=True, num_layers_dir=1: x [P, dim_xyz+dim_dir] -> [P,4].
 * blob = state-dict order: layer1, layers_xyz.{i}, layers_dir.0, fc_alpha, fc_rgb, fc_feat, each {weight[out,in], bias}. */
int nvsr_flexible_nerf_forward(int64_t P, const float* x, int dim_xyz, int dim_dir, int hidden, int num_layers, int skip_every,
                               const float* blob, float* out, nvsr_stream_t stream);

/* ---- the Mip-NeRF baseline (MipNeRF_baseline.yml; csrc/mip.hip) -------------------------------------------------------------
 * FlexibleNeRFModel(include_input_xyz=False) with the constructor defaults (train_nerf.py:342-348 passes only the encoding arguments):
 * layer1 36->128 (linear), 3 x ReLU(128->128), ReLU(fc_feat) 128->128, fc_alpha 128->1, ReLU(layers_dir(cat(feat, dir))) 155->64, fc_rgb 64->3.
 * natural = state-dict order (layer1, layers_xyz.0-2, layers_dir.0, fc_alpha, fc_rgb, fc_feat, each {weight[out,in], bias}).
 * rays [N,11] (nvsr_pack_rays), edges [N,S+1] (the S intervals of each ray), radius = ds 0.00135 2 / sqrt(12) (train_utils.py:19-27).
 * arithmetic: NVSR_ARITH_F32, NVSR_ARITH_BF16X3 or NVSR_ARITH_F16X2 (3 v_mfma_f32_32x32x16_f16 per product block on 2 round-to-nearest limbs,
 * weights x 2^8 and activations x 2^4 as above, split where they are multiplied: the weights stay the natural f32 blob).  F16X2 has the range
 * contract of the decoder kernels: a weight |W| >= 255 or an activation / encoding |x| >= 4094 enters the products as NaN (a ReLU keeps it),
 * and a launch that writes a non-finite raw row or gradient ORs 1 into the range flag (nvsr_set_range_flag); a gradient chain that grows
 * beyond the f16 range in the backward does the same.  The backward scales each point's chains by powers of two: the rgb chain by the one that
 * puts max |dL/drgb| into [8, 16), the chain from fc_feat down (where dL/dalpha joins) by the one of max |dL/draw|; grad_record is written
 * unscaled (a loss scaled by 2^k gives the same bits times 2^k).  NVSR_ARITH_INHERIT = the decoder default with NVSR_ARITH_F16X2 read as
 * NVSR_ARITH_BF16X3: a caller who never names F16X2 runs what these entry points ran before they had it. */
#define NVSR_MIP_NERF_NATURAL_FLOATS 81092
#define NVSR_MIP_NERF_RECORD_FLOATS 767        /* per point: [enc 36 | dir 27 | h1 | h2 | h3 | h4 | feat (128 each) | hd 64] */
#define NVSR_MIP_NERF_GRAD_RECORD_FLOATS 708   /* per point: pre-activation gradients [layer1 | x0 | x1 | x2 | feat (128 each) | alpha | dir 64 | rgb 3] */
/* cast_rays + IntegratedPositionalEncoding (mip.py:9-44,154-199; degrees 2^0..2^5) and positional_encoding(viewdir, 4):
 * -> out [N*S, 63] = [18 sin | 18 cos (IPE, (degree, axis) with the degree major) | 27 direction columns] */
int nvsr_mip_encode(int64_t N, int S, const float* rays, const float* edges, double radius, float* out, nvsr_stream_t stream);
/* encoding + model on one 32-interval tile per wave, the encoded rows never leave the chip -> raw [N,S,4] (16-byte aligned);
 * record [N*S, NVSR_MIP_NERF_RECORD_FLOATS] or NULL: every layer input and ReLU output, for the backward */
int nvsr_mip_nerf_forward_arith(int64_t N, int S, const float* rays, const float* edges, double radius, const float* natural, float* raw,
                                float* record, int arithmetic, nvsr_stream_t stream);
/* g_raw [P,4] -> grad_record [P, NVSR_MIP_NERF_GRAD_RECORD_FLOATS] (the gradient of every layer's pre-activation output) */
int nvsr_mip_nerf_backward_arith(int64_t P, const float* natural, const float* record, const float* g_raw, float* grad_record, int arithmetic,
                                 nvsr_stream_t stream);
/* grad_natural [NVSR_MIP_NERF_NATURAL_FLOATS] = sum over the P points of every layer's G^T X and G (overwritten, not accumulated).
 * Exact-f32 products, partial sums per slab of points in workspace [nvsr_mip_nerf_wgrad_workspace_floats(P)] added in a fixed order:
 * no float atomics, the same inputs give the same bits. */
int64_t nvsr_mip_nerf_wgrad_workspace_floats(int64_t P);
int nvsr_mip_nerf_weight_grad(int64_t P, const float* record, const float* grad_record, float* workspace, float* grad_natural, nvsr_stream_t stream);

/* ---- the positional-encoding NeRF baseline (MipNeRF_baseline.yml with encode_position_fn: positional_encoding; csrc/pe.hip) ------------
 * FlexibleNeRFModel(num_encoding_fn_xyz=6, num_encoding_fn_dir=4, include_input_xyz=True, include_input_dir=True) with the constructor
 * defaults (train_nerf.py:338-348): the Mip-NeRF model above with layer1 39->128.  Same natural order, the same layer engine (csrc/nerf_mlp.h).
 * rays [N,11] (nvsr_pack_rays), z [N,S] (the S sample depths of each ray); arithmetic (F16X2 and INHERIT included) as for the Mip-NeRF baseline. */
#define NVSR_PE_NERF_NATURAL_FLOATS 81476
#define NVSR_PE_NERF_RECORD_FLOATS 770         /* per point: [enc 39 | dir 27 | h1 | h2 | h3 | h4 | feat (128 each) | hd 64] */
#define NVSR_PE_NERF_GRAD_RECORD_FLOATS 708    /* per point: pre-activation gradients, the layout of NVSR_MIP_NERF_GRAD_RECORD_FLOATS */
/* pts = ro + rd z (train_utils.py:111,156; two f32 roundings) -> positional_encoding(pts, 6, True) and positional_encoding(viewdir, 4, True)
 * (nerf_helpers.py:552-575): out [N*S, 66] = [x | sin(2^0 x) | cos(2^0 x) | .. | sin(2^5 x) | cos(2^5 x) (3 columns each) | 27 direction columns] */
int nvsr_pe_encode(int64_t N, int S, const float* rays, const float* z, float* out, nvsr_stream_t stream);
/* run_network + FlexibleNeRFModel.forward (train_utils.py:15-64 with mip_nerf=False, models.py:83-108): encoding + model on one 32-point
 * tile per wave, the encoded rows never leave the chip -> raw [N,S,4] (16-byte aligned);
 * record [N*S, NVSR_PE_NERF_RECORD_FLOATS] or NULL: every layer input and ReLU output, for the backward */
int nvsr_pe_nerf_forward_arith(int64_t N, int S, const float* rays, const float* z, const float* natural, float* raw, float* record, int arithmetic,
                               nvsr_stream_t stream);
/* the backward of FlexibleNeRFModel.forward (models.py:83-108): g_raw [P,4] -> grad_record [P, NVSR_PE_NERF_GRAD_RECORD_FLOATS] */
int nvsr_pe_nerf_backward_arith(int64_t P, const float* natural, const float* record, const float* g_raw, float* grad_record, int arithmetic,
                                nvsr_stream_t stream);
/* the nn.Linear weight and bias gradients of FlexibleNeRFModel (models.py:14-108): grad_natural [NVSR_PE_NERF_NATURAL_FLOATS] (overwritten),
 * fixed-order sums over slabs of points in workspace [nvsr_pe_nerf_wgrad_workspace_floats(P)]: no float atomics, the same inputs give the
 * same bits. */
int64_t nvsr_pe_nerf_wgrad_workspace_floats(int64_t P);
int nvsr_pe_nerf_weight_grad(int64_t P, const float* record, const float* grad_record, float* workspace, float* grad_natural, nvsr_stream_t stream);

/* ---- training: gradient with respect to the feature planes -------------------------------------------------------------
 * The reference differentiates run_one_iter_of_nerf with torch.autograd (train_nerf.py:860-903); with the decoder frozen
 * (Feature_Planes_Only.yml) the leaves are the planes.  z_samples carry no gradient (`.detach()`, train_utils.py:153). */
/* nvsr_render_pass that also returns the decoder outputs raw [N,S,4] (needed by nvsr_composite_backward); raw_out may be NULL */
int nvsr_render_pass_ex(const nvsr_scene* scene, const float* packed_decoder, int64_t N, int S, const float* rays, const float* z,
                        const float* noise, int white_bkgd, float* rgb, float* disp, float* acc, float* weights, float* depth,
                        float* raw_out, nvsr_stream_t stream);
/* transposed decoder layers in MFMA-fragment order (NVSR_DECODER_PACKED_BWD_FLOATS floats) from the natural blob */
int nvsr_pack_decoder_bwd(const float* natural, float* packed_bwd, nvsr_stream_t stream);
/* backward of volume_render_radiance_field (volume_rendering_utils.py:18-49): g_rgb [N,3], g_acc [N] or NULL -> g_raw [N,S,4]; S <= 512 */
int nvsr_composite_backward(int64_t N, int S, const float* raw, const float* z, const float* rd, const float* noise, int white_bkgd,
                            const float* g_rgb, const float* g_acc, float* g_raw, nvsr_stream_t stream);
/* the same with the gradient of depth_map (volume_rendering_utils.py:42-43: depth_map = sum_s w_s z_s; mip_nerf: z [N,S+1], z_s = interval
 * midpoints) as a third incoming gradient, g_depth [N] or NULL.  disp_map = 1 / max(1e-10, depth_map / acc_map) (:46) is a function of
 * depth_map and acc_map: its gradient is folded into g_depth / g_acc by the caller (ops.py `composite` does). */
int nvsr_composite_backward_depth(int64_t N, int S, const float* raw, const float* z, const float* rd, const float* noise, int white_bkgd,
                                  const float* g_rgb, const float* g_acc, const float* g_depth, int mip_nerf, float* g_raw, nvsr_stream_t stream);
/* nvsr_composite_backward_depth with the ray directions read out of packed rays [N,11] (columns 3..5 of nvsr_pack_rays' rows, what
 * nvsr_composite_rays reads in the forward): a training step's backward needs no [N,3] copy of them */
int nvsr_composite_backward_rays(int64_t N, int S, const float* raw, const float* z, const float* rays, const float* noise, int white_bkgd,
                                 const float* g_rgb, const float* g_acc, const float* g_depth, int mip_nerf, float* g_raw, nvsr_stream_t stream);
/* the same for nvsr_composite_mip (z [N,S+1]) */
int nvsr_composite_backward_mip(int64_t N, int S, const float* raw, const float* z, const float* rd, const float* noise, int white_bkgd,
                                const float* g_rgb, const float* g_acc, float* g_raw, nvsr_stream_t stream);
/* backward of one decode pass: g_raw [N,S,4] -> grad_planes[4] (host array of 4 device pointers, CHANNEL-LAST like the scene's
 * planes, accumulated with float atomics: zero them first) */
int nvsr_render_pass_backward(const nvsr_scene* scene, const float* packed_decoder, const float* packed_bwd, int64_t N, int S,
                              const float* rays, const float* z, const float* g_raw, float* const* grad_planes, nvsr_stream_t stream);

/* Faster path when the decoder is frozen: the training forward publishes every layer's ReLU gate (gates: N*S*32 uint32, 128 B
 * per point) and the backward runs the transposed layers only, without recomputing the forward. */
int nvsr_decode_rays_ex(const nvsr_scene* scene, const float* packed_decoder, int64_t N, int S, const float* rays, const float* z,
                        float* raw, uint32_t* gates /* or NULL */, float* record /* or NULL; needs gates */, nvsr_stream_t stream);
int nvsr_render_pass_backward_gates(const nvsr_scene* scene, const float* packed_decoder, const float* packed_bwd, int64_t N, int S,
                                    const float* rays, const float* z, const float* g_raw, const uint32_t* gates, float* const* grad_planes,
                                    float* view_ws /* or NULL, see below */, float* record /* or NULL */, nvsr_stream_t stream);

/* ---- training: gradient with respect to the decoder parameters ('decoder' in nerf.train.what, train_nerf.py:75-77) ------
 * torch.autograd's addmm backward (dW = delta^T @ input, db = sum delta) through models.py:169-195,395-421 becomes two calls:
 * the backward pass additionally RECORDS every layer's input and pre-activation gradient, then one contraction over all points
 * adds the weight / bias gradients into a blob in the natural (state-dict) order of nvsr_pack_decoder. */
/* floats of the record workspace of one pass (9.2 KB per point, one row per point: row = ray * S + s; every array of the record is allocated
 * for N * S rows rounded up to 8 + 32 DUMP rows -- round 6: the limb kernels write a tile's 32 rows as whole cache lines through an LDS stage and
 * send the padding points of a partial tile there; rows >= N * S are never read).  The half that the forward
 * layers produce (layer inputs) is written either by nvsr_decode_rays_ex(record) at forward time or by the recomputing
 * nvsr_render_pass_backward_ex(record); the gradient half by whichever backward entry receives the record. */
int64_t nvsr_decoder_record_floats(int64_t N, int S);
/* nvsr_render_pass_backward with optional outputs: grad_planes may be NULL (planes frozen) or hold NULL entries (that plane
 * frozen); record may be NULL (decoder frozen) or a workspace of nvsr_decoder_record_floats(N, S) floats, fully overwritten */
int nvsr_render_pass_backward_ex(const nvsr_scene* scene, const float* packed_decoder, const float* packed_bwd, int64_t N, int S,
                                 const float* rays, const float* z, const float* g_raw, float* const* grad_planes, float* record,
                                 float* view_ws, nvsr_stream_t stream);
/* view_ws (optional, nvsr_view_grad_workspace_floats(N, S) = N*S*48 floats): all samples of a ray hit the same 4 texels of the small
 * view-direction plane; with the workspace their gradients are first written as plain rows and summed per ray, and only N*4*48
 * atomics reach the plane (without it: N*S*4*48 atomics on 1 024 texels -- correct but 2x slower overall). */
int64_t nvsr_view_grad_workspace_floats(int64_t N, int S);
/* grad_natural [NVSR_DECODER_NATURAL_FLOATS] += gradient of this pass (float atomics: zero it before the first pass) */
int nvsr_decoder_weight_grad(int64_t N, int S, const float* record, float* grad_natural, nvsr_stream_t stream);

/* ---- training: the deterministic route (opt-in) -----------------------------------------------------------
 * The entries above add plane and decoder-weight gradients with float atomics: two runs from the same state differ in their last
 * bits.  The entries below compute the same gradients in a fixed order, for the limb arithmetics (NVSR_ARITH_BF16X3 / _F16X2; an
 * arithmetic that resolves to NVSR_ARITH_F32 is answered with NVSR_ERR_SHAPE).  None of them allocates, creates a stream or
 * synchronises; what they need comes out of the caller's workspaces.
 *
 * nvsr_render_pass_backward_rows_arith: nvsr_render_pass_backward_gates_arith with the plane scatter replaced by plain stores.
 *   rows: 3 pointers or NULL; rows[d] (or NULL: plane d is frozen, nothing is written) receives the feature gradient of every point
 *   with respect to position plane d as rows[d][ray * S + s][48] -- whole 192-byte rows, no atomics, no plane is touched.
 *   view_ws (or NULL: the view plane is frozen): nvsr_view_grad_workspace_floats(N, S) floats; receives one pre-summed row per
 *   (ray, 32-sample chunk) as in the atomic route; nvsr_view_rows_reduce adds a ray's (S + 31) / 32 rows in ascending chunk order into
 *   view_rows[ray][48].  record: as in nvsr_render_pass_backward_gates_arith.  At least one of rows, view_ws, record is given.
 *
 * nvsr_internal_plane_taps: texel[M][4] (int32, iy * W + ix) and weight[M][4] of the bilinear taps, in the order nw, ne, sw, se, formed
 *   by the backward kernel's own tap functions; d in 0..2: M = N * S, one entry per point (m = ray * S + s); d == 3 (view plane, z may be
 *   NULL): M = N, one entry per ray.  A neighbour clamped at the border names the border texel and carries weight 0, as in the kernels.
 *
 * nvsr_rows_scatter: rows[M][48], texel[M][4], weight[M][4] -> g[H * W][48] (a channel-last gradient plane), exactly:
 *     entry e = 4 m + j belongs to texel texel[e];
 *     for every texel t that at least one entry names, and every channel c:
 *         s = +0.0f;  for that texel's entries in ascending e:  s = __fadd_rn(s, __fmul_rn(rows[m][c], weight[e]));
 *         g[t][c] = __fadd_rn(g[t][c], s);
 *     every entry takes part, weight 0 included (a NaN row reaches exactly its four texels); a texel no entry names is not written.
 *   Texel numbers outside [0, H * W) are never written to.  workspace: nvsr_rows_scatter_workspace_bytes(M) bytes, 16-byte aligned
 *   (sorted keys, sorted entry numbers and the temporary storage of the stable radix sort); its contents need not be initialised.
 *   The cost is linear in M, also when every entry names the same texel.
 *
 * nvsr_decoder_weight_grad_det_arith: nvsr_decoder_weight_grad_arith's limb contractions with every slab of rows writing its block into a
 *   partial blob of its own (workspace: nvsr_decoder_weight_grad_det_workspace_floats(N, S) floats, contents need not be initialised); a
 *   reduce kernel adds the slabs in ascending order and adds the sum into grad_natural.  The slab boundaries depend on N * S alone. */
int nvsr_render_pass_backward_rows_arith(const nvsr_scene* scene, const float* packed_decoder, const float* packed_bwd, int64_t N, int S,
                                         const float* rays, const float* z, const float* g_raw, const uint32_t* gates, float* const* rows,
                                         float* view_ws, float* record, int arithmetic, nvsr_stream_t stream);
int nvsr_view_rows_reduce(int64_t N, int S, const float* view_ws, float* view_rows, nvsr_stream_t stream);
int nvsr_internal_plane_taps(const nvsr_scene* scene, int d, int64_t N, int S, const float* rays, const float* z, int32_t* texel, float* weight,
                             nvsr_stream_t stream);
int64_t nvsr_rows_scatter_workspace_bytes(int64_t M);
int nvsr_rows_scatter(int64_t M, const float* rows, const int32_t* texel, const float* weight, int H, int W, float* g, void* workspace,
                      int64_t workspace_bytes, nvsr_stream_t stream);
int64_t nvsr_decoder_weight_grad_det_workspace_floats(int64_t N, int S);
int nvsr_decoder_weight_grad_det_arith(int64_t N, int S, const float* record, float* grad_natural, float* workspace, int arithmetic,
                                       nvsr_stream_t stream);

/* ---- input gradients: sample positions and view directions (csrc/points_grad.hip) ---------------------------
 * The last link behind the ROWS backward: rows[d][m][48] = dL/d(feature of position plane d) of point m = ray * S + s (what
 * nvsr_render_pass_backward_rows_arith leaves) and view_rows[ray][48] (nvsr_view_rows_reduce) -> d_points[m][3] = dL/d(o + z d) and
 * d_viewdir[ray][3] = dL/d(rays[ray][8..10]).  The positions' derivative is the TRUE one: the reference projects under torch.no_grad()
 * and returns 0 there (an extension, like the occupancy grids); the view half is the reference's.
 *   rows: 3 pointers or NULL; rows[d] == NULL: plane d adds nothing.  view_rows NULL: d_viewdir is 0.  d_points / d_viewdir: either may
 *   be NULL (not computed); both are OVERWRITTEN.  rows[d] and view_rows are 16-byte aligned.  z is needed for d_points only.
 *   Status: NVSR_ERR_NULL (scene, a plane of it, rays; z with d_points), NVSR_ERR_ALIGN, NVSR_ERR_SHAPE (N < 0, S < 1, S > 4096,
 *   N * S >= 2^29), NVSR_OK with nothing launched for N == 0 or no output.  Never allocates, never synchronises, no atomics.
 * Exactly, every operation one correctly rounded float operation (a b: __fmul_rn, +: __fadd_rn, /: __fdiv_rn), left to right:
 *   slope(d, gx, gy, row) -> (Gx, Gy), W x H the plane, hx = (W - 1) / 2, hy = (H - 1) / 2:
 *     x = (gx + 1) hx, y = (gy + 1) hy;  xc = min(W - 1, max(x, 0)), yc likewise (max(NaN, 0) = 0);
 *     w = xc - floor(xc), e = 1 - w, n = yc - floor(yc), s = 1 - n;  the texels T00 = (floor yc, floor xc), T01 = its east, T10 = its south,
 *     T11 neighbour, a neighbour beyond the border clamped onto it: the forward's cell (an integer coordinate takes the cell floor selects);
 *     per channel c:  dx_c = s (T01 - T00)_c + n (T11 - T10)_c,   dy_c = e (T10 - T00)_c + w (T11 - T01)_c;
 *     12 partial sums over 4 channels each, l = 0..11:  a_l = ((row[4l] dx_4l + row[4l+1] dx_4l+1) + row[4l+2] dx_4l+2) + row[4l+3] dx_4l+3;
 *     a_12..15 = +0;  A = a balanced tree over neighbours: b_i = a_2i + a_2i+1, c_i = b_2i + b_2i+1, d_i = c_2i + c_2i+1, A = d_0 + d_1;
 *     Gx = 0 if x <= 0 or x >= W - 1, else hx A;   Gy likewise from dy with y, H - 1, hy   (torch's clip_coordinates_set_grad).
 *   d_points: p_k = o_k + d_k z (as the kernels form it), n_k = (2 (p_k - lo_k)) / range_k - 1; per plane d, M = proj[d] (3 x 2):
 *     gx = (n_0 M[0][0] + n_1 M[1][0]) + n_2 M[2][0], gy with column 1 (ray_pos_taps);  (Gx, Gy) = slope(d, gx, gy, rows[d][m]);
 *     dn_k = +0;  for d = 0, 1, 2 with rows[d] != NULL:  dn_k = dn_k + (M[k][0] Gx + M[k][1] Gy);     d_points[m][k] = (2 dn_k) / range_k.
 *     A NaN among p_0..2 makes all three components NaN; no other row changes (its taps are in range: max(NaN, 0) = 0).
 *   d_viewdir: q = vx vx + vy vy, r = sqrt(q), az = atan2f(vy, vx), el = atan2f(vz, r) (view_taps);
 *     (Gx, Gy) = slope(3, (2 (az - lo_3)) / range_3 - 1, (2 (el - lo_4)) / range_4 - 1, view_rows[ray]);
 *     d_az = (2 Gx) / range_3, d_el = (2 Gy) / range_4;  h = q + vz vz;  a = d_az / q, b = d_el / h, c = (b vz) / r;
 *     d_viewdir[ray] = ((-vy) a - vx c,  vx a - vy c,  r b).   A NaN component makes the row NaN.  At a pole (vx = vy = 0) the result is
 *     unspecified (torch's is not finite either). */
int nvsr_triplane_points_grad(const nvsr_scene* scene, int64_t N, int S, const float* rays, const float* z, const float* const* rows,
                              const float* view_rows, float* d_points, float* d_viewdir, nvsr_stream_t stream);

/* ---- surface normals of a rendered view (csrc/normals.hip) ------------------------------------------------------
 * The density gradient on the LIVE samples of a pass only, composited per ray with the compositor's weights: normal[ray] = sum_s w_s n_s,
 * n_s = -g_s / |g_s|, g_s = d sigma_raw / d p at p_s = o + z_s d.  A sample with w != 0 has sigma > 0, so relu' = 1 there and g is the
 * gradient of sigma.  The sum is NOT renormalised: its length is at most about acc, background pixels go to 0; callers normalise if they want
 * unit vectors.  The normals live in the coordinate system of the rays passed in (NDC space for an NDC scene).
 * The route around the two entries (ops.normals_of_pass): nvsr_generic_live_list on weights [N,S] -> index (ascending) and its count;
 * nvsr_live_ray_points; nvsr_decode_rays_arith with gates on the M one-sample rays; nvsr_render_pass_backward_rows_arith with
 * g_raw = (0, 0, 0, 1) for the three position planes (no view workspace, no record); nvsr_normals_composite.
 * Neither entry allocates, synchronises or uses atomics.  Status of both: NVSR_ERR_SHAPE (N < 0, M < 0, S < 1, S > 4096, N * S >= 2^31;
 * M >= 2^31 for the points, M >= 2^29 for the compositor), then NVSR_OK with nothing launched for M == 0 or N == 0, then NVSR_ERR_NULL (any
 * pointer; the scene and its planes are checked first by the compositor), NVSR_ERR_ALIGN (rows[d] not 16-byte aligned).
 *
 * nvsr_live_ray_points: for list entry i < M with p = index[i], ray = p / S (s = p % S):
 *   live_rays[i] = [o_k + d_k z[p] (k = 0..2; one __fmul_rn, one __fadd_rn: nvsr_ray_points' position), 0, 0, 0, 0, 0, rays[ray][8..10]]
 *   -- the one-sample ray (direction 0, near = far = 0; depth 0 is the caller's z) that TwoDimPlanesModel.density_gradient builds per point.
 *   An index outside [0, N * S) is skipped: its row is not written.
 *
 * nvsr_normals_composite: index [M] ASCENDING (int32; entries outside [0, N * S) belong to no ray), live_rays [M,11] (what
 *   nvsr_live_ray_points wrote for the same M entries), rows: 3 pointers, rows[d] [M][48] = d sigma_raw / d (feature of position plane d) of
 *   entry i (16-byte aligned, all three required), weights [N,S], normal [N,3]: ACCUMULATED INTO.
 *   Per ray, its run = the entries i with ray S <= index[i] < (ray + 1) S (two binary searches), in ascending i:
 *     g = d_points of nvsr_triplane_points_grad above for the point p = live_rays[i][0..2] and the rows rows[d][i]: the same slope, the same
 *         order, the same NaN rule (the kernels share the device functions, csrc/points_grad_core.h);
 *     q = (g_0 g_0 + g_1 g_1) + g_2 g_2,  r = sqrt(q);   n_k = +0 if q == 0, else -(g_k / r);   w = weights[index[i]];
 *     normal[ray][k] = normal[ray][k] + w n_k                        (one __fmul_rn, one __fadd_rn; a ray with an empty run is not touched)
 *   Every operation is one correctly rounded float operation; NaN propagates: a NaN weight or gradient reaches its own ray and no other.
 *   The fold is sequential and in place: cutting the live list into slabs at ANY position, mid-ray included -- index, live_rays and the rows
 *   of entries [a, b) with the whole weights and normal -- and launching the slabs in ascending order on one stream gives the bits of one
 *   launch over the whole list.
 *   Roundings on the longest path of one term: g 18 (above), q: 2 g's relative error + 1 + 2 = 3 more on q, halved by the square root, + 1;
 *   g_k / r: + 1; w n_k: + 1; one per addition of the fold (tests/normals_ref.py derives the bound the tests apply). */
int nvsr_live_ray_points(int64_t N, int S, int64_t M, const int32_t* index, const float* rays, const float* z, float* live_rays,
                         nvsr_stream_t stream);
int nvsr_normals_composite(const nvsr_scene* scene, int64_t N, int S, int64_t M, const int32_t* index, const float* live_rays,
                           const float* const* rows, const float* weights, float* normal, nvsr_stream_t stream);

/* ---- ray and camera-pose gradients of a training render (csrc/ray_grad.hip) ----------------------------------
 * What consumes d_points / d_viewdir: the packed rays' gradient, then the adjoints of nvsr_pack_rays, nvsr_ndc_rays and
 * nvsr_get_ray_bundle[_at] down to the camera-to-world matrix.  None of these entries allocates, synchronises or uses atomics; each sum has
 * the fixed order stated below, every operation is one correctly rounded float operation (a b: __fmul_rn, + -: __fadd_rn / __fsub_rn,
 * /: __fdiv_rn), never contracted into an FMA, so the same inputs give the same bits.  N == 0: NVSR_OK with nothing launched.
 * "tree(x)" below is a sum over the 64 lanes of a wave as a balanced tree over neighbouring lanes:
 *   b_i = x_2i + x_2i+1, c_i = b_2i + b_2i+1, ... six levels down to one value.
 *
 * nvsr_rays_grad: one pass of one render -> d_rays [N,11] = d loss / d rays.  rays [N,11], z [N,S], d_points [N*S,3] or NULL (adds
 *   nothing), d_viewdir [N,3] or NULL (adds nothing), raw [N,S,4] (the pass's decoder output), noise [N,S] or NULL (the density noise the
 *   compositor added), g_raw [N,S,4] (d loss / d raw, what nvsr_composite_backward_rays returned).  Per ray, lane l = 0..63 of its wave:
 *     A_k[l] = +0;  for s = l, l + 64, ... < S ascending:  A_k[l] = A_k[l] + d_points[s][k]            (k = 0..2; p = o + z d, z a constant
 *     B_k[l] = +0;  likewise                                B_k[l] = B_k[l] + z[s] d_points[s][k]        of the backward: the coarse depths depend
 *     T[l]   = +0;  likewise  sn = raw[s][3] + noise[s] (raw[s][3] without noise), sigma = sn < 0 ? 0 : sn,     on near / far only, the fine
 *                             T[l] = T[l] + g_raw[s][3] sigma                                                    depths are detached)
 *     d_rays[0..2] = tree(A_k);   rr = (rd_0 rd_0 + rd_1 rd_1) + rd_2 rd_2,  rd = rays[3..5];
 *     d_rays[3 + k] = tree(B_k) + (tree(T) rd_k) / rr:  the compositor reads sigma and |rd| through their product sigma dist |rd| only, so
 *                     d loss / d|rd| = sum_s sigma_s (d loss / d sigma_s) / |rd|  (nvsr_composite_backward_rays is unchanged and still
 *                     treats |rd| as a constant; this is its missing term);
 *     d_rays[6..7] = +0: near and far are constants of the scene, never differentiated;   d_rays[8..10] = d_viewdir.
 *   accumulate != 0: columns 0..5 and 8..10 are ADDED onto what d_rays holds (one more rounding: old + value; the coarse pass writes, the
 *   fine pass adds); columns 6..7 are written +0 either way.  A NaN among rays[0..5], rays[8..10] of a ray makes its columns 0..5 and 8..10
 *   NaN; no other row changes.  A NaN density stays a NaN (the compositor's relu).
 *   Roundings on the longest path, n = ceil(S / 64): columns 0..2: n + 6;  columns 3..5: the larger of (1 + n + 6) for B and
 *   (2 + n + 6) + 1 + 3 + 1 for the T term (noise add, product, lane sum, tree; times rd_k; rr; the division), + 1 for the last addition:
 *   n + 14;  + 1 each with accumulate.
 *   Status: NVSR_ERR_NULL (rays, raw, g_raw, d_rays; z with d_points), NVSR_ERR_SHAPE (N < 0, S < 1, S > 4096, N * S >= 2^29).
 *
 * nvsr_pack_rays_backward: adjoint of nvsr_pack_rays.  d_rays [N,11], view_src [N,3] (the forward's) -> d_ro [N,3] = d_rays[0..2],
 *   d_rd [N,3] = d_rays[3..5], and the chain through viewdir = v / |v|:  n = sqrt((v_0 v_0 + v_1 v_1) + v_2 v_2), u_k = v_k / n (the
 *   forward's), dot = (u_0 g_8 + u_1 g_9) + u_2 g_10, c_k = (g_(8+k) - u_k dot) / n.  view_is_rd != 0 (the view source IS the direction
 *   tensor): d_rd[k] = d_rays[3 + k] + c_k and d_view_src is not touched; otherwise d_view_src [N,3] (or NULL) = c.  Columns 6..7 are ignored.
 *   Roundings (relative errors add under a product or a quotient, + 1 for its own rounding; a square root halves its operand's):
 *   n: 3 / 2 + 1 = 2.5, u_k: 3.5, dot: 4.5 + 2 = 6.5, u_k dot: 11, g - .: 12, / n: 15.5: c_k lies within 16 2^-24 (|g_(8+k)| + |u_k| sum_j |u_j g_(8+j)|) / n
 *   of the exact value; d_rd with view_is_rd: 17, |d_rays[3 + k]| joining the terms.
 *   Status: NVSR_ERR_NULL (d_rays, view_src, d_ro, d_rd), NVSR_ERR_SHAPE (N < 0, N >= 2^31).
 *
 * nvsr_ndc_rays_backward: adjoint of nvsr_ndc_rays with respect to ro and rd (the focal length and near are constants).  With the forward's
 *   t = (-(near + o_2)) / d_2, ox = o_0 + t d_0, oy, oz likewise, sx, sy as the forward forms them, go = d_ro_out, gd = d_rd_out:
 *     h_0 = sx (go_0 - gd_0), h_1 = sy (go_1 - gd_1), h_2 = (2 near) (go_2 - gd_2);   g_ox = h_0 / oz, g_oy = h_1 / oz,
 *     g_oz = -(((ox h_0 + oy h_1) + h_2) / (oz oz));   k_0 = sx gd_0, k_1 = sy gd_1;   g_t = (g_ox d_0 + g_oy d_1) + g_oz d_2,  q = g_t / d_2;
 *     d_ro = (g_ox, g_oy, g_oz - q);   d_rd_0 = k_0 / d_2 + t g_ox,  d_rd_1 = k_1 / d_2 + t g_oy,
 *     d_rd_2 = (t g_oz - (k_0 d_0 + k_1 d_1) / (d_2 d_2)) - t q.
 *   Roundings: oz is a cancelling sum (its exact value is -near) that divides, twice in g_oz: its relative error is <= 4 kappa 2^-24 with
 *   kappa = (|o_2| + |t d_2|) / |oz| >= 1 per ray, not a few roundings.  With A the same expressions on absolute values (every difference a
 *   sum, t taken as (|near| + |o_2|) / |d_2|, the divisor |oz| exact) each component lies within (20 + 8 kappa) 2^-24 A of the exact value:
 *   19 roundings on the longest path (d_rd_2: ox 4, ox h_0 7, the numerator 9, / (oz oz) 11, g_oz d_2 12, g_t 14, q 15, t q 18, the last
 *   difference 19), one of slack for the second-order terms, 8 kappa for the two divisions by oz.
 *   Status: NVSR_ERR_NULL (any pointer), NVSR_ERR_SHAPE (N < 0, N >= 2^31, H < 1, W < 1).
 *
 * nvsr_ray_bundle_backward: adjoint of nvsr_get_ray_bundle_at (row_col [N,2]) or, row_col NULL, of nvsr_get_ray_bundle's padded grid
 *   (N == (H + 2 padding)(W + 2 padding), ray i = pixel (i / Wp, i % Wp); padding is ignored with row_col) -> d_c2w [16], row-major 4 x 4:
 *   with dir exactly as the forward forms it,  d_c2w[k][j] = sum_rays d_rd[ray][k] dir_j (j < 3),  d_c2w[k][3] = sum_rays d_ro[ray][k],
 *   row 3 = +0.  The focal lengths stay constants: their gradient is out of scope (in NDC scenes the focal length also enters the warp, and
 *   half a gradient would mislead).
 *   Two stages over `workspace` (nvsr_ray_bundle_backward_workspace_floats(N) floats, contents need not be initialised): slab w = rays
 *   [256 w, 256 w + 256), a ray beyond N contributing +0; per entry the slab's 4 waves each form tree(x), x_l the entry's term of ray
 *   256 w + 64 wave + l, and partials[w] = (t_0 + t_1) + (t_2 + t_3); then ONE wave: lane l adds partials[l], partials[l + 64], ... in
 *   ascending order from +0, and d_c2w's entry is the tree over the lanes.  The slab boundaries depend on N alone.
 *   Roundings on the longest path: 2 (dir_j: a difference, a quotient) + 1 (product) + 6 + 2 + ceil(slabs / 64) + 6 = 17 + ceil(slabs / 64).
 *   Status: NVSR_ERR_NULL (d_ro, d_rd, d_c2w; workspace with N > 0), NVSR_ERR_ALIGN (d_c2w not 16-byte aligned), NVSR_ERR_SHAPE (H, W < 1,
 *   N < 0, N >= 2^31, padding < 0, a full grid whose N is not the padded grid's size). */
int nvsr_rays_grad(int64_t N, int S, const float* rays, const float* z, const float* d_points, const float* d_viewdir, const float* raw,
                   const float* noise, const float* g_raw, int accumulate, float* d_rays, nvsr_stream_t stream);
int nvsr_pack_rays_backward(int64_t N, const float* d_rays, const float* view_src, int view_is_rd, float* d_ro, float* d_rd, float* d_view_src,
                            nvsr_stream_t stream);
int nvsr_ndc_rays_backward(int H, int W, double focal, double near_, int64_t N, const float* ro, const float* rd, const float* d_ro_out,
                           const float* d_rd_out, float* d_ro, float* d_rd, nvsr_stream_t stream);
int64_t nvsr_ray_bundle_backward_workspace_floats(int64_t N);
int nvsr_ray_bundle_backward(int H, int W, double focal_x, double focal_y, double offset, int64_t N, const int32_t* row_col, int padding,
                             const float* d_ro, const float* d_rd, float* d_c2w, float* workspace, nvsr_stream_t stream);


/* ---- training: gradients of the super-resolution CNN ('SR' in nerf.train.what) -------------------------------------------
 * torch.autograd through EDSR.forward (models.py:818-822), _Residual_Block.forward (:777-786), PlanesSR.forward (:884-926). */
/* weights [Cout][Cin][3][3] -> fragments of the conv's data gradient (nvsr_conv3x3_packed_floats(Cout, Cin) floats) */
int nvsr_pack_conv3x3_dgrad(const float* w, int Cin, int Cout, float* packed_dgrad, nvsr_stream_t stream);
/* data gradient of nvsr_conv3x3 (epilogue 0): dy [Cout][H-2][W-2] -> dx [Cin][H][W] */
int nvsr_conv3x3_dgrad(const float* dy, int Cin, int H, int W, const float* packed_dgrad, int Cout, float* dx, nvsr_stream_t stream);
/* weight gradient: dw [Cout][Cin][3][3] += scale * sum_{y,x} dy[co][y][x] * x[ci][y+ky][x+kx];  x [Cin][H][W], dy [Cout][H-2][W-2];
 * deterministic (fixed-order reduction of per-row-slab partial sums held in the workspace) */
int64_t nvsr_conv3x3_wgrad_workspace_floats(int Cin, int H, int W, int Cout);
int nvsr_conv3x3_wgrad(const float* dy, const float* x, int Cin, int H, int W, int Cout, float scale, float* dw, float* workspace,
                       nvsr_stream_t stream);
/* EDSR forward that keeps every layer's input in `acts` (nvsr_edsr_acts_floats floats) for nvsr_edsr_backward */
int64_t nvsr_edsr_acts_floats(int Cin, int Cout, int hid, int nblocks, int n_up, int H, int W);
int nvsr_edsr_forward_train(const float* x, int Cin, int H, int W, const float* packed, int Cout, int hid, int nblocks, int n_up, float* out,
                            float* acts, nvsr_stream_t stream);
int64_t nvsr_edsr_packed_dgrad_floats(int Cin, int Cout, int hid, int nblocks, int n_up);
int nvsr_pack_edsr_dgrad(const float* natural, int Cin, int Cout, int hid, int nblocks, int n_up, float* packed_dgrad, nvsr_stream_t stream);
int nvsr_pack_edsr_dgrad_arith(const float* natural, int Cin, int Cout, int hid, int nblocks, int n_up, float* packed_dgrad, int arithmetic,
                               nvsr_stream_t stream);      /* (see nvsr_pack_edsr_arith) */
int64_t nvsr_edsr_backward_workspace_floats(int Cin, int Cout, int hid, int nblocks, int n_up, int H, int W);
/* d_out [Cout][Ho][Wo] -> grad_natural (state-dict order) += weight gradients, dx [Cin][H][W] (or NULL) = input gradient.
 * Streams: everything the call enqueues is ordered on `stream`, and the library creates no stream of its own.  (A build with -DWG_REDUCE_LANE=1
 * runs the per-layer reductions of the weight gradients' partial sums on a library-owned side stream that `stream` waits for before the call
 * returns; measured and switched off: one more hardware queue in a process that already uses four costs more than the overlap gains, sr_bwd.hip.)
 * The same holds for nvsr_planes_sr_backward and nvsr_planes_sr_backward_batch_arith. */
int nvsr_edsr_backward(const float* x, int Cin, int H, int W, const float* acts, const float* packed_dgrad, int Cout, int hid, int nblocks,
                       int n_up, const float* d_out, float* grad_natural, float* dx, float* workspace, nvsr_stream_t stream);
/* PlanesSR: forward that keeps the prepared input + activation record, and its backward.  d_lr (or NULL: LR plane detached,
 * models.py:272) += gradient of the LR plane through the network input and the bilinear residual. */
int64_t nvsr_planes_sr_keep_floats(int C, int R0, int R1, int hid, int nblocks, int n_up, int pad, const float* roi);
int nvsr_planes_sr_train(const float* lr, int C, int R0, int R1, const float* packed, int hid, int nblocks, int n_up, int pad, int over,
                         const float* roi, const float* mean, const float* stdv, float* out, float* workspace, float* keep,
                         nvsr_stream_t stream);
int64_t nvsr_planes_sr_backward_workspace_floats(int C, int R0, int R1, int hid, int nblocks, int n_up, int pad, const float* roi);
int nvsr_planes_sr_backward(int C, int R0, int R1, const float* keep, const float* packed_dgrad, int hid, int nblocks, int n_up, int pad,
                            int over, const float* roi, const float* stdv, const float* d_out, float* grad_natural, float* d_lr,
                            float* workspace, nvsr_stream_t stream);

/* ---- decoder geometries other than the shipped one (inference) --------------------------------------------------------------------
 * TwoDimPlanesModel (models.py:118-434) is configurable: dec_channels, layer counts, skip_connect_every, num_plane_channels,
 * proj_combination, viewdir_proj_combination (config/TrainModels.yml:78,82,92 list alternatives).  The MFMA kernels above are compiled for
 * the shipped configuration; every other one the reference's own layer sizes admit runs through this generic path (plain kernels,
 * activations through HBM, exact-f32 MFMA layers): forward and backward. */
typedef struct nvsr_decoder_geometry {
    int32_t plane_channels;        /* num_plane_channels */
    int32_t viewdir_channels;      /* num_viewdir_plane_channels */
    int32_t hidden;                /* dec_channels */
    int32_t density_layers;        /* dec_density_layers */
    int32_t rgb_layers;            /* dec_rgb_layers */
    int32_t skip_connect_every;    /* 0 = None (models.py:203-207) */
    int32_t proj_combination;      /* 0 'sum' | 1 'avg' | 2 'concat'                              (models.py:355-361) */
    int32_t viewdir_combination;   /* 0 'sum' | 1 'avg' | 2 'mult' | 3 'concat' | 4 'concat_pos'  (models.py:363-379) */
} nvsr_decoder_geometry;
/* parameters in state-dict order: density_dec.0.{l}.{weight[out,in],bias}, fc_alpha.0.{weight,bias}, rgb_dec.0.{l}.{weight,bias},
 * fc_rgb.0.{weight,bias}; -1 for a geometry whose layer sizes are inconsistent in the reference itself (e.g. 'concat' view features on
 * summed position features) */
int64_t nvsr_generic_decoder_natural_floats(const nvsr_decoder_geometry* geometry);
int64_t nvsr_generic_decode_workspace_floats(const nvsr_decoder_geometry* geometry, int64_t P);
/* TwoDimPlanesModel.forward: x [P,6] = [xyz, viewdir] -> out [P,4].  scene: planes channel-last [H][W][plane_channels] (the view plane:
 * [H][W][viewdir_channels]); natural: the blob above (device). */
int nvsr_generic_decode(const nvsr_scene* scene, const nvsr_decoder_geometry* geometry, const float* natural, int64_t P, const float* x,
                        float* out, float* workspace, nvsr_stream_t stream);
/* Backward of nvsr_generic_decode (the reference: torch.autograd through models.py:381-421): d_out [P,4] -> the gradients of the
 * parameters (d_natural, the blob's layout; NULL = not wanted) and of the four planes (d_plane0..3, channel-last like the planes; NULL =
 * not wanted), all ACCUMULATED into what is there (float atomics: last-bit run-to-run differences, like grid_sampler_2d_backward).
 * The forward is recomputed chunk by chunk with every layer's output kept in the workspace. */
int64_t nvsr_generic_decode_backward_workspace_floats(const nvsr_decoder_geometry* geometry, int64_t P);
int nvsr_generic_decode_backward(const nvsr_scene* scene, const nvsr_decoder_geometry* geometry, const float* natural, int64_t P, const float* x,
                                 const float* d_out, float* d_natural, float* d_plane0, float* d_plane1, float* d_plane2, float* d_plane3,
                                 float* workspace, nvsr_stream_t stream);
/* ---- generic decoder, extended scene (round 4) ------------------------------------------------------------------------------------
 * The options of TwoDimPlanesModel that nvsr_scene cannot express, for the generic kernels only (the MFMA kernels of the shipped
 * geometry keep nvsr_scene):
 *   - any number of position planes with their projections (num_planes_or_rot_mats > 3: models.py:140,471-490 -- CoordProjector draws
 *     random orthonormal frames; grid_d = n_xyz @ rot_mats[d][:, 1:]); combine_pos_planes sums / averages / concatenates all of them;
 *   - grid_sample(align_corners=False) and grid_sample(mode='bicubic') (plane_interp, models.py:303-309,320-326; config/TrainModels.yml:72);
 *   - point_coords_noise (models.py:291-293): `coord_noise` [P,3] (device; NULL = none) is ADDED TO THE NORMALISED sample position
 *     before the projections -- the caller draws it (the reference: torch.normal(0, point_coords_noise * 2 / (1 + plane resolution)) on
 *     the CPU generator, once per model call, training only).
 * planes[0 .. num_position_planes-1] are the position planes, planes[num_position_planes] is the view-direction plane. */
#define NVSR_MAX_POSITION_PLANES 15
typedef struct nvsr_scene_ext {
    int32_t num_position_planes;                          /* 1 .. NVSR_MAX_POSITION_PLANES */
    int32_t align_corners;                                /* grid_sample's align_corners: 1 = True (every shipped config), 0 = False */
    int32_t plane_interp;                                 /* grid_sample's mode: NVSR_PLANE_INTERP_BILINEAR (every shipped config) | _BICUBIC */
    const float* planes[NVSR_MAX_POSITION_PLANES + 1];    /* device, channel-last */
    int32_t ph[NVSR_MAX_POSITION_PLANES + 1], pw[NVSR_MAX_POSITION_PLANES + 1];
    float lo[5], range[5];                                /* as in nvsr_scene */
    float proj[NVSR_MAX_POSITION_PLANES][6];              /* row-major 3x2 per position plane */
} nvsr_scene_ext;
int64_t nvsr_generic_decoder_natural_floats_ext(const nvsr_decoder_geometry* geometry, int num_position_planes);
int64_t nvsr_generic_decode_workspace_floats_ext(const nvsr_decoder_geometry* geometry, int num_position_planes, int64_t P);
int64_t nvsr_generic_decode_backward_workspace_floats_ext(const nvsr_decoder_geometry* geometry, int num_position_planes, int64_t P);
/* nvsr_generic_decode / nvsr_generic_decode_backward on an extended scene; d_planes: num_position_planes + 1 device pointers (host
 * array; NULL array or NULL entries = not wanted), accumulated into like d_plane0..3 */
int nvsr_generic_decode_ext(const nvsr_scene_ext* scene, const nvsr_decoder_geometry* geometry, const float* natural, int64_t P, const float* x,
                            const float* coord_noise, float* out, float* workspace, nvsr_stream_t stream);
int nvsr_generic_decode_backward_ext(const nvsr_scene_ext* scene, const nvsr_decoder_geometry* geometry, const float* natural, int64_t P,
                                     const float* x, const float* coord_noise, const float* d_out, float* d_natural, float* const* d_planes,
                                     float* workspace, nvsr_stream_t stream);
/* ---- generic decoder, fused evaluation ----------------------------------------------------------------------------------------
 * TwoDimPlanesModel.forward (models.py:381-421) of a generic geometry in ONE launch: the input features, every layer of both decoders and
 * both heads; the activations stay in LDS.  The result has the bits of nvsr_generic_decode_ext (the same v_mfma_f32_32x32x2_f32 chains over
 * the same operand pairs in the same order).  Its backward is the plane-gradient launch of "generic decoder, fused plane gradients" below;
 * decoder-weight gradients keep the layered route unless the caller takes nvsr_generic_decode_backward_fused_record_ext (below).
 * Capacity: a point's row in LDS holds the decoder inputs and one hidden activation,
 *   row = Kr (+ Kd where the density decoder's input is not a prefix of the colour decoder's: 'sum' / 'avg' position features under
 *         'concat_pos') + hidden floats, rounded up to 2 x an odd number;
 * supported = hidden <= 256, max(Kd, Kr) <= 512 and 32 rows fit in 160 KB (Kd, Kr: in_features of the decoders' first layers).
 * nvsr_generic_fused_supported (models.py:381-421; host only, no device needed): 1 / 0, or the negated status (-NVSR_ERR_NULL,
 * -NVSR_ERR_SHAPE) for a geometry that nvsr_generic_decoder_natural_floats_ext refuses. */
int nvsr_generic_fused_supported(const nvsr_decoder_geometry* geometry, int num_position_planes);
/* nvsr_generic_decode_ext (models.py:381-421) without a workspace: one launch for any P (pieces of whole point blocks only where the grid
 * limit forces them); NVSR_ERR_SHAPE for a geometry beyond the capacity above; P == 0: NVSR_OK without a launch. */
int nvsr_generic_decode_fused_ext(const nvsr_scene_ext* scene, const nvsr_decoder_geometry* geometry, const float* natural, int64_t P,
                                  const float* x, const float* coord_noise, float* out, nvsr_stream_t stream);
/* ---- generic decoder, fused plane gradients (csrc/generic_fused_bwd.hip) -----------------------------------------------------------------
 * The backward of TwoDimPlanesModel.forward (the reference: torch.autograd through models.py:381-421) of a generic geometry for an iteration
 * in which the decoder's parameters take NO gradient, in ONE launch and exact f32: d_out [P,4] -> the gradients of the planes.  The kernel
 * recomputes the forward in LDS as nvsr_generic_decode_fused_ext does, keeps one gate bit per hidden unit (its output is > 0; NaN and 0 are
 * closed), runs the transposed chain of both decoders and scatters through the combination rule and the taps (bilinear or bicubic, either
 * align_corners, coord_noise).  Up to the scatter every value carries the bits of nvsr_generic_decode_backward_ext: dX[p][k] is one
 * v_mfma_f32_32x32x2_f32 chain from +0.0 over the pairs (2s, 2s + 1) of the output index in ascending order, the gradient of a decoder's
 * input starts at +0.0 and takes, layers descending, a skip layer's part and last layer 0's part with one rounded addition each.  The scatter
 * adds the density decoder's and the colour decoder's product of a (texel, channel) with one rounded addition in front of ONE atomic (the
 * layered route issues two): where no two points share a texel the result is the layered route's bit for bit, elsewhere the two differ by
 * the order of their float atomics only.  The lanes of an atomic instruction run over the channels of one texel.
 * Capacity: a point's row in LDS holds both decoders' inputs apart, one hidden activation, the cotangent and the gate words,
 *   row = Kr + Kd + hidden + 4 + (density_layers + rgb_layers) x ceil(hidden / 32) floats, rounded up to 2 x an odd number;
 * supported = nvsr_generic_fused_supported's limits (hidden <= 256, max(Kd, Kr) <= 512) and 32 such rows fit in 160 KB (row <= 1280).
 * nvsr_generic_backward_fused_supported (models.py:381-421; host only, no device needed): 1 / 0, or the negated status for a geometry that
 * nvsr_generic_decoder_natural_floats_ext refuses; never 1 where nvsr_generic_fused_supported answers 0. */
int nvsr_generic_backward_fused_supported(const nvsr_decoder_geometry* geometry, int num_position_planes);
/* The plane gradients of nvsr_generic_decode_ext (models.py:381-421 under torch.autograd) without a workspace and without d_natural:
 * ACCUMULATED into d_planes like nvsr_generic_decode_backward_ext (num_position_planes + 1 device pointers in a host array; a NULL entry is
 * not wanted and costs no atomics; a NULL array or no wanted plane: NVSR_OK without a launch).  One launch for any P (pieces of whole point
 * blocks only where the grid limit forces them); P == 0: NVSR_OK without a launch; NVSR_ERR_SHAPE for a geometry beyond the capacity above;
 * NVSR_ERR_NULL without natural, x or d_out.  Never allocates or synchronises. */
int nvsr_generic_decode_backward_fused_ext(const nvsr_scene_ext* scene, const nvsr_decoder_geometry* geometry, const float* natural, int64_t P,
                                           const float* x, const float* coord_noise, const float* d_out, float* const* d_planes,
                                           nvsr_stream_t stream);
/* ---- generic decoder, fused plane gradients with the decoder's weight gradients (csrc/generic_fused_bwd.hip) -------------------------------
 * nvsr_generic_decode_backward_ext (the reference: torch.autograd through models.py:381-421) for a geometry the fused backward holds, exact f32:
 * per chunk of nvsr_generic_backward_chunk() points ONE launch of the kernel above compiled to RECORD what the weight-gradient contraction needs
 * as it forms it in LDS -- both decoders' inputs Xd [n][Kd] and Xr [n][Kr], every hidden layer's output H [layer][n][hidden] and every hidden
 * layer's gated output gradient dZ [layer][n][hidden], the layered workspace's shapes, whole 16-byte stores wherever hidden / K is a multiple
 * of 4 -- and then the layered route's own contraction launches (generic_wgrad_kernel per layer and head) on that record, in the same slabs
 * of 2 048 points, onto the same offsets of d_natural.  When no plane gradient is wanted the launch leaves out the decoder inputs' gradients
 * and both scatters.
 * Bit contract: every recorded value has the bits the layered route computes for it, so each slab's accumulator is the layered route's and
 * d_natural equals nvsr_generic_decode_backward_ext's up to the arrival order of the slabs' and waves' float atomics; for P <= 512 only one wave of
 * one slab has points, the others add +0, and d_natural is the layered route's bit for bit.  The plane gradients keep the contract of
 * nvsr_generic_decode_backward_fused_ext.  Everything is ACCUMULATED into what is there.
 * nvsr_generic_backward_fused_record_workspace_floats_ext: (Kd + Kr + 2 (density_layers + rgb_layers) hidden) x min(P, chunk) floats of record
 * + 16 floats with which the entry starts each of the four arrays at a multiple of 16 bytes in ANY workspace; -1 for a geometry that
 * nvsr_generic_decoder_natural_floats_ext refuses or P < 0.  Capacity: nvsr_generic_backward_fused_supported -- the row does not grow.
 * nvsr_generic_decode_backward_fused_record_ext: status codes in the order of nvsr_generic_decode_backward_fused_ext -- scene, geometry,
 * NVSR_ERR_SHAPE beyond the capacity, NVSR_ERR_NULL without natural, x or d_out or with d_natural but no workspace, the scene's planes,
 * NVSR_ERR_SHAPE for P < 0; P == 0: NVSR_OK without a launch.  d_natural == NULL: nvsr_generic_decode_backward_fused_ext (workspace is not
 * read); neither d_natural nor a plane wanted: NVSR_OK without a launch.  Never allocates or synchronises. */
int64_t nvsr_generic_backward_chunk(void);
int64_t nvsr_generic_backward_fused_record_workspace_floats_ext(const nvsr_decoder_geometry* geometry, int num_position_planes, int64_t P);
int nvsr_generic_decode_backward_fused_record_ext(const nvsr_scene_ext* scene, const nvsr_decoder_geometry* geometry, const float* natural, int64_t P,
                                                  const float* x, const float* coord_noise, const float* d_out, float* d_natural,
                                                  float* const* d_planes, float* workspace, nvsr_stream_t stream);
/* ---- generic decoder, fused evaluation in NVSR_ARITH_F16X2 (csrc/generic_fused_limb.hip) ---------------------------------------------
 * The launch above with the HIDDEN layers of both decoders in two f16 limbs: per layer w^ = limbs of 2^8 W, x^ = limbs of 2^4 x (hi = RN_f16(v),
 * lo = RN_f16(v - hi)), the products Wh xl, Wh xh, Wl xh on v_mfma_f32_32x32x16_f16 per 16-column K-block of [X1 | X2] in ascending order, f32
 * accumulation, act = relu(fma(acc, 2^-12, b)) with a ReLU that keeps NaN.  The input features, the biases, both heads (on the f32 activations,
 * from the natural blob) and the outputs are f32 and computed exactly as by nvsr_generic_decode_fused_ext.  BY NAME only: there is no process
 * default here.  Its backward for a frozen decoder is nvsr_generic_decode_backward_fused_arith_ext below; decoder-weight gradients stay exact f32.
 * Range contract: F16X2's -- |W| < 255 for the hidden matrices, |feature / activation| < 4094; beyond them the outputs that depend on the
 * operand are NaN, never a finite wrong number, and a NaN in the planes, the points or the weights comes out as NaN.  A launch that writes a
 * non-finite out row ORs 1 into the range flag (nvsr_set_range_flag), wherever the NaN came from.
 * Packed weights (nvsr_pack_generic_decoder_ext; nvsr_generic_packed_floats_ext 32-bit words, or the negated status for a geometry that
 * nvsr_generic_decoder_natural_floats_ext refuses): every hidden layer in state-dict order -- the density layers, then the rgb layers; heads and
 * biases are NOT packed.  A layer with K = in_features (the natural matrix's columns [X1 | X2]) holds KB = ceil(K / 16) x TT = ceil(hidden / 32)
 * x 2 fragments of 256 words, ordered [kb][t][limb].  Word 4 lane + j (j = 0 .. 3) of lane (m = lane & 31, h = lane >> 5) holds the f16
 * W~[32 t + m][16 kb + 8 h + 2 j] in its low half and W~[32 t + m][16 kb + 8 h + 2 j + 1] in its high half, W~ = 2^8 W and +0 beyond row
 * hidden and column K; limb 0 = RN_f16(W~), limb 1 = RN_f16(W~ - limb 0) (the subtraction is exact in f32).  A lane's A operand of one MFMA is
 * 16 contiguous bytes.  tests/generic_limb_ref.py restates the layout and the arithmetic in numpy.
 * Capacity: nvsr_generic_fused_supported's limits with rows whose parts start at multiples of 4 floats: row = Kr (+ Kd, as above) + hidden, each
 * rounded up to 4 floats, the sum rounded up to 4 x an odd number.
 * nvsr_generic_fused_supported_arith (host only): NVSR_ARITH_F32 answers nvsr_generic_fused_supported, NVSR_ARITH_F16X2 the limb kernel's
 * capacity (1 / 0), any other arithmetic 0; the negated status for an inconsistent geometry.
 * nvsr_generic_decode_fused_arith_ext: NVSR_ARITH_F32 forwards to nvsr_generic_decode_fused_ext (`packed` may be NULL); NVSR_ARITH_F16X2
 * launches the limb kernel (NVSR_ERR_NULL without `packed`, NVSR_ERR_SHAPE beyond the capacity); NVSR_ARITH_F16, NVSR_ARITH_BF16X3,
 * NVSR_ARITH_INHERIT and everything else: NVSR_ERR_SHAPE.  P == 0: NVSR_OK without a launch. */
int64_t nvsr_generic_packed_floats_ext(const nvsr_decoder_geometry* geometry, int num_position_planes);
int nvsr_pack_generic_decoder_ext(const nvsr_decoder_geometry* geometry, int num_position_planes, const float* natural, float* packed,
                                  nvsr_stream_t stream);
int nvsr_generic_fused_supported_arith(const nvsr_decoder_geometry* geometry, int num_position_planes, int arith);
int nvsr_generic_decode_fused_arith_ext(const nvsr_scene_ext* scene, const nvsr_decoder_geometry* geometry, const float* natural,
                                        const float* packed, int64_t P, const float* x, const float* coord_noise, float* out, int arith,
                                        nvsr_stream_t stream);
/* ---- generic decoder, fused plane gradients in NVSR_ARITH_F16X2 (csrc/generic_fused_bwd_limb.hip) ------------------------------------------
 * nvsr_generic_decode_backward_fused_ext with the HIDDEN layers in two f16 limbs, forward and transposed, in ONE launch: the backward of
 * nvsr_generic_decode_fused_arith_ext(NVSR_ARITH_F16X2) for an iteration in which the decoder's parameters take NO gradient.  BY NAME only.
 * The kernel recomputes the forward exactly as that launch does (the same packed blob, the same operand order): the gate bits (output > 0; NaN
 * and 0 closed) belong to the activations the forward produced.  The heads' data gradients from d_out are exact f32 from the natural blob.
 * A transposed hidden layer: dX[p][k] = sum_m dZ[p][m] W[m][k] over the 16-row blocks of the output index m in ascending order on
 * v_mfma_f32_32x32x16_f16, f32 accumulation, per block the products Wh zl, Wh zh, Wl zh.  w^ = limbs of 2^8 W (the transposed blob below);
 * z^ = limbs of 2^e dZ[p][.] with ONE exact power of two per point and layer: e puts the largest |dZ[p][m]| of the gated row into [2^14, 2^15)
 * (a zero row: e = 0 and exact zeros); dX = acc 2^(-8 - e).  Multiplying a point's cotangent by 2^k multiplies its gradients by 2^k bit for bit
 * (but for underflow).  The additions of a skip layer's part and layer 0's part into the decoder inputs' gradients, the view plane, the
 * combination rules, the taps and the one atomic per (tap, channel) are nvsr_generic_decode_backward_fused_ext's own code.
 * Range contract: |W| < 255 for the hidden matrices and the forward's |feature / activation| < 4094; a row of dZ that holds an inf or a NaN, or
 * a weight beyond the range, gives NaN gradients -- never a finite wrong number -- and the launch ORs 1 into the range flag
 * (nvsr_set_range_flag).  The cotangent's magnitude is free: 1e30 and 1e-30 are scaled exactly.
 * Transposed blob (nvsr_pack_generic_decoder_bwd_ext, one kernel, one thread per word; nvsr_generic_packed_bwd_floats_ext 32-bit words, or the
 * negated status for a geometry that nvsr_generic_decoder_natural_floats_ext refuses): every hidden layer in state-dict order -- the density
 * layers, then the rgb layers.  A layer holds its column part [0, K1) (K1 = the decoder's input width for layer 0, hidden otherwise) and, if a
 * skip layer, the part [K1, K1 + K2) behind it; a part of `cols` columns starting at column c0 holds MB = ceil(hidden / 16) x TT = ceil(cols / 32)
 * x 2 fragments of 256 words, ordered [mb][t][limb].  Word 4 lane + j (j = 0 .. 3) of lane (k = lane & 31, h = lane >> 5) holds the f16
 * W~[16 mb + 8 h + 2 j][c0 + 32 t + k] in its low half and W~[16 mb + 8 h + 2 j + 1][c0 + 32 t + k] in its high half, W~ = 2^8 W and +0 beyond
 * row hidden and beyond the part's columns; limb 0 = RN_f16(W~), limb 1 = RN_f16(W~ - limb 0).  A lane's A operand of one MFMA is 16 contiguous
 * bytes.  tests/generic_train_limb_ref.py restates the layout and the arithmetic in numpy.
 * Capacity: nvsr_generic_fused_supported_arith(NVSR_ARITH_F16X2)'s limits and the row = Kr + Kd (each rounded up to 4 floats) + hidden (rounded
 * up to 16) + 4 + (density_layers + rgb_layers) x ceil(hidden / 32), rounded up to 4 x an odd number, 32 of which fit in 160 KB.
 * nvsr_generic_backward_fused_supported_arith (host only): NVSR_ARITH_F32 answers nvsr_generic_backward_fused_supported, NVSR_ARITH_F16X2 this
 * capacity (1 / 0), any other arithmetic 0; the negated status for an inconsistent geometry.
 * nvsr_generic_decode_backward_fused_arith_ext: NVSR_ARITH_F32 forwards to nvsr_generic_decode_backward_fused_ext (`packed`, `packed_bwd` may be
 * NULL); NVSR_ARITH_F16X2 launches the limb kernel (NVSR_ERR_NULL without natural, packed, packed_bwd, x or d_out; NVSR_ERR_SHAPE beyond the
 * capacity); every other arithmetic: NVSR_ERR_SHAPE.  d_planes, P == 0 and "no plane wanted" as nvsr_generic_decode_backward_fused_ext. */
int nvsr_generic_backward_fused_supported_arith(const nvsr_decoder_geometry* geometry, int num_position_planes, int arith);
int64_t nvsr_generic_packed_bwd_floats_ext(const nvsr_decoder_geometry* geometry, int num_position_planes);
int nvsr_pack_generic_decoder_bwd_ext(const nvsr_decoder_geometry* geometry, int num_position_planes, const float* natural, float* packed_bwd,
                                      nvsr_stream_t stream);
int nvsr_generic_decode_backward_fused_arith_ext(const nvsr_scene_ext* scene, const nvsr_decoder_geometry* geometry, const float* natural,
                                                 const float* packed, const float* packed_bwd, int64_t P, const float* x, const float* coord_noise,
                                                 const float* d_out, float* const* d_planes, int arith, nvsr_stream_t stream);
/* ---- generic decoder, fused evaluation in two phases (csrc/generic_fused.hip, csrc/generic_fused_limb.hip, csrc/generic_live.hip) --------
 * The launch above split at the decoders, for a frame that runs the colour decoder on the samples of nonzero weight only: the density
 * phase on every point, the compositing weights, their live list, the colour phase on the listed points.  Both phases are the one-launch
 * kernels compiled with a phase argument: the same rows in LDS, the same operand pairs in the same order, so sigma and the colour logits
 * carry the BITS of nvsr_generic_decode_fused_arith_ext at the same points, in NVSR_ARITH_F32 and in NVSR_ARITH_F16X2 (the same packed blob).
 * Contract of a frame: a sample the list leaves out behaves as if its colour logits were +0.  With weight exactly 0 that is the one-launch
 * frame bit for bit -- except that a NaN colour logit at such a sample gives NaN there (0 x NaN) and a finite pixel here, and that in
 * NVSR_ARITH_F16X2 a range overflow of the colour decoder alone at such a sample no longer raises the range flag.
 * Capacity: nvsr_generic_fused_supported_arith answers for both phases -- each holds a part of the full kernel's row, so either fits wherever
 * the one-launch kernel fits.  Beyond it, and for every arithmetic but NVSR_ARITH_F32 / NVSR_ARITH_F16X2: NVSR_ERR_SHAPE.
 * nvsr_generic_decode_fused_density_arith_ext: position, the position planes' taps, combine_pos_planes, the density layers and fc_alpha on
 * all P points (no atan2f, no view plane, no colour layer); writes the 16-byte row [+0, +0, +0, sigma_raw] of every point into raw_out [P,4]:
 * the compositors read the tensor as it is.  F16X2: a non-finite sigma raises bit 1 of the range flag.  P == 0: NVSR_OK without a launch.
 * nvsr_generic_decode_fused_colour_arith_ext: the points index[i], i < min(*count_dev, max_count), of x [P,6] (coord_noise [P,3] by the same
 * index): the colour decoder's input, the colour layers and fc_rgb; writes the 12 bytes raw_inout[index[i]][0:3] and NOTHING else -- not
 * column 3, no row outside the list.  index (int32, device; any order; distinct) and count_dev (int32, device, read by the kernel: no host
 * synchronisation between the phases) usually come from nvsr_generic_live_list; entries at or beyond the count are not read, an index outside
 * [0, P) is skipped.  The launch is sized for max_count (0 <= max_count <= P < 2^31, else NVSR_ERR_SHAPE; P for a list of unknown length);
 * workgroups beyond the count return at once.  F16X2: non-finite colour logits of a listed point raise bit 1 of the range flag. */
int nvsr_generic_decode_fused_density_arith_ext(const nvsr_scene_ext* scene, const nvsr_decoder_geometry* geometry, const float* natural,
                                                const float* packed, int64_t P, const float* x, const float* coord_noise, float* raw_out, int arith,
                                                nvsr_stream_t stream);
int nvsr_generic_decode_fused_colour_arith_ext(const nvsr_scene_ext* scene, const nvsr_decoder_geometry* geometry, const float* natural,
                                               const float* packed, int64_t P, const float* x, const float* coord_noise, const int32_t* index,
                                               const int32_t* count_dev, int64_t max_count, float* raw_inout, int arith, nvsr_stream_t stream);
/* the live list of weights w [P] (the compositor's, any float array): index_out [P] (int32) receives, in ASCENDING order, every p with
 * !(w[p] == 0) -- NaN is live, +0.0 and -0.0 are dead -- and *count_dev their number; entries of index_out beyond the count are left as they
 * were.  Two launches (per-workgroup counts; their sum in front of every workgroup, a ballot prefix within it), no atomics: the same list
 * on every run.  workspace: nvsr_generic_live_list_workspace_bytes(P) bytes on the device (at most 16 KB; -NVSR_ERR_SHAPE for P < 0 or
 * P >= 2^31, which nvsr_generic_live_list refuses with NVSR_ERR_SHAPE).  P == 0: *count_dev = 0. */
int64_t nvsr_generic_live_list_workspace_bytes(int64_t P);
int nvsr_generic_live_list(int64_t P, const float* w, int32_t* index_out, int32_t* count_dev, void* workspace, nvsr_stream_t stream);
/* ---- generic decoder, occupancy grid (csrc/occupancy.hip, csrc/generic_fused*.hip; opt-in: without a grid nothing above changes) ------------
 * The grid of "Occupancy grid" above -- the same layout, the same probe positions, the same rule for a bit (sigma_raw > threshold or NaN), the
 * same dilation, the same slabs and nvsr_occupancy_workspace_floats(G, K) floats of workspace, out of the same kernels -- for a generic
 * geometry, and a density phase that runs on the KEPT samples only.
 * Contract of a frame: a CULLED sample behaves as if the density decoder had answered NVSR_CULLED_SIGMA (-1e30f, the value the native route's
 * contract uses): relu makes it 0, so alpha = 0, w = +0.0, T unchanged, and the live list leaves the sample out.  A KEPT sample carries the
 * bits of nvsr_generic_decode_fused_arith_ext at the same point.  A point with a NaN coordinate is kept, and so is a point OUTSIDE the box
 * (a normalised coordinate with |n| > 1; n = +-1 exactly is inside and goes by its cell): a generic geometry may sample its planes through
 * rotated frames, where border padding clamps the projected coordinates, not n, so such a point does not have its clamped cell's features.
 * The one documented difference is the native route's: a NaN sigma inside a culled cell no longer reaches the pixel.
 * nvsr_generic_occupancy_build_ext: nvsr_occupancy_build with nvsr_generic_decode_fused_density_arith_ext (NVSR_ARITH_F32 / _F16X2; `packed`
 * is read in F16X2 only) as the decode in the middle.  A geometry or arithmetic beyond nvsr_generic_fused_supported_arith, G outside 1..512, K
 * outside 1..4, dilate < 0: NVSR_ERR_SHAPE with nothing launched.
 * nvsr_generic_occupancy_keep: for x [P,6], n = 2 (x - lo) / range - 1 as the decode kernels form it (no jitter); keep[p] = 1.0f if the point is
 * kept by the rules above, else 0.0f, and a culled point's row raw[p] = [+0, +0, +0, NVSR_CULLED_SIGMA]; kept rows of raw [P,4] are not
 * touched.  Only lo, range and num_position_planes of the scene are read.  nvsr_generic_live_list on `keep` gives the ascending kept list.
 * nvsr_generic_decode_fused_density_list_arith_ext: the density phase on the points index[i], i < min(*count_dev, max_count), listed exactly as
 * for the colour phase (entries at or beyond the count are not read, an index outside [0, P) is skipped, workgroups beyond the count return at
 * once; 0 <= max_count <= P < 2^31): writes the 16-byte row [+0, +0, +0, sigma_raw] at raw_inout[index[i]] and no other row.  F16X2: a
 * non-finite sigma of a listed point raises bit 1 of the range flag. */
#define NVSR_CULLED_SIGMA (-1e30f)
int nvsr_generic_occupancy_build_ext(const nvsr_scene_ext* scene, const nvsr_decoder_geometry* geometry, const float* natural, const float* packed,
                                     int G, int K, float threshold, int dilate, int arith, uint32_t* grid, float* workspace, nvsr_stream_t stream);
int nvsr_generic_occupancy_keep(const nvsr_scene_ext* scene, int64_t P, const float* x, const uint32_t* grid, int G, float* keep, float* raw,
                                nvsr_stream_t stream);
int nvsr_generic_decode_fused_density_list_arith_ext(const nvsr_scene_ext* scene, const nvsr_decoder_geometry* geometry, const float* natural,
                                                     const float* packed, int64_t P, const float* x, const float* coord_noise, const int32_t* index,
                                                     const int32_t* count_dev, int64_t max_count, float* raw_inout, int arith, nvsr_stream_t stream);

/* run_network's model input for a pass (train_utils.py:15-64,111): x [N*S,6] = [ro + rd * z, viewdir] from packed rays [N,11], z [N,S] */
int nvsr_ray_points(int64_t N, int S, const float* rays, const float* z, float* x, nvsr_stream_t stream);

/* ---- per-call arithmetic -----------------------------------------------------------------------------------------------------
 * Twins of the entry points above that run decoder GEMMs or SR convolutions, with the arithmetic as an explicit argument
 * (NVSR_ARITH_F32 | NVSR_ARITH_BF16X3 | NVSR_ARITH_F16X2 | NVSR_ARITH_INHERIT; the convolution, EDSR and PlanesSR families -- nvsr_conv3x3*_arith,
 * nvsr_edsr_*_arith, nvsr_planes_sr*_arith and their batch forms, nvsr_pack_edsr[_dgrad]_arith -- also NVSR_ARITH_F16).  Same arguments, same
 * semantics; the un-suffixed entry points are these called with NVSR_ARITH_INHERIT.  A backward call must be given the mode of the
 * forward whose gates / record / activations it consumes (the host mirror stores it with the autograd context).
 * rows_per_tile (convolutions): 0 = the launcher's choice, 2 | 3 | 4 = force that row-tile instantiation of the wide kernels (two output
 * blocks per wave), 8 = the bf16-limb kernel's one-output-block x 8-row wave tile (round 3; equally fast; 2 | 3 | 4 | 8 give the same
 * bits), 16 = the bf16-limb kernel on v_mfma_f32_16x16x32_bf16 (round 3; layers with Cin % 32 == 0 and Cout % 128 == 0 only, their default:
 * the K dimension of an instruction spans 32 input channels, so the f32 accumulation order -- not the limb products -- differs from the
 * other instantiations; same tolerance against the oracle), 18 | 19 | 20 = that kernel with 2 | 3 | 4 rows forced, 22 = its 6-row tile
 * (NVSR_ARITH_F16X2 and NVSR_ARITH_F16 only; NVSR_ARITH_F16 runs its one-limb kernel at 0 | 16 | 18 | 19 | 20 | 22 and, like F16X2, bf16
 * limbs at 2 | 3 | 4 | 8)
 * (the results are identical; the parity tests force every instantiation). */
int nvsr_render_pass_arith(const nvsr_scene* scene, const float* packed_decoder, int64_t N, int S, const float* rays, const float* z,
                           const float* noise, int white_bkgd, float* rgb, float* disp, float* acc, float* weights, float* depth,
                           float* raw_out /* or NULL */, int arithmetic, nvsr_stream_t stream);
int nvsr_decode_rays_arith(const nvsr_scene* scene, const float* packed_decoder, int64_t N, int S, const float* rays, const float* z,
                           float* raw, uint32_t* gates /* or NULL */, float* record /* or NULL */, int arithmetic, nvsr_stream_t stream);
int nvsr_render_rays_arith(const nvsr_scene* scene, const float* packed_coarse, const float* packed_fine, int64_t N, int Nc, int Nf,
                           const float* rays, int lindisp, int white_bkgd, const float* t_rand, const float* u,
                           const float* noise_coarse, const float* noise_fine, float* rgb_c, float* disp_c, float* acc_c,
                           float* rgb_f, float* disp_f, float* acc_f, float* workspace, int arithmetic, nvsr_stream_t stream);
/* One decoder for both passes (models.fine.type == 'use_same': train_nerf.py:353-355 makes model_fine the coarse model itself).  Same
 * arguments and results as nvsr_render_rays_arith with packed_fine == packed_coarse; the fine pass evaluates the decoder on the Nf importance
 * samples only and takes the Nc coarse samples' outputs from the coarse pass (same decoder, same planes, same points: the reference
 * recomputes them, train_utils.py:155-170), then composites the merged list.  Taken for frames without stratified jitter on the fused limb
 * passes (N >= nvsr_fused_min_rays(), t_rand == NULL, a limb arithmetic); otherwise -- and with NVSR_NO_SHARED_DECODER in the environment --
 * it forwards to nvsr_render_rays_arith.  workspace: nvsr_render_shared_workspace_floats floats. */
int64_t nvsr_render_shared_workspace_floats(int64_t N, int Nc, int Nf);
int nvsr_render_rays_shared_arith(const nvsr_scene* scene, const float* packed_decoder, int64_t N, int Nc, int Nf, const float* rays, int lindisp,
                                  int white_bkgd, const float* t_rand, const float* u, const float* noise_coarse, const float* noise_fine,
                                  float* rgb_c, float* disp_c, float* acc_c, float* rgb_f, float* disp_f, float* acc_f, float* workspace,
                                  int arithmetic, nvsr_stream_t stream);
/* The merge of that route alone: the Nc un-jittered coarse depths of a ray (recomputed from near / far of the packed rays [N,11] -- what
 * nvsr_coarse_z writes, bit for bit) and its Nf new samples z_new [N,Nf] -> z_merged [N,Nc+Nf], and the decoder outputs raw_coarse [N,Nc,4],
 * raw_new [N,Nf,4] gathered into the same order -> raw_merged [N,Nc+Nf,4] (verbatim 16-byte copies).  The order is the stable sort of
 * [coarse | new]: a coarse depth stands behind the samples that are smaller, a sample behind the coarse depths that are smaller or equal, ties
 * inside a list go by index, NaNs go last (coarse before samples, by index) like torch.sort's.  The samples need not be sorted.
 * 3 <= Nc <= 256, 1 <= Nf <= 256; the three raw pointers 16-byte aligned. */
int nvsr_shared_merge(int64_t N, int Nc, int Nf, const float* rays, int lindisp, const float* z_new, const float* raw_coarse, const float* raw_new,
                      float* z_merged, float* raw_merged, nvsr_stream_t stream);
int nvsr_render_pass_backward_gates_arith(const nvsr_scene* scene, const float* packed_decoder, const float* packed_bwd, int64_t N, int S,
                                          const float* rays, const float* z, const float* g_raw, const uint32_t* gates,
                                          float* const* grad_planes, float* view_ws, float* record, int arithmetic, nvsr_stream_t stream);
int nvsr_decoder_weight_grad_arith(int64_t N, int S, const float* record, float* grad_natural, int arithmetic, nvsr_stream_t stream);
int nvsr_conv3x3_arith(const float* in, int Cin, int H, int W, const float* packed, int Cout, int epilogue, const float* skip, float* out,
                       int arithmetic, int rows_per_tile, nvsr_stream_t stream);
int nvsr_conv3x3_dgrad_arith(const float* dy, int Cin, int H, int W, const float* packed_dgrad, int Cout, float* dx, int arithmetic,
                             int rows_per_tile, nvsr_stream_t stream);
int nvsr_conv3x3_wgrad_arith(const float* dy, const float* x, int Cin, int H, int W, int Cout, float scale, float* dw, float* workspace,
                             int arithmetic, nvsr_stream_t stream);
int nvsr_edsr_forward_batch_arith(const float* x, int B, int Cin, int H, int W, const float* packed, int Cout, int hid, int nblocks, int n_up,
                                  float* out, float* workspace, int arithmetic, nvsr_stream_t stream);
int nvsr_edsr_forward_train_arith(const float* x, int Cin, int H, int W, const float* packed, int Cout, int hid, int nblocks, int n_up,
                                  float* out, float* acts, int arithmetic, nvsr_stream_t stream);
int nvsr_edsr_backward_arith(const float* x, int Cin, int H, int W, const float* acts, const float* packed_dgrad, int Cout, int hid,
                             int nblocks, int n_up, const float* d_out, float* grad_natural, float* dx, float* workspace, int arithmetic,
                             nvsr_stream_t stream);
int nvsr_planes_sr_arith(const float* lr, int C, int R0, int R1, const float* packed, int hid, int nblocks, int n_up, int pad, int over,
                         const float* roi, const float* mean, const float* std_, float* out, float* workspace, int arithmetic,
                         nvsr_stream_t stream);
int nvsr_planes_sr_batch_arith(const float* const* lr, int B, int C, int R0, int R1, const float* packed, int hid, int nblocks, int n_up,
                               int pad, int over, const float* roi, const float* mean, const float* stdv, float* const* out,
                               float* workspace, int arithmetic, nvsr_stream_t stream);
int nvsr_planes_sr_train_arith(const float* lr, int C, int R0, int R1, const float* packed, int hid, int nblocks, int n_up, int pad, int over,
                               const float* roi, const float* mean, const float* stdv, float* out, float* workspace, float* keep,
                               int arithmetic, nvsr_stream_t stream);
int nvsr_planes_sr_backward_arith(int C, int R0, int R1, const float* keep, const float* packed_dgrad, int hid, int nblocks, int n_up,
                                  int pad, int over, const float* roi, const float* stdv, const float* d_out, float* grad_natural,
                                  float* d_lr, float* workspace, int arithmetic, nvsr_stream_t stream);

/* ---- SR training on the regions of interest of B planes at once (round 5) -------------------------------------------------------------------
 * Replaces: the B calls `self.SR_model((plane_name, roi))` a training iteration makes from `TwoDimPlanesModel.planes()` (models.py:270-284 ->
 * PlanesSR.forward :884-926), one per position plane of the scene, and their autograd backward (train_nerf.py:903 `loss.backward()`).  Every
 * plane has its own region of interest, i.e. its own crop size; the network is the same.  One launch per layer convolves all B crops (a
 * ragged batch: one crop of a 200^2 plane leaves the last of its 2-3 workgroup rounds a fifth full), one weight-gradient pass and one reduction
 * per layer accumulates all planes' contributions, one magnitude reduction per gradient tensor serves all planes (f16 limbs).
 *   lr / out / d_out / d_lr   HOST arrays of B device pointers (B <= 4); planes [C][R0][R1], outputs / output gradients [C][sf R0][sf R1]
 *   rois                      B x 4 HOST floats, [[ymin,xmin],[ymax,xmax]] in [-1,1] per plane, or NULL (full planes)
 *   keep                      one device buffer of nvsr_planes_sr_batch_keep_floats floats: forward -> backward
 *   align_corners, plane_interp   of the residual up-sampling (PlanesSR.align_corners / .plane_interp), ARGUMENTS of the call (the
 *                             one-plane entry points read the process-wide nvsr_set_sr_* setting)
 *   d_lr                      NULL, or per plane NULL (LR plane detached: models.py:272) or [C][R0][R1], += the plane's gradient
 * Values: those of B one-plane calls up to the order of the weight-gradient sums and (f16 limbs) the shared power-of-two gradient scale. */
/* nvsr_planes_sr_batch_arith (evaluation: B equally sized planes, ONE region of interest or none) with the residual's settings as arguments */
int nvsr_planes_sr_batch_ex(const float* const* lr, int B, int C, int R0, int R1, const float* packed, int hid, int nblocks, int n_up, int pad,
                            int over, const float* roi, const float* mean, const float* stdv, float* const* out, float* workspace,
                            int arithmetic, int align_corners, int plane_interp, nvsr_stream_t stream);
int64_t nvsr_planes_sr_batch_keep_floats(int B, int C, int R0, int R1, int hid, int nblocks, int n_up, int pad, const float* rois);
int64_t nvsr_planes_sr_batch_workspace_floats(int B, int C, int R0, int R1, int hid, int nblocks, int n_up, int pad, const float* rois);
int64_t nvsr_planes_sr_batch_backward_workspace_floats(int B, int C, int R0, int R1, int hid, int nblocks, int n_up, int pad, const float* rois);
int nvsr_planes_sr_train_batch_arith(const float* const* lr, int B, int C, int R0, int R1, const float* packed, int hid, int nblocks, int n_up,
                                     int pad, int over, const float* rois, const float* mean, const float* stdv, float* const* out,
                                     float* workspace, float* keep, int arithmetic, int align_corners, int plane_interp, nvsr_stream_t stream);
int nvsr_planes_sr_backward_batch_arith(int B, int C, int R0, int R1, const float* keep, const float* packed_dgrad, int hid, int nblocks,
                                        int n_up, int pad, int over, const float* rois, const float* stdv, const float* const* d_out,
                                        float* grad_natural, float* const* d_lr, float* workspace, int arithmetic, int align_corners,
                                        int plane_interp, nvsr_stream_t stream);
/* The same with PROGRESS MARKS for a data-parallel caller (the 173 MB EDSR gradient is all-reduced every refinement iteration;
 * the reference has no distributed code -- models.py:789-822 under torch.autograd is what the marks follow).  The backward walks the layers from
 * conv_output to conv_input; grad_natural is in state-dict order, so the gradients become final from the END of the blob.  mark_events[i] (a
 * hipEvent_t of the caller) is recorded on `stream` as soon as the weight gradients of layer mark_layers[i] (0 = conv_input ... 2 nblocks + 4 =
 * conv_output with two upscale stages) and of every layer behind it are final: the caller's collective stream waits for it and reduces that part
 * of the blob while the remaining layers are still being computed.  Exact f32 / one plane: every mark is recorded at the end of the pass. */
int nvsr_planes_sr_backward_batch_marks(int B, int C, int R0, int R1, const float* keep, const float* packed_dgrad, int hid, int nblocks,
                                        int n_up, int pad, int over, const float* rois, const float* stdv, const float* const* d_out,
                                        float* grad_natural, float* const* d_lr, float* workspace, int arithmetic, int align_corners,
                                        int plane_interp, int n_marks, const int32_t* mark_layers, void* const* mark_events, nvsr_stream_t stream);

/* ---- low-rank feature planes ---------------------------------------------------------------------------------------------------------------
 * Replaces: `TwoDimPlanesModel.gen_plane` (models.py:223-230) -- with `plane_rank[name] = r` a position plane is stored as ONE parameter
 * F [1,C,R,2r] (contiguous NCHW), U = F[..., :r], V = F[..., r:], and sampled as plane = U @ V^T per channel (torch.matmul + permute) -- and
 * that product's autograd backward.  Square planes only; ranks and resolutions may differ between the planes of a call; r == R is legal.
 *   factors[p]     device, [C][R][2r] f32 (4-byte alignment is enough: rows are 8r bytes)
 *   planes[p]      device, CHANNEL-LAST [R][R][C]: written by nvsr_lowrank_planes; READ by nvsr_lowrank_planes_backward as dL/d plane
 *   d_factors[p]   device, [C][R][2r]: written (every element, no accumulation) by nvsr_lowrank_planes_backward; unused by the forward
 * Arithmetic: exact f32, no limb mode.  plane[y][x][c] = the fmaf chain over k = 0 .. r-1 ASCENDING from +0.0 (the f32 matrix instruction,
 * k zero-padded to its step of 4); dU[c][y][k] = the fmaf chain over x ascending of G[y][x][c] V[c][x][k], dV[c][x][k] over y ascending of
 * G[y][x][c] U[c][y][k].  No atomics and no split sums: the results are a function of the inputs alone, bit for bit run to run and whether a
 * plane is alone in the call or not.  One kernel launch per call for all planes.
 * NVSR_ERR_SHAPE (nothing is launched): num_planes outside 1 .. NVSR_MAX_POSITION_PLANES, channels < 1, a res or rank < 1. */
typedef struct nvsr_lowrank_planes_args {
    int32_t num_planes;                                   /* 1 .. NVSR_MAX_POSITION_PLANES */
    int32_t channels;                                     /* C >= 1 (any; 48 in the shipped configs) */
    const float* factors[NVSR_MAX_POSITION_PLANES];
    float* planes[NVSR_MAX_POSITION_PLANES];
    float* d_factors[NVSR_MAX_POSITION_PLANES];
    int32_t res[NVSR_MAX_POSITION_PLANES];                /* R per plane */
    int32_t rank[NVSR_MAX_POSITION_PLANES];               /* r per plane (the reference's plane_rank: ceil(planes_rank_ratio R), models.py:541) */
} nvsr_lowrank_planes_args;
int nvsr_lowrank_planes(nvsr_lowrank_planes_args args, nvsr_stream_t stream);
int nvsr_lowrank_planes_backward(nvsr_lowrank_planes_args args, nvsr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NVSR_H */
