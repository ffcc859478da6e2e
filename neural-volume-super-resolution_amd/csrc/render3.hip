// Fused render pass, third generation: the decoder GEMMs on the bf16 matrix pipe with every f32 operand split into bf16 limbs
// (limb_core.h; error bound there) -- products at 2.7x (3 limbs) or 16-bit operands at 5.3x (2 limbs) the rate of v_mfma_f32_32x32x2_f32.
//
// Same skeleton as render2.hip: one wave per SIMD owns two 32-point tiles X and Y; while the matrix pipe multiplies one tile, the other
// tile's gathers / bias + ReLU / heads are issued in the gaps.  What changes with a 32-cycle MFMA: a gap hides ~5 single-issue
// instructions (measured, tools/limb_ubench.hip: 32.5 cycles per MFMA bare, 34.4 with the limb split of the next K-block in the gaps,
// 35.4 with 3 more VALU per gap, 42 with 5 more), so all side work is cut into slices of <= 3 VALU and spread over the slots of a block.
//
// Per sample and tile: 63 K-blocks (16 input channels) x 4 output blocks x NP MFMAs; weights stream through a 2-slot LDS ring in 17
// chunks (a plane's share of a feature layer = 3 K-blocks, half a hidden layer = 4), 12 * LIMBS KB per K-block.
// Biases are not preloaded into the accumulators: the first MFMA of a layer takes C = 0 and act = max(acc + bias, 0).
#include "pair_core.h"

#include "colour_order.h"
#include "occupancy.h"
#include "nvsr_internal.h"

namespace nvsr {

// =====================================================================================================================
// The body of both kernels below (one instantiation per LIMBS; the kernels are thin shells so that the coarse and the fine pass are two
// symbols in a rocprofv3 kernel trace -- a second template parameter on one kernel trips hipcc's host pass over the LDS-DMA builtins).
// ZCOMP: the depths are the un-jittered coarse ones (train_utils.py:95-100) and are computed from the ray's near / far in registers
// (coarse_depth, bit for bit what nvsr_coarse_z writes) instead of being read: `z` is NULL and `lindisp` selects the spacing
// (ONE template parameter, LZ = LIMBS + 8 * ZCOMP + 16 * PHASE, PHASE three bits wide: with a second one hipcc's host pass fails to resolve the LDS-DMA helpers inside the body)
//
// PHASE: 0 = the fused pass (both decoders on every sample: the path of raw_out != NULL and of NVSR_RENDER_ONE_PHASE=1).
// The two-phase route runs the colour decoder only where it can reach the pixel -- w = alpha T is +0.0 exactly wherever sigma + noise <= 0,
// and such a sample adds +0.0 to every accumulator:
//   1 = density pass: planes 0..2 -> D, density layers 0..3, sigma head, the whole compositing recurrence of T, w, depth, acc (composite_weight:
//       the operations of composite_sample) -- writes disp / acc / depth / weights and, per ray, the live list: (z or sample index, w) of every
//       sample with !(w == 0) in sample order (rows of S entries, like z) and their count.  The gathers of sample s + 1 roll through the blocks of
//       sample s in halves of two taps (gather_half, pair_core.h).
//   2 = colour pass: the loop runs over k < trip = max live count of the workgroup's 256 rays (workgroup-uniform: the four waves share the
//       ring); a lane evaluates its ray's k-th live sample -- today's rgb layer 0 (same K-block order), rgb layers 1..3, rgb head -- and adds
//       w sigmoid(raw) with the operations of composite_sample.  A lane past its own count re-evaluates its last entry and KEEPS its
//       accumulators (a select, no + 0 x: padding cannot inject a NaN).
//       WHICH ray a lane owns comes from live_n.  The density pass writes live_n[ray] = count; live_order_kernel, launched between the two
//       passes, rewrites every block of ORDER_RAYS consecutive rays in place: entry j = (count << ORDER_SHIFT) | index of a ray in the block,
//       the block's rays stably sorted by the bin of their count, fullest bin first.  The lane that used to own ray j of the block (slot j)
//       owns the ray entry j names, for the whole launch: a workgroup's 256 rays then have similar counts and trip is close to each of them.
//       A slot >= N is invalid as before (clamped ray, count 0, nothing written).  A ray's sums and the order of its additions do not depend
//       on the lane that holds them, so the pixels do not change.  NVSR_COLOUR_ORDER=0 (read at every launch) makes every entry name its own slot.
//   3 = point-major colour pass (the default; NVSR_COLOUR_POINTS=0 keeps phase 2): the same rgb chain, but a lane evaluates one live POINT per
//       step, not its ray's k-th: point_order_kernel (colour_order.hip) lists the points of the workgroup's 256 slots in the order (depth band,
//       slot, k), cut into steps of 256 and sorted by (slot, k) inside a step, and the loop runs the group's ceil(points / 256) steps -- no
//       padding but in the last step, and the 64 points of a wave are a few rays x consecutive samples of one band: neighbouring texels.
//       A lane no longer owns a ray: the ray cache is indexed by the entry's slot; the view features V, blended in the prologue as before, go to
//       a global table (POINT_VIEW_FLOATS per slot, 48 KB per group) and each step loads its points' rows, a step ahead; every lane stores its
//       point's three terms w sigmoid(raw) in LDS, and behind a barrier the first point of every run adds its run's terms, in order, to the
//       ray's sums in LDS: the same operands in the same order as phase 2.  Entries are read two steps ahead, list entries one.
//   4 = density pass over the kept lists of the occupancy route (occupancy.hip; include/nvsr.h, "Occupancy grid"): phase 1's decoder, gathers and
//       compositing, but the loop runs over k < trip = max kept count of the workgroup's 256 rays, as phase 2's does: a lane evaluates its ray's
//       k-th KEPT sample idx = kept[ray][k] -- zc = depth(idx); dist from the sample's own successor in the full row, depth(idx + 1) - zc, or
//       1e10 for idx = S - 1 -- and a lane past its own count re-evaluates its last entry and keeps T, depth, acc and its list cursor by selects.
//       A culled sample is never seen: it would have had alpha = 0, w = +0.0 and left T as it was.  The next step's gathers roll through the
//       current one as in phase 1; the kept entries are read in the epilogue, up to two steps ahead, so that (depths read) the next step's depth
//       can be loaded a step ahead; an invalid slot (ray >= N) reads the clamped ray's row but is never active.
//       Which ray a lane owns and which block a workgroup runs come from live_order_kernel / group_order_kernel on the kept counts (kept_n:
//       packed entries, an array of its own); the pass writes live_n[ray] and the live lists as phase 1 does, and weights at [ray][idx] only.
// Neither chain's K-order changes and dead samples contributed +0.0 to non-negative sums, so the pixels are bit for bit the fused pass's.
template <int LZ>
__device__ __forceinline__ void render_pass3_body(const SceneDev& sc, const float* __restrict__ packed, long N, int S,
                                                  const float* __restrict__ rays, const float* __restrict__ z, int lindisp,
                                                  const float* __restrict__ noise, int white,
                                                  float* __restrict__ rgb, float* __restrict__ disp,
                                                  float* __restrict__ acc, float* __restrict__ weights,
                                                  float* __restrict__ depth, float* __restrict__ raw_out, unsigned* __restrict__ flag,
                                                  float* __restrict__ live_z = nullptr, float* __restrict__ live_w = nullptr,
                                                  int* __restrict__ live_n = nullptr, const int* __restrict__ group_slot = nullptr,
                                                  const int* __restrict__ pts = nullptr, const int* __restrict__ pt_steps = nullptr, float* views = nullptr,
                                                  const int* __restrict__ kept = nullptr, const int* __restrict__ kept_n = nullptr) {
    constexpr int LIMBS = LZ & 7;
    constexpr bool ZCOMP = (LZ & 8) != 0;
    constexpr int PHASE = (LZ >> 4) & 7;
    constexpr bool FUSED = PHASE == 0, KEPT = PHASE == 4, DENSITY = PHASE == 1 || KEPT, POINTS = PHASE == 3, COLOUR = PHASE == 2 || POINTS;
    constexpr bool F16 = limb_f16(LIMBS);             // the f16 mode (static scales, range flag, LDS layout) -- not the limb count
    using L = Lds3<LIMBS>;
    constexpr int NP = limb_products(LIMBS);
    constexpr int NSF = 3 * 4 * NP, NSH = 4 * 4 * NP;          // slots of a feature block / of half a hidden layer
    __shared__ __attribute__((aligned(16))) unsigned lds[L::TOTAL];
    NVSR_RACE_PROBE_DELAY(lds);      // (probe builds only, nvsr_common.h)
    Ring3<LIMBS> rs{__builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(packed + limb_region(LIMBS)), 0, KB_TOTAL * kb_words(region_limbs(LIMBS)) * 4, 0x00020000),
                    lds, 0, __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), (int)(threadIdx.x & 63), ring3_voff<LIMBS>(threadIdx.x)};
    // (wave index as a SCALAR: the LDS destination of every weight-copy piece is then scalar arithmetic into M0 instead of a vector add + v_readfirstlane per piece)
    float* ldsf = reinterpret_cast<float*>(lds);
    // (f16 limbs: activations are held as x 2^F16_SX -- biases scaled up, head weights scaled down, all exact; limb_core.h)
    // A weight beyond the f16 range was packed as inf: the packer then left a NaN in the blob's spare slot S_F16_POISON, which goes into
    // the head biases here -- every output of such a decoder is NaN instead of a wrong number.
    for (int i = threadIdx.x; i < SMALL_FLOATS; i += TPB2) {
        float v = packed[P_SMALL + i] * (!F16 ? 1.0f : i < S_ALPHA_W ? F16_X_SCALE : i < S_HEAD_B ? F16_HEAD_SCALE : 1.0f);
        if (F16 && i >= S_HEAD_B && i < S_HEAD_B + 4) v += packed[P_SMALL + S_F16_POISON];
        ldsf[L::SMALL + i] = v;
    }
    const float* small = ldsf + L::SMALL;

    const int lane0 = rs.lane;
    // XCD-aware ray blocks: workgroup b runs on XCD b % 8 (round-robin dispatch), each XCD has its own L2.  Give XCD x the x-th contiguous
    // eighth of the ray blocks, so that the workgroups that share an L2 render neighbouring image rows (their taps share texels).
    // Colour pass: the ray block comes from group_slot (group_order_kernel, colour_order.hip): the blocks heaviest first, rank r -> workgroup r -> XCD
    // r % 8, so that the long lists start first and are dealt round the XCDs; with NVSR_COLOUR_GROUP_ORDER=0 the table holds this formula.
    const unsigned nblk = gridDim.x, xcd = blockIdx.x & 7u, per = nblk >> 3, rem = nblk & 7u;
    unsigned blk_ = xcd * per + (xcd < rem ? xcd : rem) + (blockIdx.x >> 3);
    if constexpr (COLOUR || KEPT) blk_ = (unsigned)__builtin_amdgcn_readfirstlane(group_slot[blockIdx.x]);
    const unsigned blk = blk_;
    const long base = (long)blk * RAYS2 + rs.wave * 64 + (lane0 & 31);
    long rayX = base, rayY = base + 32;
    const bool validX = rayX < N, validY = rayY < N;
    if (!validX) rayX = N - 1;
    if (!validY) rayY = N - 1;
    int nX = 0, nY = 0;
    if constexpr (COLOUR || KEPT) {
        // the slot names the ray (packed entries of live_order_kernel); an invalid slot keeps the clamped ray and count 0: it cannot lengthen trip
        const int* const order = KEPT ? kept_n : live_n;
        const long block_base = (long)(blk / (ORDER_RAYS / RAYS2)) * ORDER_RAYS;
        if (validX) { const int e = order[base]; rayX = block_base + (e & (ORDER_RAYS - 1)); nX = e >> ORDER_SHIFT; }
        if (validY) { const int e = order[base + 32]; rayY = block_base + (e & (ORDER_RAYS - 1)); nY = e >> ORDER_SHIFT; }
    }
    constexpr int RAY3_FLOATS = L::RAY_FLOATS;
    const int ownX = rs.wave * 64 + (lane0 & 31), ownY = ownX + 32;      // the slots whose ray the lane loads (and, but for POINTS, owns)
    float* rcX = ldsf + L::RAYS + ownX * RAY3_FLOATS;
    float* rcY = rcX + 32 * RAY3_FLOATS;
    float* rtX = F16 ? ldsf + L::VTAPS + (rs.wave * 64 + (lane0 & 31)) * L::TAP_FLOATS : rcX + 8;     // view-plane taps of the ray
    float* rtY = rtX + 32 * (F16 ? L::TAP_FLOATS : RAY3_FLOATS);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const float* r = rays + (k ? rayY : rayX) * 11;
        float* rc = k ? rcY : rcX;
        float* rtp = k ? rtY : rtX;
        const float dx = r[3], dy = r[4], dz = r[5];
        const Taps vt = view_taps(sc, r[8], r[9], r[10]);
        const float nrm = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz)));
        if (lane0 < 32) {
            reinterpret_cast<f32x4*>(rc)[0] = f32x4{r[0], r[1], r[2], dx};
            reinterpret_cast<f32x4*>(rc)[1] = f32x4{dy, dz, nrm, r[6]};
            if constexpr (L::FAR >= 0) ldsf[L::FAR + rs.wave * 64 + (lane0 & 31) + 32 * k] = r[7];
            else rc[16] = r[7];
            reinterpret_cast<f32x4*>(rtp)[0] = f32x4{__int_as_float(vt.o00), __int_as_float(vt.o01), __int_as_float(vt.o10), __int_as_float(vt.o11)};
            reinterpret_cast<f32x4*>(rtp)[1] = f32x4{vt.nw, vt.ne, vt.sw, vt.se};
        }
    }
    // (kept lists: the depth rows' pointers, like the kept rows', are formed where they are used: z_row)
    const float* zX = ZCOMP || COLOUR || KEPT ? nullptr : z + rayX * S;
    const float* zY = ZCOMP || COLOUR || KEPT ? nullptr : z + rayY * S;
    auto depth_of = [&](const float* zp, const float* rc, int k) NVSR_INL {
        if constexpr (ZCOMP) return coarse_depth(rc[7], L::FAR >= 0 ? ldsf[L::FAR + rs.wave * 64 + (rs.lane & 31) + (rc == rcX ? 0 : 32)] : rc[16], k, S, lindisp);
        else return zp[k];
    };

    Tile3 X, Y;
    X.T = Y.T = 1.0f;
    X.cr = X.cg = X.cb = X.dep = X.ac = 0.0f;
    Y.cr = Y.cg = Y.cb = Y.dep = Y.ac = 0.0f;
    // colour pass: the rays' live lists (rows of S entries; nX, nY entries are valid) and the workgroup's trip count
    const float* lzX = COLOUR ? live_z + rayX * S : nullptr;
    const float* lzY = COLOUR ? live_z + rayY * S : nullptr;
    const float* lwX = COLOUR ? live_w + rayX * S : nullptr;
    const float* lwY = COLOUR ? live_w + rayY * S : nullptr;
    int trip = S;
    float wX = 0.0f, wY = 0.0f, wXn = 0.0f, wYn = 0.0f;
    // density pass over the kept lists: the rays' lists (rows of S sample indices; nX, nY are valid), the entries of this step, the next and the
    // one after it, the depth of this sample's successor in the full row, and the cursors of the live lists (phase 1 too)
    // (a row of `kept` starts rayX * S words into it: the row pointers are formed where they are used, not held over the decoder's blocks)
    auto kept_row = [&](long ray) NVSR_INL -> const int* {
        asm volatile("" : "+v"(ray));
        return kept + ray * S;
    };
    auto z_row = [&](long ray) NVSR_INL -> const float* {
        if constexpr (ZCOMP) return nullptr;
        asm volatile("" : "+v"(ray));
        return z + ray * S;
    };
    int idxX = 0, idxY = 0, idxXn = 0, idxYn = 0, cX = 0, cY = 0;
    bool actX = false, actY = false;                 // does the lane's list reach this step?  (past it the lane keeps what it has)
    // entry k of a kept list; behind the list's end (the cull kernel wrote -1 there) the entry before it, so the index stops advancing: a
    // step is the list's own iff its index differs from the previous step's.  An empty list gives sample 0 (evaluated, never composited).
    auto kept_at = [&](const int* kp, int k, int prev) NVSR_INL -> int { const int e = kp[k < S ? k : S - 1]; return e < 0 ? prev : e; };
    // entry k of a live list, clamped to the last valid one; an empty list gives the ray's near depth and weight 0 (never composited)
    auto live_depth = [&](const float* lzp, const float* rc, int n, int k) NVSR_INL -> float {
        if (n == 0) return rc[7];
        const float e = lzp[k < n ? k : n - 1];
        if constexpr (ZCOMP) return depth_of(nullptr, rc, __float_as_int(e));      // (the density pass stored the sample index)
        else return e;
    };
    auto live_weight = [](const float* lwp, int n, int k) NVSR_INL -> float { return n == 0 ? 0.0f : lwp[k < n ? k : n - 1]; };
    // point-major colour pass: the step's points.  slot: whose ray; live: not padding; e1: the entry of the step after this one
    int slotX = ownX, slotY = ownY, slotXn = ownX, slotYn = ownY, eX1 = POINT_NONE, eY1 = POINT_NONE;
    bool liveX = false, liveY = false, liveXn = false, liveYn = false;
    float* const pt_sums = ldsf + L::PTS;                    // [RAYS2][3]: the rays' colour sums
    float* const pt_exch = pt_sums + 3 * RAYS2;              // [RAYS2][3]: the step's terms
    int* const pt_slot = reinterpret_cast<int*>(pt_exch + 3 * RAYS2);      // [RAYS2]: the slot of every point of the step (-1: padding)
    int* const pt_ray = pt_slot + RAYS2;                     // [RAYS2]: a slot's ray, as its index in the block of the ray order
    const long pt_block = (long)(blk / (ORDER_RAYS / RAYS2)) * ORDER_RAYS;
    const int* const peX = POINTS ? pts + (long)blk * RAYS2 * S + ownX : nullptr;      // the lane's entries: step t at [t RAYS2] (Y: + 32)
    // entry e -> the point's slot, whether it is one, and its list entry (depth or, ZCOMP, the depth of that sample index) and weight
    auto point_of = [&](int e, int own, int& slot, bool& live, float& zv, float& wv) NVSR_INL {
        live = e != POINT_NONE;
        slot = live ? (int)((unsigned)e >> 24) : own;
        const float* rc = ldsf + L::RAYS + slot * RAY3_FLOATS;
        zv = rc[7]; wv = 0.0f;                               // (padding: the slot's near depth, never composited)
        if (live) {
            const long at = (pt_block + pt_ray[slot]) * S + (e & 0xffffff);
            const float ze = live_z[at];
            wv = live_w[at];
            if constexpr (ZCOMP) zv = coarse_depth(rc[7], L::FAR >= 0 ? ldsf[L::FAR + slot] : rc[16], __float_as_int(ze), S, lindisp);
            else zv = ze;
        }
    };
    auto load_view = [&](int slot, float (&V)[HALF_C]) NVSR_INL {
        const f32x4* vp = reinterpret_cast<const f32x4*>(views + ((long)blk * RAYS2 + slot) * POINT_VIEW_FLOATS + HALF_C * (lane0 >> 5));
#pragma unroll
        for (int i = 0; i < HALF_C / 4; ++i) { const f32x4 v = vp[i]; V[4 * i] = v[0]; V[4 * i + 1] = v[1]; V[4 * i + 2] = v[2]; V[4 * i + 3] = v[3]; }
    };
    if constexpr (POINTS) {
        static_assert(!R3_BOUNCE, "the points' LDS region is the f16 kernels' bounce slot");
        trip = __builtin_amdgcn_readfirstlane(pt_steps[blk]);
        __syncthreads();                              // the ray cache, written by lanes 0..31 and read by all 64
    } else if constexpr (COLOUR || KEPT) {
        __shared__ int trip_s[NW2];                   // (the colour kernels' and the kept density kernels' alone: the other phases declare nothing)
        int m = max(nX, nY);
#pragma unroll
        for (int o = 16; o >= 1; o >>= 1) m = max(m, __shfl_xor(m, o));
        if (lane0 == 0) trip_s[rs.wave] = m;
        __syncthreads();                              // the wave maxima; also the ray cache, written by lanes 0..31 and read by all 64
        trip = __builtin_amdgcn_readfirstlane(max(max(trip_s[0], trip_s[1]), max(trip_s[2], trip_s[3])));
        if constexpr (KEPT) {
            const int* kX = kept_row(rayX);
            const int* kY = kept_row(rayY);
            actX = nX > 0; actY = nY > 0;
            idxX = kept_at(kX, 0, 0); idxY = kept_at(kY, 0, 0);
            idxXn = kept_at(kX, 1, idxX); idxYn = kept_at(kY, 1, idxY);
            X.zc = depth_of(z_row(rayX), rcX, idxX); Y.zc = depth_of(z_row(rayY), rcY, idxY);
        } else {
            X.zc = live_depth(lzX, rcX, nX, 0); Y.zc = live_depth(lzY, rcY, nY, 0);
            wX = live_weight(lwX, nX, 0); wY = live_weight(lwY, nY, 0);
        }
    } else {
        if constexpr (ZCOMP) __syncthreads();         // (the ray cache is written by lanes 0..31 and read by all 64, see below)
        X.zc = depth_of(zX, rcX, 0); Y.zc = depth_of(zY, rcY, 0);
    }
    RawTaps4 rt;
    RawTaps2 r2;      // (density pass)

    auto point_norm = [&](const float* rc, float zc, float& n0, float& n1, float& n2) NVSR_INL {
        const f32x4 c0 = reinterpret_cast<const f32x4*>(rc)[0], c1 = reinterpret_cast<const f32x4*>(rc)[1];
        n0 = norm_coord(__fadd_rn(c0[0], __fmul_rn(c0[3], zc)), sc.lo[0], sc.range[0]);
        n1 = norm_coord(__fadd_rn(c0[1], __fmul_rn(c1[0], zc)), sc.lo[1], sc.range[1]);
        n2 = norm_coord(__fadd_rn(c0[2], __fmul_rn(c1[1], zc)), sc.lo[2], sc.range[2]);
    };
    // f16 limbs: features carry the activation scale 2^F16_SX, put on the four blend weights (exact; D = (F0 + F1 + F2) / 3 inherits it)
    auto scale_taps = [](Taps& t) NVSR_INL {
        if constexpr (F16) { t.nw *= F16_X_SCALE; t.ne *= F16_X_SCALE; t.sw *= F16_X_SCALE; t.se *= F16_X_SCALE; }
    };
    auto view_job = [&](const float* rtp) NVSR_INL {
        const f32x4 c2 = reinterpret_cast<const f32x4*>(rtp)[0], c3 = reinterpret_cast<const f32x4*>(rtp)[1];
        GatherJob j;
        j.plane = sc.plane[3];
        j.t.o00 = __float_as_int(c2[0]); j.t.o01 = __float_as_int(c2[1]); j.t.o10 = __float_as_int(c2[2]); j.t.o11 = __float_as_int(c2[3]);
        j.t.nw = c3[0]; j.t.ne = c3[1]; j.t.sw = c3[2]; j.t.se = c3[3];
        scale_taps(j.t);
        return j;
    };

    __syncthreads();   // the ray cache is written by lanes 0..31 and read by all 64: without a barrier hipcc moves the reads of the upper
                       // half above the writes (per lane there is no dependence)
    // The view-plane features (project_viewdir, models.py:312-326) depend on the ray only: gathered once.  They open every sample's rgb
    // layer 0, so that the first plane gathers of a sample have two blocks to land in.
    if constexpr (!DENSITY) {
#pragma unroll
        for (int k2 = 0; k2 < 2; ++k2) {
            Tile3& t = k2 ? Y : X;
            const GatherJob vj = view_job(k2 ? rtY : rtX);
#pragma unroll
            for (int k = 0; k < 12; ++k) gather4_load(k, vj, lane0 >> 5, rt);
#pragma unroll
            for (int c = 0; c < HALF_C; ++c) gather4_blend(c, vj, rt, t.V);
        }
        if constexpr (POINTS) {
            // the slots' view features -> the table; the sums, the slots' rays; then the first two steps' entries and the first step's point
#pragma unroll
            for (int k2 = 0; k2 < 2; ++k2) {
                const Tile3& t = k2 ? Y : X;
                f32x4* vp = reinterpret_cast<f32x4*>(views + ((long)blk * RAYS2 + (k2 ? ownY : ownX)) * POINT_VIEW_FLOATS + HALF_C * (lane0 >> 5));
#pragma unroll
                for (int i = 0; i < HALF_C / 4; ++i) vp[i] = f32x4{t.V[4 * i], t.V[4 * i + 1], t.V[4 * i + 2], t.V[4 * i + 3]};
            }
            __syncthreads();                          // (f16 limbs: the taps, read above, lie where the sums go)
            if (lane0 < 32) {
#pragma unroll
                for (int c = 0; c < 3; ++c) pt_sums[ownX * 3 + c] = pt_sums[ownY * 3 + c] = 0.0f;
                pt_ray[ownX] = (int)(rayX - pt_block); pt_ray[ownY] = (int)(rayY - pt_block);
            }
            __syncthreads();                          // pt_ray and the table (global memory written by other waves of the workgroup)
            const int eX0 = trip > 0 ? peX[0] : POINT_NONE, eY0 = trip > 0 ? peX[32] : POINT_NONE;
            eX1 = trip > 1 ? peX[RAYS2] : POINT_NONE; eY1 = trip > 1 ? peX[RAYS2 + 32] : POINT_NONE;
            point_of(eX0, ownX, slotX, liveX, X.zc, wX);
            point_of(eY0, ownY, slotY, liveY, Y.zc, wY);
            load_view(slotX, X.V); load_view(slotY, Y.V);
        }
    } else {
        // density pass: D of sample 0 (every later sample's is gathered during the sample before it) -- the operations of the rolling gather
#pragma unroll
        for (int k2 = 0; k2 < 2; ++k2) {
            Tile3& t = k2 ? Y : X;
            float n0, n1, n2;
            point_norm(k2 ? rcY : rcX, t.zc, n0, n1, n2);
#pragma unroll
            for (int p = 0; p < 3; ++p) {
                GatherJob pj;
                pj.plane = sc.plane[p]; pj.t = pos_taps2(sc, p, n0, n1, n2); scale_taps(pj.t);
#pragma unroll
                for (int k = 0; k < 12; ++k) gather4_load(k, pj, lane0 >> 5, rt);
#pragma unroll
                for (int c = 0; c < HALF_C; ++c) gather4_blend(c, pj, rt, t.F);
#pragma unroll
                for (int c = 0; c < HALF_C; ++c) {
                    t.D[c] = p == 0 ? t.F[c] : p == 1 ? __fadd_rn(t.D[c], t.F[c]) : div3(__fadd_rn(t.D[c], t.F[c]));
                    asm volatile("" : "+v"(t.D[c]));
                }
                __builtin_amdgcn_sched_barrier(0);      // (one plane at a time: the scheduler would issue all six gathers' 144 loads first)
            }
        }
    }
    // one limb: a head that overflowed is NaN, like an accumulator (relu_bias_step): no +-inf leaves the decoder
    auto head_out = [](float v) NVSR_INL { if constexpr (LIMBS == 1) return fabsf(v) == __builtin_inff() ? __builtin_nanf("") : v; else return v; };
    Limbs<LIMBS> cur, fa;
    f32x2_t nsc = {-F16_ACC_UNSCALE, -F16_ACC_UNSCALE};                  // relu_bias_step
    asm volatile("" : "+s"(nsc));
#if R3_STAMP
    float stamp[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long tprev = __builtin_amdgcn_s_memtime();
#endif
    constexpr bool RESIDENT = L::RES_KB > 0 && !DENSITY;
    // density pass, two f16 limbs (Lds3, "the density kernels' view"): K-blocks KB_DEN0 .. KB_DEN0 + 8 resident, the step's first ring chunk is
    // the last 2 K-blocks of layer 1; otherwise the density pass streams KB_DEN0 .. through the ring and keeps nothing resident
    constexpr bool DRES = DENSITY && L::DEN_RES_KB > 0;
    static_assert(!DRES || L::DEN_RES_KB == 9, "the split of layer 1 chunk b below is written for 3 + 4 + 2 resident K-blocks");
    constexpr int KB_FIRST = DRES ? KB_DEN0 + L::DEN_RES_KB : DENSITY ? KB_DEN0 : RESIDENT ? KB_RGB0 + 9 : KB_RGB0;      // the first chunk of a step that goes through the ring
    constexpr int NKB_FIRST = DRES ? KB_DEN1 + 8 - KB_FIRST : 3;
    unsigned* const res = lds + L::RES;
    if constexpr (RESIDENT) ring3_load_resident<LIMBS, L::RES_KB>(rs, res, KB_RGB0);
    if constexpr (DRES) ring3_load_resident<LIMBS, L::DEN_RES_KB>(rs, res, KB_DEN0);
    unsigned* cw = const_cast<unsigned*>(ring3_issue<LIMBS, NKB_FIRST>(rs, KB_FIRST));     // first ring chunk of sample 0; every later one is issued during the previous sample
    // DRES: the first blocks of a step read the resident region and stand behind no ring wait, so the launch's first wait is here -- younger
    // than the region's last piece: the NKB_FIRST * LIMBS = 4 pieces per wave of the chunk just issued, which stay in flight
    if constexpr (DRES) ring3_sync<NKB_FIRST * LIMBS>();
    const int steps = COLOUR || KEPT ? trip : S;
    for (int s = 0; s < steps; ++s) {
        asm volatile("" : "+v"(rs.voff), "+v"(rs.lane));
#if R3_NO_VIEW_HOIST
        if constexpr (!POINTS) {
        // The view features are loop-invariant and so are their limbs: hipcc hoists the two split_feat(V) of a step out of the sample loop
        // (72 registers of limbs), runs out of registers and spills 8 of them plus the two depth-row pointers -- 4 scratch reloads per
        // sample, each behind an s_waitcnt vmcnt(0) that also waits for every gather and weight copy in flight.  Opaque per iteration.
#pragma unroll
        for (int c = 0; c < HALF_C; ++c) asm volatile("" : "+v"(X.V[c]), "+v"(Y.V[c]));
        }
#endif
        if constexpr (POINTS) { rcX = ldsf + L::RAYS + slotX * RAY3_FLOATS; rcY = ldsf + L::RAYS + slotY * RAY3_FLOATS; }
        const int lane = rs.lane, h = lane >> 5;
        const bool last = (s + 1 == S);
        if constexpr (!COLOUR && !KEPT) {
            X.zn = depth_of(zX, rcX, last ? s : s + 1);        // (unconditional loads unless ZCOMP: ring3_sync<2> below counts them)
            Y.zn = depth_of(zY, rcY, last ? s : s + 1);
        }
        const float nzX = !COLOUR && noise ? noise[rayX * S + s] : 0.0f;
        const float nzY = !COLOUR && noise ? noise[rayY * S + s] : 0.0f;
        float xn0, xn1, xn2, yn0, yn1, yn2;
        // (density pass: the planes gathered during this step are the NEXT sample's; after the last sample they are gathered again and dropped)
        if constexpr (!KEPT) {
            point_norm(rcX, DENSITY ? X.zn : X.zc, xn0, xn1, xn2);
            point_norm(rcY, DENSITY ? Y.zn : Y.zc, yn0, yn1, yn2);
        }
        BiasPend4 bp;
        bp.slot = bounce_slot(ldsf + L::VTAPS + rs.wave * 64 * L::TAP_FLOATS + lane * 4);     // (f16 limbs: the wave's tap region, dead since the prologue)
        HeadPend<3> hp3;
        HeadPend<1> hp1;
        SplitPend tp;

        // side-work pieces
        auto feat = [](const float (&f)[HALF_C]) NVSR_INL { return [&f](int kb, int i) NVSR_INL { return f[8 * kb + i]; }; };
        auto hid = [](const f32x16 (&a)[4], int kb0) NVSR_INL { return [&a, kb0](int kb, int i) NVSR_INL { const int k = kb0 + kb; return a[k >> 1][8 * (k & 1) + i]; }; };
        auto split_feat = [&](const float (&f)[HALF_C]) NVSR_INL { split_all<LIMBS>([&f](int i) NVSR_INL { return f[i]; }, cur); };
        // tail: split K-block kb of t.act into the limbs the next block starts with
        auto tail_of = [&](const f32x16 (&a)[4], int kb) NVSR_INL {
            return [&a, kb, &tp](int slice, Limbs<LIMBS>& nxt) NVSR_INL { split_slice<LIMBS>(slice, [&a, kb](int i) NVSR_INL { return a[kb >> 1][8 * (kb & 1) + i]; }, nxt, tp); };
        };
        auto none = [](int) NVSR_INL {};

        // ---- rgb layer 0: (view plane, planes 0..2) x (X block, Y block).  The gathers roll through the blocks (gather_roll): the block that
        // multiplies plane p - 1 of a tile loads plane p of the same tile, the next block blends it.
        GatherJob ja, jb;
        R3_MARK(0)      // loop top
        // the step's first ring chunk (issued during the previous sample) -- younger: the two z loads above.  DRES: no wait here -- density
        // layer 0 and layer 1 chunk a multiply out of the resident region; the step's first chunk is waited for inside layer 1
        if constexpr (!DRES) ring3_sync<(ZCOMP || COLOUR || KEPT) ? 0 : 2>();
        int eX2 = POINT_NONE, eY2 = POINT_NONE;
        if constexpr (POINTS) {
            // the entries of the step after the next, and the next step's point: both a whole step ahead of their use
            if (s + 2 < steps) { eX2 = peX[(s + 2) * RAYS2]; eY2 = peX[(s + 2) * RAYS2 + 32]; }
            point_of(eX1, ownX, slotXn, liveXn, X.zn, wXn);
            point_of(eY1, ownY, slotYn, liveYn, Y.zn, wYn);
        } else if constexpr (COLOUR) {
            // the next live entry, a whole step ahead of its use (issued behind the wait: no ring wait has to count these loads)
            X.zn = live_depth(lzX, rcX, nX, s + 1); Y.zn = live_depth(lzY, rcY, nY, s + 1);
            wXn = live_weight(lwX, nX, s + 1); wYn = live_weight(lwY, nY, s + 1);
        } else if constexpr (KEPT) {
            // behind the wait, like the colour pass's: the next sample's depth (its gathers roll through this step)
            X.zn = depth_of(z_row(rayX), rcX, idxXn); Y.zn = depth_of(z_row(rayY), rcY, idxYn);
            point_norm(rcX, X.zn, xn0, xn1, xn2);
            point_norm(rcY, Y.zn, yn0, yn1, yn2);
        }
        // RESIDENT (f16 limbs): view plane, planes 0 and 1 multiply out of the resident region; the ring chunk that has just landed is plane 2's,
        // and the blocks that issue gathers (B0 .. B5) issue no weight copy and need no ring wait
        unsigned* nw = (RESIDENT || DENSITY) ? nullptr : ring3_take(rs);
        float hx[3] = {0.0f, 0.0f, 0.0f};
        if constexpr (!DENSITY) {
        const unsigned* const w_view = RESIDENT ? res : cw;
        R3_MARK(1)      // first ring wait
        R3_RESET
#define NVSR_ROLL(TL, JL, TB, JB, LOADS, BLENDS) [&](int slot) NVSR_INL { gather_roll<NSF, LOADS, BLENDS, F16 && R3_BLEND_PK>(slot, JL, TL.F, JB, TB.F, h, rt); }
#define NVSR_ROLL_DMA(TL, JL, TB, JB, LOADS, BLENDS, NKB, KB0) \
        [&](int slot) NVSR_INL { gather_roll<NSF, LOADS, BLENDS, F16 && R3_BLEND_PK>(slot, JL, TL.F, JB, TB.F, h, rt); dma_side<LIMBS, NKB>(slot, rs, nw, KB0); }
        // X view | loads X plane 0
        ja.plane = sc.plane[0]; ja.t = pos_taps2(sc, 0, xn0, xn1, xn2); scale_taps(ja.t);
        split_feat(X.V);
        if constexpr (RESIDENT) limb_block<LIMBS, 3, true, true>(w_view, lane, X.acc, cur, fa, feat(X.V), NVSR_ROLL(X, ja, Y, jb, true, false), NoTail{});
        else limb_block<LIMBS, 3, true, true>(cw, lane, X.acc, cur, fa, feat(X.V), NVSR_ROLL_DMA(X, ja, Y, jb, true, false, 3, KB_RGB0 + 3), NoTail{});
        R3_MARKB(0)
        if constexpr (POINTS) load_view(slotXn, X.V);           // (X.V is dead from here: the next step's, a step ahead)
        // Y view | blends X plane 0, loads Y plane 0
        jb.plane = sc.plane[0]; jb.t = pos_taps2(sc, 0, yn0, yn1, yn2); scale_taps(jb.t);
        split_feat(Y.V);
        limb_block<LIMBS, 3, true, false>(w_view, lane, Y.acc, cur, fa, feat(Y.V), NVSR_ROLL(Y, jb, X, ja, true, true), NoTail{});
        R3_MARKB(1)
        if constexpr (POINTS) load_view(slotYn, Y.V);
        const unsigned* w_p0 = res + 3 * kb_words(LIMBS);
        if constexpr (!RESIDENT) {
            cw = nw;
            ring3_sync<YOUNGER_THAN_CHUNK>();
            nw = ring3_take(rs);
            w_p0 = cw;
        }
        // X plane 0 | blends Y plane 0, loads X plane 1
#pragma unroll
        for (int c = 0; c < HALF_C; ++c) X.D[c] = X.F[c];
        ja.plane = sc.plane[1]; ja.t = pos_taps2(sc, 1, xn0, xn1, xn2); scale_taps(ja.t);
        split_feat(X.F);
        if constexpr (RESIDENT) limb_block<LIMBS, 3, false, true>(w_p0, lane, X.acc, cur, fa, feat(X.F), NVSR_ROLL(X, ja, Y, jb, true, true), NoTail{});
        else limb_block<LIMBS, 3, false, true>(cw, lane, X.acc, cur, fa, feat(X.F), NVSR_ROLL_DMA(X, ja, Y, jb, true, true, 3, KB_RGB0 + 6), NoTail{});
        R3_MARKB(2)
        // Y plane 0 | blends X plane 1, loads Y plane 1
#pragma unroll
        for (int c = 0; c < HALF_C; ++c) Y.D[c] = Y.F[c];
        jb.plane = sc.plane[1]; jb.t = pos_taps2(sc, 1, yn0, yn1, yn2); scale_taps(jb.t);
        split_feat(Y.F);
        limb_block<LIMBS, 3, false, false>(w_p0, lane, Y.acc, cur, fa, feat(Y.F), NVSR_ROLL(Y, jb, X, ja, true, true), NoTail{});
        R3_MARKB(3)
        const unsigned* w_p1 = res + 6 * kb_words(LIMBS);
        if constexpr (!RESIDENT) {
            cw = nw;
            ring3_sync<YOUNGER_THAN_CHUNK>();
            nw = ring3_take(rs);
            w_p1 = cw;
        }
        // X plane 1 | blends Y plane 1, loads X plane 2
#pragma unroll
        for (int c = 0; c < HALF_C; ++c) X.D[c] = __fadd_rn(X.D[c], X.F[c]);
        ja.plane = sc.plane[2]; ja.t = pos_taps2(sc, 2, xn0, xn1, xn2); scale_taps(ja.t);
        split_feat(X.F);
        if constexpr (RESIDENT) limb_block<LIMBS, 3, false, true>(w_p1, lane, X.acc, cur, fa, feat(X.F), NVSR_ROLL(X, ja, Y, jb, true, true), NoTail{});
        else limb_block<LIMBS, 3, false, true>(cw, lane, X.acc, cur, fa, feat(X.F), NVSR_ROLL_DMA(X, ja, Y, jb, true, true, 3, KB_RGB0 + 9), NoTail{});
        R3_MARKB(4)
        // Y plane 1 | blends X plane 2, loads Y plane 2
#pragma unroll
        for (int c = 0; c < HALF_C; ++c) Y.D[c] = __fadd_rn(Y.D[c], Y.F[c]);
        jb.plane = sc.plane[2]; jb.t = pos_taps2(sc, 2, yn0, yn1, yn2); scale_taps(jb.t);
        split_feat(Y.F);
        limb_block<LIMBS, 3, false, false>(w_p1, lane, Y.acc, cur, fa, feat(Y.F), NVSR_ROLL(Y, jb, X, ja, true, true), NoTail{});
        R3_MARKB(5)
        if constexpr (!RESIDENT) {
            cw = nw;
            ring3_sync<YOUNGER_THAN_CHUNK>();
        }
        nw = ring3_take(rs);                                     // (RESIDENT: cw is plane 2's chunk since the top of the step)
        // X plane 2 | blends Y plane 2;  D = (D + F) / 3   (combine_pos_planes 'avg', models.py:358-359)
#pragma unroll
        for (int c = 0; c < HALF_C; ++c) X.D[c] = div3(__fadd_rn(X.D[c], X.F[c]));
        split_feat(X.F);
        limb_block<LIMBS, 3, false, true>(cw, lane, X.acc, cur, fa, feat(X.F), NVSR_ROLL_DMA(X, ja, Y, jb, false, true, 4, KB_RGB1), NoTail{});
        R3_MARKB(6)
        // Y plane 2 | X: act = max(acc + bias, 0); tail: limbs of X's K-block 0
#pragma unroll
        for (int c = 0; c < HALF_C; ++c) Y.D[c] = div3(__fadd_rn(Y.D[c], Y.F[c]));
        split_feat(Y.F);
        limb_block<LIMBS, 3, false, false>(cw, lane, Y.acc, cur, fa, feat(Y.F),
                                           [&](int slot) NVSR_INL { spread<RELU_STEPS, 0, NSF>(slot, [&](int k) NVSR_INL { relu_bias_step<LIMBS>(k, small + S_BIAS + 4 * HID, h, X.acc, X.act, bp, nsc); }); },
                                           tail_of(X.act, 0));
        R3_MARKB(7)
        cw = nw;
        R3_MARK(2)      // rgb layer 0
        }

        // ---- hidden layers.  Layer l of a decoder = chunks a (K-blocks 0..3), b (4..7):
        //   X a | Y: act of layer l-1; tail Y kb 0        Y a | tail X kb 4        X b | tail Y kb 4        Y b | X: act of layer l; tail X kb 0
        auto relu_side = [&](Tile3& t, int bias_vec) NVSR_INL {
            return [&, bias_vec](int slot) NVSR_INL { spread<RELU_STEPS, 0, NSH>(slot, [&](int k) NVSR_INL { relu_bias_step<LIMBS>(k, small + S_BIAS + bias_vec * HID, h, t.acc, t.act, bp, nsc); }); };
        };
        // hidden layer with bias vectors: vprev (layer l-1, finishing Y) and vthis (layer l, finishing X); kbn = next chunk to issue (two per layer)
#define NVSR_HIDDEN_LAYER_(SYNC, XA_SIDE, VPREV, VTHIS, KB_NEXT_A, NKB_A, KB_NEXT_B, NKB_B, X_B_SIDE)                                \
        R3_RESETH                                                                                                                   \
        SYNC;                                                                                                                       \
        R3_MARKH(0)                                                                                                                 \
        nw = ring3_take(rs);                                                                                                        \
        R3_MARKH(1)                                                                                                                 \
        limb_block<LIMBS, 4, true, true>(cw, lane, X.acc, cur, fa, hid(X.act, 0),                                                   \
                                         [&](int slot) NVSR_INL { (XA_SIDE)(slot); dma_side<LIMBS, NKB_A>(slot, rs, nw, KB_NEXT_A); }, tail_of(Y.act, 0)); \
        R3_MARKH(2)                                                                                                                 \
        limb_block<LIMBS, 4, true, false>(cw, lane, Y.acc, cur, fa, hid(Y.act, 0), none, tail_of(X.act, 4));                        \
        R3_MARKH(3)                                                                                                                 \
        cw = nw;                                                                                                                    \
        ring3_sync<0>();                                                                                                               \
        nw = ring3_take(rs);                                                                                                        \
        R3_MARKH(4)                                                                                                                 \
        limb_block<LIMBS, 4, false, true>(cw, lane, X.acc, cur, fa, hid(X.act, 4),                                                  \
                                          [&](int slot) NVSR_INL { dma_side<LIMBS, NKB_B>(slot, rs, nw, KB_NEXT_B); }, tail_of(Y.act, 4));   \
        R3_MARKH(5)                                                                                                                 \
        X_B_SIDE;                                                                                                                   \
        R3_MARKH(6)                                                                                                                 \
        cw = nw;

#define NVSR_HIDDEN_LAYER(VPREV, ...) NVSR_HIDDEN_LAYER_(ring3_sync<0>(), relu_side(Y, VPREV), VPREV, __VA_ARGS__)
        // rgb layers 1, 2: Y b | X relu, tail X kb 0
#define NVSR_YB_PLAIN(VTHIS) (limb_block<LIMBS, 4, false, false>(cw, lane, Y.acc, cur, fa, hid(Y.act, 4), relu_side(X, VTHIS), tail_of(X.act, 0)))
        if constexpr (!DENSITY) {
        NVSR_HIDDEN_LAYER(4, 5, KB_RGB1 + 4, 4, KB_RGB1 + 8, 4, NVSR_YB_PLAIN(5))
        NVSR_HIDDEN_LAYER(5, 6, KB_RGB1 + 12, 4, KB_RGB1 + 16, 4, NVSR_YB_PLAIN(6))
        // rgb layer 3: Y b | X relu (no tail: X continues with the density decoder from X.D).  The chunk issued last is the density decoder's
        // first -- colour pass: chunk 0 of the NEXT step, and X's rgb heads follow its activation in the second half of the block
        NVSR_HIDDEN_LAYER(6, 7, KB_RGB1 + 20, 4, (COLOUR ? KB_FIRST : KB_DEN0), 3,
                          (limb_block<LIMBS, 4, false, false>(cw, lane, Y.acc, cur, fa, hid(Y.act, 4),
                                                              [&](int slot) NVSR_INL {
                                                                  if constexpr (COLOUR) {
                                                                      spread<RELU_STEPS, 0, NSH / 2>(slot, [&](int k) NVSR_INL { relu_bias_step<LIMBS>(k, small + S_BIAS + 7 * HID, h, X.acc, X.act, bp, nsc); });
                                                                      spread<64, NSH / 2, NSH>(slot, [&](int k) NVSR_INL { heads_side<3>(k >> 2, k & 3, small + S_RGB_W, h, X.act, hx, hp3); });
                                                                  } else relu_side(X, 7)(slot);
                                                              },
                                                              NoTail{})))
        }

        R3_MARK(3)      // rgb layers 1..3
        if constexpr (FUSED) {
        // ---- density layer 0 (from D) -------------------------------------------------------------------------------------------
        ring3_sync<0>();
        nw = ring3_take(rs);
        // X density 0 | Y: act of rgb layer 3; X: rgb heads
        split_feat(X.D);
        limb_block<LIMBS, 3, true, true>(cw, lane, X.acc, cur, fa, feat(X.D),
                                         [&](int slot) NVSR_INL {
                                             spread<RELU_STEPS, 0, NSF>(slot, [&](int k) NVSR_INL { relu_bias_step<LIMBS>(k, small + S_BIAS + 7 * HID, h, Y.acc, Y.act, bp, nsc); });
                                             spread<64, 0, NSF>(slot, [&](int k) NVSR_INL { heads_side<3>(k >> 2, k & 3, small + S_RGB_W, h, X.act, hx, hp3); });
                                             dma_side<LIMBS, 4>(slot, rs, nw, KB_DEN1);
                                         },
                                         NoTail{});
#pragma unroll
        for (int c = 0; c < 3; ++c) X.raw[c] = head_out((hx[c] + __shfl_xor(hx[c], 32)) + small[S_HEAD_B + 1 + c]);
        // Y density 0 | Y: rgb heads, then X: act of density layer 0; tail X kb 0
        float hy[3] = {0.0f, 0.0f, 0.0f};
        split_feat(Y.D);
        limb_block<LIMBS, 3, true, false>(cw, lane, Y.acc, cur, fa, feat(Y.D),
                                          [&](int slot) NVSR_INL {
                                              spread<64, 0, NSF>(slot, [&](int k) NVSR_INL { heads_side<3>(k >> 2, k & 3, small + S_RGB_W, h, Y.act, hy, hp3); });
                                              spread<RELU_STEPS, 0, NSF>(slot, [&](int k) NVSR_INL { relu_bias_step<LIMBS>(k, small + S_BIAS + 0 * HID, h, X.acc, X.act, bp, nsc); });
                                          },
                                          tail_of(X.act, 0));
#pragma unroll
        for (int c = 0; c < 3; ++c) Y.raw[c] = head_out((hy[c] + __shfl_xor(hy[c], 32)) + small[S_HEAD_B + 1 + c]);
        cw = nw;

        R3_MARK(4)      // density layer 0
        // ---- density layers 1..3 -------------------------------------------------------------------------------------------------
        NVSR_HIDDEN_LAYER(0, 1, KB_DEN1 + 4, 4, KB_DEN1 + 8, 4, NVSR_YB_PLAIN(1))
        NVSR_HIDDEN_LAYER(1, 2, KB_DEN1 + 12, 4, KB_DEN1 + 16, 4, NVSR_YB_PLAIN(2))
        } else if constexpr (DENSITY) {
        // ---- density pass: the whole density decoder, with the NEXT sample's six plane gathers (X planes 0..2, then Y planes 0..2) rolling
        // through its blocks in halves (gather_half, pair_core.h: two tap buffers and ONE blend buffer -- both tiles' activations are live
        // beside them): block i = 0..11 loads half i, block i + 1 blends it; a plane is complete behind every second block and goes into D
        // there, in the order (F0 + F1) + F2, then div3.  A ring chunk is issued in the first half of an X block and waited for behind the Y
        // block that follows it, whose 12 gather loads are younger than the chunk's last piece (ring3_sync<12>; the X block's own loads are
        // blended by then).
        // DRES (two f16 limbs): layer 0, layer 1 chunk a and half of chunk b read the resident region -- no copy, no slot, no wait; the
        // step's ring chunks are layer 1 K-blocks 6, 7 | 2 a | 2 b | 3 a | 3 b, five per step, so the two slots swap roles every step as
        // they did with seven.
        float (&Fg)[HALF_C] = X.F;
#define NVSR_HALF(JL, HL, JB, HB, LOADS, BLENDS, NS_) gather_half<NS_, LOADS, HL, BLENDS, HB>(slot, JL, JB, Fg, h, r2)
#define NVSR_JOB(J, P, N0, N1, N2) J.plane = sc.plane[P]; J.t = pos_taps2(sc, P, N0, N1, N2); scale_taps(J.t);
        // density layer 0 (DRES: out of the resident region -- no ring slot, no copy)
        const unsigned* const w_d0 = DRES ? res : cw;
        if constexpr (!DRES) nw = ring3_take(rs);
        NVSR_JOB(ja, 0, xn0, xn1, xn2)
        split_feat(X.D);
        limb_block<LIMBS, 3, true, true>(w_d0, lane, X.acc, cur, fa, feat(X.D),
                                         [&](int slot) NVSR_INL {
                                             NVSR_HALF(ja, 0, ja, 0, true, false, NSF);
                                             if constexpr (!DRES) dma_side<LIMBS, 4>(slot, rs, nw, KB_DEN1);
                                         },
                                         NoTail{});
        split_feat(Y.D);
        limb_block<LIMBS, 3, true, false>(w_d0, lane, Y.acc, cur, fa, feat(Y.D),
                                          [&](int slot) NVSR_INL {
                                              spread<RELU_STEPS, 0, NSF>(slot, [&](int k) NVSR_INL { relu_bias_step<LIMBS>(k, small + S_BIAS + 0 * HID, h, X.acc, X.act, bp, nsc); });
                                              NVSR_HALF(ja, 1, ja, 0, true, true, NSF);
                                          },
                                          tail_of(X.act, 0));
        if constexpr (!DRES) cw = nw;
        // one hidden layer: X a | Y a | X b | Y b, each with the gather halves (JL, HL) it loads and (JB, HB) it blends, and the statements
        // (D updates, the next job's taps) that go in front of it
#define NVSR_DEN_LAYER(VPREV, KB_NEXT_A, KB_NEXT_B, NKB_B, PRE_XA, G_XA, PRE_YA, G_YA, PRE_XB, G_XB, PRE_YB, YB_SIDE, YB_TAIL)                      \
        ring3_sync<12>();                                                                                                           \
        nw = ring3_take(rs);                                                                                                        \
        PRE_XA                                                                                                                      \
        limb_block<LIMBS, 4, true, true>(cw, lane, X.acc, cur, fa, hid(X.act, 0),                                                   \
                                         [&](int slot) NVSR_INL { relu_side(Y, VPREV)(slot); G_XA; dma_side<LIMBS, 4>(slot, rs, nw, KB_NEXT_A); }, tail_of(Y.act, 0)); \
        PRE_YA                                                                                                                      \
        limb_block<LIMBS, 4, true, false>(cw, lane, Y.acc, cur, fa, hid(Y.act, 0), [&](int slot) NVSR_INL { G_YA; }, tail_of(X.act, 4)); \
        cw = nw;                                                                                                                    \
        ring3_sync<12>();                                                                                                           \
        nw = ring3_take(rs);                                                                                                        \
        PRE_XB                                                                                                                      \
        limb_block<LIMBS, 4, false, true>(cw, lane, X.acc, cur, fa, hid(X.act, 4),                                                  \
                                          [&](int slot) NVSR_INL { G_XB; dma_side<LIMBS, NKB_B>(slot, rs, nw, KB_NEXT_B); }, tail_of(Y.act, 4)); \
        PRE_YB                                                                                                                      \
        limb_block<LIMBS, 4, false, false>(cw, lane, Y.acc, cur, fa, hid(Y.act, 4), [&](int slot) NVSR_INL { YB_SIDE; }, YB_TAIL);     \
        cw = nw;
        // (D is read by the NEXT iteration only: without the opaque statement the compiler sinks every blend and D update of the step into the
        //  loop's last basic block, behind the list stores, and keeps all 144 tap registers of the step alive until there -- in scratch)
#define NVSR_D_SET(T) _Pragma("unroll") for (int c = 0; c < HALF_C; ++c) { T.D[c] = Fg[c]; asm volatile("" : "+v"(T.D[c])); }
#define NVSR_D_ADD(T) _Pragma("unroll") for (int c = 0; c < HALF_C; ++c) { T.D[c] = __fadd_rn(T.D[c], Fg[c]); asm volatile("" : "+v"(T.D[c])); }
#define NVSR_D_AVG(T) _Pragma("unroll") for (int c = 0; c < HALF_C; ++c) { T.D[c] = div3(__fadd_rn(T.D[c], Fg[c])); asm volatile("" : "+v"(T.D[c])); }
        // density layer 1: X p0 -> D, X p1, X p2 (first half)
        if constexpr (DRES) {
            // The same blocks, products and side work in the same order; only where the fragments are read from changes.  Chunk a is
            // resident.  Chunk b is cut behind its second K-block: X b = [K-blocks 4, 5: resident | 6, 7: the ring chunk], then Y b
            // likewise -- two limb_blocks of 2 K-blocks each, the side work of slots 0 .. NSH/2 - 1 in the first and NSH/2 .. NSH - 1
            // in the second, the tail of the first splitting the second's first K-block (what the undivided block did in its own
            // K-block 1).  Every accumulator sees K-blocks 0 .. 7 in order, as before.
            const unsigned* const w_1a = res + 3 * kb_words(LIMBS);
            const unsigned* const w_1b = res + 7 * kb_words(LIMBS);
            NVSR_JOB(jb, 1, xn0, xn1, xn2)
            limb_block<LIMBS, 4, true, true>(w_1a, lane, X.acc, cur, fa, hid(X.act, 0),
                                             [&](int slot) NVSR_INL { relu_side(Y, 0)(slot); NVSR_HALF(jb, 0, ja, 1, true, true, NSH); }, tail_of(Y.act, 0));
            NVSR_D_SET(X)
            limb_block<LIMBS, 4, true, false>(w_1a, lane, Y.acc, cur, fa, hid(Y.act, 0), [&](int slot) NVSR_INL { NVSR_HALF(jb, 1, jb, 0, true, true, NSH); },
                                              tail_of(X.act, 4));
            NVSR_JOB(ja, 2, xn0, xn1, xn2)
            limb_block<LIMBS, 2, false, true>(w_1b, lane, X.acc, cur, fa, hid(X.act, 4), [&](int slot) NVSR_INL { NVSR_HALF(ja, 0, jb, 1, true, true, NSH); },
                                              tail_of(X.act, 6));
            // The step's first ring chunk (layer 1, K-blocks 6 and 7), issued in X b of layer 3 of the previous sample (before the loop for
            // sample 0).  Vector-memory operations issued behind its last piece and certain to exist: the 12 gather loads each of X and Y
            // density layer 0 and of X a and Y a above = 48 (the half-block just done blends and loads nothing).  Older than those 48 and
            // not counted: the previous epilogue's loads and stores and this step's depth and noise loads, whose number varies with the
            // launch -- all consumed or drained by the time the first of the 48 is waited for, so leaving them out costs no stall.
            ring3_sync<48>();
            nw = ring3_take(rs);
            limb_block<LIMBS, 2, false, true>(cw, lane, X.acc, cur, fa, hid(X.act, 6),
                                              [&](int sl) NVSR_INL {
                                                  const int slot = sl + NSH / 2;
                                                  NVSR_HALF(ja, 0, jb, 1, true, true, NSH);
                                                  dma_side<LIMBS, 4>(sl, rs, nw, KB_DEN1 + 8);       // 8 pieces per wave: slots 2, 5 .. 23 of the 24
                                              },
                                              tail_of(Y.act, 4));
            NVSR_D_ADD(X)
            limb_block<LIMBS, 2, false, true>(w_1b, lane, Y.acc, cur, fa, hid(Y.act, 4),
                                              [&](int slot) NVSR_INL { relu_side(X, 1)(slot); NVSR_HALF(ja, 1, ja, 0, true, true, NSH); }, tail_of(Y.act, 6));
            // (the wait in front of layer 2 keeps its 12: the copy's last piece goes out in the last slot of X b's second half, behind that
            //  half's own loads; Y b's first half loads nothing, its second half issues the 12 loads that are younger)
            limb_block<LIMBS, 2, false, true>(cw, lane, Y.acc, cur, fa, hid(Y.act, 6),
                                              [&](int sl) NVSR_INL {
                                                  const int slot = sl + NSH / 2;
                                                  relu_side(X, 1)(slot); NVSR_HALF(ja, 1, ja, 0, true, true, NSH);
                                              },
                                              tail_of(X.act, 0));
            cw = nw;
        } else {
        NVSR_DEN_LAYER(0, KB_DEN1 + 4, KB_DEN1 + 8, 4,
                       NVSR_JOB(jb, 1, xn0, xn1, xn2), NVSR_HALF(jb, 0, ja, 1, true, true, NSH),
                       NVSR_D_SET(X), NVSR_HALF(jb, 1, jb, 0, true, true, NSH),
                       NVSR_JOB(ja, 2, xn0, xn1, xn2), NVSR_HALF(ja, 0, jb, 1, true, true, NSH),
                       NVSR_D_ADD(X), relu_side(X, 1)(slot); NVSR_HALF(ja, 1, ja, 0, true, true, NSH), tail_of(X.act, 0))
        }
        // density layer 2: X p2 -> D done; Y p0, Y p1
        NVSR_DEN_LAYER(1, KB_DEN1 + 12, KB_DEN1 + 16, 4,
                       NVSR_JOB(jb, 0, yn0, yn1, yn2), NVSR_HALF(jb, 0, ja, 1, true, true, NSH),
                       NVSR_D_AVG(X), NVSR_HALF(jb, 1, jb, 0, true, true, NSH),
                       NVSR_JOB(ja, 1, yn0, yn1, yn2), NVSR_HALF(ja, 0, jb, 1, true, true, NSH),
                       NVSR_D_SET(Y), relu_side(X, 2)(slot); NVSR_HALF(ja, 1, ja, 0, true, true, NSH), tail_of(X.act, 0))
        // density layer 3: Y p2 -> D done behind X b.  The chunk issued last is chunk 0 of the NEXT sample (after the last sample: a harmless
        // copy); Y b | X: act, then the sigma head
        float sx[1] = {0.0f};
        auto sigma_side = [&](int slot) NVSR_INL {
            spread<RELU_STEPS, 0, NSH / 2>(slot, [&](int k) NVSR_INL { relu_bias_step<LIMBS>(k, small + S_BIAS + 3 * HID, h, X.acc, X.act, bp, nsc); });
            spread<64, NSH / 2, NSH>(slot, [&](int k) NVSR_INL { heads_side<1>(k >> 2, k & 3, small + S_ALPHA_W, h, X.act, sx, hp1); });
        };
        NVSR_DEN_LAYER(2, KB_DEN1 + 20, KB_FIRST, NKB_FIRST,
                       NVSR_JOB(jb, 2, yn0, yn1, yn2), NVSR_HALF(jb, 0, ja, 1, true, true, NSH),
                       NVSR_D_ADD(Y), NVSR_HALF(jb, 1, jb, 0, true, true, NSH),
                       , NVSR_HALF(jb, 1, jb, 1, false, true, NSH),
                       NVSR_D_AVG(Y), sigma_side(slot), NoTail{})
#undef NVSR_DEN_LAYER
#undef NVSR_D_SET
#undef NVSR_D_ADD
#undef NVSR_D_AVG
#undef NVSR_HALF
#undef NVSR_JOB
        X.raw[3] = head_out((sx[0] + __shfl_xor(sx[0], 32)) + small[S_HEAD_B]);
        }
        if constexpr (FUSED) {
        // density layer 3: the chunk issued last is chunk 0 of the NEXT sample (after the last sample: a harmless copy);
        // Y b | X: act, then the sigma head
        float sx[1] = {0.0f};
        NVSR_HIDDEN_LAYER(2, 3, KB_DEN1 + 20, 4, KB_FIRST, 3,
                          (limb_block<LIMBS, 4, false, false>(cw, lane, Y.acc, cur, fa, hid(Y.act, 4),
                                                              [&](int slot) NVSR_INL {
                                                                  spread<RELU_STEPS, 0, NSH / 2>(slot, [&](int k) NVSR_INL { relu_bias_step<LIMBS>(k, small + S_BIAS + 3 * HID, h, X.acc, X.act, bp, nsc); });
                                                                  spread<64, NSH / 2, NSH>(slot, [&](int k) NVSR_INL { heads_side<1>(k >> 2, k & 3, small + S_ALPHA_W, h, X.act, sx, hp1); });
                                                              },
                                                              NoTail{})))
        X.raw[3] = head_out((sx[0] + __shfl_xor(sx[0], 32)) + small[S_HEAD_B]);
        }
        R3_MARK(5)      // density layers 1..3
        if constexpr (!COLOUR) {

        // ---- epilogue (exposed): Y's last activation + sigma head, both tiles' compositing -----------------------------------------
        // kept lists: the depth of this sample's successor in the full row (its dist) and the raw entries of the next step and of the one after
        // it -- two steps ahead, so that the next step can load its depth a step ahead (waited for at the loop's top) -- are fetched here, in
        // front of Y's head, and held over the compositing only: the decoder's blocks carry the current entry alone
        float zsX = 0.0f, zsY = 0.0f;
        int e1X = 0, e1Y = 0, e2X = 0, e2Y = 0;
        const bool lastX = KEPT ? idxX + 1 == S : last, lastY = KEPT ? idxY + 1 == S : last;
        if constexpr (KEPT) {
            zsX = depth_of(z_row(rayX), rcX, lastX ? idxX : idxX + 1); zsY = depth_of(z_row(rayY), rcY, lastY ? idxY : idxY + 1);
            { const int* kX = kept_row(rayX); e1X = kX[s + 1 < S ? s + 1 : S - 1]; e2X = kX[s + 2 < S ? s + 2 : S - 1]; }
            { const int* kY = kept_row(rayY); e1Y = kY[s + 1 < S ? s + 1 : S - 1]; e2Y = kY[s + 2 < S ? s + 2 : S - 1]; }
        }
#pragma unroll
        for (int k = 0; k < RELU_STEPS; ++k) relu_bias_step<LIMBS>(k, small + S_BIAS + 3 * HID, h, Y.acc, Y.act, bp, nsc);
        {
            float hd[1];
            head_dots<1>(small + S_ALPHA_W, h, Y.act, hd);
            Y.raw[3] = head_out(hd[0] + small[S_HEAD_B]);
        }
        if (raw_out && lane < 32) {
            if (validX) *reinterpret_cast<f32x4*>(raw_out + (rayX * S + s) * 4) = f32x4{X.raw[0], X.raw[1], X.raw[2], X.raw[3]};
            if (validY) *reinterpret_cast<f32x4*>(raw_out + (rayY * S + s) * 4) = f32x4{Y.raw[0], Y.raw[1], Y.raw[2], Y.raw[3]};
        }
        if constexpr (!KEPT) actX = actY = true;
        if constexpr (KEPT) {
            // one tile at a time: the successor's depth stands in for zn during the compositing; a lane past its list keeps what it had
            {
                const float t0 = X.T, d0 = X.dep, a0 = X.ac, g0 = X.zn;
                X.zn = zsX;
                composite_weight(X, reinterpret_cast<const f32x4*>(rcX)[1][2], 0.0f, lastX);
                X.zn = g0; X.T = actX ? X.T : t0; X.dep = actX ? X.dep : d0; X.ac = actX ? X.ac : a0;
            }
            {
                const float t0 = Y.T, d0 = Y.dep, a0 = Y.ac, g0 = Y.zn;
                Y.zn = zsY;
                composite_weight(Y, reinterpret_cast<const f32x4*>(rcY)[1][2], 0.0f, lastY);
                Y.zn = g0; Y.T = actY ? Y.T : t0; Y.dep = actY ? Y.dep : d0; Y.ac = actY ? Y.ac : a0;
            }
        } else if constexpr (DENSITY) {
            composite_weight(X, reinterpret_cast<const f32x4*>(rcX)[1][2], nzX, last);
            composite_weight(Y, reinterpret_cast<const f32x4*>(rcY)[1][2], nzY, last);
        } else {
            composite_sample(X, reinterpret_cast<const f32x4*>(rcX)[1][2], nzX, last);
            composite_sample(Y, reinterpret_cast<const f32x4*>(rcY)[1][2], nzY, last);
        }
        if (weights && lane < 32) {
            if (validX && actX) weights[rayX * S + (KEPT ? idxX : s)] = X.raw[3];
            if (validY && actY) weights[rayY * S + (KEPT ? idxY : s)] = Y.raw[3];
        }
        if constexpr (DENSITY) {
            // the live list: every sample whose weight is not zero (a NaN weight is live), in sample order
            const bool liveX = actX && !(X.raw[3] == 0.0f), liveY = actY && !(Y.raw[3] == 0.0f);
            if (lane < 32) {
                if (validX && liveX) { live_z[rayX * S + cX] = ZCOMP ? __int_as_float(KEPT ? idxX : s) : X.zc; live_w[rayX * S + cX] = X.raw[3]; }
                if (validY && liveY) { live_z[rayY * S + cY] = ZCOMP ? __int_as_float(KEPT ? idxY : s) : Y.zc; live_w[rayY * S + cY] = Y.raw[3]; }
            }
            cX += liveX; cY += liveY;
            if constexpr (KEPT) {
                // the next step is the list's own iff its entry exists; behind the list's end the index stops advancing (kept_at)
                actX = validX && s + 1 < S && e1X >= 0; actY = validY && s + 1 < S && e1Y >= 0;      // (an invalid slot reads the clamped ray's row: never active)
                idxX = e1X < 0 ? idxX : e1X; idxY = e1Y < 0 ? idxY : e1Y;
                idxXn = e2X < 0 ? idxX : e2X; idxYn = e2Y < 0 ? idxY : e2Y;
            }
        }
        } else {
        // ---- colour pass epilogue (exposed): X's raw colours, Y's last activation + rgb heads, both tiles' w sigmoid(raw) ------------
#pragma unroll
        for (int c = 0; c < 3; ++c) X.raw[c] = head_out((hx[c] + __shfl_xor(hx[c], 32)) + small[S_HEAD_B + 1 + c]);
#pragma unroll
        for (int k = 0; k < RELU_STEPS; ++k) relu_bias_step<LIMBS>(k, small + S_BIAS + 7 * HID, h, Y.acc, Y.act, bp, nsc);
        {
            float hd[3];
            head_dots<3>(small + S_RGB_W, h, Y.act, hd);        // (the fmaf chain and the half-wave sum of heads_side)
#pragma unroll
            for (int c = 0; c < 3; ++c) Y.raw[c] = head_out(hd[c] + small[S_HEAD_B + 1 + c]);
        }
        if constexpr (POINTS) {
            // the step's terms and slots -> LDS; the first point of every run (position p: lane p of the workgroup) adds its run to the ray's sums
            if (lane < 32) {
#pragma unroll
                for (int c = 0; c < 3; ++c) { pt_exch[ownX * 3 + c] = colour_term(wX, X.raw[c]); pt_exch[ownY * 3 + c] = colour_term(wY, Y.raw[c]); }
                pt_slot[ownX] = liveX ? slotX : -1; pt_slot[ownY] = liveY ? slotY : -1;
            }
            __syncthreads();
            const int p = rs.wave * 64 + lane, sl = pt_slot[p];
            if (sl >= 0 && (p == 0 || pt_slot[p - 1] != sl)) {
                float a0 = pt_sums[sl * 3], a1 = pt_sums[sl * 3 + 1], a2 = pt_sums[sl * 3 + 2];
                int q = p;
                do {
                    a0 = __fadd_rn(a0, pt_exch[q * 3]); a1 = __fadd_rn(a1, pt_exch[q * 3 + 1]); a2 = __fadd_rn(a2, pt_exch[q * 3 + 2]);
                    ++q;
                } while (q < RAYS2 && pt_slot[q] == sl);
                pt_sums[sl * 3] = a0; pt_sums[sl * 3 + 1] = a1; pt_sums[sl * 3 + 2] = a2;
            }
            __syncthreads();                          // the next step's terms go where these were read; after the last step: the sums
            slotX = slotXn; slotY = slotYn; liveX = liveXn; liveY = liveYn; eX1 = eX2; eY1 = eY2;
        } else {
            composite_colour(X, wX, s < nX);
            composite_colour(Y, wY, s < nY);
        }
        wX = wXn; wY = wYn;
        }
#undef NVSR_HIDDEN_LAYER
#undef NVSR_HIDDEN_LAYER_
#undef NVSR_ROLL
#undef NVSR_ROLL_DMA
#undef NVSR_YB_PLAIN
        X.zc = X.zn; Y.zc = Y.zn;
        R3_MARK(6)      // epilogue
    }
#if R3_STAMP
    if (raw_out && rs.lane < 32 && validX) {
        for (int i = 0; i < 8; ++i) raw_out[(rayX * S + (i >> 2)) * 4 + (i & 3)] = stamp[i] / (float)S;
    }
#endif
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // the copy issued for a sample after the last one must land before the wave ends

    if constexpr (POINTS) {
        if (rs.lane < 32) {
            X.cr = pt_sums[ownX * 3]; X.cg = pt_sums[ownX * 3 + 1]; X.cb = pt_sums[ownX * 3 + 2];
            Y.cr = pt_sums[ownY * 3]; Y.cg = pt_sums[ownY * 3 + 1]; Y.cb = pt_sums[ownY * 3 + 2];
        }
    }
    if (rs.lane < 32) {
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const Tile3& t = k ? Y : X;
            const long ray = k ? rayY : rayX;
            if (!(k ? validY : validX)) continue;
            float cr = t.cr, cg = t.cg, cb = t.cb;
            const float ac = COLOUR ? acc[ray] : t.ac;          // (colour pass: the density pass wrote it)
            if constexpr (!COLOUR) {
                const float q = t.dep / t.ac;                   // NaN when acc == 0, like torch.max(1e-10, nan)
                disp[ray] = 1.0f / ((q != q) ? q : fmaxf(1e-10f, q));
                acc[ray] = t.ac;
                if (depth) depth[ray] = t.dep;
            }
            if constexpr (DENSITY) {
                live_n[ray] = k ? cY : cX;
                cr = cg = cb = 0.0f;                            // (the range flag below then looks at acc alone; the colour pass looks at rgb)
            } else {
                if (white) { const float bg = 1.0f - ac; cr += bg; cg += bg; cb += bg; }
                rgb[ray * 3 + 0] = cr; rgb[ray * 3 + 1] = cg; rgb[ray * 3 + 2] = cb;
            }
            // range flag of the f16 limbs (nvsr.h: nvsr_set_range_flag): a non-finite colour / opacity is an operand beyond the static scales
            if (F16 && flag && !(fabsf(cr + cg + cb + ac) <= 3.0e38f)) __hip_atomic_fetch_or(flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// coarse pass: also writes the per-sample compositing weights (the input of the importance resampling)
template <int LIMBS>
__global__ __launch_bounds__(TPB2, 1) void render_pass3_coarse_kernel(SceneDev sc, const float* __restrict__ packed, long N, int S,
                                                                     const float* __restrict__ rays, const float* __restrict__ z,
                                                                     const float* __restrict__ noise, int white,
                                                                     float* __restrict__ rgb, float* __restrict__ disp,
                                                                     float* __restrict__ acc, float* __restrict__ weights,
                                                                     float* __restrict__ depth, float* __restrict__ raw_out, unsigned* __restrict__ flag) {
    render_pass3_body<LIMBS>(sc, packed, N, S, rays, z, 0, noise, white, rgb, disp, acc, weights, depth, raw_out, flag);
}
// coarse pass of an inference frame: un-jittered depths computed in registers (no [N,S] depth tensor is written or read)
template <int LIMBS>
__global__ __launch_bounds__(TPB2, 1) void render_pass3_coarse_z_kernel(SceneDev sc, const float* __restrict__ packed, long N, int S,
                                                                       const float* __restrict__ rays, int lindisp,
                                                                       const float* __restrict__ noise, int white,
                                                                       float* __restrict__ rgb, float* __restrict__ disp,
                                                                       float* __restrict__ acc, float* __restrict__ weights,
                                                                       float* __restrict__ depth, float* __restrict__ raw_out, unsigned* __restrict__ flag) {
#if defined(__HIP_DEVICE_COMPILE__)      // (hipcc's host pass cannot resolve the LDS-DMA helpers inside this instantiation; it only needs the stub)
    render_pass3_body<LIMBS + 8>(sc, packed, N, S, rays, nullptr, lindisp, noise, white, rgb, disp, acc, weights, depth, raw_out, flag);
#endif
}
// fine pass (or any pass whose weights are not wanted)
template <int LIMBS>
__global__ __launch_bounds__(TPB2, 1) void render_pass3_kernel(SceneDev sc, const float* __restrict__ packed, long N, int S,
                                                              const float* __restrict__ rays, const float* __restrict__ z,
                                                              const float* __restrict__ noise, int white,
                                                              float* __restrict__ rgb, float* __restrict__ disp,
                                                              float* __restrict__ acc, float* __restrict__ depth,
                                                              float* __restrict__ raw_out, unsigned* __restrict__ flag) {
    render_pass3_body<LIMBS>(sc, packed, N, S, rays, z, 0, noise, white, rgb, disp, acc, nullptr, depth, raw_out, flag);
}

// ---- the two-phase route: density pass, then the colour decoder on the live samples (PHASE 1 and 2 of the body) ---------------------
// live_z / live_w: [N, S] rows (the first live_n[ray] entries are written), live_n: [N].  `_z`: the coarse pass of an inference frame
// (depths in registers; live_z holds sample indices).  Device pass only, like the coarse_z kernel above.
template <int LIMBS>
__global__ __launch_bounds__(TPB2, 1) void render_pass3_density_kernel(SceneDev sc, const float* __restrict__ packed, long N, int S,
                                                                      const float* __restrict__ rays, const float* __restrict__ z,
                                                                      const float* __restrict__ noise, float* __restrict__ disp,
                                                                      float* __restrict__ acc, float* __restrict__ weights,
                                                                      float* __restrict__ depth, unsigned* __restrict__ flag,
                                                                      float* __restrict__ live_z, float* __restrict__ live_w, int* __restrict__ live_n) {
#if defined(__HIP_DEVICE_COMPILE__)
    render_pass3_body<LIMBS + 16>(sc, packed, N, S, rays, z, 0, noise, 0, nullptr, disp, acc, weights, depth, nullptr, flag, live_z, live_w, live_n);
#endif
}
template <int LIMBS>
__global__ __launch_bounds__(TPB2, 1) void render_pass3_density_z_kernel(SceneDev sc, const float* __restrict__ packed, long N, int S,
                                                                        const float* __restrict__ rays, int lindisp,
                                                                        const float* __restrict__ noise, float* __restrict__ disp,
                                                                        float* __restrict__ acc, float* __restrict__ weights,
                                                                        float* __restrict__ depth, unsigned* __restrict__ flag,
                                                                        float* __restrict__ live_z, float* __restrict__ live_w, int* __restrict__ live_n) {
#if defined(__HIP_DEVICE_COMPILE__)
    render_pass3_body<LIMBS + 8 + 16>(sc, packed, N, S, rays, nullptr, lindisp, noise, 0, nullptr, disp, acc, weights, depth, nullptr, flag, live_z, live_w, live_n);
#endif
}
template <int LIMBS>
__global__ __launch_bounds__(TPB2, 1) void render_pass3_colour_kernel(SceneDev sc, const float* __restrict__ packed, long N, int S,
                                                                     const float* __restrict__ rays, int white, float* __restrict__ rgb,
                                                                     float* __restrict__ acc, unsigned* __restrict__ flag,
                                                                     float* __restrict__ live_z, float* __restrict__ live_w, int* __restrict__ live_n,
                                                                     const int* __restrict__ group_slot) {
#if defined(__HIP_DEVICE_COMPILE__)
    render_pass3_body<LIMBS + 32>(sc, packed, N, S, rays, nullptr, 0, nullptr, white, rgb, nullptr, acc, nullptr, nullptr, nullptr, flag, live_z, live_w, live_n, group_slot);
#endif
}
template <int LIMBS>
__global__ __launch_bounds__(TPB2, 1) void render_pass3_colour_z_kernel(SceneDev sc, const float* __restrict__ packed, long N, int S,
                                                                       const float* __restrict__ rays, int lindisp, int white,
                                                                       float* __restrict__ rgb, float* __restrict__ acc, unsigned* __restrict__ flag,
                                                                       float* __restrict__ live_z, float* __restrict__ live_w, int* __restrict__ live_n,
                                                                       const int* __restrict__ group_slot) {
#if defined(__HIP_DEVICE_COMPILE__)
    render_pass3_body<LIMBS + 8 + 32>(sc, packed, N, S, rays, nullptr, lindisp, nullptr, white, rgb, nullptr, acc, nullptr, nullptr, nullptr, flag, live_z, live_w, live_n, group_slot);
#endif
}

// the density pass over the kept lists of the occupancy route (PHASE 4): kept [N, S] sample indices, kept_n [N] packed entries of the ray order
// on the kept counts, group_slot: the order of dispatch on them.  No noise: the route serves evaluation.
template <int LIMBS>
__global__ __launch_bounds__(TPB2, 1) void render_pass3_density_kept_kernel(SceneDev sc, const float* __restrict__ packed, long N, int S,
                                                                           const float* __restrict__ rays, const float* __restrict__ z,
                                                                           float* __restrict__ disp, float* __restrict__ acc, float* __restrict__ weights,
                                                                           float* __restrict__ depth, unsigned* __restrict__ flag,
                                                                           float* __restrict__ live_z, float* __restrict__ live_w, int* __restrict__ live_n,
                                                                           const int* __restrict__ group_slot, const int* __restrict__ kept,
                                                                           const int* __restrict__ kept_n) {
#if defined(__HIP_DEVICE_COMPILE__)
    render_pass3_body<LIMBS + 64>(sc, packed, N, S, rays, z, 0, nullptr, 0, nullptr, disp, acc, weights, depth, nullptr, flag, live_z, live_w, live_n, group_slot,
                                  nullptr, nullptr, nullptr, kept, kept_n);
#endif
}
template <int LIMBS>
__global__ __launch_bounds__(TPB2, 1) void render_pass3_density_kept_z_kernel(SceneDev sc, const float* __restrict__ packed, long N, int S,
                                                                             const float* __restrict__ rays, int lindisp,
                                                                             float* __restrict__ disp, float* __restrict__ acc, float* __restrict__ weights,
                                                                             float* __restrict__ depth, unsigned* __restrict__ flag,
                                                                             float* __restrict__ live_z, float* __restrict__ live_w, int* __restrict__ live_n,
                                                                             const int* __restrict__ group_slot, const int* __restrict__ kept,
                                                                             const int* __restrict__ kept_n) {
#if defined(__HIP_DEVICE_COMPILE__)
    render_pass3_body<LIMBS + 8 + 64>(sc, packed, N, S, rays, nullptr, lindisp, nullptr, 0, nullptr, disp, acc, weights, depth, nullptr, flag, live_z, live_w, live_n,
                                      group_slot, nullptr, nullptr, nullptr, kept, kept_n);
#endif
}

// the point-major colour pass (PHASE 3): pts, pt_steps: point_order_kernel's entries and step counts; views: the slots' view features
template <int LIMBS>
__global__ __launch_bounds__(TPB2, 1) void render_pass3_points_kernel(SceneDev sc, const float* __restrict__ packed, long N, int S,
                                                                     const float* __restrict__ rays, int white, float* __restrict__ rgb,
                                                                     float* __restrict__ acc, unsigned* __restrict__ flag,
                                                                     float* __restrict__ live_z, float* __restrict__ live_w, int* __restrict__ live_n,
                                                                     const int* __restrict__ group_slot, const int* __restrict__ pts,
                                                                     const int* __restrict__ pt_steps, float* views) {
#if defined(__HIP_DEVICE_COMPILE__)
    render_pass3_body<LIMBS + 48>(sc, packed, N, S, rays, nullptr, 0, nullptr, white, rgb, nullptr, acc, nullptr, nullptr, nullptr, flag, live_z, live_w, live_n, group_slot,
                                  pts, pt_steps, views);
#endif
}
template <int LIMBS>
__global__ __launch_bounds__(TPB2, 1) void render_pass3_points_z_kernel(SceneDev sc, const float* __restrict__ packed, long N, int S,
                                                                       const float* __restrict__ rays, int lindisp, int white,
                                                                       float* __restrict__ rgb, float* __restrict__ acc, unsigned* __restrict__ flag,
                                                                       float* __restrict__ live_z, float* __restrict__ live_w, int* __restrict__ live_n,
                                                                       const int* __restrict__ group_slot, const int* __restrict__ pts,
                                                                       const int* __restrict__ pt_steps, float* views) {
#if defined(__HIP_DEVICE_COMPILE__)
    render_pass3_body<LIMBS + 8 + 48>(sc, packed, N, S, rays, nullptr, lindisp, nullptr, white, rgb, nullptr, acc, nullptr, nullptr, nullptr, flag, live_z, live_w, live_n,
                                      group_slot, pts, pt_steps, views);
#endif
}

// ---- natural blob -> bf16 limb fragments (the tail of the packed blob) -----------------------------------------------------------
template <int LIMBS>
__global__ void pack_decoder_limbs_kernel(const float* __restrict__ nat, unsigned* __restrict__ out) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= KB_TOTAL * kb_words(LIMBS)) return;
    const int w = idx & 3, lane = (idx >> 2) & 63, frag = (idx >> 8) % (4 * LIMBS), rec = idx / kb_words(LIMBS);
    const int t = frag % LIMBS, ob = frag / LIMBS;
    const int i = 32 * ob + (lane & 31), h = lane >> 5;
    unsigned word = 0;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const int e = 2 * w + half;
        int src;
        if (rec < KB_RGB1) {
            const int plane = rec < 3 ? 3 : rec / 3 - 1;          // consumption order: view plane, then planes 0..2
            src = N_RGB_W0 + i * (4 * C) + C * plane + HALF_C * h + 8 * (rec % 3) + e;
        } else if (rec >= KB_DEN0 && rec < KB_DEN1) {
            src = N_DEN_W0 + i * C + HALF_C * h + 8 * (rec - KB_DEN0) + e;
        } else {
            const bool is_rgb = rec < KB_DEN0;
            const int r = rec - (is_rgb ? KB_RGB1 : KB_DEN1), l = r / 8, kb = r % 8;
            const int k = 32 * (kb >> 1) + 16 * (kb & 1) + 8 * (e >> 2) + 4 * h + (e & 3);
            src = (is_rgb ? N_RGB_W1 : N_DEN_W1) + l * N_HID_STRIDE + i * HID + k;
        }
        float v = nat[src];
        unsigned bits = 0;
        if (LIMBS == 3) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                if (k == t) bits = __float_as_uint(v) >> 16;
                v = limb_rest(v);
            }
        } else {
            v *= F16_W_SCALE;                                   // limb_core.h: W 2^F16_SW as hi + lo, both rounded to nearest
            const _Float16 hi = (_Float16)v, lo = (_Float16)(v - (float)hi);
            if (!(fabsf(v) <= 65504.0f)) reinterpret_cast<float*>(out)[P_SMALL + S_F16_POISON - P_LIMB2] = __builtin_nanf("");   // (out = packed + P_LIMB2)
            bits = __builtin_bit_cast(unsigned short, t == 0 ? hi : lo);
        }
        word |= bits << (16 * half);
    }
    out[idx] = word;
}

// ---- the arithmetic primitive alone: Y[32 x 32] = W[32 x K] X[K x 32] by one wave, operands split exactly as the kernels / the pack
// kernel split them (LIMBS = 0: v_mfma_f32_32x32x2_f32).  Test hook (nvsr_limb_gemm_probe): error bounds on chosen operands.
template <int LIMBS>
__global__ void limb_gemm_probe_kernel(int K, const float* __restrict__ W, const float* __restrict__ X, float* __restrict__ Y) {
    const int lane = threadIdx.x, m = lane & 31, h = lane >> 5;
    f32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    float unscale = 1.0f;
    if constexpr (LIMBS == 0) {
        for (int k = 0; k < K; k += 2) acc = mfma32(W[m * K + k + h], X[(k + h) * 32 + m], acc);
    } else {
        const float sw = LIMBS == 2 ? F16_W_SCALE : 1.0f, sx = LIMBS == 2 ? F16_X_SCALE : 1.0f;
        unscale = 1.0f / (sw * sx);
        for (int kb = 0; kb < K / 16; ++kb) {
            Limbs<LIMBS> a, b;
            float wa[8], xb[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) { wa[i] = W[m * K + 16 * kb + 8 * h + i] * sw; xb[i] = X[(16 * kb + 8 * h + i) * 32 + m] * sx; }
            split_all<LIMBS>([&](int i) NVSR_INL { return wa[i]; }, a);
            split_all<LIMBS>([&](int i) NVSR_INL { return xb[i]; }, b);
#pragma unroll
            for (int p = 0; p < limb_products(LIMBS); ++p) acc = mfma_limb<LIMBS>(a.v[limb_w(LIMBS, p)], b.v[limb_x(LIMBS, p)], acc);
        }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) Y[(8 * (r >> 2) + 4 * h + (r & 3)) * 32 + m] = acc[r] * unscale;
}

}  // namespace nvsr

using namespace nvsr;

extern "C" int nvsr_limb_gemm_probe(int arithmetic, int K, const float* W, const float* X, float* Y, nvsr_stream_t stream) {
    if (!W || !X || !Y) return NVSR_ERR_NULL;
    if (K < 16 || K % 16) return NVSR_ERR_SHAPE;
    if (arithmetic == NVSR_ARITH_F32) hipLaunchKernelGGL(limb_gemm_probe_kernel<0>, dim3(1), dim3(64), 0, (hipStream_t)stream, K, W, X, Y);
    else if (arithmetic == NVSR_ARITH_BF16X3) hipLaunchKernelGGL(limb_gemm_probe_kernel<3>, dim3(1), dim3(64), 0, (hipStream_t)stream, K, W, X, Y);
    else if (arithmetic == NVSR_ARITH_F16X2) hipLaunchKernelGGL(limb_gemm_probe_kernel<2>, dim3(1), dim3(64), 0, (hipStream_t)stream, K, W, X, Y);
    else return NVSR_ERR_SHAPE;
    return NVSR_CHECK_LAUNCH();
}

extern "C" int nvsr_pack_decoder_limbs_launch(const float* natural, float* packed, nvsr_stream_t stream) {
    unsigned* out = reinterpret_cast<unsigned*>(packed);
    const int n3 = KB_TOTAL * kb_words(3), n2 = KB_TOTAL * kb_words(2);
    hipLaunchKernelGGL(pack_decoder_limbs_kernel<3>, dim3((n3 + 255) / 256), dim3(256), 0, (hipStream_t)stream, natural, out + P_LIMB3);
    hipLaunchKernelGGL(pack_decoder_limbs_kernel<2>, dim3((n2 + 255) / 256), dim3(256), 0, (hipStream_t)stream, natural, out + P_LIMB2);
    return NVSR_CHECK_LAUNCH();
}

// ---- the launches of one render pass: what the extern "C" entry points below receive, by name.  z = NULL: the coarse pass with its depths
// computed in the kernel from (near, far, s, S, lindisp); it always writes the weights.
struct PassArgs { const nvsr_scene* scene; const float* packed; int64_t N; int S; const float *rays, *z; int lindisp; const float* noise; int white;
                  float *rgb, *disp, *acc, *weights, *depth, *raw_out; hipStream_t stream; };
struct OccLaunch { const uint32_t* grid; int G; KeptLists kept; };
// NVSR_DENSITY_ONE_TILE, read at every launch like NVSR_COLOUR_POINTS: 1 = the plain density pass on two f16 limbs runs the one-tile kernels of
// density_tile.hip, 0 = the tile-pair kernels above; unset: DENSITY_ONE_TILE_DEFAULT (the measurement that set it).  The
// kept-list density pass, one and three limbs and the fused kernel have no one-tile form.
constexpr bool DENSITY_ONE_TILE_DEFAULT = true;
static bool density_one_tile() {
    const char* e = getenv("NVSR_DENSITY_ONE_TILE");
    return e && (e[0] == '0' || e[0] == '1') ? e[0] == '1' : DENSITY_ONE_TILE_DEFAULT;
}
// ll: the two-phase route (density pass, the colour pass's orders, colour pass on the lists), NULL: the fused kernel.  occ (with ll): the occupancy
// route -- the cull kernel and the orders on its counts in front, the density pass over the kept lists.
template <int LIMBS>
static int launch_pass3(const PassArgs& a, const LiveLists* ll, const OccLaunch* occ) {
    const SceneDev sc = to_dev(a.scene);
    unsigned* flag = nvsr_get_range_flag();
    auto launch = [&](auto kernel, auto... args) {      // (every kernel's arguments start alike)
        hipLaunchKernelGGL(kernel, dim3((unsigned)((a.N + RAYS2 - 1) / RAYS2)), dim3(TPB2), 0, a.stream, sc, a.packed, (long)a.N, a.S, a.rays, args...);
    };
    if (ll) {
        if (occ) {
            // (the kept kernels have no one-limb instantiation: the occupancy entry refuses the mode)
            if constexpr (LIMBS == 1) return NVSR_ERR_SHAPE;
            else {
                const KeptLists& kl = occ->kept;
                launch_occupancy_cull(sc, a.N, a.S, a.rays, a.z, a.lindisp, occ->grid, occ->G, kl.idx, kl.n, a.stream);
                launch_kept_order(kl, a.N, a.S, a.stream);
                // a culled sample has weight +0.0: the pass writes the kept samples' weights only
                if (a.weights && hipMemsetAsync(a.weights, 0, (size_t)a.N * (size_t)a.S * sizeof(float), a.stream) != hipSuccess) return NVSR_ERR_LAUNCH;
                if (a.z) launch(render_pass3_density_kept_kernel<LIMBS>, a.z, a.disp, a.acc, a.weights, a.depth, flag, ll->z, ll->w, ll->n, kl.slot, kl.idx, kl.n);
                else launch(render_pass3_density_kept_z_kernel<LIMBS>, a.lindisp, a.disp, a.acc, a.weights, a.depth, flag, ll->z, ll->w, ll->n, kl.slot, kl.idx, kl.n);
            }
        } else if (LIMBS == 2 && density_one_tile()) {
            // two f16 limbs: the one-tile density kernels (density_tile.hip), same bits; NVSR_DENSITY_ONE_TILE=0 keeps the tile-pair kernels below
            if (int e = nvsr_density_tile_launch(a.scene, a.packed, a.N, a.S, a.rays, a.z, a.lindisp, a.noise, a.disp, a.acc, a.weights, a.depth, ll->z, ll->w, ll->n,
                                                 (nvsr_stream_t)a.stream)) return e;
            note_density_kernel(a.stream, 1);
        } else if (a.z) launch(render_pass3_density_kernel<LIMBS>, a.z, a.noise, a.disp, a.acc, a.weights, a.depth, flag, ll->z, ll->w, ll->n);
        else launch(render_pass3_density_z_kernel<LIMBS>, a.lindisp, a.noise, a.disp, a.acc, a.weights, a.depth, flag, ll->z, ll->w, ll->n);
        launch_colour_order(*ll, a.N, a.S, a.stream);
        if (ll->pts) {
            launch_point_order(*ll, a.z ? a.rays : nullptr, a.N, a.S, a.stream);
            if (a.z) launch(render_pass3_points_kernel<LIMBS>, a.white, a.rgb, a.acc, flag, ll->z, ll->w, ll->n, ll->slot, ll->pts, ll->steps, ll->views);
            else launch(render_pass3_points_z_kernel<LIMBS>, a.lindisp, a.white, a.rgb, a.acc, flag, ll->z, ll->w, ll->n, ll->slot, ll->pts, ll->steps, ll->views);
        } else if (a.z) launch(render_pass3_colour_kernel<LIMBS>, a.white, a.rgb, a.acc, flag, ll->z, ll->w, ll->n, ll->slot);
        else launch(render_pass3_colour_z_kernel<LIMBS>, a.lindisp, a.white, a.rgb, a.acc, flag, ll->z, ll->w, ll->n, ll->slot);
    } else if (!a.z) launch(render_pass3_coarse_z_kernel<LIMBS>, a.lindisp, a.noise, a.white, a.rgb, a.disp, a.acc, a.weights, a.depth, a.raw_out, flag);
    else if (a.weights) launch(render_pass3_coarse_kernel<LIMBS>, a.z, a.noise, a.white, a.rgb, a.disp, a.acc, a.weights, a.depth, a.raw_out, flag);
    else launch(render_pass3_kernel<LIMBS>, a.z, a.noise, a.white, a.rgb, a.disp, a.acc, a.depth, a.raw_out, flag);
    return NVSR_CHECK_LAUNCH();
}
// one pass: its scratch, asked for once, names the route; grid (NULL: none) asks for the occupancy route, which falls back to the plain one
static int launch_pass3(int limbs, const PassArgs& a, const uint32_t* grid = nullptr, int G = 0) {
    LiveLists lists; OccLaunch occ{grid, G, {}};
    const PassRoute route = acquire_pass_scratch(a.N, a.S, a.stream, a.raw_out != nullptr, grid != nullptr, true, lists, occ.kept);
    const LiveLists* ll = route == PassRoute::Fused ? nullptr : &lists;
    const OccLaunch* oc = route == PassRoute::Occupancy ? &occ : nullptr;
    return limbs == 3 ? launch_pass3<3>(a, ll, oc) : limbs == 1 ? launch_pass3<1>(a, ll, oc) : launch_pass3<2>(a, ll, oc);
}

extern "C" int nvsr_render_pass3_launch(int limbs, const nvsr_scene* scene, const float* packed_decoder, int64_t N, int S, const float* rays, const float* z,
                                        const float* noise, int white_bkgd, float* rgb, float* disp, float* acc, float* weights, float* depth, float* raw_out,
                                        nvsr_stream_t stream) {
    if ((N + RAYS2 - 1) / RAYS2 > 0x7fffffff || limbs < 1 || limbs > 3) return NVSR_ERR_SHAPE;
    PassArgs a{}; a.scene = scene; a.packed = packed_decoder; a.N = N; a.S = S; a.rays = rays; a.z = z; a.noise = noise; a.white = white_bkgd;
    a.rgb = rgb; a.disp = disp; a.acc = acc; a.weights = weights; a.depth = depth; a.raw_out = raw_out; a.stream = (hipStream_t)stream;
    return launch_pass3(limbs, a);
}

// the coarse pass with its depths computed in the kernel (z = coarse_depth(near, far, s, S, lindisp)); weights are always written
extern "C" int nvsr_render_pass3_coarse_z_launch(int limbs, const nvsr_scene* scene, const float* packed_decoder, int64_t N, int S, const float* rays, int lindisp,
                                                 const float* noise, int white_bkgd, float* rgb, float* disp, float* acc, float* weights, float* depth,
                                                 float* raw_out, nvsr_stream_t stream) {
    if ((N + RAYS2 - 1) / RAYS2 > 0x7fffffff || limbs < 1 || limbs > 3 || !weights) return NVSR_ERR_SHAPE;
    PassArgs a{}; a.scene = scene; a.packed = packed_decoder; a.N = N; a.S = S; a.rays = rays; a.lindisp = lindisp; a.noise = noise; a.white = white_bkgd;
    a.rgb = rgb; a.disp = disp; a.acc = acc; a.weights = weights; a.depth = depth; a.raw_out = raw_out; a.stream = (hipStream_t)stream;
    return launch_pass3(limbs, a);
}

// The occupancy route (include/nvsr.h, "Occupancy grid"): the pass above, without noise, with the density decoder run on the samples of set cells only.  Declines
// -- and runs the plain route, which is what the grid approximates -- where the two-phase route declines or the kept lists cannot be had.
// z == NULL: the depths of coarse_depth in registers (lindisp); weights are then required, as by the coarse_z launch.
extern "C" int nvsr_render_pass_occupancy_arith(const nvsr_scene* scene, const float* packed_decoder, int64_t N, int S, const float* rays, const float* z, int lindisp,
                                                int white_bkgd, float* rgb, float* disp, float* acc, float* weights, float* depth, const uint32_t* grid, int G,
                                                int arithmetic, nvsr_stream_t stream) {
    const int arith = nvsr_internal_resolve_decoder_arith(arithmetic);
    if ((arith != NVSR_ARITH_F16X2 && arith != NVSR_ARITH_BF16X3) || G < 1 || G > OCC_MAX_G) return NVSR_ERR_SHAPE;
    if (int e = check_scene(scene)) return e;
    if (!packed_decoder || !rays || !rgb || !disp || !acc || !grid || (!z && !weights)) return NVSR_ERR_NULL;
    if (!aligned16(packed_decoder)) return NVSR_ERR_ALIGN;
    if (N < 0 || S < 1 || S > 4096 || (N + RAYS2 - 1) / RAYS2 > 0x7fffffff) return NVSR_ERR_SHAPE;
    if (N == 0) return NVSR_OK;
    PassArgs a{}; a.scene = scene; a.packed = packed_decoder; a.N = N; a.S = S; a.rays = rays; a.z = z; a.lindisp = lindisp; a.white = white_bkgd;
    a.rgb = rgb; a.disp = disp; a.acc = acc; a.weights = weights; a.depth = depth; a.stream = (hipStream_t)stream;
    return launch_pass3(arith == NVSR_ARITH_F16X2 ? 2 : 3, a, grid, G);
}
