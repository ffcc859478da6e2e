// The density pass of the two-phase render route (render3.hip, PHASE 1) for two f16 limbs with ONE 32-ray tile per wave, written on the
// one-tile skeleton of decode_limb.hip: no side lambdas, no rolling gathers, no hand-placed slices -- a wave gathers, multiplies, applies
// bias + ReLU and composites in program order, and the OTHER wave of its SIMD is the side work.
//
// Shape: one workgroup of 8 waves = 256 rays per CU (the grid and the XCD-aware block mapping of the tile-pair kernels), two waves per SIMD,
// at most 256 registers each.  Two independent 4-wave workgroups per CU -- decode_limb.hip's shape, the first form of this file -- have to
// stream every weight once per 128 rays, 2.7 times the tile-pair kernels' stream per point, through the texture path the gathers use: 41.0
// against 39.4 ms on the benchmark's fine pass, 31.6 ms in a timing build without the copies (profiles/density_one_tile_ab.txt).  One
// workgroup shares one ring among all eight tiles, but its waves meet at every ring barrier: left alone the two waves of a SIMD gather at
// the same time and multiply at the same time (39.6 ms).  So they are staggered by what needs no barrier:
//   waves 0 .. 3   gather sample s | layers 0, 1 of s (resident) | layers 2, 3 of s (ring) | epilogue of s
//   waves 4 .. 7   layers 0, 1 of s (resident) | gather sample s + 1 | layers 2, 3 of s (ring) | epilogue of s
// -- while one wave of a SIMD waits for its texels the other one has the matrix pipe, and both reach the step's first ring barrier
// together.  The gather of waves 4 .. 7 sits between two layers, where the accumulators are dead and one activation set is live (inside a
// layer both are: 128 registers beside the 96 of a plane's taps); D is held over layers 2 and 3 (24 registers).
//
// Per step and tile, the operations of PHASE 1 in its order: point_norm, pos_taps2 / scaled taps and the blend of gather24 for planes
// 0..2, D = div3((F0 + F1) + F2), density layer 0 (3 K-blocks) and layers 1..3 (8 K-blocks each) through limb_block<2> -- K-blocks in
// order, three products per fragment pair, C = 0 on a layer's first MFMA --, bias_relu<2>, head_dots<1>, composite_weight, the stores of
// weights and the live list.  Same operands in the same order: bit for bit what render_pass3_density[_z]_kernel<2> writes.
//
// LDS (LdsTile, 158 KB): a ring of two 32-KB slots, density layers 0 and 1 resident (11 K-blocks, 88 KB, loaded once per launch and waited
// for in front of the loop), the small constants.  The ray's constants live in registers (a lane owns one ray for the whole launch).  A
// step streams layers 2 and 3 in 4 chunks of 4 K-blocks -- 128 KB per 256 rays, where the tile-pair kernels stream 144 --; a chunk is
// copied one block ahead, 1-KiB pieces round-robin over the eight waves, and the block that multiplies it stands behind s_waitcnt vmcnt(0)
// + a workgroup barrier.  The blocks of layers 0 and 1 read the resident region: no copy, no wait, no barrier.  The first chunk of step
// s + 1 is issued by the last block of step s (behind the last sample: a harmless copy, waited for before the wave ends).
#include "pair_core.h"

#include "nvsr_internal.h"

#ifndef DT_ABLATE
#define DT_ABLATE 0      // timing experiments only (wrong results): 1 no weight copies, 2 no gather loads, 4 no ring waits and barriers, 8 no bias + ReLU
#endif
#ifndef DT_STAGGER
#define DT_STAGGER 1     // 0 (A/B): every wave gathers at the top of its step
#endif

namespace nvsr {

constexpr int DT_TPB = 512, DT_WAVES = DT_TPB / 64, DT_RAYS = DT_WAVES * 32;
static_assert(DT_RAYS == RAYS2, "the grid is the tile-pair kernels'");
struct LdsTile {
    static constexpr int SLOT = 4 * kb_words(2);                      // words: 32 KB
    static constexpr int RES = 2 * SLOT;                              // density layers 0 and 1
    static constexpr int RES_KB = KB_DEN1 + 8 - KB_DEN0;
    static constexpr int SMALL = RES + RES_KB * kb_words(2);
    static constexpr int TOTAL = SMALL + SMALL_FLOATS;
};
static_assert(KB_DEN1 - KB_DEN0 == 3 && LdsTile::RES_KB == 11, "density layer 0 is one block of three K-blocks, layer 1 two of four");
static_assert(LdsTile::TOTAL * 4 <= 160 * 1024, "LDS budget");

// NKB K-blocks from kb0 on -> dst, in 1-KiB pieces round-robin over the waves
template <int NKB>
__device__ __forceinline__ void tile_copy(const Ring3<2>& rs, unsigned* dst, int kb0) {
    constexpr int PIECES = NKB * 4 * 2;
    static_assert(PIECES % DT_WAVES == 0, "a copy must split evenly over the waves");
#pragma unroll
    for (int i = 0; i < PIECES / DT_WAVES; ++i)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs.rsrc, (__attribute__((address_space(3))) void*)(dst + (i * DT_WAVES + rs.wave) * 256), 16,
                                                 (int)rs.voff, kb0 * kb_words(2) * 4 + i * (DT_WAVES * 1024), 0, R3_DMA_AUX);
}
// chunk = K-blocks kb0 .. kb0 + NKB - 1 -> the free slot
template <int NKB>
__device__ __forceinline__ const unsigned* tile_issue(Ring3<2>& rs, int kb0) {
    static_assert(NKB * kb_words(2) <= LdsTile::SLOT, "a chunk fits the slot");
    unsigned* dst = rs.lds + rs.slot * LdsTile::SLOT;
#if !(DT_ABLATE & 1)
    tile_copy<NKB>(rs, dst, kb0);
#endif
    rs.slot ^= 1;
    return dst;
}
// every copy this wave has issued has landed; behind the barrier every wave's has, and the slot read one block ago is free
__device__ __forceinline__ void tile_sync() {
#if !(DT_ABLATE & 4)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
#endif
}

struct TileD { float T, dep, ac, zc, zn; float raw[4]; };      // what composite_weight touches

template <int ZCOMP>
__device__ __forceinline__ void density_tile_body(const SceneDev& sc, const float* __restrict__ packed, long N, int S, const float* __restrict__ rays,
                                                  const float* __restrict__ z, int lindisp, const float* __restrict__ noise, float* __restrict__ disp,
                                                  float* __restrict__ acc_out, float* __restrict__ weights, float* __restrict__ depth,
                                                  unsigned* __restrict__ flag, float* __restrict__ live_z, float* __restrict__ live_w,
                                                  int* __restrict__ live_n) {
    using L = LdsTile;
    __shared__ __attribute__((aligned(16))) unsigned lds[L::TOTAL];
    NVSR_RACE_PROBE_DELAY(lds);      // (probe builds only, nvsr_common.h)
    Ring3<2> rs{__builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(packed + limb_region(2)), 0, KB_TOTAL * kb_words(2) * 4, 0x00020000),
                lds, 0, __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), (int)(threadIdx.x & 63), ring3_voff<2>(threadIdx.x)};
    float* ldsf = reinterpret_cast<float*>(lds);
    // biases x 2^SX, head weights x 2^-SX, the packer's poison into the head biases (render3.hip)
    for (int i = threadIdx.x; i < SMALL_FLOATS; i += DT_TPB) {
        float v = packed[P_SMALL + i] * (i < S_ALPHA_W ? F16_X_SCALE : i < S_HEAD_B ? F16_HEAD_SCALE : 1.0f);
        if (i >= S_HEAD_B && i < S_HEAD_B + 4) v += packed[P_SMALL + S_F16_POISON];
        ldsf[L::SMALL + i] = v;
    }
    const float* small = ldsf + L::SMALL;
    float nsc = -F16_ACC_UNSCALE;                    // bias_relu<2>: opaque, or the compiler folds the two negations away
    asm volatile("" : "+s"(nsc));
    tile_copy<L::RES_KB>(rs, lds + L::RES, KB_DEN0);

    // XCD-aware ray blocks (render_pass3_body): workgroup b runs on XCD b % 8; XCD x gets the x-th contiguous eighth of the blocks
    const unsigned nblk = gridDim.x, xcd = blockIdx.x & 7u, per = nblk >> 3, rem = nblk & 7u;
    const unsigned blk = xcd * per + (xcd < rem ? xcd : rem) + (blockIdx.x >> 3);
    long ray = (long)blk * DT_RAYS + rs.wave * 32 + (rs.lane & 31);
    const bool valid = ray < N;
    if (!valid) ray = N - 1;
    const float* r = rays + ray * 11;
    const float ox = r[0], oy = r[1], oz = r[2], dx = r[3], dy = r[4], dz = r[5], near = r[6], far = r[7];
    const float nrm = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz)));
    const float* zrow = ZCOMP ? nullptr : z + ray * S;
    auto depth_of = [&](int k) NVSR_INL -> float {
        if constexpr (ZCOMP) return coarse_depth(near, far, k, S, lindisp);
        else return zrow[k];
    };
    TileD t;
    t.T = 1.0f; t.dep = t.ac = 0.0f;
    t.zc = depth_of(0);
    int cursor = 0;                                  // of the ray's live list
    // (waves w and w + 4 of a workgroup share a SIMD)
    const bool ahead = DT_STAGGER && rs.wave >= DT_WAVES / 2;

    tile_sync();                                     // the resident layers and the small constants
    const unsigned* cw = tile_issue<4>(rs, KB_DEN1 + 8);      // first ring chunk of sample 0; every later one is issued a block ahead

    f32x16 acc[4], act[4];
    float D[HALF_C], F[HALF_C];
    Limbs<2> cur, fa;
    SplitPend tp;
    auto feat = [](const float (&f)[HALF_C]) { return [&f](int kb, int i) { return f[8 * kb + i]; }; };
    auto hid = [](const f32x16 (&a)[4], int kb0) { return [&a, kb0](int kb, int i) { const int k = kb0 + kb; return a[k >> 1][8 * (k & 1) + i]; }; };
    auto none = [](int) {};
    auto tail_of = [&tp](const f32x16 (&a)[4], int kb) {
        return [&a, kb, &tp](int slice, Limbs<2>& nxt) { split_slice<2>(slice, [&a, kb](int i) { return a[kb >> 1][8 * (kb & 1) + i]; }, nxt, tp); };
    };
    // Nothing moves across the end of a block (decode_limb.hip, L3_FENCE): left alone hipcc hoists the next gather's loads above the MFMAs
#define DT_FENCE                                                                                    \
    asm volatile("" : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]), "+v"(acc[3]) : : "memory");         \
    __builtin_amdgcn_sched_barrier(0);
    // One block = half a hidden layer (layer 0: all of it).  FIRST: the block's first K-block is split here, otherwise the previous block's
    // tail produced it.  Out of the resident region (K-block KB_OFF of it): no copy, no wait, no barrier ...
#define DT_RES_BLOCK(KB_OFF, NKB, ZERO, FIRST, SRC, TAIL)                                          \
    {                                                                                              \
        if (FIRST) { auto s_ = SRC; split_all<2>([&](int i) { return s_(0, i); }, cur); }          \
        limb_block<2, NKB, ZERO, true>(lds + L::RES + (KB_OFF) * kb_words(2), lane, acc, cur, fa, SRC, none, TAIL);      \
        DT_FENCE                                                                                   \
    }
    // ... out of the ring: wait for the chunk, start the copy of the next one (K-blocks KB_NEXT .. + 3), multiply
#define DT_BLOCK(ZERO, FIRST, SRC, KB_NEXT, TAIL)                                                  \
    {                                                                                              \
        tile_sync();                                                                               \
        const unsigned* nw = tile_issue<4>(rs, KB_NEXT);                                           \
        if (FIRST) { auto s_ = SRC; split_all<2>([&](int i) { return s_(0, i); }, cur); }          \
        limb_block<2, 4, ZERO, true>(cw, lane, acc, cur, fa, SRC, none, TAIL);                     \
        cw = nw;                                                                                   \
        DT_FENCE                                                                                   \
    }
#if DT_ABLATE & 8
#define DT_RELU(VEC) { _Pragma("unroll") for (int ib = 0; ib < 4; ++ib) act[ib] = acc[ib]; }
#else
#define DT_RELU(VEC) bias_relu<2>(acc, small + S_BIAS + (VEC) * HID, h, act, nsc);
#endif

    for (int s = 0; s < S; ++s) {
        asm volatile("" : "+v"(rs.voff), "+v"(rs.lane));      // (keeps hipcc from hoisting per-lane addresses out of the sample loop)
        const int lane = rs.lane, h = lane >> 5;
        const bool last = (s + 1 == S);
        t.zn = depth_of(last ? s : s + 1);
        const float nz = noise ? noise[ray * S + s] : 0.0f;
        // the position features of the sample at depth zc -> D: a plane's loads, its blend, the next plane
        auto gather_d = [&](float zc) NVSR_INL {
            const float n0 = norm_coord(__fadd_rn(ox, __fmul_rn(dx, zc)), sc.lo[0], sc.range[0]);
            const float n1 = norm_coord(__fadd_rn(oy, __fmul_rn(dy, zc)), sc.lo[1], sc.range[1]);
            const float n2 = norm_coord(__fadd_rn(oz, __fmul_rn(dz, zc)), sc.lo[2], sc.range[2]);
#pragma unroll
            for (int p = 0; p < 3; ++p) {
                Taps tap = pos_taps2(sc, p, n0, n1, n2);
                tap.nw *= F16_X_SCALE; tap.ne *= F16_X_SCALE; tap.sw *= F16_X_SCALE; tap.se *= F16_X_SCALE;      // features carry 2^F16_SX (exact)
#if DT_ABLATE & 2
                for (int c = 0; c < HALF_C; ++c) F[c] = tap.nw * (float)(c + h);
#else
                gather24(sc.plane[p], tap, h, F);
#endif
#pragma unroll
                for (int c = 0; c < HALF_C; ++c) {
                    D[c] = p == 0 ? F[c] : p == 1 ? __fadd_rn(D[c], F[c]) : div3(__fadd_rn(D[c], F[c]));
                    asm volatile("" : "+v"(D[c]));
                }
                __builtin_amdgcn_sched_barrier(0);      // (one plane at a time: 24 loads, 96 registers of taps)
            }
        };
        // waves 4 .. 7 hold this sample's D since the step before (sample 0: gathered here)
        if (!ahead || s == 0) gather_d(t.zc);
        // ---- density layers 0 and 1 out of the resident region
        DT_RES_BLOCK(0, 3, true, true, feat(D), NoTail{})
        DT_RELU(0)
        DT_RES_BLOCK(3, 4, true, true, hid(act, 0), tail_of(act, 4))
        DT_RES_BLOCK(7, 4, false, false, hid(act, 4), NoTail{})
        DT_RELU(1)
        // waves 4 .. 7: the NEXT sample's D (behind the last sample: the last depth again, dropped)
        if (ahead) gather_d(t.zn);
        // ---- density layers 2 and 3 through the ring
        DT_BLOCK(true, true, hid(act, 0), KB_DEN1 + 12, tail_of(act, 4))
        DT_BLOCK(false, false, hid(act, 4), KB_DEN1 + 16, NoTail{})
        DT_RELU(2)
        DT_BLOCK(true, true, hid(act, 0), KB_DEN1 + 20, tail_of(act, 4))
        DT_BLOCK(false, false, hid(act, 4), KB_DEN1 + 8, NoTail{})      // (the chunk issued last is the NEXT sample's first)
        DT_RELU(3)
        // ---- sigma head, compositing, the weight and the live list (PHASE 1's epilogue)
        {
            float hd[1];
            head_dots<1>(small + S_ALPHA_W, h, act, hd);
            t.raw[3] = hd[0] + small[S_HEAD_B];
        }
        composite_weight(t, nrm, nz, last);
        const float w = t.raw[3];
        const bool live = !(w == 0.0f);                  // (a NaN weight is live)
        if (lane < 32 && valid) {
            if (weights) weights[ray * S + s] = w;
            if (live) { live_z[ray * S + cursor] = ZCOMP ? __int_as_float(s) : t.zc; live_w[ray * S + cursor] = w; }
        }
        cursor += live;
        t.zc = t.zn;
    }
#undef DT_RELU
#undef DT_BLOCK
#undef DT_RES_BLOCK
#undef DT_FENCE
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // the copy issued for a sample after the last one must land before the wave ends

    if (rs.lane < 32 && valid) {
        const float q = t.dep / t.ac;                       // NaN when acc == 0, like torch.max(1e-10, nan)
        disp[ray] = 1.0f / ((q != q) ? q : fmaxf(1e-10f, q));
        acc_out[ray] = t.ac;
        if (depth) depth[ray] = t.dep;
        live_n[ray] = cursor;
        // range flag of the f16 limbs (nvsr.h: nvsr_set_range_flag): the density pass looks at acc alone
        if (flag && !(fabsf(t.ac) <= 3.0e38f)) __hip_atomic_fetch_or(flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// two thin kernels, one symbol each in a kernel trace: depths read / depths in registers (live_z then holds sample indices)
__global__ __launch_bounds__(DT_TPB, 1) void density_tile_kernel(SceneDev sc, const float* __restrict__ packed, long N, int S, const float* __restrict__ rays,
                                                                 const float* __restrict__ z, const float* __restrict__ noise, float* __restrict__ disp,
                                                                 float* __restrict__ acc, float* __restrict__ weights, float* __restrict__ depth,
                                                                 unsigned* __restrict__ flag, float* __restrict__ live_z, float* __restrict__ live_w,
                                                                 int* __restrict__ live_n) {
#if defined(__HIP_DEVICE_COMPILE__)      // (hipcc's host pass cannot resolve the LDS-DMA helpers; it only needs the stub)
    density_tile_body<0>(sc, packed, N, S, rays, z, 0, noise, disp, acc, weights, depth, flag, live_z, live_w, live_n);
#endif
}
__global__ __launch_bounds__(DT_TPB, 1) void density_tile_z_kernel(SceneDev sc, const float* __restrict__ packed, long N, int S, const float* __restrict__ rays,
                                                                   int lindisp, const float* __restrict__ noise, float* __restrict__ disp,
                                                                   float* __restrict__ acc, float* __restrict__ weights, float* __restrict__ depth,
                                                                   unsigned* __restrict__ flag, float* __restrict__ live_z, float* __restrict__ live_w,
                                                                   int* __restrict__ live_n) {
#if defined(__HIP_DEVICE_COMPILE__)
    density_tile_body<1>(sc, packed, N, S, rays, nullptr, lindisp, noise, disp, acc, weights, depth, flag, live_z, live_w, live_n);
#endif
}

}  // namespace nvsr

using namespace nvsr;

// z = NULL: the depths of coarse_depth in registers (lindisp).  Arguments already validated by the pass launcher (render3.hip), whose grid this is
extern "C" int nvsr_density_tile_launch(const nvsr_scene* scene, const float* packed_decoder, int64_t N, int S, const float* rays, const float* z, int lindisp,
                                        const float* noise, float* disp, float* acc, float* weights, float* depth, float* live_z, float* live_w, int* live_n,
                                        nvsr_stream_t stream) {
    const int64_t blocks = (N + DT_RAYS - 1) / DT_RAYS;
    if (N < 1 || blocks > 0x7fffffff) return NVSR_ERR_SHAPE;
    const SceneDev sc = to_dev(scene);
    unsigned* flag = nvsr_get_range_flag();
    if (z) hipLaunchKernelGGL(density_tile_kernel, dim3((unsigned)blocks), dim3(DT_TPB), 0, (hipStream_t)stream, sc, packed_decoder, (long)N, S, rays, z, noise,
                              disp, acc, weights, depth, flag, live_z, live_w, live_n);
    else hipLaunchKernelGGL(density_tile_z_kernel, dim3((unsigned)blocks), dim3(DT_TPB), 0, (hipStream_t)stream, sc, packed_decoder, (long)N, S, rays, lindisp,
                            noise, disp, acc, weights, depth, flag, live_z, live_w, live_n);
    return NVSR_CHECK_LAUNCH();
}
