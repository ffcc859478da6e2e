// Occupancy grid (include/nvsr.h, "Occupancy grid"): a bit per cell of the scene's normalised box, built by probing the density decoder, and
// the cull kernel that turns the samples of a render pass into per-ray lists of the samples whose cell is set.  The density pass over those
// lists is render3.hip's (PHASE 4); their scratch is colour_order.hip's.
//
// Layout: cell (ix, iy, iz) is bit i & 31 of word i >> 5, i = (iz G + iy) G + ix; ceil(G^3 / 32) words; the unused bits of the last word are 0.
// The grid is APPROXIMATE by nature: no finite set of probes bounds an MLP over a cell.  K (probes per axis and cell), the threshold and the
// rounds of dilation are the caller's knobs.
#include "occupancy.h"
#include "generic_fused_core.h"
#include "nvsr_internal.h"

namespace nvsr {

// ---- build ------------------------------------------------------------------------------------------------------------------------------
// Probe p = i K^3 + (jz K + jy) K + jx of cell i = (iz G + iy) G + ix sits, along each axis, at u = ((float)(c K + j) + 0.5f) / (float)(G K) of
// the box: world coordinate lo + u range (one rounding per operation).  x[p] = (world xyz, view direction (1, 0, 0)): sigma does not depend
// on the direction.  The kernel writes the probes of cells [cell0, cell0 + cells); rows of cells >= G^3 (the padding of the last word) repeat
// cell G^3 - 1 and are never marked.
__global__ __launch_bounds__(256) void occupancy_probe_kernel(float lo0, float lo1, float lo2, float r0, float r1, float r2, int G, int K, long cell0, long cells,
                                                              float* __restrict__ x) {
    const int K3 = K * K * K;
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= cells * K3) return;
    const long G3 = (long)G * G * G;
    long i = cell0 + p / K3;
    if (i >= G3) i = G3 - 1;
    const int j = (int)(p % K3);
    const int ix = (int)(i % G), iy = (int)((i / G) % G), iz = (int)(i / ((long)G * G));
    const int jx = j % K, jy = (j / K) % K, jz = j / (K * K);
    const float gk = (float)(G * K);
    const float ux = __fdiv_rn(__fadd_rn((float)(ix * K + jx), 0.5f), gk);
    const float uy = __fdiv_rn(__fadd_rn((float)(iy * K + jy), 0.5f), gk);
    const float uz = __fdiv_rn(__fadd_rn((float)(iz * K + jz), 0.5f), gk);
    float* o = x + p * 6;
    o[0] = __fadd_rn(lo0, __fmul_rn(ux, r0));
    o[1] = __fadd_rn(lo1, __fmul_rn(uy, r1));
    o[2] = __fadd_rn(lo2, __fmul_rn(uz, r2));
    o[3] = 1.0f; o[4] = 0.0f; o[5] = 0.0f;
}

// out[P, 4] of the probes of cells [cell0, cell0 + 32 words) -> words [cell0 / 32, ...) of the grid: a thread per cell, a cell's bit is set iff
// any of its K^3 probes has sigma_raw > threshold or a NaN sigma_raw; the wave's ballot is two whole words (lanes 0 and 32 store them).
__global__ __launch_bounds__(256) void occupancy_mark_kernel(const float* __restrict__ out, int K3, long G3, long cell0, long words, float threshold,
                                                             uint32_t* __restrict__ grid) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;      // the cell of the slab; whole waves run past the slab's end (ballot)
    const long i = cell0 + t;
    bool any = false;
    if (t < words * 32 && i < G3) {
        const float* o = out + t * K3 * 4 + 3;
        for (int j = 0; j < K3; ++j) {
            const float s = o[j * 4];
            any = any || s > threshold || s != s;
        }
    }
    const unsigned long long m = __ballot(any);
    const int lane = threadIdx.x & 63;
    const long w = t >> 5;
    if ((lane & 31) == 0 && w < words) grid[(cell0 >> 5) + w] = (uint32_t)(lane ? m >> 32 : m);
}

// one round of a 3 x 3 x 3 OR, gather form: a thread forms one output word from the input grid's bits (two buffers, no atomics)
__global__ __launch_bounds__(256) void occupancy_dilate_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, int G, long words) {
    const long w = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= words) return;
    const long G3 = (long)G * G * G;
    uint32_t word = 0;
    for (int b = 0; b < 32; ++b) {
        const long i = w * 32 + b;
        if (i >= G3) break;
        const int ix = (int)(i % G), iy = (int)((i / G) % G), iz = (int)(i / ((long)G * G));
        bool any = false;
        for (int dz = -1; dz <= 1; ++dz) {
            const int z = iz + dz;
            if (z < 0 || z >= G) continue;
            for (int dy = -1; dy <= 1; ++dy) {
                const int y = iy + dy;
                if (y < 0 || y >= G) continue;
                const long row = ((long)z * G + y) * G;
                for (int xx = (ix > 0 ? ix - 1 : 0); xx <= (ix + 1 < G ? ix + 1 : G - 1); ++xx) {
                    const long n = row + xx;
                    any = any || ((in[n >> 5] >> (n & 31)) & 1u);
                }
            }
        }
        word |= (any ? 1u : 0u) << b;
    }
    out[w] = word;
}

// ---- cull -------------------------------------------------------------------------------------------------------------------------------
// One wave per ray, 64 samples per trip: sample s is kept iff its cell's bit is set or its normalised point has a NaN coordinate.  The point is
// the render body's (render3.hip, point_norm): norm_coord(o + d z, lo, range), one rounding per operation.  The wave's ballot and its count
// below the lane give the kept samples their places, in sample order; entries behind the count are -1.  The grid is read through the cache
// (256 KB at G = 128: it stays in an XCD's L2).
constexpr int CULL_WAVES = 4;
__global__ __launch_bounds__(CULL_WAVES * 64) void occupancy_cull_kernel(SceneDev sc, long N, int S, const float* __restrict__ rays, const float* __restrict__ z,
                                                                         int lindisp, const uint32_t* __restrict__ grid, int G, int* __restrict__ kept,
                                                                         int* __restrict__ kept_n) {
    const long ray = (long)blockIdx.x * CULL_WAVES + (threadIdx.x >> 6);
    if (ray >= N) return;                                            // (a whole wave)
    const int lane = threadIdx.x & 63;
    const float* r = rays + ray * 11;
    const float ox = r[0], oy = r[1], oz = r[2], dx = r[3], dy = r[4], dz = r[5], nr = r[6], fr = r[7];
    int* row = kept + ray * S;
    int base = 0;
    for (int s0 = 0; s0 < S; s0 += 64) {
        const int s = s0 + lane;
        bool keep = false;
        if (s < S) {
            const float zc = z ? z[ray * S + s] : coarse_depth(nr, fr, s, S, lindisp);
            const float n0 = norm_coord(__fadd_rn(ox, __fmul_rn(dx, zc)), sc.lo[0], sc.range[0]);
            const float n1 = norm_coord(__fadd_rn(oy, __fmul_rn(dy, zc)), sc.lo[1], sc.range[1]);
            const float n2 = norm_coord(__fadd_rn(oz, __fmul_rn(dz, zc)), sc.lo[2], sc.range[2]);
            if (n0 != n0 || n1 != n1 || n2 != n2) keep = true;
            else {
                const int i = (occupancy_cell(n2, G) * G + occupancy_cell(n1, G)) * G + occupancy_cell(n0, G);      // < 2^27
                keep = (grid[i >> 5] >> (i & 31)) & 1u;
            }
        }
        const unsigned long long m = __ballot(keep);
        const int at = base + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
        if (keep) row[at] = s;
        base += __popcll(m);
    }
    for (int k = base + lane; k < S; k += 64) row[k] = -1;
    if (lane == 0) kept_n[ray] = base;
}

void launch_occupancy_cull(const SceneDev& sc, int64_t N, int S, const float* rays, const float* z, int lindisp, const uint32_t* grid, int G, int* kept, int* kept_n,
                           hipStream_t stream) {
    hipLaunchKernelGGL(occupancy_cull_kernel, dim3((unsigned)((N + CULL_WAVES - 1) / CULL_WAVES)), dim3(CULL_WAVES * 64), 0, stream, sc, (long)N, S, rays, z, lindisp,
                       grid, G, kept, kept_n);
}

namespace {
// the build works through the grid in slabs of whole words, at most SLAB_PROBES probes each: the workspace stays bounded (80 MB)
constexpr int64_t SLAB_PROBES = (int64_t)1 << 21;
int64_t grid_words(int G) { return ((int64_t)G * G * G + 31) / 32; }
int64_t slab_words(int G, int K) {
    const int64_t w = SLAB_PROBES / ((int64_t)32 * K * K * K), all = grid_words(G);
    return w < all ? w : all;
}
bool build_shape_ok(int G, int K) { return G >= 1 && G <= OCC_MAX_G && K >= 1 && K <= OCC_MAX_K; }
unsigned blocks256(int64_t n) { return (unsigned)((n + 255) / 256); }
}  // namespace

}  // namespace nvsr

using namespace nvsr;

extern "C" int64_t nvsr_occupancy_words(int G) { return G >= 1 && G <= OCC_MAX_G ? grid_words(G) : 0; }

// out [P, 4], x [P, 6] of a slab (P = 32 K^3 words of it), then a second grid for the dilation
extern "C" int64_t nvsr_occupancy_workspace_floats(int G, int K) {
    if (!build_shape_ok(G, K)) return 0;
    const int64_t P = slab_words(G, K) * 32 * K * K * K;
    return 10 * P + round4(grid_words(G));
}

namespace nvsr {
namespace {
// the build both entries share: per slab the probes, `decode(P, x, out)` -- the density decoder of the caller's geometry on the slab's probes --
// and the marks; then the dilation.  Everything has been checked by the caller.
template <typename Decode>
int occupancy_build_slabs(const float* lo, const float* range, int G, int K, float threshold, int dilate, uint32_t* grid, float* workspace, hipStream_t st,
                          Decode decode) {
    const int K3 = K * K * K;
    const int64_t G3 = (int64_t)G * G * G, words = grid_words(G), sw = slab_words(G, K);
    float* out = workspace;
    float* x = out + 4 * sw * 32 * K3;
    uint32_t* other = reinterpret_cast<uint32_t*>(x + 6 * sw * 32 * K3);
    for (int64_t w0 = 0; w0 < words; w0 += sw) {
        const int64_t nw = words - w0 < sw ? words - w0 : sw, P = nw * 32 * K3;
        hipLaunchKernelGGL(occupancy_probe_kernel, dim3(blocks256(P)), dim3(256), 0, st, lo[0], lo[1], lo[2], range[0], range[1], range[2], G, K, (long)(w0 * 32),
                           (long)(nw * 32), x);
        if (hipGetLastError() != hipSuccess) return NVSR_ERR_LAUNCH;
        if (int e = decode(P, x, out)) return e;
        hipLaunchKernelGGL(occupancy_mark_kernel, dim3(blocks256(nw * 32)), dim3(256), 0, st, out, K3, (long)G3, (long)(w0 * 32), (long)nw, threshold, grid);
        if (hipGetLastError() != hipSuccess) return NVSR_ERR_LAUNCH;
    }
    // `dilate` rounds between the two buffers; an odd number ends in the workspace and is copied back
    uint32_t* src = grid;
    uint32_t* dst = other;
    for (int r = 0; r < dilate; ++r) {
        hipLaunchKernelGGL(occupancy_dilate_kernel, dim3(blocks256(words)), dim3(256), 0, st, src, dst, G, (long)words);
        uint32_t* t = src; src = dst; dst = t;
    }
    if (src != grid && hipMemcpyAsync(grid, src, (size_t)words * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) return NVSR_ERR_LAUNCH;
    return NVSR_CHECK_LAUNCH();
}
}  // namespace

// ---- generic decoder geometries: the keep mask of a point list -----------------------------------------------------------------------------
// A thread per point of x [P, 6].  n = the normalised position exactly as gen_position forms it (no jitter).  KEPT iff a coordinate of n is NaN,
// or lies outside the box (|n[a]| > 1: a generic geometry may sample its planes through rotated frames, where border padding clamps the
// PROJECTED coordinates -- a point outside the box does not have its clamped cell's features), or the cell's bit is set.  keep[p] = 1.0f / 0.0f
// (the live list builder reads it as weights); a culled point gets the raw row [+0, +0, +0, NVSR_CULLED_SIGMA], a kept row is left alone.
__global__ __launch_bounds__(256) void generic_occupancy_keep_kernel(SceneDevN sc, long P, const float* __restrict__ x, const uint32_t* __restrict__ grid, int G,
                                                                     float* __restrict__ keep, float* __restrict__ raw) {
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    float n0, n1, n2;
    gen_position(sc, x + p * 6, nullptr, p, n0, n1, n2);
    bool k = n0 != n0 || n1 != n1 || n2 != n2 || fabsf(n0) > 1.0f || fabsf(n1) > 1.0f || fabsf(n2) > 1.0f;
    if (!k) {
        const int i = (occupancy_cell(n2, G) * G + occupancy_cell(n1, G)) * G + occupancy_cell(n0, G);      // < 2^27
        k = (grid[i >> 5] >> (i & 31)) & 1u;
    }
    keep[p] = k ? 1.0f : 0.0f;
    if (!k) {
        const f32x4 row = {0.0f, 0.0f, 0.0f, NVSR_CULLED_SIGMA};
        *reinterpret_cast<f32x4*>(raw + p * 4) = row;
    }
}

}  // namespace nvsr

extern "C" int nvsr_occupancy_build(const nvsr_scene* scene, const float* packed_decoder, int G, int K, float threshold, int dilate, int arithmetic, uint32_t* grid,
                                    float* workspace, nvsr_stream_t stream) {
    if (!build_shape_ok(G, K) || dilate < 0 || nvsr_internal_resolve_decoder_arith(arithmetic) < 0) return NVSR_ERR_SHAPE;
    if (int e = check_scene(scene)) return e;
    if (!packed_decoder || !grid || !workspace) return NVSR_ERR_NULL;
    if (!aligned16(packed_decoder) || !aligned16(workspace)) return NVSR_ERR_ALIGN;
    return occupancy_build_slabs(scene->lo, scene->range, G, K, threshold, dilate, grid, workspace, (hipStream_t)stream,
                                 [&](int64_t P, const float* x, float* out) { return nvsr_triplane_decode_arith(scene, packed_decoder, P, x, out, arithmetic, stream); });
}

// the same build for a generic decoder geometry: the decode in the middle is the fused kernel's density phase (GF_DENSITY) in `arith`
extern "C" int nvsr_generic_occupancy_build_ext(const nvsr_scene_ext* scene, const nvsr_decoder_geometry* geometry, const float* natural, const float* packed,
                                                int G, int K, float threshold, int dilate, int arith, uint32_t* grid, float* workspace, nvsr_stream_t stream) {
    if (!build_shape_ok(G, K) || dilate < 0) return NVSR_ERR_SHAPE;
    GenGeom g;
    GenFusedPlan pl;
    if (int e = gf_check_capacity(scene, geometry, &g, [&](const GenGeom& gg) { return gen_fused_plan_arith(gg, &pl, arith); })) return e;      // (nothing launched)
    if (!natural || (arith == NVSR_ARITH_F16X2 && !packed) || !grid || !workspace) return NVSR_ERR_NULL;
    if (!aligned16(workspace)) return NVSR_ERR_ALIGN;
    return occupancy_build_slabs(scene->lo, scene->range, G, K, threshold, dilate, grid, workspace, (hipStream_t)stream, [&](int64_t P, const float* x, float* out) {
        return nvsr_generic_decode_fused_density_arith_ext(scene, geometry, natural, packed, P, x, nullptr, out, arith, stream);
    });
}

extern "C" int nvsr_generic_occupancy_keep(const nvsr_scene_ext* scene, int64_t P, const float* x, const uint32_t* grid, int G, float* keep, float* raw,
                                           nvsr_stream_t stream) {
    if (int e = gen_check_ext(scene)) return e;
    if (G < 1 || G > OCC_MAX_G || P < 0 || (P + 255) / 256 > 0x7fffffff) return NVSR_ERR_SHAPE;
    if (P == 0) return NVSR_OK;
    if (!x || !grid || !keep || !raw) return NVSR_ERR_NULL;
    if (!aligned16(raw)) return NVSR_ERR_ALIGN;
    // (the kernel reads lo and range only: the planes of the scene need not be set)
    SceneDevN sc = {};
    for (int i = 0; i < 5; ++i) { sc.lo[i] = scene->lo[i]; sc.range[i] = scene->range[i]; }
    hipLaunchKernelGGL(generic_occupancy_keep_kernel, dim3(blocks256(P)), dim3(256), 0, (hipStream_t)stream, sc, (long)P, x, grid, G, keep, raw);
    return NVSR_CHECK_LAUNCH();
}

// ---- internal hooks (tests and tools) ---------------------------------------------------------------------------------------------------
// the probe kernel alone over the whole grid: x [G^3 K^3, 6]
extern "C" int nvsr_internal_occupancy_probes(const nvsr_scene* scene, int G, int K, float* x, nvsr_stream_t stream) {
    if (!scene || !x) return NVSR_ERR_NULL;
    if (!build_shape_ok(G, K)) return NVSR_ERR_SHAPE;
    const int64_t G3 = (int64_t)G * G * G, P = G3 * K * K * K;
    if ((P + 255) / 256 > 0x7fffffff) return NVSR_ERR_SHAPE;
    hipLaunchKernelGGL(occupancy_probe_kernel, dim3(blocks256(P)), dim3(256), 0, (hipStream_t)stream, scene->lo[0], scene->lo[1], scene->lo[2], scene->range[0],
                       scene->range[1], scene->range[2], G, K, 0L, (long)G3, x);
    return NVSR_CHECK_LAUNCH();
}
// the cull kernel alone: kept [N, S], kept_n [N] (z = NULL: the depths of nvsr_coarse_z without jitter, from the rays' near / far)
extern "C" int nvsr_internal_occupancy_cull(const nvsr_scene* scene, int64_t N, int S, const float* rays, const float* z, int lindisp, const uint32_t* grid, int G,
                                            int* kept, int* kept_n, nvsr_stream_t stream) {
    if (!scene || !rays || !grid || !kept || !kept_n) return NVSR_ERR_NULL;
    if (G < 1 || G > OCC_MAX_G || N < 1 || S < 1 || (N + CULL_WAVES - 1) / CULL_WAVES > 0x7fffffff) return NVSR_ERR_SHAPE;
    launch_occupancy_cull(to_dev(scene), N, S, rays, z, lindisp, grid, G, kept, kept_n, (hipStream_t)stream);
    return NVSR_CHECK_LAUNCH();
}
