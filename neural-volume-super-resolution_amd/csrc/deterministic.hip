// Deterministic route of the tri-plane training step: the plane gradients without float atomics.
//
// The limb backward's ROWS variant (render_bwd_limb.hip) leaves every point's feature gradient as a plain row rows[d][m][48]; here
//   nvsr_internal_plane_taps   emits, with the backward kernel's own tap functions (bwd_core.h ray_pos_taps, decode_core.h view_taps), the four
//                              texels and bilinear weights of every point (planes 0..2) or ray (view plane) in the order nw, ne, sw, se;
//   nvsr_rows_scatter          adds the weighted rows into a channel-last gradient plane IN A FIXED ORDER (include/nvsr.h has the contract):
//                              the entries e = 4 m + j are sorted stably by texel (rocPRIM radix sort: deterministic, O(M)) and one wave per
//                              texel gathers its segment in ascending e.
// Nothing here allocates, creates a stream or synchronises: the sort's temporary storage is part of the caller's workspace.
#include "bwd_core.h"
#include "nvsr_internal.h"

#if !defined(__has_include)
#error "deterministic.hip needs __has_include to find rocPRIM"
#elif !__has_include(<rocprim/rocprim.hpp>)
#error "deterministic.hip needs rocPRIM (rocprim/rocprim.hpp under the ROCm include directory): nvsr_rows_scatter sorts with rocprim::radix_sort_pairs; there is no build of this library without the deterministic route"
#endif
#include <cstring>      // (rocPRIM's texture iterator calls memset without including it)
#include <rocprim/rocprim.hpp>

namespace nvsr {

// one thread per point (d < 3: m = ray * S + s) or per ray (d == 3: m = ray)
__global__ __launch_bounds__(256) void plane_taps_kernel(SceneDev sc, int d, long N, int S, const float* __restrict__ rays, const float* __restrict__ z,
                                                         int* __restrict__ texel, float* __restrict__ weight) {
    typedef int i32x4 __attribute__((ext_vector_type(4)));
    const long m = (long)blockIdx.x * 256 + threadIdx.x;
    const long M = d < 3 ? N * S : N;
    if (m >= M) return;
    Taps t;
    if (d < 3) {
        const long ray = m / S;
        int ix, iy;
        t = ray_pos_taps(sc, rays + ray * 11, z[m], d, ix, iy);
    } else {
        const float* r = rays + m * 11;
        t = view_taps(sc, r[8], r[9], r[10]);
    }
    reinterpret_cast<i32x4*>(texel)[m] = i32x4{t.o00 / C, t.o01 / C, t.o10 / C, t.o11 / C};
    reinterpret_cast<f32x4*>(weight)[m] = f32x4{t.nw, t.ne, t.sw, t.se};
}

// One wave per texel t: its entries are the segment [a, b) of the sorted keys; ids[a..b) are their entry numbers e in ascending order (the sort is
// stable and the values went in ascending).  Lane = channel.  64 ids and weights are loaded at once and walked with v_readlane; RS_AHEAD rows are
// loaded ahead of the additions that consume them, so that only the additions are serial.  Cost: linear in b - a.
constexpr int RS_AHEAD = 16;
__global__ __launch_bounds__(256) void rows_gather_kernel(long E, int ntexels, const unsigned* __restrict__ keys, const unsigned* __restrict__ ids,
                                                          const float* __restrict__ rows, const float* __restrict__ weight, float* __restrict__ g) {
    const int lane = threadIdx.x & 63;
    const int t = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    if (t >= ntexels) return;
    // lower bounds of t and t + 1 in the sorted keys
    long lo = 0, hi = E;
    while (lo < hi) { const long mid = (lo + hi) >> 1; if (keys[mid] < (unsigned)t) lo = mid + 1; else hi = mid; }
    long lo2 = lo;
    hi = E;
    while (lo2 < hi) { const long mid = (lo2 + hi) >> 1; if (keys[mid] <= (unsigned)t) lo2 = mid + 1; else hi = mid; }
    const int a = __builtin_amdgcn_readfirstlane((int)lo), b = __builtin_amdgcn_readfirstlane((int)lo2);
    if (a == b) return;                                             // a texel no entry names is not written
    const int ch = lane < C ? lane : C - 1;                         // (lanes 48..63 run along on the last channel and write nothing)
    float s = 0.0f;
    for (int base = a; base < b; base += 64) {
        const int n = b - base < 64 ? b - base : 64;                // (wave-uniform)
        const unsigned id = lane < n ? ids[base + lane] : 0u;
        const float w = lane < n ? weight[id] : 0.0f;
        for (int j = 0; j < n; j += RS_AHEAD) {
            const int cnt = n - j < RS_AHEAD ? n - j : RS_AHEAD;    // (wave-uniform)
            float v[RS_AHEAD], wj[RS_AHEAD];
#pragma unroll
            for (int k = 0; k < RS_AHEAD; ++k) {
                const int jj = j + k < n ? j + k : n - 1;
                const unsigned e = (unsigned)__builtin_amdgcn_readlane((int)id, jj);
                wj[k] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(w), jj));
                v[k] = rows[(long)(e >> 2) * C + ch];               // (a clamped slot re-reads the segment's last row: in bounds, not added)
            }
#pragma unroll
            for (int k = 0; k < RS_AHEAD; ++k)
                if (k < cnt) s = __fadd_rn(s, __fmul_rn(v[k], wj[k]));
        }
    }
    if (lane < C) {
        float* p = g + (long)t * C + lane;
        *p = __fadd_rn(*p, s);
    }
}

// The sort's configuration, fixed here rather than left to rocPRIM's per-device default: 8 radix bits per pass over 256 x 12 items per
// block with the `basic` block ranking.  The default for this key / value pair picks the `match` ranking, whose one-sweep kernel keeps a
// per-lane array in scratch memory (64-80 B per lane); this one uses none, like every other kernel of the library (tools/kernel_resources.py).
using RowsSortConfig =
    rocprim::radix_sort_config<rocprim::default_config, rocprim::default_config,
                               rocprim::radix_sort_onesweep_config<rocprim::kernel_config<256, 12>, rocprim::kernel_config<256, 12>, 8,
                                                                   rocprim::block_radix_rank_algorithm::basic>>;

inline int64_t round256(int64_t n) { return (n + 255) / 256 * 256; }
// rocPRIM's temporary storage for E pairs of 32-bit words: its own double buffers (8 E bytes) + the look-back states of its blocks; reserved with
// a margin and checked against what rocPRIM asks for at every call
inline int64_t sort_temp_bytes(int64_t E) { return round256(16 * E) + (1 << 20); }

}  // namespace nvsr

using namespace nvsr;

extern "C" {

int nvsr_internal_plane_taps(const nvsr_scene* scene, int d, int64_t N, int S, const float* rays, const float* z, int32_t* texel, float* weight,
                             nvsr_stream_t stream) {
    if (!scene || !rays || !texel || !weight || (d >= 0 && d < 3 && !z)) return NVSR_ERR_NULL;
    if (d < 0 || d > 3) return NVSR_ERR_SHAPE;
    if (int e = check_scene(scene)) return e;
    if (!aligned16(texel) || !aligned16(weight)) return NVSR_ERR_ALIGN;
    if (N < 0 || S < 1 || S > 4096) return NVSR_ERR_SHAPE;
    const int64_t M = d < 3 ? N * (int64_t)S : N;
    if (M >= (int64_t)1 << 29) return NVSR_ERR_SHAPE;
    if (M == 0) return NVSR_OK;
    hipLaunchKernelGGL(plane_taps_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, (hipStream_t)stream, to_dev(scene), d, (long)N, S, rays, z,
                       texel, weight);
    return NVSR_CHECK_LAUNCH();
}

int64_t nvsr_rows_scatter_workspace_bytes(int64_t M) {
    if (M < 0 || M >= (int64_t)1 << 29) return 0;
    const int64_t E = 4 * M;
    return 2 * round256(4 * E) + sort_temp_bytes(E);               // sorted keys, sorted ids, rocPRIM's temporary storage
}

int nvsr_rows_scatter(int64_t M, const float* rows, const int32_t* texel, const float* weight, int H, int W, float* g, void* workspace,
                      int64_t workspace_bytes, nvsr_stream_t stream) {
    if (!rows || !texel || !weight || !g || !workspace) return NVSR_ERR_NULL;
    if (!aligned16(rows) || !aligned16(texel) || !aligned16(weight) || !aligned16(g) || !aligned16(workspace)) return NVSR_ERR_ALIGN;
    if (M < 0 || M >= (int64_t)1 << 29 || H < 1 || W < 1 || (int64_t)H * W * C >= (int64_t)1 << 31) return NVSR_ERR_SHAPE;
    if (workspace_bytes < nvsr_rows_scatter_workspace_bytes(M)) return NVSR_ERR_SHAPE;
    if (M == 0) return NVSR_OK;
    const int64_t E = 4 * M;
    const int ntexels = H * W;
    char* ws = static_cast<char*>(workspace);
    unsigned* keys = reinterpret_cast<unsigned*>(ws);
    unsigned* ids = reinterpret_cast<unsigned*>(ws + round256(4 * E));
    void* temp = ws + 2 * round256(4 * E);
    unsigned end_bit = 1;
    while (end_bit < 32 && ((int64_t)1 << end_bit) < ntexels) ++end_bit;      // the keys are texel numbers < H * W
    const unsigned* keys_in = reinterpret_cast<const unsigned*>(texel);
    const rocprim::counting_iterator<unsigned> ids_in(0u);                     // entry e carries the value e
    size_t need = 0;
    if (rocprim::radix_sort_pairs<RowsSortConfig>(nullptr, need, keys_in, keys, ids_in, ids, (unsigned)E, 0u, end_bit, (hipStream_t)stream) != hipSuccess)
        return NVSR_ERR_LAUNCH;
    if ((int64_t)need > sort_temp_bytes(E)) return NVSR_ERR_SHAPE;
    need = (size_t)sort_temp_bytes(E);
    if (rocprim::radix_sort_pairs<RowsSortConfig>(temp, need, keys_in, keys, ids_in, ids, (unsigned)E, 0u, end_bit, (hipStream_t)stream) != hipSuccess)
        return NVSR_ERR_LAUNCH;
    hipLaunchKernelGGL(rows_gather_kernel, dim3((unsigned)((ntexels + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (long)E, ntexels, keys, ids, rows,
                       weight, g);
    return NVSR_CHECK_LAUNCH();
}

}  // extern "C"
