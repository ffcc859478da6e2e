// Low-rank feature planes (reference models.py:223-230 `gen_plane`): a position plane stored as ONE parameter F [1,C,R,2r], U = F[..., :r],
// V = F[..., r:], plane[0,c,y,x] = sum_k U[c,y,k] V[c,x,k].
//
//   lowrank_generate_kernel   F (NCHW) -> plane, CHANNEL-LAST [R][R][C] (what the render kernels sample; no re-layout pass)
//   lowrank_backward_kernel   channel-last gradient plane G [R][R][C] + F -> dF [C][R][2r]:
//                             dU[c,y,k] = sum_x G[y,x,c] V[c,x,k],  dV[c,x,k] = sum_y G[y,x,c] U[c,y,k]
//
// Both run in exact f32 on v_mfma_f32_16x16x4_f32, whose result is bit for bit the fmaf chain over ascending k.  So every output element is a
// DEFINED function of its inputs:
//   generate   acc = +0.0; for k = 0 .. r-1 ascending: acc = fmaf(U[c,y,k], V[c,x,k], acc); k is zero-padded to a multiple of 4 (both operands
//              0: fmaf(0, 0, acc) == acc)
//   backward   acc = +0.0; for x (resp. y) = 0 .. R-1 ascending: acc = fmaf(G, V (resp. U), acc), zero-padded to a multiple of 16
// No atomics, no split contraction: a workgroup owns its output tile and walks the whole contraction itself, so the results do not depend on
// the launch (a plane alone == the plane inside a ragged launch) and repeat bit for bit.
//
// All planes of a call go in ONE launch each way: a compact list of 16-row tiles over (plane, tile, ...), found by a search over <= 15 prefix sums.
// The batch dimension of the matrix products is the channel; a workgroup handles the 16 x 16 tile for a group of <= 48 channels (wave w takes
// channels w, w + 4, ...) and transposes through LDS, so that global memory sees whole texel rows
// (C floats = 192 bytes at 48 channels) on the channel-last side; with more than 48 channels a group's share of a texel row (<= 192 bytes).
// Factor rows are 8r bytes and the U | V split sits at float offset r: for odd r neither is 16-byte aligned.  The generate kernel loads
// 16 bytes per lane only where r % 4 == 0 and the tensor itself is 16-byte aligned, dwords otherwise; the backward uses dwords throughout.
#include "nvsr_common.h"

namespace nvsr {
namespace {

constexpr int LR_TILE = 16;                 // texels per tile side = the MFMA's M and N
constexpr int LR_CG = 48;                   // channels per workgroup
constexpr int LR_CP = LR_CG + 1;            // LDS texel stride (odd: the 16 texels of a fragment column fall into different banks)
constexpr int LR_WAVES = 4;
constexpr int LR_Q = LR_CG / LR_WAVES;      // channels per wave
constexpr int LR_LDS = LR_TILE * LR_TILE * LR_CP;
constexpr int LR_KB = 8;                    // MFMA k-steps per round of the generate kernel
constexpr int LR_PS = 4 * LR_KB + 4;        // row stride of an operand panel in LDS, floats
constexpr int LR_PANEL = 2 * LR_TILE * LR_PS;                           // one wave's U + V panel
static_assert(LR_WAVES * LR_PANEL <= LR_TILE * LR_TILE * LR_CP, "the panels fit into the output tile's array");
constexpr int LR_THREADS = LR_WAVES * 64;
constexpr int LR_GLOADS = LR_TILE * LR_TILE * LR_CG / LR_THREADS;       // elements of a 16 x 16 x 48 tile per thread

struct LowrankDev {
    const float* factors[NVSR_MAX_POSITION_PLANES];
    float* planes[NVSR_MAX_POSITION_PLANES];      // generate: output; backward: the gradient planes (read only)
    float* d_factors[NVSR_MAX_POSITION_PLANES];
    int res[NVSR_MAX_POSITION_PLANES], rank[NVSR_MAX_POSITION_PLANES];
    int tile_end[NVSR_MAX_POSITION_PLANES];       // running sum of the planes' work items
    int vec[NVSR_MAX_POSITION_PLANES];            // factor rows and the U | V split are 16-byte aligned: r % 4 == 0 and an aligned tensor
    int num_planes, channels;
};

__device__ __forceinline__ int find_plane(const LowrankDev& d, int item, int& local) {
    int p = 0, start = 0;
    while (p + 1 < d.num_planes && item >= d.tile_end[p]) { start = d.tile_end[p]; ++p; }
    local = item - start;
    return p;
}

// work item = (plane, y-tile, x-tile, channel group)
__global__ __launch_bounds__(LR_THREADS) void lowrank_generate_kernel(const LowrankDev d) {
    __shared__ __attribute__((aligned(16))) float lds[LR_LDS];
    NVSR_RACE_PROBE_DELAY(lds);
    int local;
    const int p = find_plane(d, (int)blockIdx.x, local);
    const int R = d.res[p], r = d.rank[p], Cc = d.channels;
    const int nt = (R + LR_TILE - 1) / LR_TILE;
    const int cg = local / (nt * nt);
    const int ty = (local - cg * nt * nt) / nt, tx = local - cg * nt * nt - ty * nt;
    const int y0 = ty * LR_TILE, x0 = tx * LR_TILE, c0 = cg * LR_CG;
    const int CH = min(LR_CG, Cc - c0);
    const float* __restrict__ F = d.factors[p];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const long row2 = 2L * r;

    // Operand panels go through LDS.  A round is one channel per wave and LR_KB k-steps: the wave brings the 16 x 32 floats of its U rows and
    // of its V rows in with 16 bytes per lane -- 8 lanes cover one row's 128-byte line, so a load instruction fetches 8 WHOLE lines (a dword per
    // lane and MFMA operand touched 16 lines for 256 bytes and left the CU's address unit, not the matrix pipe, setting the pace) -- parks
    // them in its panel (row stride 36 floats: 16-byte aligned rows, and the 16 x 4 operand reads of an MFMA fall into 64 different banks) and
    // reads the MFMA operands back.  The next round's loads are in flight while this round multiplies.  The 16-byte loads need
    // r % 4 == 0 and a 16-byte aligned factor tensor (`vec`); otherwise the same lanes load their four floats one by one, guarded.
    // The panels share the LDS array with the output tile, which is written once all rounds are done.
    const bool vec = d.vec[p] != 0;
    const int nkb = (r + 4 * LR_KB - 1) / (4 * LR_KB), nq = (CH + LR_WAVES - 1) / LR_WAVES;      // (the same rounds for every wave: barriers)
    const int prow = lane >> 3, pk = 4 * (lane & 7);
    float* __restrict__ panel = lds + w * LR_PANEL;           // U rows at [row][k], V rows at [16 + row][k]
    f32x4 g[4];                                               // U rows prow, prow + 8; V rows prow, prow + 8: floats pk .. pk + 3 of the k-block
    auto fetch = [&](int q, int kb) {
        const int cl = w + LR_WAVES * q, k = 4 * LR_KB * kb + pk;
        const long cb = (long)(c0 + min(cl, CH - 1)) * R;
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            const int row = prow + 8 * (h & 1), t0 = (h < 2 ? y0 : x0) + row;
            const float* __restrict__ src = F + (cb + min(t0, R - 1)) * row2 + (h < 2 ? 0 : r) + k;
            const bool ok = cl < CH && t0 < R;
            if (vec) {
                g[h] = (ok && k < r) ? *reinterpret_cast<const f32x4*>(src) : f32x4{0.f, 0.f, 0.f, 0.f};
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) g[h][e] = (ok && k + e < r) ? src[e] : 0.f;
            }
        }
    };
    f32x4 acc[LR_Q];
#pragma unroll
    for (int q = 0; q < LR_Q; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
    fetch(0, 0);
#pragma unroll
    for (int q = 0; q < LR_Q; ++q) {
        if (q < nq) {
            for (int kb = 0; kb < nkb; ++kb) {
                __syncthreads();                              // the previous round's operand reads are done
#pragma unroll
                for (int h = 0; h < 4; ++h)
                    *reinterpret_cast<f32x4*>(panel + ((h < 2 ? 0 : LR_TILE) + prow + 8 * (h & 1)) * LR_PS + pk) = g[h];
                __syncthreads();
                if (kb + 1 < nkb) fetch(q, kb + 1);
                else if (q + 1 < nq) fetch(q + 1, 0);
#pragma unroll
                for (int s = 0; s < LR_KB; ++s)
                    if (4 * (LR_KB * kb + s) < r)             // ascending k; A[i = y][k], B[k][j = x]
                        acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(panel[li * LR_PS + 4 * s + lk], panel[(LR_TILE + li) * LR_PS + 4 * s + lk],
                                                                      acc[q], 0, 0, 0);
            }
        }
    }
    __syncthreads();                                          // the panels are dead: the array becomes the output tile
    // D: column (x) = lane & 15, row (y) = 4 (lane >> 4) + register
#pragma unroll
    for (int q = 0; q < LR_Q; ++q) {
        const int cl = w + LR_WAVES * q;
        if (cl < CH)
#pragma unroll
            for (int e = 0; e < 4; ++e) lds[((4 * lk + e) * LR_TILE + li) * LR_CP + cl] = acc[q][e];
    }
    __syncthreads();
    // a tile row is 16 texels x CH channels: with C <= 48 one contiguous run of whole texel rows of the plane, with more channels 16 runs of
    // CH floats (192 bytes for a full group) at the texel stride
    float* __restrict__ out = d.planes[p];
    const int xn = min(LR_TILE, R - x0);
    const int dq = LR_THREADS / CH, dr = LR_THREADS - dq * CH;     // (one division per thread: the walk below adds 256 elements per step)
    for (int yy = 0; yy < LR_TILE && y0 + yy < R; ++yy) {
        float* __restrict__ orow = out + ((long)(y0 + yy) * R + x0) * Cc + c0;
        int xx = (int)threadIdx.x / CH, c = (int)threadIdx.x - xx * CH;
        while (xx < xn) {
            orow[(long)xx * Cc + c] = lds[(yy * LR_TILE + xx) * LR_CP + c];
            xx += dq; c += dr;
            if (c >= CH) { c -= CH; ++xx; }
        }
    }
}

// work item = (plane, side: 0 = dU | 1 = dV, 16-row tile of the factor, 16-column tile of its r columns, channel group)
__global__ __launch_bounds__(LR_THREADS) void lowrank_backward_kernel(const LowrankDev d) {
    __shared__ float lds[LR_LDS];
    NVSR_RACE_PROBE_DELAY(lds);
    int local;
    const int p = find_plane(d, (int)blockIdx.x, local);
    const int R = d.res[p], r = d.rank[p], Cc = d.channels;
    const int nt = (R + LR_TILE - 1) / LR_TILE, nk = (r + LR_TILE - 1) / LR_TILE;
    const int per_cg = 2 * nt * nk;
    const int cg = local / per_cg;
    int rest = local - cg * per_cg;
    const int side = rest / (nt * nk);
    rest -= side * nt * nk;
    const int t = rest / nk, kt = rest - t * nk;
    const int t0 = t * LR_TILE, kc0 = kt * LR_TILE, c0 = cg * LR_CG;
    const int CH = min(LR_CG, Cc - c0);
    const float* __restrict__ F = d.factors[p];
    const float* __restrict__ G = d.planes[p];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const long row2 = 2L * r;
    const int foff = side == 0 ? r : 0;          // dU contracts G with V, dV contracts G^T with U
    const bool kin = kc0 + li < r;
    const int dq = LR_THREADS / CH, dr = LR_THREADS - dq * CH;

    f32x4 acc[LR_Q];
#pragma unroll
    for (int q = 0; q < LR_Q; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int j0 = 0; j0 < R; j0 += LR_TILE) {     // the contraction index (x for dU, y for dV), ascending
        // G[y][x][c0 ..] of the 16 x 16 texels into lds[yy][xx][cl]; out-of-plane texels are zero
        const int gy0 = side == 0 ? t0 : j0, gx0 = side == 0 ? j0 : t0;
        // (every load of the chunk is issued before the first LDS store: one memory latency per chunk, not one per element)
        float gv[LR_GLOADS];
        {
            int t = (int)threadIdx.x / CH, c = (int)threadIdx.x - t * CH;        // texel yy * 16 + xx of the chunk, channel
#pragma unroll
            for (int i = 0; i < LR_GLOADS; ++i) {
                const int yy = t >> 4, xx = t & 15;
                gv[i] = (t < LR_TILE * LR_TILE && gy0 + yy < R && gx0 + xx < R) ? G[((long)(gy0 + yy) * R + gx0 + xx) * Cc + c0 + c] : 0.f;
                t += dq; c += dr;
                if (c >= CH) { c -= CH; ++t; }
            }
        }
        __syncthreads();
        {
            int t = (int)threadIdx.x / CH, c = (int)threadIdx.x - t * CH;
#pragma unroll
            for (int i = 0; i < LR_GLOADS; ++i) {
                if (t < LR_TILE * LR_TILE) lds[t * LR_CP + c] = gv[i];
                t += dq; c += dr;
                if (c >= CH) { c -= CH; ++t; }
            }
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int jj = 4 * s + lk;            // contraction index inside the chunk: the MFMA's k
            const bool jin = j0 + jj < R;
            // A[i = output row][k = jj]: dU: G[t0 + i][j0 + jj], dV: G[j0 + jj][t0 + i]
            const int la = (side == 0 ? li * LR_TILE + jj : jj * LR_TILE + li) * LR_CP;
#pragma unroll
            for (int q = 0; q < LR_Q; ++q) {
                const int cl = w + LR_WAVES * q;
                if (cl < CH) {
                    const float a = lds[la + cl];
                    const float b = (jin && kin) ? F[((long)(c0 + cl) * R + j0 + jj) * row2 + foff + kc0 + li] : 0.f;    // B[k = jj][j = factor column]
                    acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[q], 0, 0, 0);
                }
            }
        }
    }
    // D: column (factor column) = lane & 15, row (factor row) = 4 (lane >> 4) + register
    float* __restrict__ dF = d.d_factors[p];
    const int ooff = side == 0 ? 0 : r;
#pragma unroll
    for (int q = 0; q < LR_Q; ++q) {
        const int cl = w + LR_WAVES * q;
        if (cl < CH && kin)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int row = t0 + 4 * lk + j;
                if (row < R) dF[((long)(c0 + cl) * R + row) * row2 + ooff + kc0 + li] = acc[q][j];
            }
    }
}

// argument checks + the work list; -> number of work items, or -1
long lowrank_prepare(const nvsr_lowrank_planes_args* a, bool backward, LowrankDev& d, int& status) {
    status = NVSR_ERR_SHAPE;
    if (!a || a->num_planes < 1 || a->num_planes > NVSR_MAX_POSITION_PLANES || a->channels < 1) return -1;
    long items = 0;
    d.num_planes = a->num_planes;
    d.channels = a->channels;
    const long cgs = (a->channels + LR_CG - 1) / LR_CG;
    for (int p = 0; p < a->num_planes; ++p) {
        const long R = a->res[p], r = a->rank[p];
        if (R < 1 || r < 1 || R > 32768 || r > 32768) return -1;
        if (!a->factors[p] || !a->planes[p] || (backward && !a->d_factors[p])) { status = NVSR_ERR_NULL; return -1; }
        const long nt = (R + LR_TILE - 1) / LR_TILE, nk = (r + LR_TILE - 1) / LR_TILE;
        items += cgs * (backward ? 2 * nt * nk : nt * nt);
        if (items > 0x7fffffffL) return -1;
        d.factors[p] = a->factors[p];
        d.planes[p] = a->planes[p];
        d.d_factors[p] = backward ? a->d_factors[p] : nullptr;
        d.res[p] = (int)R;
        d.rank[p] = (int)r;
        d.tile_end[p] = (int)items;
        d.vec[p] = (r % 4 == 0 && aligned16(a->factors[p])) ? 1 : 0;
    }
    for (int p = a->num_planes; p < NVSR_MAX_POSITION_PLANES; ++p) {
        d.factors[p] = nullptr; d.planes[p] = nullptr; d.d_factors[p] = nullptr;
        d.res[p] = d.rank[p] = d.vec[p] = 0;
        d.tile_end[p] = (int)items;
    }
    status = NVSR_OK;
    return items;
}

}  // namespace
}  // namespace nvsr

extern "C" {

int nvsr_lowrank_planes(nvsr_lowrank_planes_args args, nvsr_stream_t stream) {
    nvsr::LowrankDev d;
    int status;
    const long items = nvsr::lowrank_prepare(&args, false, d, status);
    if (items < 0) return status;
    hipLaunchKernelGGL(nvsr::lowrank_generate_kernel, dim3((unsigned)items), dim3(nvsr::LR_THREADS), 0, (hipStream_t)stream, d);
    return NVSR_CHECK_LAUNCH();
}

int nvsr_lowrank_planes_backward(nvsr_lowrank_planes_args args, nvsr_stream_t stream) {
    nvsr::LowrankDev d;
    int status;
    const long items = nvsr::lowrank_prepare(&args, true, d, status);
    if (items < 0) return status;
    hipLaunchKernelGGL(nvsr::lowrank_backward_kernel, dim3((unsigned)items), dim3(nvsr::LR_THREADS), 0, (hipStream_t)stream, d);
    return NVSR_CHECK_LAUNCH();
}

}  // extern "C"
