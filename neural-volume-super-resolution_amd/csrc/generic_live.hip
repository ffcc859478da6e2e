// The live list of a frame in two phases (generic decoder geometries): from the compositing weights w[P], the ascending list of the points p with
// !(w[p] == 0) -- NaN is live, +0.0 and -0.0 are dead -- and their number, both on the device.  The colour phase of the fused kernels
// (generic_fused_core.h: GF_COLOUR) reads them without a host round trip.
//
// Two launches, no atomics, so the list is the same on every run:
//   generic_live_count_kernel  workgroup b counts the live points of its span [b span, (b + 1) span), span = 256 x rounds, into counts[b]
//   generic_live_list_kernel   workgroup b adds up counts[0 .. b) -- integer sums, 256 threads strided over at most LIVE_MAX_GROUPS words -- and
//                              writes its span's live points behind them: per round of 256 consecutive points a ballot / mbcnt prefix within
//                              each wave and a scan over the four waves' counts in LDS.  The last workgroup writes the total.
// `rounds` grows with P so that there are never more than LIVE_MAX_GROUPS workgroups: the sum in front of a workgroup stays a few loads per thread.
#include "nvsr_common.h"

namespace nvsr {

constexpr int LIVE_TPB = 256, LIVE_WAVES = LIVE_TPB / 64, LIVE_MIN_ROUNDS = 8, LIVE_MAX_GROUPS = 4096;

struct LivePlan {
    int rounds;          // rounds of 256 points per workgroup
    long groups;         // workgroups = counts
};
static inline LivePlan live_plan(long P) {
    LivePlan pl;
    const long per = ((P + LIVE_MAX_GROUPS - 1) / LIVE_MAX_GROUPS + LIVE_TPB - 1) / LIVE_TPB;
    pl.rounds = per < LIVE_MIN_ROUNDS ? LIVE_MIN_ROUNDS : (int)per;
    const long span = (long)pl.rounds * LIVE_TPB;
    pl.groups = (P + span - 1) / span;
    return pl;
}

__device__ __forceinline__ bool live_at(const float* __restrict__ w, long p, long P) { return p < P && !(w[p] == 0.0f); }

__global__ __launch_bounds__(LIVE_TPB) void generic_live_count_kernel(long P, int rounds, const float* __restrict__ w, int* __restrict__ counts) {
    __shared__ int part[LIVE_WAVES];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const long base = (long)blockIdx.x * rounds * LIVE_TPB;
    int c = 0;                                            // (wave-uniform: every lane counts its wave's ballots)
    for (int r = 0; r < rounds; ++r) c += __popcll(__ballot(live_at(w, base + (long)r * LIVE_TPB + tid, P)));
    if (lane == 0) part[wave] = c;
    __syncthreads();
    if (tid == 0) {
        int s = 0;
        for (int v = 0; v < LIVE_WAVES; ++v) s += part[v];
        counts[blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(LIVE_TPB) void generic_live_list_kernel(long P, int rounds, const float* __restrict__ w, const int* __restrict__ counts,
                                                                     int* __restrict__ index, int* __restrict__ count) {
    __shared__ int part[LIVE_WAVES], wave_n[2][LIVE_WAVES];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, b = blockIdx.x;
    // the live points in front of this workgroup
    int c = 0;
    for (int i = tid; i < b; i += LIVE_TPB) c += counts[i];
#pragma unroll
    for (int d = 32; d; d >>= 1) c += __shfl_xor(c, d);
    if (lane == 0) part[wave] = c;
    __syncthreads();
    int at = 0;
    for (int v = 0; v < LIVE_WAVES; ++v) at += part[v];
    if (b == (int)gridDim.x - 1 && tid == 0) *count = at + counts[b];
    // its own, round by round (wave_n is double-buffered: one barrier per round)
    const long base = (long)b * rounds * LIVE_TPB;
    for (int r = 0; r < rounds; ++r) {
        const long p = base + (long)r * LIVE_TPB + tid;
        if (base + (long)r * LIVE_TPB >= P) break;        // (uniform over the workgroup)
        const bool live = live_at(w, p, P);
        const unsigned long long m = __ballot(live);
        const int before = __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
        if (lane == 0) wave_n[r & 1][wave] = __popcll(m);
        __syncthreads();
        int mine = at, all = 0;
        for (int v = 0; v < LIVE_WAVES; ++v) {
            const int nv = wave_n[r & 1][v];
            if (v < wave) mine += nv;
            all += nv;
        }
        if (live) index[mine + before] = (int)p;
        at += all;
    }
}

}  // namespace nvsr

using namespace nvsr;

extern "C" {

int64_t nvsr_generic_live_list_workspace_bytes(int64_t P) {
    if (P < 0 || P > 0x7fffffffL) return -NVSR_ERR_SHAPE;
    return (int64_t)sizeof(int) * (P ? live_plan((long)P).groups : 1);
}

int nvsr_generic_live_list(int64_t P, const float* w, int32_t* index_out, int32_t* count_dev, void* workspace, nvsr_stream_t stream) {
    if (P < 0 || P > 0x7fffffffL) return NVSR_ERR_SHAPE;            // (int32 indices)
    if (!count_dev) return NVSR_ERR_NULL;
    hipStream_t s = (hipStream_t)stream;
    if (P == 0) return hipMemsetAsync(count_dev, 0, sizeof(int32_t), s) == hipSuccess ? NVSR_OK : NVSR_ERR_LAUNCH;
    if (!w || !index_out || !workspace) return NVSR_ERR_NULL;
    const LivePlan pl = live_plan((long)P);
    int* counts = static_cast<int*>(workspace);
    hipLaunchKernelGGL(generic_live_count_kernel, dim3((unsigned)pl.groups), dim3(LIVE_TPB), 0, s, (long)P, pl.rounds, w, counts);
    if (int e = NVSR_CHECK_LAUNCH()) return e;
    hipLaunchKernelGGL(generic_live_list_kernel, dim3((unsigned)pl.groups), dim3(LIVE_TPB), 0, s, (long)P, pl.rounds, w, counts, index_out, count_dev);
    return NVSR_CHECK_LAUNCH();
}

}  // extern "C"
