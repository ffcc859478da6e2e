// Host-side bookkeeping of the two-phase route's scratch (csrc/colour_order.hip: the lists, the group table, the point-major pass's points and
// views, the occupancy route's kept lists and their group table -- grow-only buffers per (device, stream), released together) as a stand-alone CPU program for the sanitizers.  The HIP allocation and
// device calls the bookkeeping makes are defined HERE on the host heap (the executable's definitions win over the runtime library's), so the
// program needs no GPU, launches no kernel, and AddressSanitizer sees every buffer the bookkeeping allocates, frees or forgets:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Iinclude -Xarch_host -fsanitize=address,undefined \
//         neural-volume-super-resolution_amd/csrc/colour_order.hip tools/colour_scratch_host_check.hip -o /tmp/colour_scratch_host_check
//   /tmp/colour_scratch_host_check          (prints "ok"; a leak of a buffer is counted by the stubs themselves)
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <vector>

#include "../neural-volume-super-resolution_amd/csrc/colour_order.h"
#include "../neural-volume-super-resolution_amd/csrc/occupancy.h"
#include "../neural-volume-super-resolution_amd/csrc/nvsr_internal.h"

static std::set<void*> g_live_allocs;
static size_t g_bytes = 0, g_allocs = 0;
static int g_fail_in = 0;      // > 0: that allocation from now fails, once
static int g_device = 0;

extern "C" {
hipError_t hipMalloc(void** p, size_t bytes) {
    if (g_fail_in > 0 && --g_fail_in == 0) return hipErrorOutOfMemory;
    *p = malloc(bytes ? bytes : 1);
    g_live_allocs.insert(*p); g_bytes += bytes; ++g_allocs;
    return hipSuccess;
}
hipError_t hipFree(void* p) {
    if (!g_live_allocs.erase(p)) { fprintf(stderr, "hipFree of a pointer that is not live\n"); abort(); }
    free(p);
    return hipSuccess;
}
hipError_t hipGetDevice(int* d) { *d = g_device; return hipSuccess; }
hipError_t hipSetDevice(int d) { g_device = d; return hipSuccess; }
hipError_t hipGetLastError(void) { return hipSuccess; }
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind, hipStream_t) { memcpy(dst, src, bytes); return hipSuccess; }
hipError_t hipStreamIsCapturing(hipStream_t, hipStreamCaptureStatus* s) { *s = hipStreamCaptureStatusNone; return hipSuccess; }
}

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

int main() {
    using namespace nvsr;
    const hipStream_t s0 = nullptr, s1 = reinterpret_cast<hipStream_t>(0x10);
    auto lists_bytes = [](int64_t N, int S) { return (int64_t)(2 * 4 * N * S + 4 * N); };
    LiveLists ll;
    KeptLists kl;
    // one pass's acquisition (colour_order.h), as the pass launcher calls it: a plain pass takes the two-phase route or not; an occupancy pass takes its own or not
    auto plain_pass = [&](const float* raw_out, int64_t N, int S, hipStream_t s) { return acquire_pass_scratch(N, S, s, raw_out != nullptr, false, true, ll, kl) == PassRoute::TwoPhase; };
    auto occupancy_pass = [&](int64_t N, int S, hipStream_t s) { return acquire_pass_scratch(N, S, s, false, true, true, ll, kl) == PassRoute::Occupancy; };
    CHECK(nvsr_render_scratch_bytes() == 0);
    // point-major route: four buffers per (device, stream)
    unsetenv("NVSR_COLOUR_POINTS");
    CHECK(plain_pass(nullptr, 4609, 8, s0) && ll.pts && ll.steps && ll.views && g_live_allocs.size() == 4);
    CHECK(ll.steps == ll.pts + (size_t)19 * 256 * 8 && ll.trip == ll.slot + 19);
    static_cast<char*>(static_cast<void*>(ll.views))[(size_t)19 * 256 * POINT_VIEW_FLOATS * 4 - 1] = 1;      // the last byte of each buffer is the buffer's
    reinterpret_cast<char*>(ll.steps + 2 * 19)[-1] = 1;
    reinterpret_cast<char*>(ll.n + 4609)[-1] = 1;
    CHECK(nvsr_render_scratch_bytes() == lists_bytes(4609, 8));
    // growth: larger S, then larger N; a smaller launch afterwards grows nothing
    CHECK(plain_pass(nullptr, 4609, 24, s0) && g_live_allocs.size() == 4 && nvsr_render_scratch_bytes() == lists_bytes(4609, 24));
    CHECK(plain_pass(nullptr, 8705, 24, s0) && g_live_allocs.size() == 4 && nvsr_render_scratch_bytes() == lists_bytes(8705, 24));
    const size_t allocs = g_allocs;
    CHECK(plain_pass(nullptr, 4609, 8, s0) && g_allocs == allocs && nvsr_render_scratch_bytes() == lists_bytes(8705, 24));
    // what a launch leaves behind is asked for with its own N / G
    int dst[64];
    CHECK(nvsr_internal_copy_live_counts(dst, 8705, (nvsr_stream_t)s0) == NVSR_ERR_SHAPE);
    CHECK(nvsr_internal_copy_point_steps(dst, 35, (nvsr_stream_t)s0) == NVSR_ERR_SHAPE);
    // a reservation leaves no launch behind; a second stream has buffers of its own
    nvsr_internal_reserve_render_scratch(1000, 16, (nvsr_stream_t)s1);
    CHECK(g_live_allocs.size() == 8 && nvsr_render_scratch_bytes() == lists_bytes(8705, 24) + lists_bytes(1000, 16));
    CHECK(nvsr_internal_copy_live_counts(dst, 1000, (nvsr_stream_t)s1) == NVSR_ERR_SHAPE);
    // the handle off: the lockstep kernels, no growth of the points' buffers
    setenv("NVSR_COLOUR_POINTS", "0", 1);
    CHECK(plain_pass(nullptr, 20000, 24, s1) && !ll.pts && !ll.steps && !ll.views && g_live_allocs.size() == 8);
    CHECK(nvsr_internal_copy_point_steps(dst, (20000 + 255) / 256, (nvsr_stream_t)s1) == NVSR_ERR_SHAPE);      // that launch left no steps
    unsetenv("NVSR_COLOUR_POINTS");
    // a points buffer that cannot be had (the third allocation: group table, lists, points): the lockstep kernels, the lists stay
    g_fail_in = 3;
    CHECK(plain_pass(nullptr, 30000, 24, s1) && !ll.pts && ll.z && g_fail_in == 0);
    CHECK(plain_pass(nullptr, 30000, 24, s1) && ll.pts && ll.views);          // the next launch has it
    // the routes that decline: raw outputs, S beyond a packed entry, the one-phase handle
    float raw = 0;
    CHECK(!plain_pass(&raw, 1000, 8, s0) && !plain_pass(nullptr, 1000, ORDER_MAX_S, s0));
    setenv("NVSR_RENDER_ONE_PHASE", "1", 1);
    CHECK(!plain_pass(nullptr, 1000, 8, s0));
    unsetenv("NVSR_RENDER_ONE_PHASE");
    // the occupancy route: the kept lists (N S + N ints) and their group table, beside the others and not counted; a plain launch leaves them alone
    {
        const hipStream_t s2 = reinterpret_cast<hipStream_t>(0x20);
        CHECK(nvsr_internal_copy_kept_counts(dst, 300, (nvsr_stream_t)s2) == NVSR_ERR_SHAPE);       // none ran
        const size_t before = g_live_allocs.size();
        const int64_t counted = nvsr_render_scratch_bytes();
        CHECK(occupancy_pass(300, 4, s2) && g_live_allocs.size() == before + 6 && nvsr_render_scratch_bytes() == counted + lists_bytes(300, 4));
        CHECK(kl.n == kl.idx + 300 * 4 && kl.trip == kl.slot + 2 && ll.z && ll.pts);
        reinterpret_cast<char*>(kl.n + 300)[-1] = 1;                                                // the last byte of each buffer is the buffer's
        reinterpret_cast<char*>(kl.trip + 2)[-1] = 1;
        for (int i = 0; i < 300; ++i) kl.n[i] = i;
        int got[300];
        CHECK(nvsr_internal_copy_kept_counts(got, 300, (nvsr_stream_t)s2) == NVSR_OK && got[299] == 299);
        CHECK(nvsr_internal_copy_kept_counts(got, 301, (nvsr_stream_t)s2) == NVSR_ERR_SHAPE);       // asked for with the launch's own N
        CHECK(nvsr_internal_copy_live_counts(got, 300, (nvsr_stream_t)s2) == NVSR_OK);              // the two-phase launch it is part of
        // growth forgets the latest launch's counts until the launch that grew it is recorded; a smaller launch grows nothing
        CHECK(occupancy_pass(900, 8, s2) && g_live_allocs.size() == before + 6);
        CHECK(nvsr_internal_copy_kept_counts(got, 300, (nvsr_stream_t)s2) == NVSR_ERR_SHAPE);
        const size_t allocs2 = g_allocs;
        CHECK(occupancy_pass(300, 4, s2) && g_allocs == allocs2);
        // a plain two-phase launch keeps the kept lists of the latest occupancy launch; a declining occupancy launch forgets them
        CHECK(plain_pass(nullptr, 300, 4, s2) && nvsr_internal_copy_kept_counts(got, 300, (nvsr_stream_t)s2) == NVSR_OK);
        CHECK(!occupancy_pass(300, ORDER_MAX_S, s2) && nvsr_internal_copy_kept_counts(got, 300, (nvsr_stream_t)s2) == NVSR_ERR_SHAPE);
        // kept lists that cannot be had (the first allocation of a larger launch's kept buffers: the group table): the route declines, the plain lists stay
        CHECK(plain_pass(nullptr, 5000, 8, s2));
        g_fail_in = 1;
        // (the one acquisition of that pass answers the plain route and records it as the plain launch it becomes -- the caller asks no second time)
        std::vector<int> got5000(5000);
        CHECK(!occupancy_pass(5000, 8, s2) && g_fail_in == 0 && ll.z && nvsr_internal_copy_live_counts(got5000.data(), 5000, (nvsr_stream_t)s2) == NVSR_OK);
        CHECK(nvsr_internal_copy_kept_counts(got5000.data(), 5000, (nvsr_stream_t)s2) == NVSR_ERR_SHAPE);
        CHECK(occupancy_pass(5000, 8, s2));
    }
    // release: everything, on every stream; later launches allocate anew
    CHECK(nvsr_release_render_scratch() == NVSR_OK && g_live_allocs.empty() && nvsr_render_scratch_bytes() == 0);
    CHECK(plain_pass(nullptr, 300, 4, s0) && g_live_allocs.size() == 4);
    CHECK(nvsr_release_render_scratch() == NVSR_OK && g_live_allocs.empty());
    printf("ok: %zu allocations, %zu bytes, none left\n", g_allocs, g_bytes);
    return 0;
}
