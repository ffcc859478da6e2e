// The two-phase render route (render3.hip: density pass, then the colour decoder on the live samples) apart from its render kernels: WHICH
// ray a colour lane owns (live_order_kernel), WHICH ray block a colour workgroup runs (group_order_kernel), and the library's scratch that
// holds the live lists and both orders between the launches.  include/nvsr.h, "The two-phase render pass", is the contract.
#include "colour_order.h"
#include "nvsr_internal.h"

#include <cstdlib>
#include <initializer_list>
#include <mutex>
#include <vector>

namespace nvsr {

// ---- one counting sort for both orders ----------------------------------------------------------------------------------------------------
// One workgroup of SORT_TPB threads sorts up to SORT_MAX elements by key, LARGEST key first, elements of equal key in element order (stable).
// Wave w holds elements 256 w .. 256 w + 255 in four rounds of 64: key[r] is the key of element 256 w + 64 r + lane, 0..nkeys, or -1 for "no
// element" (elements 0..n-1 exist).  For every element: start = the first rank of its key's run (the elements of larger keys), place = its
// place in the run (the elements of its key in earlier waves + earlier rounds + lower lanes), len = the run's length; its rank is start +
// place.  Ballots and integer sums in a fixed order, no atomics.  Every thread of the workgroup calls it (three barriers); a wave without
// elements skips the ranking.  NKEYS sizes the tables: nkeys < NKEYS <= SORT_TPB.
constexpr int SORT_TPB = 1024, SORT_WAVES = SORT_TPB / 64, SORT_ROUNDS = 4, SORT_MAX = SORT_TPB * SORT_ROUNDS;
template <int NKEYS>
__device__ __forceinline__ void counting_sort(const int (&key)[SORT_ROUNDS], int nkeys, int n, int (&start)[SORT_ROUNDS], int (&place)[SORT_ROUNDS],
                                              int (&len)[SORT_ROUNDS]) {
    static_assert(NKEYS <= SORT_TPB, "one thread per key sums the tables");
    __shared__ int cnt_s[NKEYS * SORT_WAVES];      // [key][wave]: elements of the key in the wave, then in the waves before it
    __shared__ int tot_s[NKEYS], start_s[NKEYS];   // elements of a key; elements of all larger keys
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int b = 0; b <= nkeys; ++b) {
        int c = 0;
#pragma unroll
        for (int r = 0; r < SORT_ROUNDS; ++r) c += __popcll(__ballot(key[r] == b));
        if (lane == 0) cnt_s[b * SORT_WAVES + wave] = c;
    }
    __syncthreads();
    if ((int)threadIdx.x <= nkeys) {
        int run = 0;
        for (int w = 0; w < SORT_WAVES; ++w) { const int c = cnt_s[threadIdx.x * SORT_WAVES + w]; cnt_s[threadIdx.x * SORT_WAVES + w] = run; run += c; }
        tot_s[threadIdx.x] = run;
    }
    __syncthreads();
    if ((int)threadIdx.x <= nkeys) {
        int run = 0;
        for (int b = nkeys; b > (int)threadIdx.x; --b) run += tot_s[b];
        start_s[threadIdx.x] = run;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < SORT_ROUNDS; ++r) start[r] = place[r] = len[r] = 0;
    if (wave * (64 * SORT_ROUNDS) >= n) return;      // (a wave without elements)
    for (int b = 0; b <= nkeys; ++b) {
        int at = cnt_s[b * SORT_WAVES + wave];
#pragma unroll
        for (int r = 0; r < SORT_ROUNDS; ++r) {
            const unsigned long long m = __ballot(key[r] == b);
            if (key[r] == b) place[r] = at + __popcll(m & below);
            at += __popcll(m);
        }
    }
#pragma unroll
    for (int r = 0; r < SORT_ROUNDS; ++r)
        if (key[r] >= 0) { start[r] = start_s[key[r]]; len[r] = tot_s[key[r]]; }
}

// ---- the colour pass's ray order: live_n[ray] = count (density pass) -> packed entries, in place ---------------------------------------
// One workgroup per block of ORDER_RAYS consecutive rays (the last one may be ragged: M rays).  The counting sort above by bin, fullest bin
// first: bin = ceil(count * bins / S) -- 0 for an empty ray, `bins` equal bins over 1..S -- so rays of one bin keep their (patch) order and
// neighbouring pixels of similar count stay neighbouring lanes.  bins = 0 puts every ray into one bin: entry j names ray j (the identity,
// NVSR_COLOUR_ORDER=0).  The whole block is read before any entry is written.
// group_trip (may be NULL): group_trip[g] = the largest count among entries g RAYS2 .. g RAYS2 + RAYS2 - 1 of the sorted array -- the trip count
// of the colour workgroup that runs ray block g (a ragged last group counts what it has); wave w of the block reduces its group w.
static_assert(ORDER_RAYS == SORT_MAX && SORT_WAVES == ORDER_RAYS / RAYS2 && RAYS2 % 64 == 0, "one block of the order per sort, one wave of it per colour workgroup");
__global__ __launch_bounds__(SORT_TPB) void live_order_kernel(int* __restrict__ live_n, long N, int S, int bins, int* __restrict__ group_trip) {
    __shared__ int out_s[ORDER_RAYS];
    const long block_base = (long)blockIdx.x * ORDER_RAYS;
    const int M = (int)(N - block_base < ORDER_RAYS ? N - block_base : ORDER_RAYS);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int cnt[SORT_ROUNDS], bin[SORT_ROUNDS];
#pragma unroll
    for (int r = 0; r < SORT_ROUNDS; ++r) {
        const int i = wave * (64 * SORT_ROUNDS) + r * 64 + lane;
        cnt[r] = i < M ? live_n[block_base + i] : 0;
        const int b = (int)(((unsigned)cnt[r] * (unsigned)bins + (unsigned)(S - 1)) / (unsigned)S);      // (count <= S < 2^19, bins <= ORDER_BINS)
        bin[r] = i < M ? (b < bins ? b : bins) : -1;
    }
    int start[SORT_ROUNDS], place[SORT_ROUNDS], len[SORT_ROUNDS];
    counting_sort<ORDER_BINS + 1>(bin, bins, M, start, place, len);
#pragma unroll
    for (int r = 0; r < SORT_ROUNDS; ++r)
        if (bin[r] >= 0) out_s[start[r] + place[r]] = (cnt[r] << ORDER_SHIFT) | (wave * (64 * SORT_ROUNDS) + r * 64 + lane);
    __syncthreads();
#pragma unroll
    for (int r = 0; r < SORT_ROUNDS; ++r) {
        const int i = threadIdx.x + r * SORT_TPB;
        if (i < M) live_n[block_base + i] = out_s[i];
    }
    if (group_trip && wave * RAYS2 < M) {
        int m = 0;
#pragma unroll
        for (int r = 0; r < RAYS2 / 64; ++r) {
            const int i = wave * RAYS2 + r * 64 + lane;
            if (i < M) m = max(m, out_s[i] >> ORDER_SHIFT);
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) m = max(m, __shfl_xor(m, o));
        if (lane == 0) group_trip[(long)blockIdx.x * SORT_WAVES + wave] = m;
    }
}

// ---- the colour pass's order of dispatch: group_trip[G] -> group_slot[G] ------------------------------------------------------------------
// A colour workgroup takes trip steps, between none and S, and workgroups are dispatched in blockIdx order, b to XCD b % 8: in ray-block order
// a heavy group may start last on its XCD, and the eighths of the image are unequal.  group_slot[r] = the ray block that workgroup r runs: the
// G blocks sorted by trip, heaviest first, so rank r lands on XCD r % 8 -- the heavy groups start first and are dealt round the XCDs.
// Groups of EQUAL trip are worth nothing to deal one by one, and neighbouring groups share texels in their XCD's L2 (a frame whose every
// trip is S took 130 ms instead of 119 with its groups dealt one by one: profiles/colour_dispatch_ab.txt).  So a run of m equal trips, which
// occupies m consecutive ranks, is dealt in pieces: the ranks of the run that share an XCD take consecutive groups, the first 1/8 of the run
// (in group order) to the XCD of its first rank, the next to the following one -- the contiguous-eighths formula inside the run.  When every
// trip is equal that is the density kernels' mapping itself.
// One workgroup and the counting sort above over the keys 0..S.  Its limits: G <= GORDER_MAX_G groups (1 048 576 rays) and S <= GORDER_MAX_S;
// beyond either, or with sorted = 0 (NVSR_COLOUR_GROUP_ORDER=0, the A/B handle), group_slot is the mapping of the density and fused kernels:
// XCD x runs the x-th contiguous eighth of the blocks.
constexpr int GORDER_MAX_G = SORT_MAX, GORDER_MAX_S = 511;
__global__ __launch_bounds__(SORT_TPB) void group_order_kernel(const int* __restrict__ group_trip, int G, int S, int sorted, int* __restrict__ group_slot) {
    if (!sorted || G > GORDER_MAX_G || S > GORDER_MAX_S) {
        const unsigned per = (unsigned)G >> 3, rem = (unsigned)G & 7u;
        for (unsigned r = threadIdx.x; r < (unsigned)G; r += SORT_TPB) {
            const unsigned xcd = r & 7u;
            group_slot[r] = (int)(xcd * per + (xcd < rem ? xcd : rem) + (r >> 3));
        }
        return;
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int key[SORT_ROUNDS];
#pragma unroll
    for (int r = 0; r < SORT_ROUNDS; ++r) {
        const int g = wave * (64 * SORT_ROUNDS) + r * 64 + lane;
        const int t = g < G ? group_trip[g] : 0;
        key[r] = g < G ? (t < 0 ? 0 : t > S ? S : t) : -1;      // (a trip is 0..S; the clamp keeps a caller's array inside the tables)
    }
    int start[SORT_ROUNDS], place[SORT_ROUNDS], len[SORT_ROUNDS];
    counting_sort<GORDER_MAX_S + 1>(key, S, G, start, place, len);
#pragma unroll
    for (int r = 0; r < SORT_ROUNDS; ++r) {
        if (key[r] < 0) continue;
        const int run = len[r], per = run >> 3, rem = run & 7, thr = rem * (per + 1);      // the first `rem` pieces hold per + 1 groups
        const int j = place[r];
        const int k = j < thr ? j / (per + 1) : rem + (j - thr) / (per ? per : 1);                // the piece, i.e. rank % 8 inside the run
        const int i = j < thr ? j - k * (per + 1) : (j - thr) - (k - rem) * per;
        group_slot[start[r] + k + 8 * i] = wave * (64 * SORT_ROUNDS) + r * 64 + lane;
    }
}

// ---- scratch of the two-phase route: the live lists, [N, S] depths + [N, S] weights + [N] counts ------------------------------------
// Owned by the library, one buffer per (device, stream), grow-only: two launches on one stream are ordered, launches on two streams never
// share a buffer.  Growing frees the old buffer with hipFree, which waits for the device -- no launch can still be using it.
// Contract (include/nvsr.h): one host thread at a time enqueues render launches on a given (device, stream) -- the pointer is used after
// the table's lock is dropped; the entry of a destroyed stream keeps its buffer until nvsr_release_render_scratch.
// The order of dispatch (group_order_kernel) takes 2 G ints more, G = ceil(N / RAYS2): group_slot[G], then group_trip[G].  They live in a
// small buffer of their own beside the lists (20 KB at the benchmark size), with the same owner, growth and release;
// nvsr_render_scratch_bytes keeps counting the lists' buffer alone.
namespace {
struct Buffer { void* p; size_t bytes; };
struct LiveScratch { int device; hipStream_t stream; Buffer lists, group; int* last_n; int64_t last_N; };      // last_*: the counts of the latest launch
std::mutex g_live_mutex;
std::vector<LiveScratch> g_live;

LiveScratch* find_scratch(int device, hipStream_t stream) {      // (under the lock)
    for (LiveScratch& c : g_live)
        if (c.device == device && c.stream == stream) return &c;
    return nullptr;
}

// grow-only: free, forget the last launch (the new buffer holds no launch's lists or order), allocate
bool grow(LiveScratch& e, Buffer& b, size_t bytes) {
    if (b.bytes >= bytes) return true;
    if (b.p) (void)hipFree(b.p);
    b = Buffer{nullptr, 0};
    e.last_n = nullptr; e.last_N = 0;
    void* p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) { (void)hipGetLastError(); return false; }
    b = Buffer{p, bytes};
    return true;
}

// what the latest two-phase launch on (the current device, stream) left behind -> dst (device or host memory): its N packed entries, or
// (groups) its group_slot[G] + group_trip[G]; `count` must be that launch's N, or its G
int copy_left_behind(int* dst, int64_t count, bool groups, hipStream_t stream) {
    if (!dst) return NVSR_ERR_NULL;
    int device = 0;
    if (hipGetDevice(&device) != hipSuccess) return NVSR_ERR_LAUNCH;
    const int* src = nullptr;
    {
        std::lock_guard<std::mutex> lock(g_live_mutex);
        const LiveScratch* c = find_scratch(device, stream);
        if (c && c->last_n && (groups ? (c->last_N + RAYS2 - 1) / RAYS2 : c->last_N) == count) src = groups ? static_cast<const int*>(c->group.p) : c->last_n;
    }
    if (!src) return NVSR_ERR_SHAPE;
    return hipMemcpyAsync(dst, src, (groups ? 2 : 1) * (size_t)count * sizeof(int), hipMemcpyDefault, stream) == hipSuccess ? NVSR_OK : NVSR_ERR_LAUNCH;
}

// The three environment handles of the route, each read at every launch, for A/Bs: NVSR_RENDER_ONE_PHASE=1 keeps the fused kernel;
// NVSR_COLOUR_ORDER=0 makes the ray order the identity (bins = 0: the colour kernel groups its rays as the density kernel does);
// NVSR_COLOUR_GROUP_ORDER=0 makes the order of dispatch the contiguous eighths (same kernel, same table).
bool env_starts(const char* name, char c) {
    const char* e = getenv(name);
    return e && e[0] == c;
}
void launch_live_order(int* live_n, int64_t N, int S, int bins, int* group_trip, hipStream_t stream) {
    hipLaunchKernelGGL(live_order_kernel, dim3((unsigned)((N + ORDER_RAYS - 1) / ORDER_RAYS)), dim3(SORT_TPB), 0, stream, live_n, (long)N, S, bins, group_trip);
}
void launch_group_order(const int* group_trip, int64_t G, int S, int* group_slot, hipStream_t stream) {
    const int sorted = !env_starts("NVSR_COLOUR_GROUP_ORDER", '0');
    hipLaunchKernelGGL(group_order_kernel, dim3(1), dim3(SORT_TPB), 0, stream, group_trip, (int)G, S, sorted, group_slot);
}
}  // namespace

bool two_phase_lists(const float* raw_out, int64_t N, int S, hipStream_t stream, LiveLists& out, bool launch) {
    if (raw_out || S < 1 || S >= ORDER_MAX_S || env_starts("NVSR_RENDER_ONE_PHASE", '1')) return false;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) { (void)hipGetLastError(); return false; }
    int device = 0;
    if (hipGetDevice(&device) != hipSuccess) return false;
    const size_t rows = (size_t)N * (size_t)S * sizeof(float), G = (size_t)((N + RAYS2 - 1) / RAYS2);
    std::lock_guard<std::mutex> lock(g_live_mutex);
    LiveScratch* e = find_scratch(device, stream);
    if (!e) { g_live.push_back(LiveScratch{device, stream, Buffer{nullptr, 0}, Buffer{nullptr, 0}, nullptr, 0}); e = &g_live.back(); }
    if (!grow(*e, e->group, 2 * G * sizeof(int)) || !grow(*e, e->lists, 2 * rows + (size_t)N * sizeof(int)) || !e->lists.p) return false;
    char* p = static_cast<char*>(e->lists.p);
    out.z = reinterpret_cast<float*>(p);
    out.w = reinterpret_cast<float*>(p + rows);
    out.n = reinterpret_cast<int*>(p + 2 * rows);
    out.slot = static_cast<int*>(e->group.p);
    out.trip = out.slot + G;
    if (launch) { e->last_n = out.n; e->last_N = N; }      // (a reservation leaves no counts behind)
    return true;
}

void launch_colour_order(const LiveLists& ll, int64_t N, int S, hipStream_t stream) {
    launch_live_order(ll.n, N, S, env_starts("NVSR_COLOUR_ORDER", '0') ? 0 : ORDER_BINS, ll.trip, stream);
    launch_group_order(ll.trip, (N + RAYS2 - 1) / RAYS2, S, ll.slot, stream);
}

}  // namespace nvsr

using namespace nvsr;

// test hooks of the ray order (include/nvsr.h)
extern "C" int nvsr_internal_colour_order_bins(void) { return ORDER_BINS; }
extern "C" int nvsr_internal_live_order(int* live_n, int64_t N, int S, nvsr_stream_t stream) {
    if (!live_n) return NVSR_ERR_NULL;
    if (N < 1 || S < 1 || S >= ORDER_MAX_S || (N + ORDER_RAYS - 1) / ORDER_RAYS > 0x7fffffff) return NVSR_ERR_SHAPE;
    launch_live_order(live_n, N, S, ORDER_BINS, nullptr, (hipStream_t)stream);
    return NVSR_CHECK_LAUNCH();
}
extern "C" int nvsr_internal_copy_live_counts(int* dst, int64_t N, nvsr_stream_t stream) { return copy_left_behind(dst, N, false, (hipStream_t)stream); }
// test hooks of the order of dispatch (include/nvsr.h)
extern "C" int nvsr_internal_group_order(const int* trips, int64_t G, int S, int* out, nvsr_stream_t stream) {
    if (!trips || !out) return NVSR_ERR_NULL;
    if (G < 1 || G > 0x7fffffff || S < 1 || S >= ORDER_MAX_S) return NVSR_ERR_SHAPE;
    launch_group_order(trips, G, S, out, (hipStream_t)stream);
    return NVSR_CHECK_LAUNCH();
}
extern "C" int nvsr_internal_copy_group_order(int* dst, int64_t G, nvsr_stream_t stream) { return copy_left_behind(dst, G, true, (hipStream_t)stream); }

// a frame's driver knows its largest pass before the first launch: sizing the buffer for it up front keeps the growth (a device-wide
// wait) out of the frame -- between the coarse and the fine pass (aux.hip).  Does nothing where the two-phase route would not be taken.
extern "C" void nvsr_internal_reserve_render_scratch(int64_t N, int S, nvsr_stream_t stream) {
    LiveLists ll;
    (void)two_phase_lists(nullptr, N, S, (hipStream_t)stream, ll, false);
}

extern "C" int64_t nvsr_render_scratch_bytes(void) {
    std::lock_guard<std::mutex> lock(g_live_mutex);
    int64_t total = 0;
    for (const LiveScratch& c : g_live) total += (int64_t)c.lists.bytes;
    return total;
}

extern "C" int nvsr_release_render_scratch(void) {
    std::lock_guard<std::mutex> lock(g_live_mutex);
    int prev = 0;
    const bool have_prev = hipGetDevice(&prev) == hipSuccess;
    int rc = NVSR_OK;
    for (const LiveScratch& c : g_live)
        for (void* p : {c.lists.p, c.group.p})
            if (p && (hipSetDevice(c.device) != hipSuccess || hipFree(p) != hipSuccess)) rc = NVSR_ERR_LAUNCH;
    g_live.clear();
    if (have_prev) (void)hipSetDevice(prev);
    return rc;
}
