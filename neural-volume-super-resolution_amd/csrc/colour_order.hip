// The two-phase render route (render3.hip: density pass, then the colour decoder on the live samples) apart from its render kernels: WHICH
// ray a colour lane owns (live_order_kernel), WHICH ray block a colour workgroup runs (group_order_kernel), and the library's scratch that
// holds the live lists and both orders between the launches.  include/nvsr.h, "The two-phase render pass", is the contract.
#include "colour_order.h"
#include "occupancy.h"
#include "nvsr_internal.h"

#include <cstdlib>
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

// ---- the point-major colour pass's order of points: packed entries + live lists -> per group, its live points in steps of 256 -------------------
// The point-major colour kernels (render3.hip, PHASE 3) give a lane one live POINT per step, not a ray.  One workgroup per group of RAYS2 slots
// (the rays that the packed entries name for it); thread j is slot j.  A group's points are taken in the order (band, slot, k), k = the index
// into the ray's live list, band = a monotone function of the point's depth -- ZCOMP lists (rays_nf = NULL) hold the sample index s: band =
// s nb / S; otherwise band = (z - near) nb / (far - near), truncated and clamped to 0..nb-1 -- made monotone along the ray by a running
// maximum, so the order keeps every ray's sample order whatever the lists hold.  The sequence is cut into steps of 256 and every step is
// stably sorted by (slot, k): a ray's points of a step are one contiguous run (the kernel's run heads add them to the ray's sums in order).
// A step's points of one ray are consecutive k (the sequence holds a ray's points in k order and a step is a window of it), so the place in
// its run is k - the smallest k of that slot in the step.  Group g's entries (slot << 24) | k start at pts[g RAYS2 S] -- a fixed offset, no
// scan over the groups; steps[g] = ceil(total / 256), offs[g] = g S = that offset in steps; the last step is padded with POINT_NONE.
// Deterministic: integer prefix sums in thread order; the two LDS atomics (a minimum and a count per slot) give the same result in any order.
__global__ __launch_bounds__(RAYS2) void point_order_kernel(const int* __restrict__ live_n, const float* __restrict__ live_z, const float* __restrict__ rays_nf,
                                                            long N, int S, int nb, int* __restrict__ pts, int* __restrict__ steps, int* __restrict__ offs) {
    __shared__ int wsum_s[2][RAYS2 / 64], kmin_s[RAYS2], cnt_s[RAYS2], start_s[RAYS2], stage_s[RAYS2];
    const int j = threadIdx.x, wave = j >> 6, lane = j & 63;
    const long slot0 = (long)blockIdx.x * RAYS2;
    int n = 0;
    long ray = 0;
    if (slot0 + j < N) {
        const int e = live_n[slot0 + j];
        n = e >> ORDER_SHIFT;
        ray = slot0 / ORDER_RAYS * ORDER_RAYS + (e & (ORDER_RAYS - 1));
    }
    const float* lz = live_z + ray * S;
    const float nr = rays_nf ? rays_nf[ray * 11 + 6] : 0.0f, fr = rays_nf ? rays_nf[ray * 11 + 7] : 0.0f;
    auto band_of = [&](int k) -> int {
        const float e = lz[k];
        if (!rays_nf) {
            const long long b = (long long)__float_as_int(e) * nb / S;
            return b < 0 ? 0 : b < nb ? (int)b : nb - 1;
        }
        const float u = __fdiv_rn(__fmul_rn(__fsub_rn(e, nr), (float)nb), __fsub_rn(fr, nr));
        return u >= 0.0f ? (u < (float)nb ? (int)u : nb - 1) : 0;      // (a NaN goes to band 0)
    };
    // exclusive prefix sum of c over the workgroup's threads, and the total; buffer `buf` of the wave sums (two: one barrier per call)
    auto scan = [&](int c, int buf, int& total) -> int {
        int incl = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int v = __shfl_up(incl, o); if (lane >= o) incl += v; }
        if (lane == 63) wsum_s[buf][wave] = incl;
        __syncthreads();
        int before = 0;
        total = 0;
#pragma unroll
        for (int w = 0; w < RAYS2 / 64; ++w) { const int v = wsum_s[buf][w]; if (w < wave) before += v; total += v; }
        return before + incl - c;
    };
    int* out = pts + (long)blockIdx.x * RAYS2 * S;
    int k = 0, base = 0, nextb = n > 0 ? band_of(0) : nb;
    for (int b = 0; b < nb; ++b) {
        const int k0 = k;
        while (k < n && nextb <= b) { ++k; if (k < n) nextb = max(nextb, band_of(k)); }
        int total;
        const int at = base + scan(k - k0, b & 1, total);
        for (int i = k0; i < k; ++i) out[at + (i - k0)] = (j << 24) | i;
        base += total;
    }
    const int nsteps = (base + RAYS2 - 1) / RAYS2;
    if (base + j < nsteps * RAYS2) out[base + j] = POINT_NONE;      // (the padding: fewer than RAYS2 entries)
    if (j == 0) { steps[blockIdx.x] = nsteps; offs[blockIdx.x] = (int)blockIdx.x * S; }
    __syncthreads();                                               // the sequence, written by other threads, is read below
    for (int t = 0; t < nsteps; ++t) {
        const int e = out[t * RAYS2 + j];
        const bool valid = e != POINT_NONE;
        const int sl = (int)((unsigned)e >> 24), kk = e & 0xffffff;
        kmin_s[j] = 0x7fffffff; cnt_s[j] = 0;
        __syncthreads();
        if (valid) { atomicMin(&kmin_s[sl], kk); atomicAdd(&cnt_s[sl], 1); }
        __syncthreads();
        int total;
        start_s[j] = scan(cnt_s[j], 0, total);
        __syncthreads();
        stage_s[valid ? start_s[sl] + (kk - kmin_s[sl]) : j] = e;     // (padding follows every point of the step: it keeps its place)
        __syncthreads();
        out[t * RAYS2 + j] = stage_s[j];
    }
}

// ---- scratch of the two-phase route: the live lists, [N, S] depths + [N, S] weights + [N] counts ------------------------------------
// Owned by the library, one entry per (device, stream), grow-only: two launches on one stream are ordered, launches on two streams never
// share a buffer.  Growing frees the old buffer with hipFree, which waits for the device -- no launch can still be using it.
// Contract (include/nvsr.h): one host thread at a time enqueues render launches on a given (device, stream) -- the pointers are used after
// the table's lock is dropped; the entry of a destroyed stream keeps its buffers until nvsr_release_render_scratch.
// An entry's buffers, in the order in which a pass allocates them (GROUP, LISTS, POINTS, VIEWS, KEPT_GROUP, KEPT), G = ceil(N / RAYS2):
//   LISTS       z [N, S], w [N, S], n [N] -- the only buffer that nvsr_render_scratch_bytes counts
//   GROUP       the order of dispatch (group_order_kernel): group_slot [G], then group_trip [G] (20 KB at the benchmark size)
//   POINTS      the point-major colour pass (point_order_kernel): G RAYS2 S ints of entries, then steps [G] and offs [G]
//   VIEWS       the view features of every slot of that pass, POINT_VIEW_FLOATS floats each
//   KEPT        the occupancy route's kept lists: idx [N, S], then n [N]
//   KEPT_GROUP  the order of dispatch of the density pass over the kept lists: slot [G], then trip [G]
namespace {
enum { LISTS, GROUP, POINTS, VIEWS, KEPT, KEPT_GROUP, N_BUFFERS };
struct Buffer { void* p; size_t bytes; };
// What the latest launch of an entry left behind, for the nvsr_internal_copy_* hooks: its N, its packed counts, its points' step counts
// (NULL: it ran the lockstep colour kernels) and the packed kept counts of the latest OCCUPANCY launch with that launch's N (NULL: none).
// Lifetime: any growth of any buffer forgets all of it (a new buffer holds no launch's lists or order); a pass that takes the two-phase
// route assigns all of it -- a plain pass carries the kept counts over, an occupancy pass replaces them; an occupancy pass that declines
// forgets the kept counts and leaves the rest to the route it falls back to; a reservation assigns nothing.
struct Launch { int64_t N; int* n; int* steps; int64_t kept_N; int* kept; int density; };      // density: 0 the tile-pair density kernels, 1 the one-tile ones
struct Scratch { int device; hipStream_t stream; Buffer buf[N_BUFFERS]; Launch last; };
std::mutex g_live_mutex;
std::vector<Scratch> g_live;

Scratch* find_scratch(int device, hipStream_t stream) {      // (under the lock)
    for (Scratch& c : g_live)
        if (c.device == device && c.stream == stream) return &c;
    return nullptr;
}

// grow-only: free, forget the latest launch, allocate
bool grow(Scratch& e, int which, size_t bytes) {
    Buffer& b = e.buf[which];
    if (b.bytes >= bytes) return true;
    if (b.p) (void)hipFree(b.p);
    b = Buffer{};
    e.last = Launch{};
    void* p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) { (void)hipGetLastError(); return false; }
    b = Buffer{p, bytes};
    return true;
}

int64_t groups_of(int64_t N) { return (N + RAYS2 - 1) / RAYS2; }

// behind the nvsr_internal_copy_* hooks: `ints` ints of what the latest launch on (the current device, stream) left behind -> dst (device
// or host memory).  pick(entry) names them, or answers NULL where the caller's count is not that launch's or the launch left none.
template <class Pick>
int copy_left_behind(int* dst, int64_t ints, nvsr_stream_t stream, Pick pick) {
    if (!dst) return NVSR_ERR_NULL;
    int device = 0;
    if (hipGetDevice(&device) != hipSuccess) return NVSR_ERR_LAUNCH;
    const int* src = nullptr;
    {
        std::lock_guard<std::mutex> lock(g_live_mutex);
        const Scratch* c = find_scratch(device, (hipStream_t)stream);
        if (c) src = pick(*c);
    }
    if (!src) return NVSR_ERR_SHAPE;
    return hipMemcpyAsync(dst, src, (size_t)ints * sizeof(int), hipMemcpyDefault, (hipStream_t)stream) == hipSuccess ? NVSR_OK : NVSR_ERR_LAUNCH;
}

// The four environment handles of the route, for A/Bs, each read at every launch by the function that acts on it (named there).
bool env_starts(const char* name, char c) {
    const char* e = getenv(name);
    return e && e[0] == c;
}
void launch_live_order(int* live_n, int64_t N, int S, int bins, int* group_trip, hipStream_t stream) {
    hipLaunchKernelGGL(live_order_kernel, dim3((unsigned)((N + ORDER_RAYS - 1) / ORDER_RAYS)), dim3(SORT_TPB), 0, stream, live_n, (long)N, S, bins, group_trip);
}
void launch_group_order(const int* group_trip, int64_t G, int S, int* group_slot, hipStream_t stream) {
    const int sorted = !env_starts("NVSR_COLOUR_GROUP_ORDER", '0');      // =0: the order of dispatch is the contiguous eighths (same kernel, same table)
    hipLaunchKernelGGL(group_order_kernel, dim3(1), dim3(SORT_TPB), 0, stream, group_trip, (int)G, S, sorted, group_slot);
}
void launch_point_order(const int* live_n, const float* live_z, const float* rays_nf, int64_t N, int S, int nb, int* pts, int* steps, int* offs, hipStream_t stream) {
    nb = nb < 1 || nb > S ? S : nb;      // (POINT_BANDS = 0: a band per sample)
    hipLaunchKernelGGL(point_order_kernel, dim3((unsigned)groups_of(N)), dim3(RAYS2), 0, stream, live_n, live_z, rays_nf, (long)N, S, nb, pts, steps, offs);
}
}  // namespace

PassRoute acquire_pass_scratch(int64_t N, int S, hipStream_t stream, bool raw_out, bool want_kept, bool launch, LiveLists& live, KeptLists& kept) {
    // NVSR_RENDER_ONE_PHASE=1 keeps the fused kernel
    bool declines = raw_out || S < 1 || S >= ORDER_MAX_S || env_starts("NVSR_RENDER_ONE_PHASE", '1');
    if (!declines) {
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(stream, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) { (void)hipGetLastError(); declines = true; }
    }
    if (declines && !want_kept) return PassRoute::Fused;      // (nothing to forget: the table is not looked at)
    int device = 0;
    if (hipGetDevice(&device) != hipSuccess) return PassRoute::Fused;
    const size_t rows = (size_t)N * (size_t)S, G = (size_t)groups_of(N);
    std::lock_guard<std::mutex> lock(g_live_mutex);
    Scratch* e = find_scratch(device, stream);
    if (e && want_kept) { e->last.kept_N = 0; e->last.kept = nullptr; }      // (an occupancy pass: its own kept counts below, or none)
    if (declines) return PassRoute::Fused;
    if (!e) {
        g_live.emplace_back();
        e = &g_live.back();
        e->device = device; e->stream = stream;
    }
    if (!grow(*e, GROUP, 2 * G * sizeof(int)) || !grow(*e, LISTS, (2 * rows + (size_t)N) * sizeof(float)) || !e->buf[LISTS].p) return PassRoute::Fused;
    live = LiveLists{};
    live.z = static_cast<float*>(e->buf[LISTS].p);
    live.w = live.z + rows;
    live.n = reinterpret_cast<int*>(live.w + rows);
    live.slot = static_cast<int*>(e->buf[GROUP].p);
    live.trip = live.slot + G;
    // the point-major colour pass's buffers; NVSR_COLOUR_POINTS=0, G S >= 2^31 or a buffer that cannot be had: the lockstep colour kernels
    const size_t npts = G * RAYS2 * (size_t)S;
    if (!env_starts("NVSR_COLOUR_POINTS", '0') && G * (size_t)S <= 0x7fffffffu && grow(*e, POINTS, (npts + 2 * G) * sizeof(int)) &&
        grow(*e, VIEWS, G * RAYS2 * POINT_VIEW_FLOATS * sizeof(float))) {
        live.pts = static_cast<int*>(e->buf[POINTS].p);
        live.steps = live.pts + npts;
        live.views = static_cast<float*>(e->buf[VIEWS].p);
    }
    // the occupancy route's kept lists; where they cannot be had the pass runs the plain two-phase route on the lists above
    PassRoute route = PassRoute::TwoPhase;
    if (want_kept && grow(*e, KEPT_GROUP, 2 * G * sizeof(int)) && grow(*e, KEPT, (rows + (size_t)N) * sizeof(int))) {
        kept.idx = static_cast<int*>(e->buf[KEPT].p);
        kept.n = kept.idx + rows;
        kept.slot = static_cast<int*>(e->buf[KEPT_GROUP].p);
        kept.trip = kept.slot + G;
        route = PassRoute::Occupancy;
    }
    if (launch) e->last = route == PassRoute::Occupancy ? Launch{N, live.n, live.steps, N, kept.n} : Launch{N, live.n, live.steps, e->last.kept_N, e->last.kept};
    return route;
}

void note_density_kernel(hipStream_t stream, int which) {
    int device = 0;
    if (hipGetDevice(&device) != hipSuccess) return;
    std::lock_guard<std::mutex> lock(g_live_mutex);
    if (Scratch* e = find_scratch(device, stream)) e->last.density = which;
}

// the ray order on the counts n (in place), then the order of dispatch on the trips it leaves
static void launch_orders(int* n, int* trip, int* slot, int64_t N, int S, hipStream_t stream) {
    // NVSR_COLOUR_ORDER=0 makes the ray order the identity (bins = 0: the colour kernel groups its rays as the density kernel does)
    launch_live_order(n, N, S, env_starts("NVSR_COLOUR_ORDER", '0') ? 0 : ORDER_BINS, trip, stream);
    launch_group_order(trip, groups_of(N), S, slot, stream);
}
void launch_kept_order(const KeptLists& kl, int64_t N, int S, hipStream_t stream) { launch_orders(kl.n, kl.trip, kl.slot, N, S, stream); }
void launch_colour_order(const LiveLists& ll, int64_t N, int S, hipStream_t stream) { launch_orders(ll.n, ll.trip, ll.slot, N, S, stream); }

void launch_point_order(const LiveLists& ll, const float* rays_nf, int64_t N, int S, hipStream_t stream) {
    launch_point_order(ll.n, ll.z, rays_nf, N, S, POINT_BANDS, ll.pts, ll.steps, ll.steps + groups_of(N), stream);
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
extern "C" int nvsr_internal_copy_live_counts(int* dst, int64_t N, nvsr_stream_t stream) {
    return copy_left_behind(dst, N, stream, [N](const Scratch& c) { return c.last.N == N ? c.last.n : nullptr; });
}
// which density kernels the latest two-phase launch on `stream` ran (include/nvsr.h); -1: no such launch is on record
extern "C" int nvsr_internal_density_kernel(nvsr_stream_t stream) {
    int device = 0;
    if (hipGetDevice(&device) != hipSuccess) return -1;
    std::lock_guard<std::mutex> lock(g_live_mutex);
    const Scratch* c = find_scratch(device, (hipStream_t)stream);
    return c && c->last.n ? c->last.density : -1;
}
// test hooks of the order of dispatch (include/nvsr.h)
extern "C" int nvsr_internal_group_order(const int* trips, int64_t G, int S, int* out, nvsr_stream_t stream) {
    if (!trips || !out) return NVSR_ERR_NULL;
    if (G < 1 || G > 0x7fffffff || S < 1 || S >= ORDER_MAX_S) return NVSR_ERR_SHAPE;
    launch_group_order(trips, G, S, out, (hipStream_t)stream);
    return NVSR_CHECK_LAUNCH();
}
extern "C" int nvsr_internal_copy_group_order(int* dst, int64_t G, nvsr_stream_t stream) {      // (group_slot [G], then group_trip [G])
    return copy_left_behind(dst, 2 * G, stream, [G](const Scratch& c) { return c.last.n && groups_of(c.last.N) == G ? static_cast<int*>(c.buf[GROUP].p) : nullptr; });
}

// test hooks of the order of points (include/nvsr.h)
extern "C" int nvsr_internal_point_bands(void) { return POINT_BANDS; }
extern "C" int nvsr_internal_point_order(const int* entries, const float* lists, const float* rays, int64_t N, int S, int bands, int* points, int* steps, int* offsets,
                                         nvsr_stream_t stream) {
    if (!entries || !lists || !points || !steps || !offsets) return NVSR_ERR_NULL;
    const int64_t G = (N + RAYS2 - 1) / RAYS2;
    if (N < 1 || S < 1 || S >= ORDER_MAX_S || G * S > 0x7fffffff) return NVSR_ERR_SHAPE;
    launch_point_order(entries, lists, rays, N, S, bands, points, steps, offsets, (hipStream_t)stream);
    return NVSR_CHECK_LAUNCH();
}
extern "C" int nvsr_internal_copy_point_steps(int* dst, int64_t G, nvsr_stream_t stream) {      // (no steps: the latest launch ran the lockstep colour kernels)
    return copy_left_behind(dst, G, stream, [G](const Scratch& c) { return c.last.n && groups_of(c.last.N) == G ? c.last.steps : nullptr; });
}

// hook of the occupancy route (include/nvsr.h): the packed kept counts of the latest occupancy launch on `stream`; none ran (or it declined): an error
extern "C" int nvsr_internal_copy_kept_counts(int* dst, int64_t N, nvsr_stream_t stream) {
    return copy_left_behind(dst, N, stream, [N](const Scratch& c) { return c.last.kept_N == N ? c.last.kept : nullptr; });
}

// a frame's driver knows its largest pass before the first launch: sizing the buffer for it up front keeps the growth (a device-wide
// wait) out of the frame -- between the coarse and the fine pass (aux.hip).  Does nothing where the two-phase route would not be taken.
extern "C" void nvsr_internal_reserve_render_scratch(int64_t N, int S, nvsr_stream_t stream) {
    LiveLists live;
    KeptLists kept;
    (void)acquire_pass_scratch(N, S, (hipStream_t)stream, /*raw_out*/ false, /*want_kept*/ false, /*launch*/ false, live, kept);
}

extern "C" int64_t nvsr_render_scratch_bytes(void) {
    std::lock_guard<std::mutex> lock(g_live_mutex);
    int64_t total = 0;
    for (const Scratch& c : g_live) total += (int64_t)c.buf[LISTS].bytes;
    return total;
}

extern "C" int nvsr_release_render_scratch(void) {
    std::lock_guard<std::mutex> lock(g_live_mutex);
    int prev = 0;
    const bool have_prev = hipGetDevice(&prev) == hipSuccess;
    int rc = NVSR_OK;
    for (const Scratch& c : g_live)
        for (const Buffer& b : c.buf)
            if (b.p && (hipSetDevice(c.device) != hipSuccess || hipFree(b.p) != hipSuccess)) rc = NVSR_ERR_LAUNCH;
    g_live.clear();
    if (have_prev) (void)hipSetDevice(prev);
    return rc;
}
