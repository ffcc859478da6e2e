// Host side of the SR route (csrc/sr_core.h: conv_route, edsr_plan, sr_regions; csrc/sr.hip: the forward walk; csrc/sr_bwd.hip: the backward walk)
// as a stand-alone CPU program for the sanitizers.  The HIP launch calls are defined HERE (the executable's definitions win over the runtime
// library's): a launch is recorded, nothing runs, the program needs no GPU.  Buffers are address ranges of exactly the size the *_floats
// functions return -- never dereferenced -- and every convolution launch the entry points make is checked against them:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Iinclude -Xarch_host -fsanitize=address,undefined \
//         neural-volume-super-resolution_amd/csrc/sr.hip neural-volume-super-resolution_amd/csrc/sr_bwd.hip tools/sr_route_host_check.hip -o /tmp/sr_route_host_check
//   /tmp/sr_route_host_check          (prints "ok" and what it covered)
//
// Asserted: a launch's output range overlaps neither its input nor its skip tensor (the forward's rotating buffers and activation record, the
// backward's gradient rotation, the held input of a residual block); every input / output / skip / weight range lies inside one buffer of the
// size its *_floats function returns; a ragged launch's tile0[] is non-decreasing and ends at the grid's x extent; the grid holds exactly the tiles
// the cost model priced; the launch is the one conv_route answers for the same shape.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../neural-volume-super-resolution_amd/csrc/sr_core.h"
#include "../neural-volume-super-resolution_amd/csrc/nvsr_internal.h"

using namespace nvsr;

struct ConvLaunch { dim3 grid, block; ConvParams p; ConvRagged rg; };
static std::vector<ConvLaunch> g_convs;
static size_t g_other_launches = 0, g_memsets = 0;
static std::map<const void*, std::string>& kernel_names() { static std::map<const void*, std::string> m; return m; }
static dim3 g_grid, g_block;
static size_t g_shmem;
static hipStream_t g_stream;
struct Range { const char* what; uintptr_t lo, hi; };
static std::vector<Range> g_buffers;
static bool inside_a_buffer(uintptr_t lo, uintptr_t hi) {
    for (const Range& r : g_buffers)
        if (lo >= r.lo && hi <= r.hi && lo <= hi) return true;
    return false;
}

extern "C" {
void __hipRegisterFunction(void**, const void* host_function, char*, const char* device_name, unsigned, uint3*, uint3*, dim3*, dim3*, int*) {
    kernel_names()[host_function] = device_name;
}
hipError_t __hipPushCallConfiguration(dim3 grid, dim3 block, size_t shmem, hipStream_t stream) {
    g_grid = grid; g_block = block; g_shmem = shmem; g_stream = stream;
    return hipSuccess;
}
hipError_t __hipPopCallConfiguration(dim3* grid, dim3* block, size_t* shmem, hipStream_t* stream) {
    *grid = g_grid; *block = g_block; *shmem = g_shmem; *stream = g_stream;
    return hipSuccess;
}
hipError_t hipLaunchKernel(const void* f, dim3 grid, dim3 block, void** args, size_t, hipStream_t) {
    const std::string& name = kernel_names()[f];
    const bool limb = name.find("conv3x3_limb") != std::string::npos, f32 = name.find("conv3x3_kernel") != std::string::npos;
    if (!limb && !f32) { ++g_other_launches; return hipSuccess; }
    ConvLaunch c;
    c.grid = grid; c.block = block;
    c.p = *static_cast<const ConvParams*>(args[0]);
    if (limb) c.rg = *static_cast<const ConvRagged*>(args[1]);
    g_convs.push_back(c);
    return hipSuccess;
}
hipError_t hipGetLastError(void) { return hipSuccess; }
hipError_t hipMemsetAsync(void* dst, int, size_t bytes, hipStream_t) {          // (the magnitude words of a backward: inside its workspace)
    const uintptr_t lo = reinterpret_cast<uintptr_t>(dst);
    if (!inside_a_buffer(lo, lo + bytes)) { fprintf(stderr, "hipMemsetAsync outside every buffer\n"); abort(); }
    ++g_memsets;
    return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t, hipEvent_t, unsigned) { return hipSuccess; }
hipError_t hipGetSymbolAddress(void** p, const void*) { *p = reinterpret_cast<void*>(0x7000000000ull); return hipSuccess; }
uint32_t* nvsr_get_range_flag(void) { return nullptr; }
int nvsr_internal_parse_arith_env(const char*, int dflt, int) { return dflt; }
}

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s   [%s]\n", __FILE__, __LINE__, #c, g_context); return 1; } } while (0)
static char g_context[256] = "";

// address ranges in floats; each buffer in its own 2^40-byte stripe
static float* fake(int stripe) { return reinterpret_cast<float*>((uintptr_t)(stripe + 1) << 40); }
static float* buffer(int stripe, const char* what, int64_t floats) {
    float* p = fake(stripe);
    g_buffers.push_back({what, reinterpret_cast<uintptr_t>(p), reinterpret_cast<uintptr_t>(p + floats)});
    return p;
}
static bool overlap(const float* a, int64_t na, const float* b, int64_t nb) { return a < b + nb && b < a + na; }
static bool in_buffer(const float* a, int64_t n) { return inside_a_buffer(reinterpret_cast<uintptr_t>(a), reinterpret_cast<uintptr_t>(a + n)); }

// every recorded convolution launch against the buffers, and against the route of its own shape (rows_per_tile 0)
static int check_convs(int arith, size_t* checked) {
    for (const ConvLaunch& c : g_convs) {
        const ConvParams& p = c.p;
        const bool ragged = c.rg.n > 0;
        const int planes = ragged ? c.rg.n : (int)(c.grid.z / p.ncg);
        ConvShape s;
        s.H = p.H; s.W = p.W; s.batch = planes; s.n = ragged ? c.rg.n : 0;
        for (int b = 0; b < s.n; ++b) { s.rH[b] = c.rg.H[b]; s.rW[b] = c.rg.W[b]; }
        ConvRoute r;
        CHECK(conv_route(p.Cin, p.Cout, s, p.pad, p.epilogue, arith, 0, &r) == NVSR_OK && r.family != CONV_PLANEWISE);
        CHECK(c.grid.x == r.grid[0] && c.grid.y == r.grid[1] && c.grid.z == r.grid[2] && c.block.x == r.block && p.ncg == r.ncg);
        CHECK((long)c.grid.x * c.grid.y * c.grid.z == r.tiles);                                    // the grid holds the tiles the cost model priced
        CHECK(in_buffer(p.wpk, conv_packed_floats(p.Cin, p.Cout)));
        if (ragged) {
            unsigned t = 0;
            for (int b = 0; b < c.rg.n; ++b) {
                CHECK(c.rg.tile0[b] == t && memcmp(c.rg.tile0, r.tile0, sizeof r.tile0) == 0);
                t += (unsigned)((c.rg.W[b] - 2 + 31) / 32) * (unsigned)((c.rg.H[b] - 2 + r.tile_rows - 1) / r.tile_rows) * (unsigned)p.ncg;
            }
            CHECK(t == c.grid.x && c.grid.y == 1 && c.grid.z == 1);                                   // ... and ends at the grid's x extent
            for (int b = c.rg.n; b <= CONV_RAGGED_MAX; ++b) CHECK(c.rg.tile0[b] == (b == CONV_RAGGED_MAX && c.rg.n == CONV_RAGGED_MAX ? t : 0xffffffffu));
        }
        for (int b = 0; b < planes; ++b) {
            const int H = ragged ? c.rg.H[b] : p.H, W = ragged ? c.rg.W[b] : p.W, Ho = H - 2, Wo = W - 2;
            const float* in = ragged ? c.rg.in[b] : p.in + b * p.in_bs;
            const float* out = ragged ? c.rg.out[b] : p.out + b * p.out_bs;
            const float* skip = ragged ? c.rg.skip[b] : p.skip ? p.skip + b * p.skip_bs : nullptr;
            const int64_t n_in = (int64_t)p.Cin * (H - 2 * p.pad) * (W - 2 * p.pad), n_out = (int64_t)p.Cout * Ho * Wo;
            const int64_t n_skip = p.epilogue == EPI_RESIDUAL ? (int64_t)p.Cout * (Ho + 4) * (Wo + 4) : p.epilogue == EPI_ADD_CENTER ? (int64_t)p.Cout * (Ho - 4) * (Wo - 4)
                                   : p.epilogue == EPI_MASK_SCALE ? n_out : 0;
            CHECK(in_buffer(in, n_in) && in_buffer(out, n_out) && !overlap(in, n_in, out, n_out));
            CHECK((n_skip != 0) == (skip != nullptr));
            if (skip) CHECK(in_buffer(skip, n_skip) && !overlap(skip, n_skip, out, n_out));
            if (!ragged && b == 0 && planes > 1) CHECK(p.in_bs >= n_in && p.out_bs >= n_out);
        }
        ++*checked;
    }
    g_convs.clear();
    return 0;
}

static const float ROIS[3][4] = {{-0.6f, -0.5f, 0.1f, 0.3f}, {-0.2f, 0.1f, 0.7f, 0.9f}, {-1.0f, -0.3f, 0.2f, 1.0f}};      // (the last touches two borders)

int main() {
    size_t routes = 0, plans = 0, launches = 0, scenarios = 0;
    const int ariths[4] = {NVSR_ARITH_F32, NVSR_ARITH_BF16X3, NVSR_ARITH_F16X2, NVSR_ARITH_F16};
    // ---- 1. the route alone: every channel pair, arithmetic and rows_per_tile, uniform and ragged shapes ---------------------------------------
    const int chans[] = {3, 16, 48, 64, 128, 256, 300, 512}, rows[] = {0, 2, 3, 4, 8, 16, 18, 19, 20, 22, 5, 17};
    const int sizes[][2] = {{3, 3}, {4, 35}, {36, 36}, {67, 130}, {200, 200}};
    for (int ci : chans) for (int co : chans) for (int arith : ariths) for (int rw : rows) for (const auto& hw : sizes) for (int rag = 0; rag <= 4; rag += 2) {
        snprintf(g_context, sizeof g_context, "route %d -> %d arith %d rows %d %dx%d ragged %d", ci, co, arith, rw, hw[0], hw[1], rag);
        ConvShape s;
        s.H = hw[0]; s.W = hw[1]; s.batch = 3; s.n = rag;
        for (int b = 0; b < rag; ++b) { s.rH[b] = hw[0] + 7 * b; s.rW[b] = hw[1] + (b & 1) * 31; }
        ConvRoute r;
        const int e = conv_route(ci, co, s, 0, EPI_NONE, arith, rw, &r);
        if (rag && arith == NVSR_ARITH_F32) { CHECK(e == NVSR_ERR_SHAPE); continue; }
        if (rw == 5 || rw == 17) { CHECK(e == NVSR_ERR_SHAPE); continue; }
        if (e) { CHECK(e == NVSR_ERR_SHAPE && rw >= 8); continue; }                                       // (an opt-in kernel the layer does not have)
        ++routes;
        if (r.family == CONV_PLANEWISE) { CHECK(rag && r.region == 0); continue; }
        CHECK(r.tile_rows >= 2 && r.ncg >= 1 && r.region == (r.limbs == 0 ? 0 : r.family == CONV_LIMB16 ? (r.limbs == 3 ? 2 : 3) : 1));
        CHECK((long)r.grid[0] * r.grid[1] * r.grid[2] == r.tiles);
        if (rw == 0 && arith != NVSR_ARITH_F32) CHECK(conv_kinds_for(ci, co, arith) == 1u << r.region);
        if (rag) {
            for (int b = 0; b + 1 < rag; ++b) CHECK(r.tile0[b] <= r.tile0[b + 1]);
            const long last = (long)((s.rW[rag - 1] - 2 + 31) / 32) * ((s.rH[rag - 1] - 2 + r.tile_rows - 1) / r.tile_rows) * r.ncg;
            CHECK(r.tile0[0] == 0 && r.tile0[rag - 1] + last == r.grid[0] && r.tile0[CONV_RAGGED_MAX] == (rag == CONV_RAGGED_MAX ? r.grid[0] : 0xffffffffu));
        }
    }
    // ---- 2. plans: the activation record and the rotating buffers of every geometry ---------------------------------------------------------------
    static EdsrPlan P[CONV_RAGGED_MAX];
    const int hids[] = {16, 64, 128, 256}, nbs[] = {0, 1, 2, 16}, nups[] = {0, 1, 2}, ccs[] = {3, 48, 300};
    for (int hid : hids) for (int nb : nbs) for (int nup : nups) for (int cin : ccs) for (int cout : ccs) for (int H : {3, 8, 77, 200}) {
        snprintf(g_context, sizeof g_context, "plan hid %d nblocks %d n_up %d %d -> %d H %d", hid, nb, nup, cin, cout, H);
        const EdsrExtent x = edsr_extent(H, 200, hid, nb, nup);
        if (edsr_plan(cin, cout, hid, nb, nup, H, 200, &P[0])) { CHECK(x.Ho < 1); continue; }
        ++plans;
        const EdsrPlan& p = P[0];
        CHECK(x.Ho == p.Ho && x.Wo == p.Wo && p.n == 2 * nb + 3 + nup);
        int64_t end = 0;
        for (int l = 1; l < p.n; ++l) {                                                // tensor l = the input of layer l = the output of layer l - 1
            const int64_t floats = (int64_t)p.L[l].Cin * p.ih[l] * p.iw[l];
            CHECK(p.act_off[l] == end && floats <= p.max_tensor && floats <= x.max_rotating);
            end = p.act_off[l] + (floats + 3) / 4 * 4;
            if (l + 1 < p.n) CHECK(edsr_rotating_slot(l + 1) != edsr_rotating_slot(l));                               // output != input
            if (p.epi[l] == EPI_RESIDUAL && l >= 2 && l + 1 < p.n) CHECK(edsr_rotating_slot(l + 1) != edsr_rotating_slot(l - 1));      // ... != the held block input
        }
        CHECK(end == p.acts_floats);
    }
    CHECK(edsr_plan(3, 3, 16, 291, 1, 2000, 2000, &P[0]) == NVSR_ERR_SHAPE && edsr_plan(3, 3, 16, 1, 9, 200, 200, &P[0]) == NVSR_ERR_SHAPE);
    // ---- 3. the entry points on address ranges of exactly the *_floats sizes: every launch they make ------------------------------------------------
    const nvsr_stream_t st = nullptr;
    enum { KEEP, WS, BWS, PACKED, DGRAD, GRAD, X, OUT, DOUT, DX, LR0 = 16, OUT0 = 24, DOUT0 = 32, DLR0 = 40 };
    for (int hid : hids) for (int nb : nbs) for (int nup : nups) for (int arith : ariths) {
        const int sf = 1 << nup;
        // EDSR alone, Cin != Cout and Cout > hid: inference batch, training forward, backward
        for (const auto& cc : {std::pair<int, int>{3, 300}, {300, 48}, {48, 48}}) {
            const int cin = cc.first, cout = cc.second, H = 40 + 4 * nb, W = 57 + 4 * nb, B = 3;
            snprintf(g_context, sizeof g_context, "edsr hid %d nblocks %d n_up %d arith %d %d -> %d", hid, nb, nup, arith, cin, cout);
            int Ho, Wo;
            CHECK(nvsr_edsr_out_size(H, W, nb, nup, &Ho, &Wo) == NVSR_OK);
            g_buffers.clear();
            float* packed = buffer(PACKED, "packed", nvsr_edsr_packed_floats(cin, cout, hid, nb, nup));
            float* dgrad = buffer(DGRAD, "packed_dgrad", nvsr_edsr_packed_dgrad_floats(cin, cout, hid, nb, nup));
            float* x = buffer(X, "x", (int64_t)B * cin * H * W);
            float* out = buffer(OUT, "out", (int64_t)B * cout * Ho * Wo);
            float* ws = buffer(WS, "workspace", B * nvsr_edsr_workspace_floats(hid, nb, nup, H, W));
            CHECK(nvsr_edsr_forward_batch_arith(x, B, cin, H, W, packed, cout, hid, nb, nup, out, ws, arith, st) == NVSR_OK);
            CHECK((int)g_convs.size() == 2 * nb + 3 + nup && check_convs(arith, &launches) == 0);
            float* acts = buffer(KEEP, "acts", nvsr_edsr_acts_floats(cin, cout, hid, nb, nup, H, W));
            CHECK(nvsr_edsr_forward_train_arith(x, cin, H, W, packed, cout, hid, nb, nup, out, acts, arith, st) == NVSR_OK);
            CHECK((int)g_convs.size() == 2 * nb + 3 + nup && check_convs(arith, &launches) == 0);
            float* bws = buffer(BWS, "backward workspace", nvsr_edsr_backward_workspace_floats(cin, cout, hid, nb, nup, H, W));
            float* grad = buffer(GRAD, "grad_natural", nvsr_edsr_natural_floats(cin, cout, hid, nb, nup));
            float* dx = buffer(DX, "dx", (int64_t)cin * H * W);
            CHECK(nvsr_edsr_backward_arith(x, cin, H, W, acts, dgrad, cout, hid, nb, nup, out, grad, dx, bws, arith, st) == NVSR_OK);
            CHECK((int)g_convs.size() == 2 * nb + 3 + nup && check_convs(arith, &launches) == 0);
            ++scenarios;
        }
        // PlanesSR: full planes and three ROIs, B = 1, 3, 4; pad as the net needs it, over from the net
        for (int cc : {3, 48}) for (int R : {24, 63}) for (int B : {1, 3, 4}) for (int with_roi = 0; with_roi < 2; ++with_roi) {
            snprintf(g_context, sizeof g_context, "planes hid %d nblocks %d n_up %d arith %d Cc %d R %d B %d roi %d", hid, nb, nup, arith, cc, R, B, with_roi);
            const int R1 = R + 13, pad = 2 * nb + 3 + 2 * nup;
            float rois[CONV_RAGGED_MAX * 4];
            for (int b = 0; b < B; ++b) memcpy(rois + 4 * b, ROIS[b % 3], sizeof ROIS[0]);
            const float* roi = with_roi ? rois : nullptr;
            SrRegions g;
            CHECK(sr_regions(B, cc, R, R1, hid, nb, nup, pad, -1, roi, P, &g) == NVSR_OK);
            const int over2 = g.p[0].Ho - (g.p[0].hi[0] - g.p[0].lo[0]) * sf;
            CHECK(over2 >= 0 && over2 % 2 == 0);
            const int over = over2 / 2;
            g_buffers.clear();
            float* packed = buffer(PACKED, "packed", nvsr_edsr_packed_floats(cc, cc, hid, nb, nup));
            float* dgrad = buffer(DGRAD, "packed_dgrad", nvsr_edsr_packed_dgrad_floats(cc, cc, hid, nb, nup));
            float* grad = buffer(GRAD, "grad_natural", nvsr_edsr_natural_floats(cc, cc, hid, nb, nup));
            const float* lr[CONV_RAGGED_MAX]; float* out[CONV_RAGGED_MAX]; const float* d_out[CONV_RAGGED_MAX]; float* d_lr[CONV_RAGGED_MAX];
            for (int b = 0; b < B; ++b) {
                lr[b] = buffer(LR0 + b, "lr", (int64_t)cc * R * R1); out[b] = buffer(OUT0 + b, "out", (int64_t)cc * R * R1 * sf * sf);
                d_out[b] = buffer(DOUT0 + b, "d_out", (int64_t)cc * R * R1 * sf * sf); d_lr[b] = b == 1 ? nullptr : buffer(DLR0 + b, "d_lr", (int64_t)cc * R * R1);
            }
            // the batched training forward and its backward
            float* keep = buffer(KEEP, "keep", nvsr_planes_sr_batch_keep_floats(B, cc, R, R1, hid, nb, nup, pad, roi));
            float* ws = buffer(WS, "workspace", nvsr_planes_sr_batch_workspace_floats(B, cc, R, R1, hid, nb, nup, pad, roi));
            float* bws = buffer(BWS, "backward workspace", nvsr_planes_sr_batch_backward_workspace_floats(B, cc, R, R1, hid, nb, nup, pad, roi));
            CHECK(nvsr_planes_sr_train_batch_arith(lr, B, cc, R, R1, packed, hid, nb, nup, pad, over, roi, nullptr, nullptr, out, ws, keep, arith, 1, 0, st) == NVSR_OK);
            CHECK(!g_convs.empty() && check_convs(arith, &launches) == 0);
            CHECK(nvsr_planes_sr_backward_batch_arith(B, cc, R, R1, keep, dgrad, hid, nb, nup, pad, over, roi, nullptr, d_out, grad, d_lr, bws, arith, 1, 0, st) == NVSR_OK);
            CHECK(!g_convs.empty() && check_convs(arith, &launches) == 0);
            ++scenarios;
            if (B == 4) continue;
            // the one-plane entry points (first ROI) and the uniform inference batch: their own, smaller buffers
            g_buffers.resize(3 + 4 * B - (B > 1));
            keep = buffer(KEEP, "keep", nvsr_planes_sr_keep_floats(cc, R, R1, hid, nb, nup, pad, roi));
            ws = buffer(WS, "workspace", B * nvsr_planes_sr_workspace_floats(cc, R, R1, hid, nb, nup, pad, roi));
            bws = buffer(BWS, "backward workspace", nvsr_planes_sr_backward_workspace_floats(cc, R, R1, hid, nb, nup, pad, roi));
            CHECK(nvsr_planes_sr_batch_arith(lr, B, cc, R, R1, packed, hid, nb, nup, pad, over, roi, nullptr, nullptr, out, ws, arith, st) == NVSR_OK);
            CHECK((int)g_convs.size() == 2 * nb + 3 + nup && check_convs(arith, &launches) == 0);
            CHECK(nvsr_planes_sr_train_arith(lr[0], cc, R, R1, packed, hid, nb, nup, pad, over, roi, nullptr, nullptr, out[0], ws, keep, arith, st) == NVSR_OK);
            CHECK((int)g_convs.size() == 2 * nb + 3 + nup && check_convs(arith, &launches) == 0);
            CHECK(nvsr_planes_sr_backward_arith(cc, R, R1, keep, dgrad, hid, nb, nup, pad, over, roi, nullptr, d_out[0], grad, d_lr[0], bws, arith, st) == NVSR_OK);
            CHECK((int)g_convs.size() == 2 * nb + 3 + nup && check_convs(arith, &launches) == 0);
            ++scenarios;
        }
    }
    printf("ok: %zu routes, %zu plans, %zu scenarios of the entry points, %zu convolution launches checked (%zu other launches, %zu memsets inside a workspace)\n",
           routes, plans, scenarios, launches, g_other_launches, g_memsets);
    return 0;
}
