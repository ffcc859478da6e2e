// What the two fused evaluation kernels of the generic decoder geometries share (generic_fused.hip: exact f32; generic_fused_limb.hip: two f16
// limbs): the LDS size classes, stage 0 -- the decoder inputs of a wave's 32 points in their rows of LDS -- and the exact-f32 layer chain, which
// both kernels run for the heads.  Both compile the SAME stage 0 out of this header: the limb kernel differs from the f32 one in the hidden layers
// only.
#pragma once
#include <type_traits>

#include "generic_core.h"

namespace nvsr {

constexpr int GF_CLASSES = 3;
constexpr int GF_LDS_FLOATS[GF_CLASSES] = {10240, 20480, 40960};      // 40, 80, 160 KB: 4, 2, 1 workgroups per CU
constexpr int GF_MAX_WAVES = 4;
constexpr int GF_U = 4;             // k pairs per step of the layer loop (the padded K is a multiple of 32)
constexpr int GF_MAX_HIDDEN = 256, GF_MAX_K0 = 512;
// Phases of the two kernels (a template argument: GF_FULL compiles to the one-launch kernel as it was).
//   GF_DENSITY  every point: position, the position planes' taps, combine_pos_planes, the density layers, fc_alpha -- no atan2f, no view plane;
//               writes the 16-byte row [+0, +0, +0, sigma]
//   GF_COLOUR   the points index[i], i < min(*count, max_count): stage 0 as far as Xr needs it, the colour layers, fc_rgb; writes the 12 bytes
//               out[index[i]][0:3] and nothing else; entries at or beyond the count are not read
//   GF_DENSITY_LIST  GF_DENSITY on the points index[i], i < min(*count, max_count), listed as for GF_COLOUR (the kept samples of an occupancy
//               grid): writes the 16-byte row [+0, +0, +0, sigma] at out[index[i]] and no other row
// All keep the full kernel's rows (gen_fused_plan), operand pairs and order: the same bits as GF_FULL at the same points.
constexpr int GF_FULL = 0, GF_DENSITY = 1, GF_COLOUR = 2, GF_DENSITY_LIST = 3;
constexpr bool gf_density_only(int phase) { return phase == GF_DENSITY || phase == GF_DENSITY_LIST; }      // the density decoder alone
constexpr bool gf_listed(int phase) { return phase == GF_COLOUR || phase == GF_DENSITY_LIST; }             // the points come from a list
struct GenFusedList {
    const int* index;    // GF_COLOUR / GF_DENSITY_LIST: the points to evaluate (device)
    const int* count;    // how many of them (device, read by the kernel)
    long max_count;      // what the launch is sized for
};

struct GenFusedPlan {
    int nt;              // 32-row output tiles of a hidden layer the kernel is instantiated for: 1, 2, 3, 4, 6, 8
    int cls;             // LDS size class
    int waves;           // waves (= 32-point blocks) per workgroup
    int ld, xd_off, h_off;
};
// 1 = the fused kernel holds this geometry, 0 = it does not (the layered route does).
// limb = false: the f32 kernel's rows, 2 x an odd number of floats (4-byte B-operand reads: 64 lanes on 64 banks).
// limb = true: the limb kernel reads its B operands 16 bytes at a time, so xd_off, h_off and the stride are multiples of 4 floats, the hidden
// activation is padded to a multiple of 4 (its 16-byte writes) and the stride is 4 x an odd number (generic_fused_limb.hip has the bank argument).
static inline int gen_fused_plan(const GenGeom& g, GenFusedPlan* pl, bool limb = false) {
    const int k0 = g.Kd > g.Kr ? g.Kd : g.Kr;
    if (g.hidden > GF_MAX_HIDDEN || k0 > GF_MAX_K0) return 0;
    const bool own_xd = g.view == 4 && g.proj != 2;
    int ld;
    if (limb) {
        auto up4 = [](int v) { return (v + 3) & ~3; };
        pl->xd_off = own_xd ? up4(g.Kr) : 0;
        pl->h_off = own_xd ? pl->xd_off + up4(g.Kd) : up4(k0);
        ld = pl->h_off + up4(g.hidden);
        if ((ld / 4) % 2 == 0) ld += 4;
    } else {
        pl->xd_off = own_xd ? g.Kr : 0;
        pl->h_off = own_xd ? g.Kr + g.Kd : k0;
        ld = pl->h_off + g.hidden;
        ld += ld & 1;
        if ((ld / 2) % 2 == 0) ld += 2;
    }
    pl->ld = ld;
    int best = 0;
    for (int c = 0; c < GF_CLASSES; ++c) {
        int w = GF_LDS_FLOATS[c] / (32 * ld);
        if (w > GF_MAX_WAVES) w = GF_MAX_WAVES;
        const int per_cu = w * (4 >> c);
        if (per_cu > best) { best = per_cu; pl->cls = c; pl->waves = w; }
    }
    if (!best) return 0;
    const int tiles = (g.hidden + 31) / 32;
    pl->nt = tiles <= 4 ? tiles : tiles <= 6 ? 6 : 8;
    return 1;
}

// a wave's 32 rows of LDS, as stage 0 sees them: the row stride and where Xd stands (see the kernels' headers)
struct GenFusedRows {
    float* rows;         // this wave's 32 points
    float* row;          // this lane's point (shared by the lane's two halves)
    int ld, xd_off;
};

// features of plane d at the 32 points' grid coordinates (gx, gy: lane n holds point n's) into columns col0 + c of their rows;
// mode 0: stored, 1: added to what is there, 2: combined with what is there as the view-direction feature
__device__ __forceinline__ void gf_plane_features(const SceneDevN& sc, const GenGeom& g, const GenFusedRows& R, int n, int h, int d, int Cc, float gx,
                                                  float gy, int col0, int mode) {
    const float* __restrict__ pl = sc.plane[d];
    const int H = sc.ph[d], W = sc.pw[d];
    auto put = [&](float* r, float v) GEN_INL { *r = mode == 0 ? v : mode == 1 ? __fadd_rn(*r, v) : gen_combine_view(g.view, *r, v); };
    for (int i = 0; i < 16; ++i) {
        const int pt = 2 * i + h;
        const float px = __shfl(gx, pt), py = __shfl(gy, pt);
        float* r = R.rows + pt * R.ld + col0;
        if (sc.bicubic) {
            const CubicTaps t = gen_cubic_taps(H, W, px, py, sc.align);
            for (int c = n; c < Cc; c += 32) put(r + c, gen_cubic_blend(pl, W, Cc, t, c));
        } else {
            const GenTaps t = gen_taps(H, W, Cc, px, py, sc.align);
            for (int c = n; c < Cc; c += 32) put(r + c, gen_blend(pl, t, c));
        }
    }
}

// stage 0: per (point, plane): position, projection (atan2f for the view plane) once per point, the taps once per (point, plane) -- two points
// at a time, 32 lanes each over the channels, so a tap's channels are one contiguous read.  Leaves Xr (or Xd where the view features are combined
// in place later) in columns [0, ..) and Xd at xd_off of every row, behind a barrier; (vgx, vgy): the view plane's grid coordinates, which the
// colour decoder's in-place combination needs again.
// (a point past P takes part with the position 0: in-bounds taps, nothing stored)
// GF_DENSITY / GF_DENSITY_LIST leave out the view direction (vgx = vgy = 0, its columns of a 'concat' / 'concat_pos' row are not written); GF_COLOUR leaves out
// the combined position features where only the density decoder reads them ('sum' / 'avg' under 'concat_pos').
template <int PHASE = GF_FULL>
__device__ __forceinline__ void gf_stage0(const SceneDevN& sc, const GenGeom& g, const GenFusedRows& R, int n, int h, bool live, long p,
                                          const float* __restrict__ x, const float* __restrict__ noise, float& vgx, float& vgy) {
    float n0 = 0.0f, n1 = 0.0f, n2 = 0.0f;
    vgx = 0.0f; vgy = 0.0f;
    if (live) {
        gen_position(sc, x + p * 6, noise, p, n0, n1, n2);
        if (!gf_density_only(PHASE)) gen_view_grid(sc, x + p * 6, vgx, vgy);
    }
    const bool raw = g.proj == 2 || g.view == 4;          // the rows start as cat(pos_planes + [viewdir]) (= Xr; 'concat': Xd is its head)
    for (int d = 0; d < g.np; ++d) {
        float gx, gy;
        gen_pos_grid(sc, d, n0, n1, n2, gx, gy);
        gf_plane_features(sc, g, R, n, h, d, g.C, gx, gy, raw ? d * g.C : 0, raw || d == 0 ? 0 : 1);
    }
    if (raw && !gf_density_only(PHASE)) gf_plane_features(sc, g, R, n, h, g.np, g.Cv, vgx, vgy, g.np * g.C, 0);
    __syncthreads();
    if (g.proj != 2 && (PHASE != GF_COLOUR || !raw)) {        // combine_pos_planes 'sum' / 'avg': plane by plane, then the mean
        for (int c = h; c < g.C; c += 2) {
            float s = R.row[c];
            if (raw)
                for (int d = 1; d < g.np; ++d) s = __fadd_rn(s, R.row[d * g.C + c]);
            R.row[R.xd_off + c] = gen_combine_pos(g.proj, s, g.np);
        }
        __syncthreads();
    }
}

// natural floats of the density decoder (its layers and fc_alpha): where the colour decoder's parameters start
__host__ __device__ inline long gf_density_floats(const GenGeom& g) {
    long n = 0;
    for (int l = 0; l < g.nd; ++l) {
        const int K = l == 0 ? g.Kd : g.hidden + (gen_skip_layer(l - 1, g.skip) ? g.Kd : 0);
        n += (long)g.hidden * K + g.hidden;
    }
    return n + g.hidden + 1;
}

// the point of this lane's slot: GF_FULL / GF_DENSITY: the slot itself; GF_COLOUR / GF_DENSITY_LIST: index[slot] while slot < the count (an index outside [0, P) is
// left out).  false: the whole workgroup lies beyond the list and returns (before any barrier).
template <int PHASE>
__device__ __forceinline__ bool gf_point(const GenFusedList& list, long P, long slot0, long slot, long& p, bool& live) {
    p = slot;
    live = slot < P;
    if (gf_listed(PHASE)) {
        long cnt = *list.count;
        if (cnt > list.max_count) cnt = list.max_count;
        if (slot0 >= cnt) return false;
        live = slot < cnt;
        p = live ? list.index[slot] : 0;
        live = live && p >= 0 && p < P;
        if (!live) p = 0;
    }
    return true;
}

// acc[t] (+)= W[32 t + m][k] . [X1 | X2][point][k] over the layered route's k pairs: the chain of generic_linear_kernel, NT tiles at once.
// row: this lane's point's row in LDS; X1 = row[x1 .. x1 + K1), X2 = row[x2 .. x2 + K2); W row-major [M][K1 + K2] in global memory.
template <int NT>
__device__ __forceinline__ void gf_layer(f32x16 (&acc)[NT], const float* row, int K1, int x1, int K2, int x2, const float* __restrict__ W, int M, int n,
                                         int h) {
    const int K = K1 + K2, Kp = (K + 31) & ~31;
    const float* wrow[NT];
    bool wok[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int m = 32 * t + n;
        wok[t] = m < M;
        wrow[t] = W + (long)(m < M ? m : M - 1) * K;
    }
    // GF_U k pairs per step, the next step's operands loaded (addresses clamped, values zeroed beyond K and M like the padded stage of the
    // layered kernel) in front of this step's MFMAs.  A: lane (m, h) = W[32 t + m][2s + h];  B: lane (n, h) = X[point n][2s + h]
    float a[GF_U][NT], bv[GF_U];
    auto fetch = [&](int k0, float (&fa)[GF_U][NT], float (&fb)[GF_U]) GEN_INL {
#pragma unroll
        for (int u = 0; u < GF_U; ++u) {
            const int kk = k0 + 2 * u + h, kc = kk < K ? kk : K - 1;
            const bool kok = kk < K;
            const float xv = row[kc < K1 ? x1 + kc : x2 + (kc - K1)];
            fb[u] = kok ? xv : 0.0f;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const float wv = wrow[t][kc];
                fa[u][t] = (kok && wok[t]) ? wv : 0.0f;
            }
        }
    };
    fetch(0, a, bv);
    for (int k0 = 0; k0 < Kp; k0 += 2 * GF_U) {
        float an[GF_U][NT], bn[GF_U];
        fetch(k0 + 2 * GF_U, an, bn);
#pragma unroll
        for (int u = 0; u < GF_U; ++u)
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] = mfma32(a[u][t], bv[u], acc[t]);
#pragma unroll
        for (int u = 0; u < GF_U; ++u) {
            bv[u] = bn[u];
#pragma unroll
            for (int t = 0; t < NT; ++t) a[u][t] = an[u][t];
        }
    }
}

// head of a decoder on the f32 activations: fc_rgb -> out[:, 0:3], fc_alpha -> out[:, 3] (heads and biases are f32 in every arithmetic)
__device__ __forceinline__ void gf_head(const float* row, int K, int x0, const float* __restrict__ w, bool rgb, int n, int h, float (&o)[3]) {
    const int M = rgb ? 3 : 1;
    f32x16 acc[1];
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[0][r] = 0.0f;
    gf_layer<1>(acc, row, K, x0, 0, x0, w, M, n, h);
    const float* b = w + (long)M * K;
#pragma unroll
    for (int r = 0; r < 3; ++r) o[r] = r < M ? __fadd_rn(acc[0][r], b[r]) : 0.0f;
}

// ---- host side: what the entry points and launches of generic_fused.hip, generic_fused_limb.hip and generic_fused_bwd.hip share ----------

// the launches of a kernel over `slots` point slots, 32 per wave: launch(b0, nb) starts the workgroups [b0, b0 + nb) (grid limit: pieces of
// whole point blocks); every piece's launch is checked
template <typename Launch>
static inline int gf_launch_pieces(long slots, int waves, Launch launch) {
    const long pts = 32L * waves, blocks = (slots + pts - 1) / pts, piece = 1L << 30;
    for (long b0 = 0; b0 < blocks; b0 += piece) {
        launch(b0, (unsigned)(blocks - b0 < piece ? blocks - b0 : piece));
        if (int e = NVSR_CHECK_LAUNCH()) return e;
    }
    return NVSR_OK;
}

// the instantiations of a plan: f(NT, CLS) with the plan's tiles and LDS class as std::integral_constant, NVSR_ERR_SHAPE for any other plan
template <typename F>
static inline int gf_for_plan(int nt, int cls, F f) {
#define GF_CASE(NT, CLS) \
    if (nt == NT && cls == CLS) return f(std::integral_constant<int, NT>{}, std::integral_constant<int, CLS>{});
#define GF_CASES(NT) GF_CASE(NT, 0) GF_CASE(NT, 1) GF_CASE(NT, 2)
    GF_CASES(1) GF_CASES(2) GF_CASES(3) GF_CASES(4) GF_CASES(6) GF_CASES(8)
#undef GF_CASES
#undef GF_CASE
    return NVSR_ERR_SHAPE;
}
// the run-time phase as the kernels' template argument: f(PHASE); what is no phase runs GF_FULL
template <typename F>
static inline int gf_for_phase(int phase, F f) {
    if (phase == GF_DENSITY) return f(std::integral_constant<int, GF_DENSITY>{});
    if (phase == GF_COLOUR) return f(std::integral_constant<int, GF_COLOUR>{});
    if (phase == GF_DENSITY_LIST) return f(std::integral_constant<int, GF_DENSITY_LIST>{});
    return f(std::integral_constant<int, GF_FULL>{});
}

// 1 / 0 / -status of a *_supported entry: the geometry resolved, then plan(g)
template <typename Plan>
static inline int gf_supported(const nvsr_decoder_geometry* geometry, int num_position_planes, Plan plan) {
    GenGeom g;
    if (int e = gen_resolve(geometry, &g, num_position_planes)) return -e;      // (the status codes are positive: 1 must stay "supported")
    return plan(g);
}
// the forward kernels' plan by arithmetic; 0 for an arithmetic that is neither NVSR_ARITH_F32 nor NVSR_ARITH_F16X2
static inline int gen_fused_plan_arith(const GenGeom& g, GenFusedPlan* pl, int arith) {
    return arith == NVSR_ARITH_F32 || arith == NVSR_ARITH_F16X2 ? gen_fused_plan(g, pl, arith == NVSR_ARITH_F16X2) : 0;
}

// The checks of an entry point, in the order that fixes its status codes: scene, geometry, plan(g) (the capacity) -- gf_check_capacity, which
// nvsr_generic_occupancy_build_ext asks alone -- then the caller's pointers (have_pointers), the list's pointers, the planes of the scene,
// P < 0, the list's bounds and the int32 limit.  GF_LAUNCH: launch; NVSR_OK: nothing to do; else the status.
template <typename Plan>
static inline int gf_check_capacity(const nvsr_scene_ext* scene, const nvsr_decoder_geometry* geometry, GenGeom* g, Plan plan) {
    if (int e = gen_check_ext(scene)) return e;
    if (int e = gen_resolve(geometry, g, scene->num_position_planes)) return e;
    return plan(*g) ? NVSR_OK : NVSR_ERR_SHAPE;
}
constexpr int GF_LAUNCH = -1;
template <typename Plan>
static inline int gf_check_entry(const nvsr_scene_ext* scene, const nvsr_decoder_geometry* geometry, Plan plan, bool have_pointers, int phase,
                                 const GenFusedList& list, int64_t P, GenGeom* g, SceneDevN* sc) {
    if (int e = gf_check_capacity(scene, geometry, g, plan)) return e;
    if (!have_pointers) return NVSR_ERR_NULL;
    const bool listed = gf_listed(phase);
    if (listed && (!list.index || !list.count)) return NVSR_ERR_NULL;
    *sc = gen_scene(scene);
    if (int e = gen_check_scene(*sc, *g)) return e;
    if (P < 0) return NVSR_ERR_SHAPE;
    if (listed && (list.max_count < 0 || list.max_count > P || P > 0x7fffffffL)) return NVSR_ERR_SHAPE;      // (int32 indices)
    return P == 0 || (listed && list.max_count == 0) ? NVSR_OK : GF_LAUNCH;
}

// generic_fused.hip: a phase of the exact-f32 kernel; everything has been checked by the caller, P > 0
int gen_fused_f32_phase(int phase, const SceneDevN& sc, const GenGeom& g, const GenFusedPlan& pl, long P, const float* x, const float* noise,
                        const float* natural, float* out, const GenFusedList& list, hipStream_t stream);
// generic_fused_limb.hip: a phase in either arithmetic behind gf_check_entry (NVSR_ARITH_F32: `packed` is not read and may be null)
int gen_fused_arith_phase(int phase, const nvsr_scene_ext* scene, const nvsr_decoder_geometry* geometry, const float* natural, const float* packed,
                          int64_t P, const float* x, const float* coord_noise, float* out, const GenFusedList& list, int arith, nvsr_stream_t stream);

}  // namespace nvsr
