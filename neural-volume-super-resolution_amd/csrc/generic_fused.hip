// TwoDimPlanesModel.forward for ANY decoder geometry, evaluation only, in ONE launch: the fused twin of generic.hip's layer-by-layer forward.
//
// Reference: models.py:381-421 (see generic.hip for the layer lists and the combination rules; both files compile them out of generic_core.h).
//
// The contract is the layered route's BITS.  There, every output of a layer is one v_mfma_f32_32x32x2_f32 chain from +0.0 over the k pairs
// (2s, 2s + 1) of the concatenated input [X1 | X2] in ascending order, up to K rounded up to 32 with zero operands, followed by
// __fadd_rn(acc, b[m]) and fmaxf(., 0).  An MFMA output depends on its own row of A and its own column of B only, so the same instruction on
// the same operand pairs in the same order gives the same bits wherever the tile sits: gf_layer below is that chain, and the only place it is
// written (a limb arithmetic would swap the product there).
//
// generic_decode_fused_kernel: a workgroup of 1 .. 4 waves, 32 points per wave; a wave only ever touches its own 32 rows of LDS.
//   row of a point (GenFusedPlan::ld floats, 2 x an odd number: the 64 lanes (point n, k half h) of a B-operand read hit 64 different banks):
//     [0, Kr)           the colour decoder's input Xr -- of which the density decoder's input Xd is the first Kd columns whenever the position
//                       features are concatenated ('concat'); under 'sum' / 'avg' / 'mult' view features Xd (= Kr columns) stands here first
//                       and becomes Xr in place once the density decoder is done
//     [xd_off, + Kd)    Xd under 'sum' / 'avg' position features with 'concat_pos': made from the raw per-plane features of Xr
//     [h_off, + hidden) the current layer's input / output
//   stage 0   per (point, plane): position, projection (atan2f for the view plane) once per point, the taps once per (point, plane) -- two
//             points at a time, 32 lanes each over the channels, so a tap's channels are one contiguous read
//   layers    k outer, the layer's NT 32-row output tiles inner: one LDS read feeds NT independent MFMA chains, the whole layer's
//             accumulators are held, and the output replaces the input in place behind the last read.  Weights and biases come straight
//             from the natural blob (L2 / L1 resident: a few MB at most).
//   heads     out[p][3] behind the density decoder, out[p][0:3] behind the colour decoder
// Capacity (gen_fused_plan, documented in include/nvsr.h): hidden <= 256 (NT <= 8: 128 accumulator registers), max(Kd, Kr) <= 512, 32 rows in
// 160 KB.  The LDS array is static (40 / 80 / 160 KB instantiations, so that small geometries keep several workgroups per CU); the plan takes
// the size class that puts the most waves on a CU.
#include "generic_core.h"

namespace nvsr {

struct GenFusedPlan {
    int nt;              // 32-row output tiles of a hidden layer the kernel is instantiated for: 1, 2, 3, 4, 6, 8
    int cls;             // LDS size class
    int waves;           // waves (= 32-point blocks) per workgroup
    int ld, xd_off, h_off;
};
constexpr int GF_CLASSES = 3;
constexpr int GF_LDS_FLOATS[GF_CLASSES] = {10240, 20480, 40960};      // 40, 80, 160 KB: 4, 2, 1 workgroups per CU
constexpr int GF_MAX_WAVES = 4;
constexpr int GF_U = 4;             // k pairs per step of the layer loop (the padded K is a multiple of 32)
constexpr int GF_MAX_HIDDEN = 256, GF_MAX_K0 = 512;

// 1 = the fused kernel holds this geometry, 0 = it does not (the layered route does)
static int gen_fused_plan(const GenGeom& g, GenFusedPlan* pl) {
    const int k0 = g.Kd > g.Kr ? g.Kd : g.Kr;
    if (g.hidden > GF_MAX_HIDDEN || k0 > GF_MAX_K0) return 0;
    const bool own_xd = g.view == 4 && g.proj != 2;
    pl->xd_off = own_xd ? g.Kr : 0;
    pl->h_off = own_xd ? g.Kr + g.Kd : k0;
    int ld = pl->h_off + g.hidden;
    ld += ld & 1;
    if ((ld / 2) % 2 == 0) ld += 2;
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

template <int NT, int LDSF>
__global__ __launch_bounds__(64 * GF_MAX_WAVES) void generic_decode_fused_kernel(SceneDevN sc, GenGeom g, GenFusedPlan L, long P, long block0,
                                                                                  const float* __restrict__ x, const float* __restrict__ noise,
                                                                                  const float* __restrict__ natural, float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float lds[LDSF];
    NVSR_RACE_PROBE_DELAY(lds);      // (probe builds only, nvsr_common.h)
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, n = lane & 31, h = lane >> 5;
    const long p = ((block0 + blockIdx.x) * (long)(blockDim.x >> 6) + wave) * 32 + n;
    const bool live = p < P;
    float* rows = lds + wave * 32 * L.ld;       // this wave's 32 points
    float* row = rows + n * L.ld;               // this lane's point (shared by the lane's two halves)

    // ---- stage 0: the decoder inputs ----
    // (a point past P takes part with the position 0: in-bounds taps, nothing stored)
    float n0 = 0.0f, n1 = 0.0f, n2 = 0.0f, vgx = 0.0f, vgy = 0.0f;
    if (live) {
        gen_position(sc, x + p * 6, noise, p, n0, n1, n2);
        gen_view_grid(sc, x + p * 6, vgx, vgy);
    }
    // features of plane d at the 32 points' grid coordinates (gx, gy: lane n holds point n's) into columns col0 + c of their rows;
    // mode 0: stored, 1: added to what is there, 2: combined with what is there as the view-direction feature
    auto plane_features = [&](int d, int Cc, float gx, float gy, int col0, int mode) GEN_INL {
        const float* __restrict__ pl = sc.plane[d];
        const int H = sc.ph[d], W = sc.pw[d];
        auto put = [&](float* r, float v) GEN_INL { *r = mode == 0 ? v : mode == 1 ? __fadd_rn(*r, v) : gen_combine_view(g.view, *r, v); };
        for (int i = 0; i < 16; ++i) {
            const int pt = 2 * i + h;
            const float px = __shfl(gx, pt), py = __shfl(gy, pt);
            float* r = rows + pt * L.ld + col0;
            if (sc.bicubic) {
                const CubicTaps t = gen_cubic_taps(H, W, px, py, sc.align);
                for (int c = n; c < Cc; c += 32) put(r + c, gen_cubic_blend(pl, W, Cc, t, c));
            } else {
                const GenTaps t = gen_taps(H, W, Cc, px, py, sc.align);
                for (int c = n; c < Cc; c += 32) put(r + c, gen_blend(pl, t, c));
            }
        }
    };
    const bool raw = g.proj == 2 || g.view == 4;          // the rows start as cat(pos_planes + [viewdir]) (= Xr; 'concat': Xd is its head)
    for (int d = 0; d < g.np; ++d) {
        float gx, gy;
        gen_pos_grid(sc, d, n0, n1, n2, gx, gy);
        plane_features(d, g.C, gx, gy, raw ? d * g.C : 0, raw || d == 0 ? 0 : 1);
    }
    if (raw) plane_features(g.np, g.Cv, vgx, vgy, g.np * g.C, 0);
    __syncthreads();
    if (g.proj != 2) {                                    // combine_pos_planes 'sum' / 'avg': plane by plane, then the mean
        for (int c = h; c < g.C; c += 2) {
            float s = row[c];
            if (raw)
                for (int d = 1; d < g.np; ++d) s = __fadd_rn(s, row[d * g.C + c]);
            row[L.xd_off + c] = gen_combine_pos(g.proj, s, g.np);
        }
        __syncthreads();
    }

    // ---- the two decoders ----
    const float* w = natural;
    for (int dec = 0; dec < 2; ++dec) {
        const bool rgb = dec == 1;
        if (rgb && !raw) {                                // Xd -> Xr in place: combine_all_planes 'sum' / 'avg' / 'mult'
            plane_features(g.np, g.Cv, vgx, vgy, 0, 2);
            __syncthreads();
        }
        const int k0 = rgb ? g.Kr : g.Kd, nl = rgb ? g.nr : g.nd, in0 = rgb ? 0 : L.xd_off;
        int cur = in0, cur_k = k0;
        for (int l = 0; l < nl; ++l) {
            const bool skip = l > 0 && gen_skip_layer(l - 1, g.skip);       // x = cat(x, input) in front of this layer (models.py:397-399)
            const int K1 = cur_k, K2 = skip ? k0 : 0;
            f32x16 acc[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
            gf_layer<NT>(acc, row, K1, cur, K2, in0, w, g.hidden, n, h);
            const float* b = w + (long)g.hidden * (K1 + K2);
            __syncthreads();                              // the layer's last read is done: its output takes the input's place
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int m = 32 * t + (r & 3) + 8 * (r >> 2) + 4 * h;
                    if (m < g.hidden) row[L.h_off + m] = fmaxf(__fadd_rn(acc[t][r], b[m]), 0.0f);
                }
            __syncthreads();
            w += (long)g.hidden * (K1 + K2) + g.hidden;
            cur = L.h_off; cur_k = g.hidden;
        }
        const int M = rgb ? 3 : 1;                        // fc_rgb -> out[:, 0:3], fc_alpha -> out[:, 3]
        f32x16 acc[1];
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[0][r] = 0.0f;
        gf_layer<1>(acc, row, cur_k, cur, 0, cur, w, M, n, h);
        const float* b = w + (long)M * g.hidden;
        if (live && h == 0) {
#pragma unroll
            for (int r = 0; r < 3; ++r)
                if (r < M) out[p * 4 + (rgb ? 0 : 3) + r] = __fadd_rn(acc[0][r], b[r]);
        }
        w += (long)M * g.hidden + M;
    }
}

template <int NT, int CLS>
static int gen_fused_launch(const SceneDevN& sc, const GenGeom& g, const GenFusedPlan& pl, long P, const float* x, const float* noise, const float* natural,
                            float* out, hipStream_t stream) {
    const long pts = 32L * pl.waves, blocks = (P + pts - 1) / pts, piece = 1L << 30;       // (grid limit: pieces of whole point blocks)
    for (long b0 = 0; b0 < blocks; b0 += piece) {
        const long nb = blocks - b0 < piece ? blocks - b0 : piece;
        hipLaunchKernelGGL((generic_decode_fused_kernel<NT, GF_LDS_FLOATS[CLS]>), dim3((unsigned)nb), dim3(64 * pl.waves), 0, stream, sc, g, pl, P, b0, x,
                           noise, natural, out);
        if (int e = NVSR_CHECK_LAUNCH()) return e;
    }
    return NVSR_OK;
}

}  // namespace nvsr

using namespace nvsr;

extern "C" {

int nvsr_generic_fused_supported(const nvsr_decoder_geometry* geometry, int num_position_planes) {
    GenGeom g;
    if (int e = gen_resolve(geometry, &g, num_position_planes)) return -e;      // (the status codes are positive: 1 must stay "supported")
    GenFusedPlan pl;
    return gen_fused_plan(g, &pl);
}

int nvsr_generic_decode_fused_ext(const nvsr_scene_ext* scene, const nvsr_decoder_geometry* geometry, const float* natural, int64_t P, const float* x,
                                  const float* coord_noise, float* out, nvsr_stream_t stream) {
    if (int e = gen_check_ext(scene)) return e;
    GenGeom g;
    if (int e = gen_resolve(geometry, &g, scene->num_position_planes)) return e;
    GenFusedPlan pl;
    if (!gen_fused_plan(g, &pl)) return NVSR_ERR_SHAPE;
    if (!natural || !x || !out) return NVSR_ERR_NULL;
    const SceneDevN sc = gen_scene(scene);
    if (int e = gen_check_scene(sc, g)) return e;
    if (P < 0) return NVSR_ERR_SHAPE;
    if (P == 0) return NVSR_OK;
    hipStream_t s = (hipStream_t)stream;
#define GF_CASE(NT, CLS) \
    if (pl.nt == NT && pl.cls == CLS) return gen_fused_launch<NT, CLS>(sc, g, pl, (long)P, x, coord_noise, natural, out, s);
#define GF_CASES(NT) GF_CASE(NT, 0) GF_CASE(NT, 1) GF_CASE(NT, 2)
    GF_CASES(1) GF_CASES(2) GF_CASES(3) GF_CASES(4) GF_CASES(6) GF_CASES(8)
#undef GF_CASES
#undef GF_CASE
    return NVSR_ERR_SHAPE;
}

}  // extern "C"
