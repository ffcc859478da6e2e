// generic_fused_bwd.hip's one-launch plane gradients of ANY decoder geometry with the hidden layers in NVSR_ARITH_F16X2, forward and transposed:
// the training twin of generic_fused_limb.hip for iterations in which the decoder's parameters take no gradient.  BY NAME only.
//
// Forward recompute: gf_stage0 and gfl_layer with relu(fma(acc, 2^-12, b)) out of the headers the forward launch compiles -- the activations, and
// so the gate bits (H > 0; NaN and 0 closed), are those of nvsr_generic_decode_fused_arith_ext(F16X2) at the same points.  Only the gate words stay.
// Heads: the data gradients from d_out are exact f32 from the natural blob (gf_layer_t, as in the f32 kernel).
//
// Transposed hidden layers (gflt_tiles): dX[p][k] = sum_m dZ[p][m] W[m][k] over the 16-row blocks of m, ascending, on v_mfma_f32_32x32x16_f16 with
// f32 accumulation.  A: the transposed fragments of nvsr_pack_generic_decoder_bwd_ext (include/nvsr.h has the layout), one 16-byte load per lane
// and MFMA: lane (k, h) holds W~[16 mb + 8 h .. + 7][column k of the tile], W~ = 2^8 W in two limbs.  B: the 8 gated dZ values m = 16 mb + 8 h ..
// + 7 of the lane's point from its row (two 16-byte reads; the hidden part of a row is padded with zeros to a multiple of 16), scaled by the row's
// own power of two and split like the forward's activations (gfl_split_scaled).  Per tile Wh zl, Wh zh, Wl zh (limb_w / limb_x).  Outputs wider
// than NT tiles (layer 0 and the skip parts: Kd, Kr up to 512) run in groups of NT tiles, as gf_input_grad does.
//
// Gradient scale: ONE power of two per point and layer, exact.  s = 2^e puts the largest |dZ[p][m]| of the gated row the layer consumes into
// [2^14, 2^15): the highest binade whose every number, and its rounding to f16, is finite (2^15 .. 2^16 holds 65520 and above, which round to inf).
// The native backward anchors at 2^3 because its one scale must hold for a whole chain whose values grow from layer to layer; a scale per layer
// has nothing to leave room for, and the highest anchor keeps the small entries of a row out of the f16 subnormals longest: an entry down to
// 2^-28 of the row's maximum still has a normal high limb.  The maximum is formed on the bits of |v| (so NaN and inf win) when the row is
// written: the lane's own values, then its partner half's -- no pass over LDS.  A zero row takes e = 0 and gives exact zeros.  dX = acc 2^(-8 - e)
// (ldexpf: exact but for underflow).  Multiplying every cotangent of a point by 2^k multiplies its gradients by 2^k bit for bit.
// Range: a hidden weight beyond |W| < 255 has the limbs (inf, -inf) and meets a finite or zero dZ: NaN.  A row whose maximum is not finite gives
// NaN gradients at its point, never a finite wrong number.  A wave that saw a non-finite gradient ORs 1 into the range flag.
//
// Everything behind the chain -- the __fadd_rn joins into dXd / dXr, the view plane, the combination rules transposed, the taps, one __fadd_rn of
// the two decoders' terms in front of one atomic -- is generic_fused_bwd_core.h's, shared with the f32 kernel.
//
// Rows in LDS (gen_fused_bwd_limb_plan): the limb forward's alignment (parts at multiples of 4 floats, ld = 4 x an odd number: its bank argument
// holds for the 16-byte reads here) with the backward's parts:
//     [0, Kr)  Xr / dXr    [xd_off, + Kd)  Xd / dXd    [h_off, + hidden up to 16)  activation / dZ    [dout_off, + 4)  d_out    [gate_off, ..)  gates
#include "generic_fused_bwd_core.h"
#include "generic_fused_limb_core.h"

namespace nvsr {

constexpr int GFLT_ANCHOR = 14;       // the row maximum, scaled, lies in [2^14, 2^15)

static inline int gen_fused_bwd_limb_plan(const GenGeom& g, GenFusedBwdPlan* pl) {
    GenFusedPlan f;
    if (!gen_fused_plan(g, &f, true)) return 0;
    auto up = [](int v, int a) { return (v + a - 1) & ~(a - 1); };
    pl->nt = f.nt;
    pl->gw = (g.hidden + 31) / 32;
    pl->xd_off = up(g.Kr, 4);
    pl->h_off = pl->xd_off + up(g.Kd, 4);
    pl->dout_off = pl->h_off + up(g.hidden, 16);
    pl->gate_off = pl->dout_off + 4;
    long ld = up(pl->gate_off + (g.nd + g.nr) * pl->gw, 4);
    if ((ld / 4) % 2 == 0) ld += 4;
    if (32 * ld > GF_LDS_FLOATS[GF_CLASSES - 1]) return 0;
    pl->ld = (int)ld;
    int best = 0;
    for (int c = 0; c < GF_CLASSES; ++c) {
        int w = GF_LDS_FLOATS[c] / (32 * pl->ld);
        if (w > GF_MAX_WAVES) w = GF_MAX_WAVES;
        const int per_cu = w * (4 >> c);
        if (per_cu > best) { best = per_cu; pl->cls = c; pl->waves = w; }
    }
    return best ? 1 : 0;
}

// ---- the transposed blob: per hidden layer the column part [0, K1) and, for a skip layer, the part [K1, K1 + K2), each [mb][t][limb] ----
NVSR_CX int gflt_mb(int hidden) { return (hidden + 15) >> 4; }
// columns of part `part` (0 / 1) of decoder layer l: its first column and how many (0: no such part)
__host__ __device__ inline void gflt_part(const GenGeom& g, bool rgb, int l, int part, int& col0, int& cols) {
    const int k0 = rgb ? g.Kr : g.Kd, K1 = l == 0 ? k0 : g.hidden, K2 = l > 0 && gen_skip_layer(l - 1, g.skip) ? k0 : 0;
    col0 = part ? K1 : 0;
    cols = part ? K2 : K1;
}
// 16-byte units (= lanes' A operands) of a part with `cols` columns, and of a whole layer
__host__ __device__ inline long gflt_part_vec(const GenGeom& g, int cols) { return (long)gflt_mb(g.hidden) * gfl_tt(cols) * 128; }
__host__ __device__ inline long gflt_layer_vec(const GenGeom& g, bool rgb, int l) {
    long v = 0;
    for (int part = 0; part < 2; ++part) {
        int col0, cols;
        gflt_part(g, rgb, l, part, col0, cols);
        v += gflt_part_vec(g, cols);
    }
    return v;
}
static int64_t gflt_packed_words(const GenGeom& g) {
    int64_t v = 0;
    for (int dec = 0; dec < 2; ++dec)
        for (int l = 0; l < (dec ? g.nr : g.nd); ++l) v += gflt_layer_vec(g, dec == 1, l);
    return 4 * v;
}

// one thread per packed word
__global__ __launch_bounds__(256) void generic_pack_limb_bwd_kernel(GenGeom g, long words, const float* __restrict__ natural, unsigned* __restrict__ packed) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= words) return;
    long w0 = 0, nat = 0;             // first packed word / first natural float of the layer part that holds idx
    int K = 0, col0 = 0, cols = 0;
    bool found = false;
    for (int dec = 0; dec < 2 && !found; ++dec) {
        const int nl = dec ? g.nr : g.nd;
        for (int l = 0; l < nl && !found; ++l) {
            K = gfl_layer_in(g, dec == 1, l);
            for (int part = 0; part < 2; ++part) {
                gflt_part(g, dec == 1, l, part, col0, cols);
                const long pw = 4 * gflt_part_vec(g, cols);
                if (idx < w0 + pw) { found = true; break; }
                w0 += pw;
            }
            if (!found) nat += (long)g.hidden * K + g.hidden;
        }
        if (!found) nat += (dec ? 3 : 1) * (long)g.hidden + (dec ? 3 : 1);      // the head between the decoders
    }
    const long r = idx - w0;
    const int TT = gfl_tt(cols);
    const int frag = (int)(r >> 8), word = (int)(r & 255), lane = word >> 2, j = word & 3;
    const int limb = frag & 1, t = (frag >> 1) % TT, mb = (frag >> 1) / TT;
    const int k = 32 * t + (lane & 31), m = 16 * mb + 8 * (lane >> 5) + 2 * j;
    const float* W = natural + nat;
    float v[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const float ws = (m + e < g.hidden && k < cols) ? __fmul_rn(W[(long)(m + e) * K + col0 + k], F16_W_SCALE) : 0.0f;
        const float hi = (float)(_Float16)ws;
        v[e] = limb ? __fsub_rn(ws, hi) : ws;
    }
    packed[idx] = f16_pair(v[1], v[0]);
}

// acc[t] (+)= 2^(8 + e) sum_m dZ[point][m] W[m][col0 + 32 (t0 + t) + k] in two f16 limbs over the 16-row blocks of m, ascending.
// dz: the lane's point's gated row, 16-byte aligned, zeros from `hidden` up to 16 MB; wp: the part's fragments [mb][t][limb][64]; TT: its tiles
template <int NT>
__device__ __forceinline__ void gflt_tiles(f32x16 (&acc)[NT], const float* dz, int MB, const u32x4* __restrict__ wp, int TT, int t0, int e, int lane,
                                           int h) {
    auto fetch_a = [&](int mb, u32x4 (&fa)[NT][2]) GEN_INL {
        const u32x4* f = wp + ((long)mb * TT + t0) * 128 + lane;
#pragma unroll
        for (int t = 0; t < NT; ++t)
            if (t0 + t < TT) { fa[t][0] = f[t * 128]; fa[t][1] = f[t * 128 + 64]; }
    };
    auto fetch_b = [&](int mb, float (&v)[8]) GEN_INL {
        const float* src = dz + 16 * mb + 8 * h;
        const f32x4 a = *reinterpret_cast<const f32x4*>(src), b = *reinterpret_cast<const f32x4*>(src + 4);
#pragma unroll
        for (int i = 0; i < 4; ++i) { v[i] = ldexpf(a[i], e); v[4 + i] = ldexpf(b[i], e); }
    };
    u32x4 fa[NT][2];
    float v[8];
    Limbs<2> zb;
    fetch_a(0, fa);
    fetch_b(0, v);
    gfl_split_scaled(v, zb);
    for (int mb = 0; mb < MB; ++mb) {
        u32x4 fn[NT][2];
        float vn[8];
        const int mn = mb + 1 < MB ? mb + 1 : mb;
        fetch_a(mn, fn);
        fetch_b(mn, vn);
#pragma unroll
        for (int t = 0; t < NT; ++t)
            if (t0 + t < TT) {
#pragma unroll
                for (int p = 0; p < 3; ++p) acc[t] = mfma_limb<2>(fa[t][limb_w(2, p)], zb.v[limb_x(2, p)], acc[t]);
            }
        gfl_split_scaled(vn, zb);
#pragma unroll
        for (int t = 0; t < NT; ++t)
            if (t0 + t < TT) { fa[t][0] = fn[t][0]; fa[t][1] = fn[t][1]; }
    }
}

// the scale of a gated row from the largest |v| bits of its point (both halves): e, or a row that is not finite
struct GfltScale {
    int e;             // dZ is multiplied by 2^e, the product by 2^(-8 - e)
    bool nan;          // the row holds an inf or a NaN: its gradients are NaN
};
__device__ __forceinline__ GfltScale gflt_scale(unsigned amax) {
    const unsigned other = (unsigned)__shfl_xor((int)amax, 32);
    amax = amax > other ? amax : other;
    const int eb = (int)(amax >> 23);
    GfltScale s;
    s.nan = eb == 255;
    s.e = amax == 0u ? 0 : GFLT_ANCHOR + 127 - eb;
    return s;
}
__device__ __forceinline__ float gflt_unscale(float acc, const GfltScale& s) { return s.nan ? __uint_as_float(0x7fc00000u) : ldexpf(acc, -F16_SW - s.e); }
__device__ __forceinline__ unsigned gflt_abs_bits(float v) { return __float_as_uint(v) & 0x7fffffffu; }

// dz[m] = val(acc's value of output m) where the gate bit of m is set, +0.0 where it is not, 16 bytes per store, zeros from `hidden` to hid4;
// -> the scale of the row just written; seen: the largest |bits| of the values before the gates (for the range flag)
template <int NT, class Val>
__device__ __forceinline__ GfltScale gflt_store_gated(const f32x16 (&acc)[NT], float* dz, int hidden, const unsigned* words, int gw, int h, Val val,
                                                      unsigned& seen) {
    const int hid4 = (hidden + 3) & ~3;
    unsigned amax = 0;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const unsigned bits = t < gw ? words[t] : 0u;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int m0 = 32 * t + 8 * q + 4 * h;
            if (m0 < hid4) {
                f32x4 y;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float v = m0 + i < hidden ? val(acc[t][4 * q + i]) : 0.0f;
                    const unsigned vb = gflt_abs_bits(v);
                    seen = seen > vb ? seen : vb;
                    const bool open = (bits >> (8 * q + 4 * h + i)) & 1u;
                    y[i] = open ? v : 0.0f;
                    if (open) amax = amax > vb ? amax : vb;
                }
                *reinterpret_cast<f32x4*>(dz + m0) = y;
            }
        }
    }
    return gflt_scale(amax);
}

// row[dx + k] = row[dx + k] + 2^(-8 - e) acc of the part's column k, k < Kn, in groups of NT tiles
template <int NT>
__device__ __forceinline__ void gflt_input_grad(float* row, int dz, int MB, const u32x4* __restrict__ wp, int Kn, int dx, const GfltScale& s, unsigned& seen,
                                                int lane, int h) {
    const int TT = gfl_tt(Kn);
    for (int t0 = 0; t0 < TT; t0 += NT) {
        f32x16 acc[NT];
        gf_zero<NT>(acc);
        gflt_tiles<NT>(acc, row + dz, MB, wp, TT, t0, s.e, lane, h);
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int k = 32 * (t0 + t) + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (k < Kn) {
                    const float v = gflt_unscale(acc[t][r], s);
                    const unsigned vb = gflt_abs_bits(v);
                    seen = seen > vb ? seen : vb;
                    row[dx + k] = __fadd_rn(row[dx + k], v);
                }
            }
    }
}

template <int NT, int LDSF>
__global__ __launch_bounds__(64 * GF_MAX_WAVES) void generic_backward_fused_limb_kernel(SceneDevN sc, GenGeom g, GenFusedBwdPlan L, long P, long block0,
                                                                                         const float* __restrict__ x, const float* __restrict__ noise,
                                                                                         const float* __restrict__ natural,
                                                                                         const unsigned* __restrict__ packed,
                                                                                         const unsigned* __restrict__ packed_bwd,
                                                                                         const float* __restrict__ d_out, GradPlanesN gp, unsigned* flag) {
    __shared__ __attribute__((aligned(16))) float lds[LDSF];
    NVSR_RACE_PROBE_DELAY(lds);      // (probe builds only, nvsr_common.h)
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, n = lane & 31, h = lane >> 5;
    const long slot0 = (block0 + blockIdx.x) * (long)(blockDim.x >> 6) * 32;
    const long p = slot0 + wave * 32 + n;
    const bool live = p < P;
    float* rows = lds + wave * 32 * L.ld;
    float* row = rows + n * L.ld;
    unsigned* gate = reinterpret_cast<unsigned*>(row + L.gate_off);
    const int TT = gfl_tt(g.hidden), MB = gflt_mb(g.hidden), hid4 = (g.hidden + 3) & ~3;

    // ---- forward: stage 0 and the hidden layers of both decoders in limbs, exactly as generic_decode_fused_limb_kernel; the gate bits stay ----
    const GenFusedRows R = {rows, row, L.ld, L.xd_off};
    float vgx, vgy;
    for (int c = hid4 + h; c < 16 * MB; c += 2) row[L.h_off + c] = 0.0f;       // the B operands' zeros behind the hidden part, for the whole kernel
    gf_stage0<GF_FULL>(sc, g, R, n, h, live, p, x, noise, vgx, vgy);
    const bool raw = g.proj == 2 || g.view == 4;
    const int xd_in = g.proj == 2 ? 0 : L.xd_off;       // 'concat': Xd is the head of Xr
    if (h == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) row[L.dout_off + r] = live ? d_out[p * 4 + r] : 0.0f;
    }
    const float* const wcolour = natural + gf_density_floats(g);
    {
        const u32x4* wp = reinterpret_cast<const u32x4*>(packed);
        for (int dec = 0; dec < 2; ++dec) {
            const bool rgb = dec == 1;
            if (rgb && !raw) {                                // Xd -> Xr: the combined position features, then combine_all_planes in place
                for (int c = h; c < g.C; c += 2) row[c] = row[L.xd_off + c];
                __syncthreads();
                gf_plane_features(sc, g, R, n, h, g.np, g.Cv, vgx, vgy, 0, 2);
                __syncthreads();
            }
            const int k0 = rgb ? g.Kr : g.Kd, nl = rgb ? g.nr : g.nd, in0 = rgb ? 0 : xd_in;
            const float* w = rgb ? wcolour : natural;
            int cur = in0, cur_k = k0;
            for (int l = 0; l < nl; ++l) {
                const bool skip = l > 0 && gen_skip_layer(l - 1, g.skip);
                const int K1 = cur_k, K2 = skip ? k0 : 0;
                f32x16 acc[NT];
                gf_zero<NT>(acc);
                gfl_layer<NT>(acc, row, K1, cur, K2, in0, wp, TT, lane, h);
                const float* b = w + (long)g.hidden * (K1 + K2);
                __syncthreads();
                unsigned* gl = gate + (rgb ? g.nd + l : l) * L.gw;
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    unsigned bits = 0;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int m0 = 32 * t + 8 * q + 4 * h;
                        if (t < TT && m0 < hid4) {
                            f32x4 y;
#pragma unroll
                            for (int i = 0; i < 4; ++i) {
                                const float s = m0 + i < g.hidden ? fmaf(acc[t][4 * q + i], GFL_UNSCALE, b[m0 + i]) : 0.0f;
                                y[i] = s < 0.0f ? 0.0f : s;   // (the forward launch's ReLU: keeps NaN)
                                if (y[i] > 0.0f) bits |= 1u << (8 * q + 4 * h + i);
                            }
                            *reinterpret_cast<f32x4*>(row + L.h_off + m0) = y;
                        }
                    }
                    bits |= (unsigned)__shfl_xor((int)bits, 32);
                    if (h == 0 && t < L.gw) gl[t] = bits;
                }
                __syncthreads();
                w += (long)g.hidden * (K1 + K2) + g.hidden;
                wp += (long)gfl_kb(K1 + K2) * TT * 128;
                cur = L.h_off; cur_k = g.hidden;
            }
        }
    }

    // ---- the transposed chains: the colour decoder first (its inputs' room is free), the view plane, then the density decoder ----
    float n0 = 0.0f, n1 = 0.0f, n2 = 0.0f;
    if (live) gen_position(sc, x + p * 6, noise, p, n0, n1, n2);
    unsigned seen = 0;                 // the largest |bits| of any gradient this lane formed: inf / NaN raise the range flag
    long dens_vec = 0;
    for (int l = 0; l < g.nd; ++l) dens_vec += gflt_layer_vec(g, false, l);
    for (int dec = 1; dec >= 0; --dec) {
        const bool rgb = dec == 1;
        const int k0 = rgb ? g.Kr : g.Kd, nl = rgb ? g.nr : g.nd, Mh = rgb ? 3 : 1, dx = rgb ? 0 : L.xd_off;
        // the layers' offsets: the head follows the last layer; wq: behind the decoder's last transposed fragments
        const float* wh = rgb ? wcolour : natural;
        const u32x4* wq = reinterpret_cast<const u32x4*>(packed_bwd) + (rgb ? dens_vec : 0);
        for (int l = 0; l < nl; ++l) {
            wh += (long)g.hidden * (gfl_layer_in(g, rgb, l) + 1);
            wq += gflt_layer_vec(g, rgb, l);
        }
        for (int c = h; c < k0; c += 2) row[dx + c] = 0.0f;       // the gradient of the decoder's input starts at +0.0
        GfltScale s;
        // the head: d_out -> the gradient of the last layer's output in exact f32, gated by that layer
        {
            f32x16 acc[NT];
            gf_zero<NT>(acc);
            gf_layer_t<NT>(acc, row, L.dout_off + (rgb ? 0 : 3), Mh, wh, g.hidden, 0, g.hidden, n, h);
            __syncthreads();
            s = gflt_store_gated<NT>(acc, row + L.h_off, g.hidden, gate + (rgb ? g.nd + nl - 1 : nl - 1) * L.gw, L.gw, h, [](float a) { return a; }, seen);
            __syncthreads();
        }
        for (int l = nl - 1; l >= 0; --l) {
            int c1, K1, c2, K2;
            gflt_part(g, rgb, l, 0, c1, K1);
            gflt_part(g, rgb, l, 1, c2, K2);
            wq -= gflt_layer_vec(g, rgb, l);
            if (l == 0) {
                gflt_input_grad<NT>(row, L.h_off, MB, wq, K1, dx, s, seen, lane, h);
                __syncthreads();
                break;
            }
            if (K2) gflt_input_grad<NT>(row, L.h_off, MB, wq + gflt_part_vec(g, K1), K2, dx, s, seen, lane, h);
            f32x16 acc[NT];
            gf_zero<NT>(acc);
            gflt_tiles<NT>(acc, row + L.h_off, MB, wq, TT, 0, s.e, lane, h);
            __syncthreads();                              // the layer's last read is done: its input gradient takes dZ's place, gated
            const GfltScale prev = s;
            s = gflt_store_gated<NT>(acc, row + L.h_off, g.hidden, gate + (rgb ? g.nd + l - 1 : l - 1) * L.gw, L.gw, h,
                                     [&](float a) { return gflt_unscale(a, prev); }, seen);
            __syncthreads();
        }
        if (rgb) gfb_view_scatter(sc, g, rows, L.ld, L.xd_off, gp, vgx, vgy, slot0 + wave * 32, P, n, h);
    }
    gfb_plane_scatter(sc, g, rows, L.ld, L.xd_off, gp, n0, n1, n2, slot0 + wave * 32, P, n, h);
    // range flag of the f16 limbs (nvsr.h: nvsr_set_range_flag): one atomic per wave that formed a non-finite gradient
    if (flag && __any(seen >= 0x7f800000u) && lane == 0) __hip_atomic_fetch_or(flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace nvsr

using namespace nvsr;

extern "C" {

int nvsr_generic_backward_fused_supported_arith(const nvsr_decoder_geometry* geometry, int num_position_planes, int arith) {
    if (arith == NVSR_ARITH_F32) return nvsr_generic_backward_fused_supported(geometry, num_position_planes);
    return gf_supported(geometry, num_position_planes, [&](const GenGeom& g) {
        GenFusedBwdPlan pl;
        return arith == NVSR_ARITH_F16X2 ? gen_fused_bwd_limb_plan(g, &pl) : 0;
    });
}

int64_t nvsr_generic_packed_bwd_floats_ext(const nvsr_decoder_geometry* geometry, int num_position_planes) {
    GenGeom g;
    if (int e = gen_resolve(geometry, &g, num_position_planes)) return -e;
    return gflt_packed_words(g);
}

int nvsr_pack_generic_decoder_bwd_ext(const nvsr_decoder_geometry* geometry, int num_position_planes, const float* natural, float* packed_bwd,
                                      nvsr_stream_t stream) {
    GenGeom g;
    if (int e = gen_resolve(geometry, &g, num_position_planes)) return e;
    if (!natural || !packed_bwd) return NVSR_ERR_NULL;
    const int64_t words = gflt_packed_words(g);
    hipLaunchKernelGGL(generic_pack_limb_bwd_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, (hipStream_t)stream, g, (long)words, natural,
                       reinterpret_cast<unsigned*>(packed_bwd));
    return NVSR_CHECK_LAUNCH();
}

int nvsr_generic_decode_backward_fused_arith_ext(const nvsr_scene_ext* scene, const nvsr_decoder_geometry* geometry, const float* natural,
                                                 const float* packed, const float* packed_bwd, int64_t P, const float* x, const float* coord_noise,
                                                 const float* d_out, float* const* d_planes, int arith, nvsr_stream_t stream) {
    if (arith == NVSR_ARITH_F32) return nvsr_generic_decode_backward_fused_ext(scene, geometry, natural, P, x, coord_noise, d_out, d_planes, stream);
    if (arith != NVSR_ARITH_F16X2) return NVSR_ERR_SHAPE;      // by name only: no process default, no one-limb or bf16 mode here
    GenGeom g;
    GenFusedBwdPlan pl;
    SceneDevN sc;
    const int e = gf_check_entry(scene, geometry, [&](const GenGeom& gg) { return gen_fused_bwd_limb_plan(gg, &pl); },
                                 natural && packed && packed_bwd && x && d_out, GF_FULL, GenFusedList{nullptr, nullptr, 0}, P, &g, &sc);
    if (e != GF_LAUNCH) return e;
    GradPlanesN gp = {};
    if (!gfb_wanted(d_planes, g.np, &gp)) return NVSR_OK;
    unsigned* flag = nvsr_get_range_flag();
    return gf_for_plan(pl.nt, pl.cls, [&](auto nt, auto cls) {
        constexpr int NT = decltype(nt)::value, LDSF = GF_LDS_FLOATS[decltype(cls)::value];
        return gf_launch_pieces((long)P, pl.waves, [&](long b0, unsigned nb) {
            hipLaunchKernelGGL((generic_backward_fused_limb_kernel<NT, LDSF>), dim3(nb), dim3(64 * pl.waves), 0, (hipStream_t)stream, sc, g, pl, (long)P, b0,
                               x, coord_noise, natural, reinterpret_cast<const unsigned*>(packed), reinterpret_cast<const unsigned*>(packed_bwd), d_out, gp,
                               flag);
        });
    });
}

}  // extern "C"
