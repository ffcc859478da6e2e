// The text of the exact-f32 fused backward kernel of the generic decoder geometries.  generic_fused_bwd.hip includes it TWICE (no include guard):
//   GFB_RECORD 0  GFB_KERNEL_NAME = generic_backward_fused_kernel: the plane gradients, as documented at the head of generic_fused_bwd.hip.  The
//                 preprocessor leaves exactly the kernel that stood in that file: its instantiations keep their instructions
//                 (profiles/generic_train_decoder_isa.txt).
//   GFB_RECORD 1  GFB_KERNEL_NAME = generic_backward_fused_record_kernel: the same launch, which also stores a GenRecord -- the operands of the
//                 weight-gradient contraction -- for its P points (a chunk: the arrays are indexed by the launch's own points) as it forms
//                 them in LDS, and leaves out the decoder inputs' gradients and both scatters when rec.planes is 0.
template <int NT, int LDSF>
__global__ __launch_bounds__(64 * GF_MAX_WAVES) void GFB_KERNEL_NAME(SceneDevN sc, GenGeom g, GenFusedBwdPlan L, long P, long block0,
                                                                      const float* __restrict__ x, const float* __restrict__ noise,
                                                                      const float* __restrict__ natural,
                                                                      const float* __restrict__ d_out, GradPlanesN gp
#if GFB_RECORD
                                                                      , GenRecord rec
#endif
                                                                      ) {
    __shared__ __attribute__((aligned(16))) float lds[LDSF];
    NVSR_RACE_PROBE_DELAY(lds);      // (probe builds only, nvsr_common.h)
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, n = lane & 31, h = lane >> 5;
    const long slot0 = (block0 + blockIdx.x) * (long)(blockDim.x >> 6) * 32;
    const long p = slot0 + wave * 32 + n;
    const bool live = p < P;
    float* rows = lds + wave * 32 * L.ld;
    float* row = rows + n * L.ld;
    unsigned* gate = reinterpret_cast<unsigned*>(row + L.gate_off);

    // ---- forward: stage 0 and the hidden layers of both decoders; the gate bits stay ----
    const GenFusedRows R = {rows, row, L.ld, L.xd_off};
    float vgx, vgy;
    gf_stage0<GF_FULL>(sc, g, R, n, h, live, p, x, noise, vgx, vgy);
    const bool raw = g.proj == 2 || g.view == 4;
    const int xd_in = g.proj == 2 ? 0 : L.xd_off;       // 'concat': Xd is the head of Xr
#if GFB_RECORD
    const long base = slot0 + wave * 32;                // the wave's first point
    const bool planes = rec.planes != 0;
    gfr_store_rows(rows, L.ld, xd_in, g.Kd, rec.Xd, base, P, lane);       // Xd, behind stage 0's barrier
#endif
    if (h == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) row[L.dout_off + r] = live ? d_out[p * 4 + r] : 0.0f;
    }
    const float* const wcolour = natural + gf_density_floats(g);
    for (int dec = 0; dec < 2; ++dec) {
        const bool rgb = dec == 1;
        if (rgb && !raw) {                                // Xd -> Xr: the combined position features, then combine_all_planes in place
            for (int c = h; c < g.C; c += 2) row[c] = row[L.xd_off + c];
            __syncthreads();
            gf_plane_features(sc, g, R, n, h, g.np, g.Cv, vgx, vgy, 0, 2);
            __syncthreads();
        }
#if GFB_RECORD
        if (rgb) gfr_store_rows(rows, L.ld, 0, g.Kr, rec.Xr, base, P, lane);       // Xr, after combine_all_planes
#endif
        const int k0 = rgb ? g.Kr : g.Kd, nl = rgb ? g.nr : g.nd, in0 = rgb ? 0 : xd_in;
        const float* w = rgb ? wcolour : natural;
        int cur = in0, cur_k = k0;
        for (int l = 0; l < nl; ++l) {
            const bool skip = l > 0 && gen_skip_layer(l - 1, g.skip);
            const int K1 = cur_k, K2 = skip ? k0 : 0;
            f32x16 acc[NT];
            gf_zero<NT>(acc);
            gf_layer<NT>(acc, row, K1, cur, K2, in0, w, g.hidden, n, h);
            const float* b = w + (long)g.hidden * (K1 + K2);
            __syncthreads();
            unsigned* gl = gate + (rgb ? g.nd + l : l) * L.gw;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                unsigned bits = 0;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int j = (r & 3) + 8 * (r >> 2) + 4 * h, m = 32 * t + j;
                    if (m < g.hidden) {
                        const float v = fmaxf(__fadd_rn(acc[t][r], b[m]), 0.0f);
                        row[L.h_off + m] = v;
                        if (v > 0.0f) bits |= 1u << j;
                    }
                }
                bits |= (unsigned)__shfl_xor((int)bits, 32);
                if (h == 0 && t < L.gw) gl[t] = bits;
            }
            __syncthreads();
#if GFB_RECORD
            gfr_store_rows(rows, L.ld, L.h_off, g.hidden, rec.H + (long)(rgb ? g.nd + l : l) * P * g.hidden, base, P, lane);
#endif
            w += (long)g.hidden * (K1 + K2) + g.hidden;
            cur = L.h_off; cur_k = g.hidden;
        }
    }

    // ---- the transposed chains: the colour decoder first (its inputs' room is free), the view plane, then the density decoder ----
    float n0 = 0.0f, n1 = 0.0f, n2 = 0.0f;
    if (live) gen_position(sc, x + p * 6, noise, p, n0, n1, n2);
    for (int dec = 1; dec >= 0; --dec) {
        const bool rgb = dec == 1;
        const int k0 = rgb ? g.Kr : g.Kd, nl = rgb ? g.nr : g.nd, Mh = rgb ? 3 : 1, dx = rgb ? 0 : L.xd_off;
        // the layers' offsets: the head follows the last layer
        const float* wh = rgb ? wcolour : natural;
        for (int l = 0; l < nl; ++l) wh += (long)g.hidden * ((l == 0 ? k0 : g.hidden + (gen_skip_layer(l - 1, g.skip) ? k0 : 0)) + 1);
        for (int c = h; c < k0; c += 2) row[dx + c] = 0.0f;       // the gradient of the decoder's input starts at +0.0
        // the head: d_out -> the gradient of the last layer's output, gated by that layer
        {
            f32x16 acc[NT];
            gf_zero<NT>(acc);
            gf_layer_t<NT>(acc, row, L.dout_off + (rgb ? 0 : 3), Mh, wh, g.hidden, 0, g.hidden, n, h);
            __syncthreads();
            gf_store_gated<NT>(acc, row + L.h_off, g.hidden, gate + (rgb ? g.nd + nl - 1 : nl - 1) * L.gw, L.gw, h);
            __syncthreads();
#if GFB_RECORD
            gfr_store_rows(rows, L.ld, L.h_off, g.hidden, rec.dZ + (long)(rgb ? g.nd + nl - 1 : nl - 1) * P * g.hidden, base, P, lane);
#endif
        }
        const float* w = wh;
        for (int l = nl - 1; l >= 0; --l) {
            const bool skip = l > 0 && gen_skip_layer(l - 1, g.skip);
            const int K1 = l == 0 ? k0 : g.hidden, K2 = skip ? k0 : 0, K = K1 + K2;
            w -= (long)g.hidden * (K + 1);
            if (l == 0) {
#if GFB_RECORD
                if (!planes) break;                       // (uniform: the record needs no gradient of a decoder's input)
#endif
                gf_input_grad<NT>(row, L.h_off, g.hidden, w, K, 0, K1, dx, n, h);
                __syncthreads();
                break;
            }
#if GFB_RECORD
            if (skip && planes) gf_input_grad<NT>(row, L.h_off, g.hidden, w, K, K1, K2, dx, n, h);
#else
            if (skip) gf_input_grad<NT>(row, L.h_off, g.hidden, w, K, K1, K2, dx, n, h);
#endif
            f32x16 acc[NT];
            gf_zero<NT>(acc);
            gf_layer_t<NT>(acc, row, L.h_off, g.hidden, w, K, 0, K1, n, h);
            __syncthreads();                              // the layer's last read is done: its input gradient takes dZ's place, gated
            gf_store_gated<NT>(acc, row + L.h_off, g.hidden, gate + (rgb ? g.nd + l - 1 : l - 1) * L.gw, L.gw, h);
            __syncthreads();
#if GFB_RECORD
            gfr_store_rows(rows, L.ld, L.h_off, g.hidden, rec.dZ + (long)(rgb ? g.nd + l - 1 : l - 1) * P * g.hidden, base, P, lane);
#endif
        }

#if GFB_RECORD
        if (!planes) continue;
#endif
        if (rgb) {
            gfb_view_scatter(sc, g, rows, L.ld, L.xd_off, gp, vgx, vgy, slot0 + wave * 32, P, n, h);
        }
    }

#if GFB_RECORD
    if (!planes) return;
#endif
    gfb_plane_scatter(sc, g, rows, L.ld, L.xd_off, gp, n0, n1, n2, slot0 + wave * 32, P, n, h);
}
