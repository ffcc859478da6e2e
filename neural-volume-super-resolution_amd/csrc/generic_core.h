// What the kernels of the generic decoder geometries share: the resolved geometry, the extended scene, the grid_sample taps (bilinear and
// bicubic), the sample position and the combination rules of TwoDimPlanesModel.forward (models.py:381-421 with combine_pos_planes :355-361 and
// combine_all_planes :363-379).  generic.hip (layer by layer, forward and backward) and generic_fused.hip (one launch, evaluation) compile the
// SAME expressions out of this header: the fused route's contract is the layered route's bits.
#pragma once
#include "decode_core.h"

namespace nvsr {

// the lambdas of the input kernels read the scene out of the kernel arguments: kept as calls (the inliner's choice once the bicubic taps made them
// large) they receive the 700-byte scene through scratch memory and lose the planes' address space
#define GEN_INL __attribute__((always_inline))

struct GenGeom {
    int C, Cv, hidden, nd, nr, skip, proj, view;      // proj: 0 sum 1 avg 2 concat; view: 0 sum 1 avg 2 mult 3 concat 4 concat_pos
    int Kd, Kr;
    int np;                                           // position planes (num_density_planes, models.py:140): 3 unless a scene_ext says otherwise
};

// the scene of the generic kernels: up to NVSR_MAX_POSITION_PLANES position planes with their projections, then the view-direction plane;
// grid_sample's align_corners; the optional jitter of the normalised sample positions (models.py:291-293)
struct SceneDevN {
    const float* plane[NVSR_MAX_POSITION_PLANES + 1];
    int ph[NVSR_MAX_POSITION_PLANES + 1], pw[NVSR_MAX_POSITION_PLANES + 1];
    float lo[5], range[5];
    float proj[NVSR_MAX_POSITION_PLANES * 6];
    int np, align, bicubic;
};

static inline SceneDevN gen_scene(const nvsr_scene* s) {
    SceneDevN d = {};
    for (int i = 0; i < 4; ++i) { d.plane[i] = s->planes[i]; d.ph[i] = s->ph[i]; d.pw[i] = s->pw[i]; }
    for (int i = 0; i < 5; ++i) { d.lo[i] = s->lo[i]; d.range[i] = s->range[i]; }
    for (int i = 0; i < 18; ++i) d.proj[i] = (&s->proj[0][0])[i];
    d.np = 3; d.align = 1; d.bicubic = 0;
    return d;
}
static inline SceneDevN gen_scene(const nvsr_scene_ext* s) {
    SceneDevN d = {};
    for (int i = 0; i <= s->num_position_planes; ++i) { d.plane[i] = s->planes[i]; d.ph[i] = s->ph[i]; d.pw[i] = s->pw[i]; }
    for (int i = 0; i < 5; ++i) { d.lo[i] = s->lo[i]; d.range[i] = s->range[i]; }
    for (int i = 0; i < 6 * s->num_position_planes; ++i) d.proj[i] = (&s->proj[0][0])[i];
    d.np = s->num_position_planes; d.align = s->align_corners ? 1 : 0; d.bicubic = s->plane_interp == NVSR_PLANE_INTERP_BICUBIC ? 1 : 0;
    return d;
}

__host__ __device__ inline bool gen_skip_layer(int layer_num, int skip) { return skip > 0 && layer_num % skip == 0 && layer_num > 0; }

static inline int gen_resolve(const nvsr_decoder_geometry* g, GenGeom* o, int np = 3) {
    if (!g) return NVSR_ERR_NULL;
    if (np < 1 || np > NVSR_MAX_POSITION_PLANES) return NVSR_ERR_SHAPE;
    o->np = np;
    o->C = g->plane_channels; o->Cv = g->viewdir_channels; o->hidden = g->hidden; o->nd = g->density_layers; o->nr = g->rgb_layers;
    o->skip = g->skip_connect_every; o->proj = g->proj_combination; o->view = g->viewdir_combination;
    if (o->C < 1 || o->C > 1024 || o->Cv < 1 || o->Cv > 1024 || o->hidden < 1 || o->hidden > 4096 || o->nd < 1 || o->nd > 64 || o->nr < 1 || o->nr > 64)
        return NVSR_ERR_SHAPE;
    if (o->skip < 0 || o->proj < 0 || o->proj > 2 || o->view < 0 || o->view > 4) return NVSR_ERR_SHAPE;
    // the combinations the reference's own layer sizes admit (models.py:186-190 vs :363-379)
    const bool concat_like = o->proj == 2 || o->view == 4;
    if (o->view == 3 && o->proj != 2) return NVSR_ERR_SHAPE;              // 'concat' view needs concatenated position features
    if (o->view <= 2 && (o->proj == 2 || o->Cv != o->C)) return NVSR_ERR_SHAPE;   // sum / avg / mult combine equal-sized vectors
    o->Kd = o->C * (o->proj == 2 ? np : 1);
    o->Kr = o->Cv + (concat_like ? np * o->C : 0);
    if (o->view <= 2) o->Kr = o->C;
    return NVSR_OK;
}

// in_features of decoder layer l (models.py:173-195)
static inline int gen_layer_in(const GenGeom& g, bool rgb, int l) {
    const int k0 = rgb ? g.Kr : g.Kd;
    if (l == 0) return k0;
    return g.hidden + (gen_skip_layer(l - 1, g.skip) ? k0 : 0);
}

// ---- what the two routes of the decoder-weight gradients share (generic.hip: layered; generic_fused_bwd.hip: on the fused launch's record) ----
constexpr long GEN_BWD_CHUNK = 1L << 17;   // points per pass of a backward that keeps every layer's output of the chunk
constexpr int GW_PTS = 2048;               // points per slab of generic_wgrad_kernel, a quarter of the slab per wave
// offsets of the layers in the natural blob (state-dict order: density layers, fc_alpha, rgb layers, fc_rgb; weight then bias):
// woff[dec][l] = layer l of decoder dec, woff[dec][layers of dec] = its head
static inline void gen_blob_offsets(const GenGeom& g, long (&woff)[2][65]) {
    long o = 0;
    for (int dec = 0; dec < 2; ++dec) {
        const int nl = dec ? g.nr : g.nd;
        for (int l = 0; l < nl; ++l) { woff[dec][l] = o; o += (long)g.hidden * gen_layer_in(g, dec, l) + g.hidden; }
        woff[dec][nl] = o;
        o += (long)(dec ? 3 : 1) * g.hidden + (dec ? 3 : 1);
    }
}
// generic.hip: one generic_wgrad_kernel launch over the n points of a chunk in slabs of GW_PTS (the kernel's own arguments); the launch's status
int gen_wgrad_launch(long n, int M, int K1, int K2, const float* dY, int ldd, int doff, const float* Hmask, const float* X1, const float* X2,
                     float* dW, float* db, hipStream_t stream);

// what the entry points check of a scene before a launch: planes present, texel offsets within 31 bits
static inline int gen_check_scene(const SceneDevN& sc, const GenGeom& g) {
    for (int d = 0; d <= g.np; ++d) {
        if (!sc.plane[d]) return NVSR_ERR_NULL;
        const int64_t cc = d < g.np ? g.C : g.Cv;
        if (sc.ph[d] < 1 || sc.pw[d] < 1 || (int64_t)sc.ph[d] * sc.pw[d] * cc >= (int64_t)1 << 31) return NVSR_ERR_SHAPE;
    }
    return NVSR_OK;
}
static inline int gen_check_ext(const nvsr_scene_ext* scene) {
    if (!scene) return NVSR_ERR_NULL;
    if (scene->num_position_planes < 1 || scene->num_position_planes > NVSR_MAX_POSITION_PLANES) return NVSR_ERR_SHAPE;
    return NVSR_OK;
}

struct GenTaps { int o[4]; float w[4]; };
__device__ __forceinline__ GenTaps gen_taps(int H, int W, int Cc, float gx, float gy, int align) {
    // grid_sample(padding_mode='border'): unnormalise, clip, floor; a clamped neighbour carries weight 0.  align_corners=True maps -1 / +1 to
    // the centres of the corner texels, (g + 1) (size - 1) / 2; False to their outer edges, (g + 1) size / 2 - 0.5 (the CPU kernel's
    // ComputeLocation: one product with the pre-divided scale, then the shift)
    const float mx = (float)(W - 1), my = (float)(H - 1);
    float x, y;
    if (align) { x = (gx + 1.0f) * (mx / 2.0f); y = (gy + 1.0f) * (my / 2.0f); }
    else { x = __fsub_rn(__fmul_rn(gx + 1.0f, (float)W / 2.0f), 0.5f); y = __fsub_rn(__fmul_rn(gy + 1.0f, (float)H / 2.0f), 0.5f); }
    x = fminf(mx, fmaxf(x, 0.0f));
    y = fminf(my, fmaxf(y, 0.0f));
    const float xw = floorf(x), yn = floorf(y);
    const float w = x - xw, e = 1.0f - w, n = y - yn, s = 1.0f - n;
    const int ix = (int)xw, iy = (int)yn, ix1 = min(ix + 1, W - 1), iy1 = min(iy + 1, H - 1);
    GenTaps t;
    t.w[0] = s * e; t.w[1] = s * w; t.w[2] = n * e; t.w[3] = n * w;
    t.o[0] = (iy * W + ix) * Cc; t.o[1] = (iy * W + ix1) * Cc; t.o[2] = (iy1 * W + ix) * Cc; t.o[3] = (iy1 * W + ix1) * Cc;
    return t;
}
__device__ __forceinline__ float gen_blend(const float* __restrict__ plane, const GenTaps& t, int c) {
    return fmaf(plane[t.o[3] + c], t.w[3], fmaf(plane[t.o[2] + c], t.w[2], fmaf(plane[t.o[1] + c], t.w[1], plane[t.o[0] + c] * t.w[0])));
}

// grid_sample(mode='bicubic', padding_mode='border') (ATen GridSampler.h / GridSamplerKernel.cpp): the coordinate is unnormalised but NOT
// clipped; the 4 x 4 neighbourhood starts at floor - 1 and every TAP's index is clipped to the plane (border padding); the weights are the cubic
// convolution kernel with A = -0.75 (UpSample.h: get_cubic_upsample_coefficients), rows first: out = sum_i cy[i] (sum_j cx[j] v[i][j]).
struct CubicTaps { int ix[4], iy[4]; float cx[4], cy[4]; };
__device__ __forceinline__ void cubic_coefficients(float t, float (&c)[4]) {
    const float A = -0.75f;
    const float x0 = t + 1.0f, x1 = t, x2 = 1.0f - t, x3 = x2 + 1.0f;
    c[0] = ((A * x0 - 5.0f * A) * x0 + 8.0f * A) * x0 - 4.0f * A;
    c[1] = ((A + 2.0f) * x1 - (A + 3.0f)) * x1 * x1 + 1.0f;
    c[2] = ((A + 2.0f) * x2 - (A + 3.0f)) * x2 * x2 + 1.0f;
    c[3] = ((A * x3 - 5.0f * A) * x3 + 8.0f * A) * x3 - 4.0f * A;
}
__device__ __forceinline__ CubicTaps gen_cubic_taps(int H, int W, float gx, float gy, int align) {
    float x, y;
    if (align) { x = (gx + 1.0f) * ((float)(W - 1) / 2.0f); y = (gy + 1.0f) * ((float)(H - 1) / 2.0f); }
    else { x = __fsub_rn(__fmul_rn(gx + 1.0f, (float)W / 2.0f), 0.5f); y = __fsub_rn(__fmul_rn(gy + 1.0f, (float)H / 2.0f), 0.5f); }
    const float fx = floorf(x), fy = floorf(y);
    CubicTaps t;
    cubic_coefficients(x - fx, t.cx);
    cubic_coefficients(y - fy, t.cy);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        // (clip_coordinates on the float index, then the integer cast: the same texel as clamping the integer; NaN coordinates clamp to 0)
        const float xi = fminf((float)(W - 1), fmaxf(fx - 1.0f + (float)k, 0.0f)), yi = fminf((float)(H - 1), fmaxf(fy - 1.0f + (float)k, 0.0f));
        t.ix[k] = (int)xi; t.iy[k] = (int)yi;
    }
    return t;
}
__device__ __forceinline__ float gen_cubic_blend(const float* __restrict__ plane, int W, int Cc, const CubicTaps& t, int c) {
    float out = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float* row = plane + (long)t.iy[i] * W * Cc + c;
        const float r = row[t.ix[0] * Cc] * t.cx[0] + row[t.ix[1] * Cc] * t.cx[1] + row[t.ix[2] * Cc] * t.cx[2] + row[t.ix[3] * Cc] * t.cx[3];
        out += r * t.cy[i];
    }
    return out;
}
// one feature of one plane in either interpolation
__device__ __forceinline__ float gen_sample(const SceneDevN& sc, int d, int Cc, float gx, float gy, int c) {
    if (sc.bicubic) return gen_cubic_blend(sc.plane[d], sc.pw[d], Cc, gen_cubic_taps(sc.ph[d], sc.pw[d], gx, gy, sc.align), c);
    return gen_blend(sc.plane[d], gen_taps(sc.ph[d], sc.pw[d], Cc, gx, gy, sc.align), c);
}

// normalised sample position (models.py:261-268) + the optional jitter the reference adds to it in training (:291-293)
__device__ __forceinline__ void gen_position(const SceneDevN& sc, const float* q, const float* noise, long p, float& n0, float& n1, float& n2) {
    n0 = norm_coord(q[0], sc.lo[0], sc.range[0]); n1 = norm_coord(q[1], sc.lo[1], sc.range[1]); n2 = norm_coord(q[2], sc.lo[2], sc.range[2]);
    if (noise) { n0 = __fadd_rn(n0, noise[3 * p]); n1 = __fadd_rn(n1, noise[3 * p + 1]); n2 = __fadd_rn(n2, noise[3 * p + 2]); }
}
// grid coordinate of position plane d: the normalised position through the plane's 3x2 projection
__device__ __forceinline__ void gen_pos_grid(const SceneDevN& sc, int d, float n0, float n1, float n2, float& gx, float& gy) {
    const float* M = sc.proj + 6 * d;
    gx = n0 * M[0] + n1 * M[2] + n2 * M[4]; gy = n0 * M[1] + n1 * M[3] + n2 * M[5];
}
// grid coordinate of the view-direction plane: azimuth and elevation of q[3:6] (cart2az_el nerf_helpers.py:492-496), normalised
__device__ __forceinline__ void gen_view_grid(const SceneDevN& sc, const float* q, float& gx, float& gy) {
    const float az = atan2f(q[4], q[3]);
    const float el = atan2f(q[5], sqrtf(__fadd_rn(__fmul_rn(q[3], q[3]), __fmul_rn(q[4], q[4]))));
    gx = norm_coord(az, sc.lo[3], sc.range[3]); gy = norm_coord(el, sc.lo[4], sc.range[4]);
}
// combine_pos_planes for 'sum' / 'avg': s = the planes' features added plane by plane (stack(...).sum(0) / .mean(0))
__device__ __forceinline__ float gen_combine_pos(int proj, float s, int np) { return proj == 1 ? __fdiv_rn(s, (float)np) : s; }
// combine_all_planes for 'sum' / 'avg' / 'mult': pp = the combined position feature, vv = the view-direction feature
__device__ __forceinline__ float gen_combine_view(int view, float pp, float vv) {
    return view == 0 ? __fadd_rn(pp, vv) : view == 1 ? __fdiv_rn(__fadd_rn(pp, vv), 2.0f) : __fmul_rn(pp, __fadd_rn(1.0f, vv));
}

}  // namespace nvsr
