// The stem of the ResNet backbone (core/models/resnet.py:191-195) behind its convolution, in one pass over dense NCHW float32
// planes: a frozen norm, the ReLU and nn.MaxPool2d(3, 2, 1).
//
//   z            = relu(fl(fl(x * scale[c]) + shift[c]))             halo_affine_relu_fwd's statements (an_affine, an_relu); never stored
//   out[oh,ow]   = max of z over rows 2oh-1 .. 2oh+1, columns 2ow-1 .. 2ow+1, the taps inside the map only;
//                  OH = (H - 1) / 2 + 1, OW = (W - 1) / 2 + 1
//   scan         row-major from -inf, a tap is taken if (v > max || isnan(v)): among equal values the first wins, a NaN always
//                  wins and the last NaN of the window is the recorded tap (ATen's rule); out has the recorded tap's bits
//   tap[oh,ow]   = 3 kh + kw of the recorded tap (its place in the window, 0..8), or MP_BLOCKED (9) when its z <= 0: one byte
//
//   S[h,w]       = float32 sum of g[oh,ow] over the windows whose tap code names (h, w), ascending oh, then ascending ow, from +0
//   g_x[h,w]     = fl(S * scale[c])
//
// A blocked window names no pixel, so a pixel whose z <= 0 gets S = +0 (threshold_backward's zero; a NaN z is not blocked and lets
// the gradient through), and the backward needs neither z nor out.  A pixel lies in one window per even coordinate and in two per
// odd one: 1, 2 or 4 windows.  The backward is a gather that writes every g_x element once: no atomics, the same bits on every call.
//
// Tile walk, both ways: a lane owns a column group -- GW = 4 input columns (two outputs; 16-byte accesses of x and g_x, W % 4 == 0
// and aligned operands) or, on the one-element route, one output column (forward) / one input column (backward) -- and a strip of
// MP_R output rows (forward) or MP_R input row pairs (backward).  It issues the loads of all its rows before the first use
// (2 MP_R + 1 input rows forward: an input row feeds at most two output rows and only a strip's first row is read by two
// strips; MP_R + 1 rows of g and tap backward) and keeps them in registers: no LDS.  The (strip, column group) items of a plane are
// numbered row-major and dealt to workgroups of MP_TPB lanes in order, so a wave's lanes read consecutive groups of a row.  The
// grid is planes x chunks in one dimension; plane offsets are 64-bit, offsets inside a plane 32-bit.
#include "halo_common.hpp"
#include "halo_norm_dev.hpp"

namespace halo {

constexpr int MP_TPB = 256;
constexpr int MP_R = 4;                        // output rows per lane forward, input row pairs per lane backward
constexpr int MP_BLOCKED = 9;                  // tap code of a window whose recorded tap has z <= 0

struct MpGeom {
    int C, H, W, OH, OW;
    int ncg;      // column groups per row
    int items;    // (strip, column group) items per plane
    int cpp;      // chunks (workgroups) per plane
};

// one step of the window scan
__device__ __forceinline__ void mp_scan(float v, int code, float &m, int &t)
{
    const bool take = v > m || v != v;
    m = take ? v : m;
    t = take ? code : t;
}

// GW = 4: x of input columns 4j-1 .. 4j+3 of one row into v[0..4]; GW = 1: of columns 2ow-1 .. 2ow+1 into v[0..2].  A row or a
// column outside the map is read at the nearest place inside it (no branch in front of a load) and dropped by mp_rectify_row.
template <int GW>
__device__ __forceinline__ void mp_load_row(const float *__restrict__ xp, int row, int cg, const MpGeom &G, float *v)
{
    const float *rp = xp + min(max(row, 0), G.H - 1) * G.W;
    if constexpr (GW == 4) {
        v[0] = rp[max(cg * 4 - 1, 0)];
        an_load<4>(rp + cg * 4, v + 1);
    } else {
        const int c0 = 2 * cg;
        v[0] = rp[max(c0 - 1, 0)];
        v[1] = rp[c0];
        v[2] = rp[min(c0 + 1, G.W - 1)];
    }
}

// x -> z in place; a tap outside the map becomes -inf, which the scan never takes (z is never below +0)
template <int GW>
__device__ __forceinline__ void mp_rectify_row(float *v, int row, int cg, const MpGeom &G, float sc, float sh)
{
    constexpr int NV = GW == 4 ? 5 : 3;
    const bool row_in = row >= 0 && row < G.H;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const bool in = row_in && (k == 0 ? cg > 0 : GW == 4 || k < 2 || 2 * cg + 1 < G.W);
        v[k] = in ? an_relu(an_affine(v[k], sc, sh)) : -INFINITY;
    }
}

template <int GW, bool TAP>
__global__ void __launch_bounds__(MP_TPB) k_affine_relu_maxpool_fwd(const float *__restrict__ x, const float *__restrict__ scale,
                                                                    const float *__restrict__ shift, float *__restrict__ out,
                                                                    uint8_t *__restrict__ tap, MpGeom G)
{
    constexpr int NO = GW == 4 ? 2 : 1, NV = 2 * NO + 1, NR = 2 * MP_R + 1;
    const unsigned plane = blockIdx.x / (unsigned)G.cpp;         // 32-bit: the grid has at most 2^31 - 1 workgroups
    const int chunk = (int)(blockIdx.x - plane * (unsigned)G.cpp), c = (int)(plane % (unsigned)G.C);
    const int item = chunk * MP_TPB + (int)threadIdx.x;
    if (item >= G.items) return;
    const int strip = item / G.ncg, cg = item - strip * G.ncg;
    const float sc = scale[c], sh = shift[c];
    const float *xp = x + (size_t)plane * G.H * G.W;
    const int oh0 = strip * MP_R, r0 = 2 * oh0 - 1;

    float v[NR][NV];
#pragma unroll
    for (int i = 0; i < NR; ++i) mp_load_row<GW>(xp, r0 + i, cg, G, v[i]);
#pragma unroll
    for (int i = 0; i < NR; ++i) mp_rectify_row<GW>(v[i], r0 + i, cg, G, sc, sh);

    const size_t oo = (size_t)plane * G.OH * G.OW;
#pragma unroll
    for (int q = 0; q < MP_R; ++q) {
        const int oh = oh0 + q;
        if (oh >= G.OH) break;
        float m[NO];
        int t[NO];
#pragma unroll
        for (int o = 0; o < NO; ++o) {
            m[o] = -INFINITY, t[o] = 0;
#pragma unroll
            for (int kh = 0; kh < 3; ++kh)
#pragma unroll
                for (int kw = 0; kw < 3; ++kw) mp_scan(v[2 * q + kh][2 * o + kw], kh * 3 + kw, m[o], t[o]);
            t[o] = m[o] <= 0.0f ? MP_BLOCKED : t[o];
        }
        const size_t at = oo + (size_t)(oh * G.OW + cg * NO);
        if constexpr (GW == 4) {
            *reinterpret_cast<float2 *>(out + at) = make_float2(m[0], m[1]);
            if constexpr (TAP) *reinterpret_cast<uint16_t *>(tap + at) = (uint16_t)(t[0] | (t[1] << 8));
        } else {
            out[at] = m[0];
            if constexpr (TAP) tap[at] = (uint8_t)t[0];
        }
    }
}

// the windows' rows of g and tap that one lane reads: NW output columns from column ow0 on; a column or a row outside the map reads
// as a blocked window, which matches no pixel
template <int NW>
__device__ __forceinline__ void mp_load_windows(const float *__restrict__ gp, const uint8_t *__restrict__ tp, int oh, int ow0, const MpGeom &G,
                                                float *gv, int *tv)
{
#pragma unroll
    for (int k = 0; k < NW; ++k) {
        const bool in = oh < G.OH && ow0 + k < G.OW;
        const int at = in ? oh * G.OW + ow0 + k : 0;
        const float gk = gp[at];
        const int tk = tp[at];
        gv[k] = gk;
        tv[k] = in ? tk : MP_BLOCKED;
    }
}

// S of one input pixel continued over one row of windows: the window column (g0, t0) that holds the pixel at place (kh, 1) for an
// even input column and at (kh, 2) for an odd one, then, for an odd input column, the next window column (g1, t1) with the pixel
// at (kh, 0).  A window that does not name the pixel adds +0, which leaves S as it is (S is never -0).
__device__ __forceinline__ float mp_gather(float s, float g0, int t0, float g1, int t1, bool odd, int kh)
{
    s = s + (t0 == kh * 3 + (odd ? 2 : 1) ? g0 : 0.0f);
    s = s + (odd && t1 == kh * 3 ? g1 : 0.0f);
    return s;
}

template <int GW>
__global__ void __launch_bounds__(MP_TPB) k_affine_relu_maxpool_bwd(const float *__restrict__ g, const uint8_t *__restrict__ tap,
                                                                    const float *__restrict__ scale, float *__restrict__ gx, MpGeom G)
{
    constexpr int NW = GW == 4 ? 3 : 2;        // window columns a lane's GW input columns lie in
    const unsigned plane = blockIdx.x / (unsigned)G.cpp;         // 32-bit: the grid has at most 2^31 - 1 workgroups
    const int chunk = (int)(blockIdx.x - plane * (unsigned)G.cpp), c = (int)(plane % (unsigned)G.C);
    const int item = chunk * MP_TPB + (int)threadIdx.x;
    if (item >= G.items) return;
    const int strip = item / G.ncg, cg = item - strip * G.ncg;
    const float sc = scale[c];
    const float *gp = g + (size_t)plane * G.OH * G.OW;
    const uint8_t *tp = tap + (size_t)plane * G.OH * G.OW;
    float *xp = gx + (size_t)plane * G.H * G.W;
    const int w0 = cg * GW, ow0 = w0 >> 1, p0 = strip * MP_R;     // p0: the strip's first row pair = its first row of windows

    float gv[MP_R + 1][NW];
    int tv[MP_R + 1][NW];
#pragma unroll
    for (int i = 0; i <= MP_R; ++i) mp_load_windows<NW>(gp, tp, p0 + i, ow0, G, gv[i], tv[i]);

#pragma unroll
    for (int i = 0; i < MP_R; ++i) {
        const int h = 2 * (p0 + i);
        if (h >= G.H) break;
        float even[GW], odd[GW];
#pragma unroll
        for (int e = 0; e < GW; ++e) {
            // GW = 4: w0 is a multiple of four, input column w0 + e lies in window column e / 2 (and e / 2 + 1 when e is odd);
            // GW = 1: in window column 0 (and 1 when w0 is odd).  Compile-time indices keep gv and tv in registers.
            const int k = GW == 4 ? e >> 1 : 0;
            const bool wodd = GW == 4 ? (e & 1) != 0 : (w0 & 1) != 0;
            const float s1 = mp_gather(0.0f, gv[i][k], tv[i][k], gv[i][k + 1], tv[i][k + 1], wodd, 1);          // row 2p: the middle row of windows p
            float s2 = mp_gather(0.0f, gv[i][k], tv[i][k], gv[i][k + 1], tv[i][k + 1], wodd, 2);                // row 2p + 1: the last row of windows p,
            s2 = mp_gather(s2, gv[i + 1][k], tv[i + 1][k], gv[i + 1][k + 1], tv[i + 1][k + 1], wodd, 0);        // then the first row of windows p + 1
            even[e] = s1 * sc;
            odd[e] = s2 * sc;
        }
        an_store<GW>(xp + h * G.W + w0, even);
        if (h + 1 < G.H) an_store<GW>(xp + (h + 1) * G.W + w0, odd);
    }
}

static int mp_plan(const char *who, int64_t B, int64_t C, int64_t H, int64_t W, MpGeom &G)
{
    if (B < 1 || C < 1 || H < 1 || W < 1) return fail(HALO_E_ARG, "%s: empty shape", who);
    if (H > 0x7fffffffLL || W > 0x7fffffffLL || H * W > 0x7fffffffLL - 1025 || C > 0x7fffffffLL || B > 0x7fffffffLL || B * C > ((int64_t)1 << 40))
        return fail(HALO_E_UNSUPPORTED, "%s: %lld x %lld planes of %lld x %lld", who, (long long)B, (long long)C, (long long)H, (long long)W);
    G.C = (int)C, G.H = (int)H, G.W = (int)W, G.OH = (int)((H - 1) / 2 + 1), G.OW = (int)((W - 1) / 2 + 1);
    return HALO_OK;
}

// strips x column groups of a plane dealt to workgroups
static int mp_grid(const char *who, int64_t B, int64_t C, int64_t strips, int64_t ncg, MpGeom &G, unsigned &grid)
{
    const int64_t items = strips * ncg;                            // at most (H / 2 + 1) * W
    if (items > 0x7fffffffLL - MP_TPB) return fail(HALO_E_UNSUPPORTED, "%s: %lld items per plane", who, (long long)items);
    G.ncg = (int)ncg, G.items = (int)items, G.cpp = (int)cdiv(items, MP_TPB);
    const int64_t blocks = B * C * G.cpp;
    if (blocks > 0x7fffffffLL) return fail(HALO_E_UNSUPPORTED, "%s: %lld blocks", who, (long long)blocks);
    grid = (unsigned)blocks;
    return HALO_OK;
}

}  // namespace halo

using namespace halo;

extern "C" int halo_maxpool_affine_relu_fwd(const float *x, const float *scale, const float *shift, float *out, uint8_t *tap, int64_t B,
                                            int64_t C, int64_t H, int64_t W, void *stream)
{
    const char *who = "halo_maxpool_affine_relu_fwd";
    if (!x || !scale || !shift || !out) return fail(HALO_E_ARG, "%s: null argument", who);
    MpGeom G;
    unsigned grid;
    if (int rc = mp_plan(who, B, C, H, W, G)) return rc;
    // 16-byte loads of x, 8-byte stores of out, 2-byte stores of tap: W % 4 == 0 makes OW even and every plane start as aligned as the base
    const bool vec = W % 4 == 0 && (uintptr_t)x % 16 == 0 && (uintptr_t)out % 8 == 0 && (uintptr_t)tap % 2 == 0;
    if (int rc = mp_grid(who, B, C, cdiv(G.OH, MP_R), vec ? W / 4 : G.OW, G, grid)) return rc;
    const dim3 gd(grid), b(MP_TPB);
    hipStream_t st = (hipStream_t)stream;
    if (vec && tap) hipLaunchKernelGGL((k_affine_relu_maxpool_fwd<4, true>), gd, b, 0, st, x, scale, shift, out, tap, G);
    else if (vec) hipLaunchKernelGGL((k_affine_relu_maxpool_fwd<4, false>), gd, b, 0, st, x, scale, shift, out, tap, G);
    else if (tap) hipLaunchKernelGGL((k_affine_relu_maxpool_fwd<1, true>), gd, b, 0, st, x, scale, shift, out, tap, G);
    else hipLaunchKernelGGL((k_affine_relu_maxpool_fwd<1, false>), gd, b, 0, st, x, scale, shift, out, tap, G);
    return check_launch(who);
}

extern "C" int halo_maxpool_affine_relu_bwd(const float *g, const uint8_t *tap, const float *scale, float *g_x, int64_t B, int64_t C, int64_t H,
                                            int64_t W, void *stream)
{
    const char *who = "halo_maxpool_affine_relu_bwd";
    if (!g || !tap || !scale || !g_x) return fail(HALO_E_ARG, "%s: null argument", who);
    MpGeom G;
    unsigned grid;
    if (int rc = mp_plan(who, B, C, H, W, G)) return rc;
    const bool vec = W % 4 == 0 && (uintptr_t)g_x % 16 == 0;       // 16-byte stores of g_x; g and tap are read one element at a time
    if (int rc = mp_grid(who, B, C, cdiv(cdiv(H, 2), MP_R), vec ? W / 4 : W, G, grid)) return rc;
    const dim3 gd(grid), b(MP_TPB);
    if (vec) hipLaunchKernelGGL((k_affine_relu_maxpool_bwd<4>), gd, b, 0, (hipStream_t)stream, g, tap, scale, g_x, G);
    else hipLaunchKernelGGL((k_affine_relu_maxpool_bwd<1>), gd, b, 0, (hipStream_t)stream, g, tap, scale, g_x, G);
    return check_launch(who);
}
