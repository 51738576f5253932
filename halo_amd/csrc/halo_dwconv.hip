// The first half of a DepthwiseSeparableConv2d block with a frozen norm (core/models/classifier.py:78-81): depthwise 3 x 3
// convolution (groups = C, dilation d, padding d, stride 1, no bias), per-channel affine, ReLU -- one read and one write.
//
//   pre[b,c,i,j] = (sum_{ky,kx} w[c,ky,kx] x[b,c, i + (ky-1) d, j + (kx-1) d]) * scale[c] + shift[c],   y = max(pre, 0)
//   gp = g [y > 0] scale[c]                                   (float32, one rounding)
//   g_x[b,c,p] = sum_k w[c,k] gp[b,c,p - k d]                 (a gather with the mirrored taps: one thread writes an element once)
//   g_w[c,k]   = sum_{b,p} gp[b,c,p] x[b,c,p + k d]           (float64 products and sums, rounded to float32 once)
//
// Order of summation (every kernel, every route, whatever the tiling -- the bits depend on the operands and the shape alone):
//   the 9-term sums run over the INPUT positions in ascending row, then ascending column: (i-d, j-d), (i-d, j), (i-d, j+d),
//   (i, j-d), ... (i+d, j+d); the first product is rounded, every further term is one fma onto it; a tap outside the plane adds
//   w * 0.  (For the forward that is ky, kx ascending; for g_x it is ky, kx descending.)  * scale and + shift are two roundings.
//   g_w: a thread adds fma(gp, x, acc) in float64 over its rows in ascending order and, per row, its columns in ascending
//   order; a block adds its threads by a fixed shuffle tree and its four waves in ascending order; k_dw_wsum adds the per-block
//   rows of a channel in ascending (image, block) order.  No atomics anywhere.
//
// Tiling: no LDS.  A 3 x 3 tap set with dilation d touches rows i-d, i, i+d only, so the rows of a plane fall into d CHAINS
// (r, r+d, r+2d, ...) that never read each other's rows.  A thread owns GW adjacent columns (4: 16-byte loads; 1: any W and any
// alignment) of a chain segment of up to DW_L output rows and walks it top to bottom with a three-row window in registers:
// every input row is loaded once per segment (three loads: the columns at -d, 0, +d; one load and two scalars for d = 1) and
// serves three output rows.  Consecutive lanes take consecutive column groups, then the next chain, i.e. the next row: the loads
// and stores of a wave are contiguous.  An 80 x 160 plane at d = 6 / 12 / 18 is 240 / 480 / 720 threads with no halo row at
// all; a 160 x 320 plane at d = 1 is 10 bands of 16 rows with a one-row halo either side.  A block works inside one plane, so
// w, scale and shift are block-uniform.
//
// The decoder front (halo_upcat_*): the conv's input is cat([bilinear_align_corners(a, (H, W)), s], 1), d = 1, and neither the
// resized nor the concatenated tensor exists.  A block works inside one plane, so which operand it reads is block-uniform: a
// plane below Ca reads its window through DwUpSrc (the resize's own taps and bilerp, evaluated per window row), the others read
// s through DwSrc.  Same DwGeom for C = Ca + Cs, same walk, same k_dw_wsum: the bits are those of the conv over the stored
// concatenation.  The data gradient is written to two dense tensors split at plane Ca.
//
// The ASPP pyramid (halo_multi_dwconv3x3_*): N dilations over one input.  The one place with LDS: a workgroup keeps a plane there
// and runs the same walk once per dilation (the section in front of the entry points).
#include <type_traits>

#include "halo_common.hpp"
#include "halo_devmath.hpp"
#include "halo_half_dev.hpp"
#include "halo_softmax.hpp"

namespace halo {

constexpr int DW_TPB = 256;
constexpr int DW_L = 16;                 // output rows of one chain segment
constexpr int64_t DW_MAX_DIM = 1 << 24;  // H, W, d
enum { DW_FWD = 0, DW_BWD = 1 };

typedef float dw_f4 __attribute__((ext_vector_type(4)));
typedef float dw_f4u __attribute__((ext_vector_type(4), aligned(4)));

struct DwGeom {
    int H, W, d, C;
    int ngroups;      // column groups of GW columns per row
    int nres;         // chains: min(d, H)
    int bpp;          // blocks per plane
    long long items;  // threads with work per plane: segments x chains x column groups
};

static DwGeom dw_geom(int64_t C, int64_t H, int64_t W, int64_t d, int gw)
{
    DwGeom G;
    G.H = (int)H, G.W = (int)W, G.d = (int)d, G.C = (int)C;
    G.ngroups = (int)(W / gw);
    G.nres = (int)(d < H ? d : H);
    const int64_t nseg = cdiv(cdiv(H, d), DW_L);
    G.items = (long long)nseg * G.nres * G.ngroups;
    G.bpp = (int)cdiv(G.items, DW_TPB);
    return G;
}

// the operand a window is read from: x itself, or gp = g [y > 0] scale
template <int MODE> struct DwSrc {
    const float *a, *y;
    float scale;
    __device__ __forceinline__ float at(size_t o) const
    {
        if constexpr (MODE == DW_FWD) return a[o];
        else return (y[o] > 0.0f ? a[o] : 0.0f) * scale;
    }
    template <typename V> __device__ __forceinline__ void at4(size_t o, float *out) const
    {
        const V va = *reinterpret_cast<const V *>(a + o);
        if constexpr (MODE == DW_FWD) {
            out[0] = va.x, out[1] = va.y, out[2] = va.z, out[3] = va.w;
        } else {
            const V vy = *reinterpret_cast<const V *>(y + o);
            out[0] = (vy.x > 0.0f ? va.x : 0.0f) * scale, out[1] = (vy.y > 0.0f ? va.y : 0.0f) * scale;
            out[2] = (vy.z > 0.0f ? va.z : 0.0f) * scale, out[3] = (vy.w > 0.0f ? va.w : 0.0f) * scale;
        }
    }
    // the GW columns at c0 of row i (zeros outside the plane); ALIGNED: c0 is a multiple of 4 (16-byte loads)
    template <int GW, bool ALIGNED> __device__ __forceinline__ void cols(float *out, int i, int c0, int H, int W) const
    {
        const bool row_in = i >= 0 && i < H;
        const size_t o = (size_t)(row_in ? i : 0) * W;
        if constexpr (GW == 4) {
            if (row_in && c0 >= 0 && c0 + 4 <= W) {
                if constexpr (ALIGNED) at4<dw_f4>(o + c0, out);
                else at4<dw_f4u>(o + c0, out);
                return;
            }
        }
#pragma unroll
        for (int e = 0; e < GW; ++e) out[e] = row_in && c0 + e >= 0 && c0 + e < W ? at(o + (c0 + e)) : 0.0f;
    }
    // win[kx * GW + e] = the operand at (i, c0 + (kx - 1) d + e)
    template <int GW, bool D1> __device__ __forceinline__ void row(float *win, int i, int c0, int H, int W, int d) const
    {
        if constexpr (D1 && GW == 4) {
            cols<4, true>(win + 4, i, c0, H, W);
            const bool row_in = i >= 0 && i < H;
            const size_t o = (size_t)(row_in ? i : 0) * W;
            win[0] = row_in && c0 > 0 ? at(o + (c0 - 1)) : 0.0f;
            win[1] = win[4], win[2] = win[5], win[3] = win[6];
            win[8] = win[5], win[9] = win[6], win[10] = win[7];
            win[11] = row_in && c0 + 4 < W ? at(o + (c0 + 4)) : 0.0f;
        } else {
            cols<GW, false>(win, i, c0 - d, H, W);
            cols<GW, true>(win + GW, i, c0, H, W);
            cols<GW, false>(win + 2 * GW, i, c0 + d, H, W);
        }
    }
};

// The operand of a plane below Ca of the decoder front: element (i, j) is the align_corners=True resize of the (h, w) plane `a`
// to (H, W) -- bilerp over make_taps<float>(i, sh, h) / make_taps<float>(j, sw, w), halo_bilinear_upsample's expression, so its
// bits -- and zero outside the plane.  d = 1 only.  bilerp interpolates along the columns first, and that half does not depend on
// the output row: the thread keeps the column-interpolated values of the two source rows its last window row used (lo, hi), and
// a row entering the window loads a source row only when its taps leave that pair -- at most one new row per output row when
// walking down an upsampling.  A thread's GW + 2 columns (its own and the two neighbours) do not change down its segment: their
// taps are computed once, a row's taps once per row entering the window.  Whether a source row is loaded is decided for the
// whole wave (a load under a lane condition serialises); the loads themselves are unconditional from clamped addresses, and
// the zero of the padding is selected afterwards.
template <int GW> struct DwUpSrc {
    const float *a;
    int h, w;
    float sh;
    int x0[GW + 2], x1[GW + 2];
    float lx0[GW + 2], lx1[GW + 2];
    bool left_in, right_in;
    int rl, rh;                      // the source rows held in lo and hi (-1: none yet)
    float lo[GW + 2], hi[GW + 2];
    __device__ __forceinline__ void init(const float *plane, int h_, int w_, float sh_, float sw, int c0, int W)
    {
        a = plane, h = h_, w = w_, sh = sh_;
        left_in = c0 > 0, right_in = c0 + GW < W;
        rl = rh = -1;
#pragma unroll
        for (int q = 0; q < GW + 2; ++q) {
            int X = c0 - 1 + q;
            X = X < 0 ? 0 : (X > W - 1 ? W - 1 : X);
            const Taps<float> t = make_taps<float>(X, sw, w);
            x0[q] = t.i0, x1[q] = t.i1, lx0[q] = t.l0, lx1[q] = t.l1;
            lo[q] = hi[q] = 0.0f;
        }
    }
    // bilerp's first half over source row r (0 <= r < h) at this thread's columns
    __device__ __forceinline__ void source_row(float *v, int r) const
    {
        const float *p = a + (size_t)r * w;
#pragma unroll
        for (int q = 0; q < GW + 2; ++q) v[q] = col_lerp(lx0[q], lx1[q], p[x0[q]], p[x1[q]]);
    }
    // win[kx * GW + e] = the operand at (i, c0 + (kx - 1) + e)
    template <int GWT, bool D1> __device__ __forceinline__ void row(float *win, int i, int c0, int H, int W, int d)
    {
        static_assert(GWT == GW, "one column group width per source");
        const bool row_in = i >= 0 && i < H;
        const Taps<float> ty = make_taps<float>(i < 0 ? 0 : (i > H - 1 ? H - 1 : i), sh, h);
        const bool have0 = ty.i0 == rl || ty.i0 == rh, have1 = ty.i1 == rl || ty.i1 == rh;
        float n0[GW + 2], n1[GW + 2];
#pragma unroll
        for (int q = 0; q < GW + 2; ++q) n0[q] = n1[q] = 0.0f;
        if (__any(!have1)) source_row(n1, ty.i1);
        if (__any(!have0 && ty.i0 != ty.i1)) source_row(n0, ty.i0);
#pragma unroll
        for (int q = 0; q < GW + 2; ++q) {
            const float v1 = ty.i1 == rl ? lo[q] : (ty.i1 == rh ? hi[q] : n1[q]);
            const float v0 = ty.i0 == rl ? lo[q] : (ty.i0 == rh ? hi[q] : (ty.i0 == ty.i1 ? n1[q] : n0[q]));
            lo[q] = v0, hi[q] = v1;
        }
        rl = ty.i0, rh = ty.i1;
        float v[GW + 2];
#pragma unroll
        for (int q = 0; q < GW + 2; ++q) {
            const float e = col_lerp(ty.l0, ty.l1, lo[q], hi[q]);          // bilerp's second half
            v[q] = row_in && (q > 0 || left_in) && (q < GW + 1 || right_in) ? e : 0.0f;
        }
#pragma unroll
        for (int kx = 0; kx < 3; ++kx)
#pragma unroll
            for (int e = 0; e < GW; ++e) win[kx * GW + e] = v[kx + e];
    }
};

// the operands of the decoder front: a (B, Ca, h, w) resized to (H, W) with the scales sh, sw in front of s (B, Cs, H, W)
struct DwCat {
    int Ca, Cs, h, w;
    float sh, sw;
    int c_lo, c_n;    // bwd_data: the channels [c_lo, c_lo + c_n) whose gradient is wanted
};

// this thread's column group and chain segment: false when it has none
struct DwItem { int c0, i0, iend; };
template <int GW> __device__ __forceinline__ bool dw_item(const DwGeom &G, int blk, DwItem &it)
{
    const long long item = (long long)blk * DW_TPB + threadIdx.x;
    if (item >= G.items) return false;
    const int g = (int)(item % G.ngroups);
    const long long t = item / G.ngroups;
    const int r = (int)(t % G.nres);
    const long long k0 = (t / G.nres) * DW_L;
    const long long i0 = r + k0 * G.d, iend = i0 + (long long)DW_L * G.d;
    it.c0 = g * GW;
    it.i0 = (int)(i0 < G.H ? i0 : G.H);
    it.iend = (int)(iend < G.H ? iend : G.H);
    return true;
}

// One thread's walk down its segment.  MODE DW_FWD: src = x, op = y.  MODE DW_BWD: src = gp, wk mirrored, op = g_x.
template <int MODE, int GW, bool D1, typename SRC>
__device__ __forceinline__ void dw_walk_apply(SRC &src, const float (&wk)[9], float sc, float sh, float *__restrict__ op, const DwItem &it,
                                              const DwGeom &G)
{
    const int d = D1 ? 1 : G.d;
    float win[3][3 * GW];
    src.template row<GW, D1>(win[0], it.i0 - d, it.c0, G.H, G.W, d);
    src.template row<GW, D1>(win[1], it.i0, it.c0, G.H, G.W, d);
    for (int i = it.i0; i < it.iend; i += d) {
        src.template row<GW, D1>(win[2], i + d, it.c0, G.H, G.W, d);
        float res[GW];
#pragma unroll
        for (int e = 0; e < GW; ++e) {
            float acc = wk[0] * win[0][e];
#pragma unroll
            for (int k = 1; k < 9; ++k) acc = __builtin_fmaf(wk[k], win[k / 3][(k % 3) * GW + e], acc);
            if constexpr (MODE == DW_FWD) {
                float pre = acc * sc;
                pre = pre + sh;
                acc = pre <= 0.0f ? 0.0f : pre;          // a NaN stays a NaN, as torch's ReLU leaves it
            }
            res[e] = acc;
        }
        if constexpr (GW == 4) {
            dw_f4 v;
            v.x = res[0], v.y = res[1], v.z = res[2], v.w = res[3];
            *reinterpret_cast<dw_f4 *>(op + (size_t)i * G.W + it.c0) = v;
        } else {
            op[(size_t)i * G.W + it.c0] = res[0];
        }
#pragma unroll
        for (int q = 0; q < 3 * GW; ++q) win[0][q] = win[1][q], win[1][q] = win[2][q];
    }
}

// MODE DW_FWD: a = x, out = y.  MODE DW_BWD: a = g, yv = y, out = g_x.
template <int MODE, int GW, bool D1>
__global__ void __launch_bounds__(DW_TPB) k_dw_apply(const float *__restrict__ a, const float *__restrict__ yv, const float *__restrict__ w,
                                                     const float *__restrict__ scale, const float *__restrict__ shift, float *__restrict__ out, DwGeom G)
{
    const long long plane = blockIdx.x / G.bpp;
    const int blk = (int)(blockIdx.x - plane * G.bpp), c = (int)(plane % G.C);
    DwItem it;
    if (!dw_item<GW>(G, blk, it)) return;
    const size_t po = (size_t)plane * G.H * G.W;
    const float sc = scale[c];
    DwSrc<MODE> src;
    src.a = a + po, src.y = MODE == DW_BWD ? yv + po : nullptr, src.scale = sc;
    float wk[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) wk[k] = MODE == DW_FWD ? w[c * 9 + k] : w[c * 9 + 8 - k];
    const float sh = MODE == DW_FWD ? shift[c] : 0.0f;
    dw_walk_apply<MODE, GW, D1>(src, wk, sc, sh, out + po, it, G);
}

// The decoder front, forward: plane (b, c) of y from a's plane (b, c) resized in place (c < Ca) or from s's plane (b, c - Ca).
template <int GW>
__global__ void __launch_bounds__(DW_TPB) k_dw_upcat_fwd(const float *__restrict__ a, const float *__restrict__ s, const float *__restrict__ w,
                                                         const float *__restrict__ scale, const float *__restrict__ shift, float *__restrict__ y,
                                                         DwGeom G, DwCat K)
{
    const long long plane = blockIdx.x / G.bpp;
    const int blk = (int)(blockIdx.x - plane * G.bpp), c = (int)(plane % G.C);
    const long long b = plane / G.C;
    DwItem it;
    if (!dw_item<GW>(G, blk, it)) return;
    const size_t hw = (size_t)G.H * G.W;
    const float sc = scale[c], sh = shift[c];
    float wk[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) wk[k] = w[c * 9 + k];
    if (c < K.Ca) {
        DwUpSrc<GW> src;
        src.init(a + (size_t)(b * K.Ca + c) * K.h * K.w, K.h, K.w, K.sh, K.sw, it.c0, G.W);
        dw_walk_apply<DW_FWD, GW, GW == 4>(src, wk, sc, sh, y + (size_t)plane * hw, it, G);
    } else {
        DwSrc<DW_FWD> src;
        src.a = s + (size_t)(b * K.Cs + (c - K.Ca)) * hw, src.y = nullptr, src.scale = sc;
        dw_walk_apply<DW_FWD, GW, GW == 4>(src, wk, sc, sh, y + (size_t)plane * hw, it, G);
    }
}

// The decoder front, data gradient: the planes [c_lo, c_lo + c_n) of dw3x3^T(gp), those below Ca into g_up (B, Ca, H, W), the
// others into g_s (B, Cs, H, W).
template <int GW>
__global__ void __launch_bounds__(DW_TPB) k_dw_upcat_bwd(const float *__restrict__ g, const float *__restrict__ yv, const float *__restrict__ w,
                                                         const float *__restrict__ scale, float *__restrict__ g_up, float *__restrict__ g_s,
                                                         DwGeom G, DwCat K)
{
    const long long q = blockIdx.x / G.bpp;
    const int blk = (int)(blockIdx.x - q * G.bpp), c = K.c_lo + (int)(q % K.c_n);
    const long long b = q / K.c_n;
    DwItem it;
    if (!dw_item<GW>(G, blk, it)) return;
    const size_t hw = (size_t)G.H * G.W, po = (size_t)(b * G.C + c) * hw;
    const float sc = scale[c];
    DwSrc<DW_BWD> src;
    src.a = g + po, src.y = yv + po, src.scale = sc;
    float wk[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) wk[k] = w[c * 9 + 8 - k];
    float *op = c < K.Ca ? g_up + (size_t)(b * K.Ca + c) * hw : g_s + (size_t)(b * K.Cs + (c - K.Ca)) * hw;
    dw_walk_apply<DW_BWD, GW, GW == 4>(src, wk, sc, 0.0f, op, it, G);
}

// One thread's float64 sums of gp[p] x[p + k d] over its segment: rows ascending, per row columns ascending
template <int GW, bool D1, typename SX>
__device__ __forceinline__ void dw_walk_wpart(SX &sx, const DwSrc<DW_BWD> &sg, const DwItem &it, const DwGeom &G, double (&acc)[9])
{
    const int d = D1 ? 1 : G.d;
    float win[3][3 * GW];
    sx.template row<GW, D1>(win[0], it.i0 - d, it.c0, G.H, G.W, d);
    sx.template row<GW, D1>(win[1], it.i0, it.c0, G.H, G.W, d);
    for (int i = it.i0; i < it.iend; i += d) {
        sx.template row<GW, D1>(win[2], i + d, it.c0, G.H, G.W, d);
        float gp[GW];
        sg.template cols<GW, true>(gp, i, it.c0, G.H, G.W);
#pragma unroll
        for (int e = 0; e < GW; ++e) {
            const double ge = (double)gp[e];
#pragma unroll
            for (int k = 0; k < 9; ++k) acc[k] = __builtin_fma(ge, (double)win[k / 3][(k % 3) * GW + e], acc[k]);
        }
#pragma unroll
        for (int q = 0; q < 3 * GW; ++q) win[0][q] = win[1][q], win[1][q] = win[2][q];
    }
}

// part[blockIdx.x * 9 + k] = the block's sum: its threads by a fixed shuffle tree, its four waves in ascending order
__device__ __forceinline__ void dw_block_sum(const double (&acc)[9], double *__restrict__ part)
{
    __shared__ double s[DW_TPB / 64][9];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        double v = acc[k];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, 64);
        if (lane == 0) s[wave][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < 9) {
        double t = s[0][threadIdx.x];
        for (int q = 1; q < DW_TPB / 64; ++q) t += s[q][threadIdx.x];
        part[(size_t)blockIdx.x * 9 + threadIdx.x] = t;
    }
}

// part[(plane * bpp + blk) * 9 + k] = this block's float64 sum of gp[p] x[p + k d]
template <int GW, bool D1>
__global__ void __launch_bounds__(DW_TPB) k_dw_wpart(const float *__restrict__ g, const float *__restrict__ yv, const float *__restrict__ x,
                                                     const float *__restrict__ scale, double *__restrict__ part, DwGeom G)
{
    const long long plane = blockIdx.x / G.bpp;
    const int blk = (int)(blockIdx.x - plane * G.bpp), c = (int)(plane % G.C);
    const size_t po = (size_t)plane * G.H * G.W;
    double acc[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) acc[k] = 0.0;
    DwItem it;
    if (dw_item<GW>(G, blk, it)) {
        DwSrc<DW_FWD> sx;
        sx.a = x + po, sx.y = nullptr, sx.scale = 0.0f;
        DwSrc<DW_BWD> sg;
        sg.a = g + po, sg.y = yv + po, sg.scale = scale[c];
        dw_walk_wpart<GW, D1>(sx, sg, it, G, acc);
    }
    dw_block_sum(acc, part);
}

// The decoder front, weight gradient: the same rows of `part`, x recomputed from a (c < Ca) or read from s.
template <int GW>
__global__ void __launch_bounds__(DW_TPB) k_dw_upcat_wpart(const float *__restrict__ g, const float *__restrict__ yv, const float *__restrict__ a,
                                                           const float *__restrict__ s, const float *__restrict__ scale, double *__restrict__ part,
                                                           DwGeom G, DwCat K)
{
    const long long plane = blockIdx.x / G.bpp;
    const int blk = (int)(blockIdx.x - plane * G.bpp), c = (int)(plane % G.C);
    const long long b = plane / G.C;
    const size_t hw = (size_t)G.H * G.W, po = (size_t)plane * hw;
    double acc[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) acc[k] = 0.0;
    DwItem it;
    if (dw_item<GW>(G, blk, it)) {
        DwSrc<DW_BWD> sg;
        sg.a = g + po, sg.y = yv + po, sg.scale = scale[c];
        if (c < K.Ca) {
            DwUpSrc<GW> sx;
            sx.init(a + (size_t)(b * K.Ca + c) * K.h * K.w, K.h, K.w, K.sh, K.sw, it.c0, G.W);
            dw_walk_wpart<GW, GW == 4>(sx, sg, it, G, acc);
        } else {
            DwSrc<DW_FWD> sx;
            sx.a = s + (size_t)(b * K.Cs + (c - K.Ca)) * hw, sx.y = nullptr, sx.scale = 0.0f;
            dw_walk_wpart<GW, GW == 4>(sx, sg, it, G, acc);
        }
    }
    dw_block_sum(acc, part);
}

// Both gradients from one walk: dw_walk_apply<DW_BWD> and dw_walk_wpart visit the same items in the same order, the first with a
// window of gp, the second with a window of x and the centre group of gp's middle row.  A thread that keeps both windows runs the
// statements of both per output row, in their order: g_x's nine terms (wk mirrored), then the float64 fmas for e ascending and k
// ascending, then the store.  g, y and x are read once.  The parents' walks stay as they are (their registers are theirs).
template <int GW, bool D1, typename SX>
__device__ __forceinline__ void dw_walk_joint(SX &sx, const DwSrc<DW_BWD> &sg, const float (&wk)[9], float *__restrict__ op, const DwItem &it,
                                              const DwGeom &G, double (&acc)[9])
{
    const int d = D1 ? 1 : G.d;
    float xwin[3][3 * GW], gwin[3][3 * GW];
    sx.template row<GW, D1>(xwin[0], it.i0 - d, it.c0, G.H, G.W, d);
    sg.template row<GW, D1>(gwin[0], it.i0 - d, it.c0, G.H, G.W, d);
    sx.template row<GW, D1>(xwin[1], it.i0, it.c0, G.H, G.W, d);
    sg.template row<GW, D1>(gwin[1], it.i0, it.c0, G.H, G.W, d);
    for (int i = it.i0; i < it.iend; i += d) {
        sx.template row<GW, D1>(xwin[2], i + d, it.c0, G.H, G.W, d);
        sg.template row<GW, D1>(gwin[2], i + d, it.c0, G.H, G.W, d);
        float res[GW];
#pragma unroll
        for (int e = 0; e < GW; ++e) {
            float s = wk[0] * gwin[0][e];
#pragma unroll
            for (int k = 1; k < 9; ++k) s = __builtin_fmaf(wk[k], gwin[k / 3][(k % 3) * GW + e], s);
            res[e] = s;
        }
#pragma unroll
        for (int e = 0; e < GW; ++e) {
            const double ge = (double)gwin[1][GW + e];       // gp at (i, c0 + e): what dw_walk_wpart loads through cols<GW, true>
#pragma unroll
            for (int k = 0; k < 9; ++k) acc[k] = __builtin_fma(ge, (double)xwin[k / 3][(k % 3) * GW + e], acc[k]);
        }
        if constexpr (GW == 4) {
            dw_f4 v;
            v.x = res[0], v.y = res[1], v.z = res[2], v.w = res[3];
            *reinterpret_cast<dw_f4 *>(op + (size_t)i * G.W + it.c0) = v;
        } else {
            op[(size_t)i * G.W + it.c0] = res[0];
        }
#pragma unroll
        for (int q = 0; q < 3 * GW; ++q) xwin[0][q] = xwin[1][q], xwin[1][q] = xwin[2][q], gwin[0][q] = gwin[1][q], gwin[1][q] = gwin[2][q];
    }
}

// g_x = k_dw_apply<DW_BWD>'s, part = k_dw_wpart's rows.  Every thread reaches dw_block_sum: one without an item adds zeros.
template <int GW, bool D1>
__global__ void __launch_bounds__(DW_TPB) k_dw_joint(const float *__restrict__ g, const float *__restrict__ yv, const float *__restrict__ x,
                                                     const float *__restrict__ w, const float *__restrict__ scale, float *__restrict__ g_x,
                                                     double *__restrict__ part, DwGeom G)
{
    const long long plane = blockIdx.x / G.bpp;
    const int blk = (int)(blockIdx.x - plane * G.bpp), c = (int)(plane % G.C);
    const size_t po = (size_t)plane * G.H * G.W;
    double acc[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) acc[k] = 0.0;
    DwItem it;
    if (dw_item<GW>(G, blk, it)) {
        DwSrc<DW_FWD> sx;
        sx.a = x + po, sx.y = nullptr, sx.scale = 0.0f;
        DwSrc<DW_BWD> sg;
        sg.a = g + po, sg.y = yv + po, sg.scale = scale[c];
        float wk[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) wk[k] = w[c * 9 + 8 - k];
        dw_walk_joint<GW, D1>(sx, sg, wk, g_x + po, it, G, acc);
    }
    dw_block_sum(acc, part);
}

// The decoder front: k_dw_upcat_bwd over all Ca + Cs planes and k_dw_upcat_wpart in one walk.
template <int GW>
__global__ void __launch_bounds__(DW_TPB) k_dw_upcat_joint(const float *__restrict__ g, const float *__restrict__ yv, const float *__restrict__ a,
                                                           const float *__restrict__ s, const float *__restrict__ w,
                                                           const float *__restrict__ scale, float *__restrict__ g_up, float *__restrict__ g_s,
                                                           double *__restrict__ part, DwGeom G, DwCat K)
{
    const long long plane = blockIdx.x / G.bpp;
    const int blk = (int)(blockIdx.x - plane * G.bpp), c = (int)(plane % G.C);
    const long long b = plane / G.C;
    const size_t hw = (size_t)G.H * G.W, po = (size_t)plane * hw;
    double acc[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) acc[k] = 0.0;
    DwItem it;
    if (dw_item<GW>(G, blk, it)) {
        DwSrc<DW_BWD> sg;
        sg.a = g + po, sg.y = yv + po, sg.scale = scale[c];
        float wk[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) wk[k] = w[c * 9 + 8 - k];
        if (c < K.Ca) {
            DwUpSrc<GW> sx;
            sx.init(a + (size_t)(b * K.Ca + c) * K.h * K.w, K.h, K.w, K.sh, K.sw, it.c0, G.W);
            dw_walk_joint<GW, GW == 4>(sx, sg, wk, g_up + (size_t)(b * K.Ca + c) * hw, it, G, acc);
        } else {
            DwSrc<DW_FWD> sx;
            sx.a = s + (size_t)(b * K.Cs + (c - K.Ca)) * hw, sx.y = nullptr, sx.scale = 0.0f;
            dw_walk_joint<GW, GW == 4>(sx, sg, wk, g_s + (size_t)(b * K.Cs + (c - K.Ca)) * hw, it, G, acc);
        }
    }
    dw_block_sum(acc, part);
}

// g_w[c, k] = sum over images b, then blocks, in ascending order
__global__ void __launch_bounds__(DW_TPB) k_dw_wsum(const double *__restrict__ part, float *__restrict__ gw, int B, int C, int bpp)
{
    const int e = blockIdx.x * DW_TPB + threadIdx.x;
    if (e >= C * 9) return;
    const int c = e / 9, k = e - c * 9;
    double t = 0.0;
    for (int b = 0; b < B; ++b) {
        const double *row = part + ((size_t)b * C + c) * bpp * 9 + k;
        for (int q = 0; q < bpp; ++q) t += row[(size_t)q * 9];
    }
    gw[e] = (float)t;
}

static int dw_check(const char *who, int64_t B, int64_t C, int64_t H, int64_t W, int64_t d)
{
    if (B < 1 || C < 1 || H < 1 || W < 1 || d < 1) return fail(HALO_E_ARG, "%s: empty shape or dilation < 1", who);
    if (H > DW_MAX_DIM || W > DW_MAX_DIM || d > DW_MAX_DIM || H * W > 0x7fffffffLL || B * C > ((int64_t)1 << 40) || C > 0x7fffffffLL / 9 ||
        B > 0x7fffffffLL)
        return fail(HALO_E_UNSUPPORTED, "%s: %lld x %lld planes of %lld x %lld, dilation %lld", who, (long long)B, (long long)C, (long long)H,
                    (long long)W, (long long)d);
    return HALO_OK;
}

static bool dw_vec(int64_t W, const void *p0, const void *p1, const void *p2, const void *p3)
{
    return W % 4 == 0 && (((uintptr_t)p0 | (uintptr_t)p1 | (uintptr_t)p2 | (uintptr_t)p3) % 16) == 0;
}

static int dw_grid(const char *who, int64_t planes, const DwGeom &G, unsigned &grid)
{
    const int64_t n = planes * G.bpp;
    if (n > 0x7fffffffLL) return fail(HALO_E_UNSUPPORTED, "%s: %lld blocks", who, (long long)n);
    grid = (unsigned)n;
    return HALO_OK;
}

template <int MODE>
static void dw_launch_apply(bool vec, unsigned grid, hipStream_t st, const float *a, const float *yv, const float *w, const float *scale,
                            const float *shift, float *out, const DwGeom &G)
{
    const dim3 g(grid), b(DW_TPB);
    if (vec && G.d == 1) hipLaunchKernelGGL((k_dw_apply<MODE, 4, true>), g, b, 0, st, a, yv, w, scale, shift, out, G);
    else if (vec) hipLaunchKernelGGL((k_dw_apply<MODE, 4, false>), g, b, 0, st, a, yv, w, scale, shift, out, G);
    else hipLaunchKernelGGL((k_dw_apply<MODE, 1, false>), g, b, 0, st, a, yv, w, scale, shift, out, G);
}

// the decoder front's shapes: dw_check for C = Ca + Cs at d = 1, then the resize's own conditions
static int upcat_check(const char *who, int64_t B, int64_t Ca, int64_t Cs, int64_t h, int64_t w, int64_t H, int64_t W)
{
    if (Ca < 0 || Cs < 0 || h < 1 || w < 1) return fail(HALO_E_ARG, "%s: empty shape", who);
    if (int rc = dw_check(who, B, Ca + Cs, H, W, 1)) return rc;
    if (H < h || W < w)
        return fail(HALO_E_ARG, "%s: the planes of s, %lld x %lld, are smaller than a's %lld x %lld (an upsampling only)", who, (long long)H,
                    (long long)W, (long long)h, (long long)w);
    return HALO_OK;
}

static DwCat upcat_operands(int64_t Ca, int64_t Cs, int64_t h, int64_t w, int64_t H, int64_t W)
{
    DwCat K;
    K.Ca = (int)Ca, K.Cs = (int)Cs, K.h = (int)h, K.w = (int)w;
    // halo_bilinear_upsample's scales (launch_bilinear_rows, halo_hyperbolic.hip)
    K.sh = H > 1 ? (float)(h - 1) / (float)(H - 1) : 0.0f, K.sw = W > 1 ? (float)(w - 1) / (float)(W - 1) : 0.0f;
    K.c_lo = 0, K.c_n = (int)(Ca + Cs);
    return K;
}

// ---------------------------------------------------------------- N dilations over one LDS-resident plane (the ASPP pyramid)
// The v3+ heads hand one tensor to three dilated blocks.  A workgroup owns one plane (b, c) at a time and keeps it in LDS:
//   forward   the plane of x is staged once (16-byte or one-element loads); for each dilation in list order the chain walk above
//             runs over the LDS copy -- DwSrc<DW_FWD> with `a` pointing into LDS, dw_walk_apply unchanged, so the three-row register
//             window, the order of the 9-term sum and the roundings are the single-dilation kernel's -- and stores y_i.
//   backward  two LDS planes.  For each dilation with a gradient, gp_i = DwSrc<DW_BWD>::at (one rounding) is staged into the first,
//             the mirrored-tap walk reads it and writes its sum s_i into the second: the first dilation stores, every later one
//             does acc = acc + s_i (one float32 add, the bits of torch's (gx_0 + gx_1) + gx_2).  g_x is written once from LDS.
//             A null g_i is neither staged nor added.  No atomics, no read-modify-write of global memory.
// A plane's items (dw_geom's column groups x chains x segments) are spread over the block by a loop.  Dilation 1 takes the
// general window (<GW, false>): its three LDS reads per row are the same values as the <4, true> route's one load and two scalars.
// LDS: H W floats forward, 2 H W backward, dynamic; DWM_MAX_PLANE is the plane whose two copies fill a CU's 160 KiB.
constexpr int DWM_MAX_N = 4;
constexpr int DWM_FWD_TPB = 512, DWM_BWD_TPB = 1024;
constexpr int DWM_LDS_BYTES = 160 * 1024;
constexpr int64_t DWM_MAX_PLANE = DWM_LDS_BYTES / (2 * sizeof(float));
constexpr int64_t DWM_MAX_GRID = 1 << 20;

struct DwMulti {
    int n;
    DwGeom G[DWM_MAX_N];
    const float *g[DWM_MAX_N];   // backward: the gradient of y_i, null when that output was not used
};

// item `item` (below G.items) of a plane: dw_item's split without the block
template <int GW> __device__ __forceinline__ DwItem dwm_item(const DwGeom &G, long long item)
{
    const int g = (int)(item % G.ngroups);
    const long long t = item / G.ngroups;
    const int r = (int)(t % G.nres);
    const long long k0 = (t / G.nres) * DW_L;
    const long long i0 = r + k0 * G.d, iend = i0 + (long long)DW_L * G.d;
    DwItem it;
    it.c0 = g * GW;
    it.i0 = (int)(i0 < G.H ? i0 : G.H);
    it.iend = (int)(iend < G.H ? iend : G.H);
    return it;
}

// dw_walk_apply<DW_BWD, GW, false> with the result stored to, or added onto, the LDS plane `acc`
template <int GW>
__device__ __forceinline__ void dwm_walk_acc(const DwSrc<DW_FWD> &src, const float (&wk)[9], float *acc, bool add, const DwItem &it, const DwGeom &G)
{
    const int d = G.d;
    float win[3][3 * GW];
    src.template row<GW, false>(win[0], it.i0 - d, it.c0, G.H, G.W, d);
    src.template row<GW, false>(win[1], it.i0, it.c0, G.H, G.W, d);
    for (int i = it.i0; i < it.iend; i += d) {
        src.template row<GW, false>(win[2], i + d, it.c0, G.H, G.W, d);
        float res[GW];
#pragma unroll
        for (int e = 0; e < GW; ++e) {
            float s = wk[0] * win[0][e];
#pragma unroll
            for (int k = 1; k < 9; ++k) s = __builtin_fmaf(wk[k], win[k / 3][(k % 3) * GW + e], s);
            res[e] = s;
        }
        float *o = acc + (size_t)i * G.W + it.c0;
        if constexpr (GW == 4) {
            dw_f4 v;
            v.x = res[0], v.y = res[1], v.z = res[2], v.w = res[3];
            if (add) {
                const dw_f4 a = *reinterpret_cast<const dw_f4 *>(o);
                v.x = a.x + v.x, v.y = a.y + v.y, v.z = a.z + v.z, v.w = a.w + v.w;
            }
            *reinterpret_cast<dw_f4 *>(o) = v;
        } else {
            o[0] = add ? o[0] + res[0] : res[0];
        }
#pragma unroll
        for (int q = 0; q < 3 * GW; ++q) win[0][q] = win[1][q], win[1][q] = win[2][q];
    }
}

// y (n, B, C, H, W): y[i] = relu((dw3x3_{d_i}(x) over w[i]) * scale[i] + shift[i]); GW = 4 needs W % 4 == 0 and 16-byte aligned x, y
template <int GW>
__global__ void __launch_bounds__(DWM_FWD_TPB) k_dwm_fwd(const float *__restrict__ x, const float *__restrict__ w, const float *__restrict__ scale,
                                                         const float *__restrict__ shift, float *__restrict__ y, DwMulti P, long long planes)
{
    extern __shared__ __attribute__((aligned(16))) float dwm_lds[];
    const int hw = P.G[0].H * P.G[0].W, C = P.G[0].C;
    for (long long plane = blockIdx.x; plane < planes; plane += gridDim.x) {
        const int c = (int)(plane % C);
        const size_t po = (size_t)plane * hw;
        if constexpr (GW == 4) {
            for (int q = threadIdx.x; q < hw / 4; q += DWM_FWD_TPB)
                reinterpret_cast<dw_f4 *>(dwm_lds)[q] = reinterpret_cast<const dw_f4 *>(x + po)[q];
        } else {
            for (int q = threadIdx.x; q < hw; q += DWM_FWD_TPB) dwm_lds[q] = x[po + q];
        }
        __syncthreads();
        for (int i = 0; i < P.n; ++i) {
            const DwGeom G = P.G[i];
            const size_t ch = (size_t)i * C + c;
            const float sc = scale[ch], sh = shift[ch];
            float wk[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) wk[k] = w[ch * 9 + k];
            DwSrc<DW_FWD> src;
            src.a = dwm_lds, src.y = nullptr, src.scale = sc;
            float *op = y + ((size_t)i * planes + plane) * hw;
            for (long long item = threadIdx.x; item < G.items; item += DWM_FWD_TPB) {
                const DwItem it = dwm_item<GW>(G, item);
                dw_walk_apply<DW_FWD, GW, false>(src, wk, sc, sh, op, it, G);
            }
        }
        __syncthreads();                                   // the next plane overwrites what the walks read
    }
}

// One plane of the backward: for each dilation whose P.g[i] is not null, gp_i is staged into `gp` and the mirrored-tap walk stores
// (first) or adds (later) its sum into `acc`, in list order.  Ends behind a barrier: acc is complete for every thread.
template <int GW>
__device__ __forceinline__ void dwm_bwd_plane(const float *__restrict__ yv, const float *__restrict__ w, const float *__restrict__ scale,
                                              const DwMulti &P, long long planes, long long plane, int hw, int C, float *gp, float *acc)
{
    const int c = (int)(plane % C);
    const size_t po = (size_t)plane * hw;
    bool add = false;
    for (int i = 0; i < P.n; ++i) {
        const float *gi = P.g[i];
        if (!gi) continue;
        const DwGeom G = P.G[i];
        const size_t ch = (size_t)i * C + c;
        DwSrc<DW_BWD> in;
        in.a = gi + po, in.y = yv + ((size_t)i * planes + plane) * hw, in.scale = scale[ch];
        if constexpr (GW == 4) {
            for (int q = threadIdx.x; q < hw / 4; q += DWM_BWD_TPB) {
                float v[4];
                in.template at4<dw_f4>((size_t)q * 4, v);
                dw_f4 o;
                o.x = v[0], o.y = v[1], o.z = v[2], o.w = v[3];
                reinterpret_cast<dw_f4 *>(gp)[q] = o;
            }
        } else {
            for (int q = threadIdx.x; q < hw; q += DWM_BWD_TPB) gp[q] = in.at((size_t)q);
        }
        __syncthreads();
        float wk[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) wk[k] = w[ch * 9 + 8 - k];
        DwSrc<DW_FWD> src;
        src.a = gp, src.y = nullptr, src.scale = 0.0f;
        for (long long item = threadIdx.x; item < G.items; item += DWM_BWD_TPB) {
            const DwItem it = dwm_item<GW>(G, item);
            dwm_walk_acc<GW>(src, wk, acc, add, it, G);
        }
        __syncthreads();                               // gp is restaged, and another thread adds onto this element next
        add = true;
    }
}

// g_x = the sum, in list order, of dw3x3_{d_i}^T(gp_i) over the dilations whose P.g[i] is not null; GW = 4 needs W % 4 == 0 and
// 16-byte aligned g_i, y, g_x
template <int GW>
__global__ void __launch_bounds__(DWM_BWD_TPB) k_dwm_bwd(const float *__restrict__ yv, const float *__restrict__ w, const float *__restrict__ scale,
                                                         float *__restrict__ g_x, DwMulti P, long long planes)
{
    extern __shared__ __attribute__((aligned(16))) float dwm_lds[];
    const int hw = P.G[0].H * P.G[0].W, C = P.G[0].C;
    float *gp = dwm_lds, *acc = dwm_lds + hw;             // hw is a multiple of 4 on the 16-byte route
    for (long long plane = blockIdx.x; plane < planes; plane += gridDim.x) {
        const size_t po = (size_t)plane * hw;
        dwm_bwd_plane<GW>(yv, w, scale, P, planes, plane, hw, C, gp, acc);
        if constexpr (GW == 4) {
            for (int q = threadIdx.x; q < hw / 4; q += DWM_BWD_TPB)
                reinterpret_cast<dw_f4 *>(g_x + po)[q] = reinterpret_cast<const dw_f4 *>(acc)[q];
        } else {
            for (int q = threadIdx.x; q < hw; q += DWM_BWD_TPB) g_x[po + q] = acc[q];
        }
        // no barrier: the next plane's first walk writes acc only behind the barrier that follows its staging
    }
}

// The fan-out variant: x has further readers whose gradients e_0 .. e_{m-1} join the sum where k_dwm_bwd copies acc to g_x,
//     g_x = ((acc + e_0) + e_1) ...   float32 adds in list order, a null e_j left out
// dense[j]: e_j is (B, C, H, W); otherwise (B, C), one value per plane, e_j[plane] at every pixel.  No LDS beyond k_dwm_bwd's.
constexpr int DWM_MAX_FAN = 4;
struct DwFan {
    const float *e[DWM_MAX_FAN];   // null: left out
    int dense[DWM_MAX_FAN];
};

// GW = 4 needs, beyond k_dwm_bwd's conditions, every dense e_j 16-byte aligned
template <int GW>
__global__ void __launch_bounds__(DWM_BWD_TPB) k_dwm_fan_bwd(const float *__restrict__ yv, const float *__restrict__ w, const float *__restrict__ scale,
                                                             float *__restrict__ g_x, DwMulti P, DwFan F, long long planes)
{
    extern __shared__ __attribute__((aligned(16))) float dwm_lds[];
    const int hw = P.G[0].H * P.G[0].W, C = P.G[0].C;
    float *gp = dwm_lds, *acc = dwm_lds + hw;
    for (long long plane = blockIdx.x; plane < planes; plane += gridDim.x) {
        const size_t po = (size_t)plane * hw;
        dwm_bwd_plane<GW>(yv, w, scale, P, planes, plane, hw, C, gp, acc);
        float ep[DWM_MAX_FAN];                             // the per-plane addends' values of this plane
#pragma unroll
        for (int j = 0; j < DWM_MAX_FAN; ++j) ep[j] = (F.e[j] && !F.dense[j]) ? F.e[j][plane] : 0.0f;
        if constexpr (GW == 4) {
            for (int q = threadIdx.x; q < hw / 4; q += DWM_BWD_TPB) {
                dw_f4 v = reinterpret_cast<const dw_f4 *>(acc)[q];
#pragma unroll
                for (int j = 0; j < DWM_MAX_FAN; ++j) {
                    if (!F.e[j]) continue;
                    if (F.dense[j]) {
                        const dw_f4 a = reinterpret_cast<const dw_f4 *>(F.e[j] + po)[q];
                        v.x = v.x + a.x, v.y = v.y + a.y, v.z = v.z + a.z, v.w = v.w + a.w;
                    } else {
                        v.x = v.x + ep[j], v.y = v.y + ep[j], v.z = v.z + ep[j], v.w = v.w + ep[j];
                    }
                }
                reinterpret_cast<dw_f4 *>(g_x + po)[q] = v;
            }
        } else {
            for (int q = threadIdx.x; q < hw; q += DWM_BWD_TPB) {
                float v = acc[q];
#pragma unroll
                for (int j = 0; j < DWM_MAX_FAN; ++j) {
                    if (!F.e[j]) continue;
                    v = v + (F.dense[j] ? F.e[j][po + q] : ep[j]);
                }
                g_x[po + q] = v;
            }
        }
        // no barrier: as in k_dwm_bwd
    }
}

static int dwm_check(const char *who, int64_t B, int64_t C, int64_t H, int64_t W, int64_t n, const int64_t *d)
{
    if (n < 2 || n > DWM_MAX_N) return fail(HALO_E_ARG, "%s: %lld dilations, 2 to %d are served", who, (long long)n, DWM_MAX_N);
    if (!d) return fail(HALO_E_ARG, "%s: null argument", who);
    for (int64_t i = 0; i < n; ++i)
        if (int rc = dw_check(who, B, C, H, W, d[i])) return rc;
    return HALO_OK;
}

static int dwm_plane_check(const char *who, int64_t H, int64_t W)
{
    if (H * W > DWM_MAX_PLANE)
        return fail(HALO_E_UNSUPPORTED, "%s: plane of %lld x %lld = %lld elements, two copies of at most %lld fit the LDS", who, (long long)H,
                    (long long)W, (long long)(H * W), (long long)DWM_MAX_PLANE);
    return HALO_OK;
}

static DwMulti dwm_operands(int64_t C, int64_t H, int64_t W, int64_t n, const int64_t *d, int gw)
{
    DwMulti P;
    P.n = (int)n;
    for (int i = 0; i < DWM_MAX_N; ++i) {
        P.G[i] = dw_geom(C, H, W, d[i < n ? i : 0], gw);
        P.g[i] = nullptr;
    }
    return P;
}

// the launch's LDS: above the default 64 KiB the limit is raised first (once per kernel and device)
static int dwm_raise_lds(const char *who,LdsLimitSeen &seen, const void *kernel, size_t bytes)
{
    if (bytes > 64 * 1024 && !raise_lds_limit(seen, kernel, DWM_LDS_BYTES))
        return fail(HALO_E_LAUNCH, "%s: the device refused %d bytes of LDS per workgroup", who, DWM_LDS_BYTES);
    return HALO_OK;
}


// ---------------------------------------------------------------- the block half under torch.autocast (halo_half_dwconv3x3_*)
// Under autocast the stock chain casts x and w to half (float16 or bfloat16), the library's half conv returns half, the frozen norm
// promotes to float32, and autocast rounds the ReLU's result to half again for the pointwise conv.  The same chain walk with every
// operand in its own element type, h() = round to nearest even to the half dtype DT, half -> float exact:
//   xh = h(x) (x float32; a half x is read as it is)      wh = h(w[c,k])
//   c16 = h( sum_k wh[k] xh[tap k] )                      the nine terms in the order above; a product of two halves is exact
//   pre = fl(fl(float(c16) scale[c]) + shift[c]);  y32 = pre <= 0 ? 0 : pre  (a NaN stays);  y16 = h(y32)      the only output
//   gp  = y16 > 0 ? fl(float(g16) scale[c]) : 0;   gc16 = h(gp)               the gate is read off y16 (include/halo_hip.h)
//   g_x = h( sum_k wh[k] gc16[p - k d] )                  stored as half, or widened for a float32 x
//   g_w[c,k] = float( h( fl32( sum_{b,p} float(gc16) float(xh[p + k d]) ) ) )  float64 fma partials, dw_block_sum, k_dw_wsum's order
// A window holds the float32 values of halves.  Routes: GW = 4 -- 8-byte accesses of half operands, 16-byte accesses of float32
// ones, W % 4 == 0 and every operand aligned to its access -- and GW = 1; DwGeom, dw_item and the workspace are the float32 passes'.
// Conversions: a float -> half rounding behind an fma or a product of widened halves is done in integer arithmetic (ac_round):
// written as a conversion the compiler folds it into v_fma_mixlo_f16, which rounds the unrounded result once.  Loaded values and
// the ReLU's result convert in pairs (ac_round_group).
enum { DH_X = 0, DH_G = 1 };

typedef unsigned short dh_h4 __attribute__((ext_vector_type(4)));
typedef unsigned short dh_h4u __attribute__((ext_vector_type(4), aligned(2)));

template <bool ALIGNED> __device__ __forceinline__ void dh_load4(const float *p, float *v)
{
    dw_f4 t;
    if constexpr (ALIGNED) t = *reinterpret_cast<const dw_f4 *>(p);
    else t = *reinterpret_cast<const dw_f4u *>(p);
    v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
}

template <bool ALIGNED> __device__ __forceinline__ void dh_load4(const ac_half *p, ac_half *v)
{
    dh_h4 t;
    if constexpr (ALIGNED) t = *reinterpret_cast<const dh_h4 *>(p);
    else t = *reinterpret_cast<const dh_h4u *>(p);
    v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
}

// the operand a window is read from, as the float32 value of a half.  KIND DH_X: xh (XT float: h(x); XT ac_half: x).  KIND DH_G:
// gc16 from a = g16 and y = y16.  cols and row are DwSrc's.
template <int DT, int KIND, typename XT> struct DhSrc {
    const XT *a;
    const ac_half *y;
    float scale;
    __device__ __forceinline__ float at(size_t o) const
    {
        if constexpr (KIND == DH_X) {
            if constexpr (sizeof(XT) == 4) return ac_float<DT>(ac_round<DT>(a[o]));
            else return ac_float<DT>(a[o]);
        } else {
            const float p = ac_float<DT>(a[o]) * scale;
            return ac_float<DT>(ac_round<DT>(ac_float<DT>(y[o]) > 0.0f ? p : 0.0f));
        }
    }
    template <bool ALIGNED> __device__ __forceinline__ void at4(size_t o, float *out) const
    {
        if constexpr (KIND == DH_X && sizeof(XT) == 4) {
            float v[4];
            ac_half h[4];
            dh_load4<ALIGNED>(a + o, v);
            ac_round_group<DT, 4>(v, h);
#pragma unroll
            for (int e = 0; e < 4; ++e) out[e] = ac_float<DT>(h[e]);
        } else if constexpr (KIND == DH_X) {
            ac_half h[4];
            dh_load4<ALIGNED>(a + o, h);
#pragma unroll
            for (int e = 0; e < 4; ++e) out[e] = ac_float<DT>(h[e]);
        } else {
            ac_half gv[4], yv[4];
            dh_load4<ALIGNED>(a + o, gv);
            dh_load4<ALIGNED>(y + o, yv);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float p = ac_float<DT>(gv[e]) * scale;
                out[e] = ac_float<DT>(ac_round<DT>(ac_float<DT>(yv[e]) > 0.0f ? p : 0.0f));
            }
        }
    }
    template <int GW, bool ALIGNED> __device__ __forceinline__ void cols(float *out, int i, int c0, int H, int W) const
    {
        const bool row_in = i >= 0 && i < H;
        const size_t o = (size_t)(row_in ? i : 0) * W;
        if constexpr (GW == 4) {
            if (row_in && c0 >= 0 && c0 + 4 <= W) {
                at4<ALIGNED>(o + c0, out);
                return;
            }
        }
#pragma unroll
        for (int e = 0; e < GW; ++e) out[e] = row_in && c0 + e >= 0 && c0 + e < W ? at(o + (c0 + e)) : 0.0f;
    }
    template <int GW, bool D1> __device__ __forceinline__ void row(float *win, int i, int c0, int H, int W, int d) const
    {
        if constexpr (D1 && GW == 4) {
            cols<4, true>(win + 4, i, c0, H, W);
            const bool row_in = i >= 0 && i < H;
            const size_t o = (size_t)(row_in ? i : 0) * W;
            win[0] = row_in && c0 > 0 ? at(o + (c0 - 1)) : 0.0f;
            win[1] = win[4], win[2] = win[5], win[3] = win[6];
            win[8] = win[5], win[9] = win[6], win[10] = win[7];
            win[11] = row_in && c0 + 4 < W ? at(o + (c0 + 4)) : 0.0f;
        } else {
            cols<GW, false>(win, i, c0 - d, H, W);
            cols<GW, true>(win + GW, i, c0, H, W);
            cols<GW, false>(win + 2 * GW, i, c0 + d, H, W);
        }
    }
};

template <int DT, int GW> __device__ __forceinline__ void dh_store(ac_half *p, const ac_half *h)
{
    if constexpr (GW == 4) {
        dh_h4 v;
        v.x = h[0], v.y = h[1], v.z = h[2], v.w = h[3];
        *reinterpret_cast<dh_h4 *>(p) = v;
    } else {
        p[0] = h[0];
    }
}

// g_x of a float32 x: the exact widening of the half result
template <int DT, int GW> __device__ __forceinline__ void dh_store(float *p, const ac_half *h)
{
    if constexpr (GW == 4) {
        dw_f4 v;
        v.x = ac_float<DT>(h[0]), v.y = ac_float<DT>(h[1]), v.z = ac_float<DT>(h[2]), v.w = ac_float<DT>(h[3]);
        *reinterpret_cast<dw_f4 *>(p) = v;
    } else {
        p[0] = ac_float<DT>(h[0]);
    }
}

// dw_walk_apply over typed operands.  MODE DW_FWD: src = xh, op = y16.  MODE DW_BWD: src = gc16, wk mirrored, op = g_x.
template <int DT, int MODE, int GW, bool D1, typename SRC, typename OT>
__device__ __forceinline__ void dh_walk_apply(const SRC &src, const float (&wk)[9], float sc, float sh, OT *__restrict__ op, const DwItem &it,
                                              const DwGeom &G)
{
    const int d = D1 ? 1 : G.d;
    float win[3][3 * GW];
    src.template row<GW, D1>(win[0], it.i0 - d, it.c0, G.H, G.W, d);
    src.template row<GW, D1>(win[1], it.i0, it.c0, G.H, G.W, d);
    for (int i = it.i0; i < it.iend; i += d) {
        src.template row<GW, D1>(win[2], i + d, it.c0, G.H, G.W, d);
        ac_half res[GW];
        float y32[GW];
#pragma unroll
        for (int e = 0; e < GW; ++e) {
            float acc = wk[0] * win[0][e];
#pragma unroll
            for (int k = 1; k < 9; ++k) acc = __builtin_fmaf(wk[k], win[k / 3][(k % 3) * GW + e], acc);
            res[e] = ac_round<DT>(acc);                      // c16, or g_x
            if constexpr (MODE == DW_FWD) {
                float pre = ac_float<DT>(res[e]) * sc;
                pre = pre + sh;
                y32[e] = pre <= 0.0f ? 0.0f : pre;           // a NaN stays a NaN, as torch's ReLU leaves it
            }
        }
        if constexpr (MODE == DW_FWD) ac_round_group<DT, GW>(y32, res);
        dh_store<DT, GW>(op + (size_t)i * G.W + it.c0, res);
#pragma unroll
        for (int q = 0; q < 3 * GW; ++q) win[0][q] = win[1][q], win[1][q] = win[2][q];
    }
}

// the block-uniform taps: wh = h(w[c, k]), mirrored for the data gradient
template <int DT, int MODE> __device__ __forceinline__ void dh_taps(const float *__restrict__ w, int c, float (&wk)[9])
{
#pragma unroll
    for (int k = 0; k < 9; ++k) wk[k] = ac_float<DT>(ac_round<DT>(MODE == DW_FWD ? w[c * 9 + k] : w[c * 9 + 8 - k]));
}

template <int DT, typename XT, int GW, bool D1>
__global__ void __launch_bounds__(DW_TPB) k_dh_fwd(const XT *__restrict__ x, const float *__restrict__ w, const float *__restrict__ scale,
                                                   const float *__restrict__ shift, ac_half *__restrict__ y16, DwGeom G)
{
    const long long plane = blockIdx.x / G.bpp;
    const int blk = (int)(blockIdx.x - plane * G.bpp), c = (int)(plane % G.C);
    DwItem it;
    if (!dw_item<GW>(G, blk, it)) return;
    const size_t po = (size_t)plane * G.H * G.W;
    DhSrc<DT, DH_X, XT> src;
    src.a = x + po, src.y = nullptr, src.scale = 0.0f;
    float wk[9];
    dh_taps<DT, DW_FWD>(w, c, wk);
    dh_walk_apply<DT, DW_FWD, GW, D1>(src, wk, scale[c], shift[c], y16 + po, it, G);
}

template <int DT, typename OT, int GW, bool D1>
__global__ void __launch_bounds__(DW_TPB) k_dh_bwd(const ac_half *__restrict__ g16, const ac_half *__restrict__ y16, const float *__restrict__ w,
                                                   const float *__restrict__ scale, OT *__restrict__ g_x, DwGeom G)
{
    const long long plane = blockIdx.x / G.bpp;
    const int blk = (int)(blockIdx.x - plane * G.bpp), c = (int)(plane % G.C);
    DwItem it;
    if (!dw_item<GW>(G, blk, it)) return;
    const size_t po = (size_t)plane * G.H * G.W;
    DhSrc<DT, DH_G, ac_half> src;
    src.a = g16 + po, src.y = y16 + po, src.scale = scale[c];
    float wk[9];
    dh_taps<DT, DW_BWD>(w, c, wk);
    dh_walk_apply<DT, DW_BWD, GW, D1>(src, wk, 0.0f, 0.0f, g_x + po, it, G);
}

// dw_walk_wpart over typed operands: float64 sums of gc16[p] xh[p + k d]
template <int GW, bool D1, typename SX, typename SG>
__device__ __forceinline__ void dh_walk_wpart(const SX &sx, const SG &sg, const DwItem &it, const DwGeom &G, double (&acc)[9])
{
    const int d = D1 ? 1 : G.d;
    float win[3][3 * GW];
    sx.template row<GW, D1>(win[0], it.i0 - d, it.c0, G.H, G.W, d);
    sx.template row<GW, D1>(win[1], it.i0, it.c0, G.H, G.W, d);
    for (int i = it.i0; i < it.iend; i += d) {
        sx.template row<GW, D1>(win[2], i + d, it.c0, G.H, G.W, d);
        float gp[GW];
        sg.template cols<GW, true>(gp, i, it.c0, G.H, G.W);
#pragma unroll
        for (int e = 0; e < GW; ++e) {
            const double ge = (double)gp[e];
#pragma unroll
            for (int k = 0; k < 9; ++k) acc[k] = __builtin_fma(ge, (double)win[k / 3][(k % 3) * GW + e], acc[k]);
        }
#pragma unroll
        for (int q = 0; q < 3 * GW; ++q) win[0][q] = win[1][q], win[1][q] = win[2][q];
    }
}

template <int DT, typename XT, int GW, bool D1>
__global__ void __launch_bounds__(DW_TPB) k_dh_wpart(const ac_half *__restrict__ g16, const ac_half *__restrict__ y16, const XT *__restrict__ x,
                                                     const float *__restrict__ scale, double *__restrict__ part, DwGeom G)
{
    const long long plane = blockIdx.x / G.bpp;
    const int blk = (int)(blockIdx.x - plane * G.bpp), c = (int)(plane % G.C);
    const size_t po = (size_t)plane * G.H * G.W;
    double acc[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) acc[k] = 0.0;
    DwItem it;
    if (dw_item<GW>(G, blk, it)) {
        DhSrc<DT, DH_X, XT> sx;
        sx.a = x + po, sx.y = nullptr, sx.scale = 0.0f;
        DhSrc<DT, DH_G, ac_half> sg;
        sg.a = g16 + po, sg.y = y16 + po, sg.scale = scale[c];
        dh_walk_wpart<GW, D1>(sx, sg, it, G, acc);
    }
    dw_block_sum(acc, part);
}

// k_dw_wsum with the chain's two roundings behind the float64 sum: to float32, then to the half whose value g_w holds
template <int DT>
__global__ void __launch_bounds__(DW_TPB) k_dh_wsum(const double *__restrict__ part, float *__restrict__ gw, int B, int C, int bpp)
{
    const int e = blockIdx.x * DW_TPB + threadIdx.x;
    if (e >= C * 9) return;
    const int c = e / 9, k = e - c * 9;
    double t = 0.0;
    for (int b = 0; b < B; ++b) {
        const double *row = part + ((size_t)b * C + c) * bpp * 9 + k;
        for (int q = 0; q < bpp; ++q) t += row[(size_t)q * 9];
    }
    gw[e] = ac_float<DT>(ac_round<DT>((float)t));
}

static bool dh_half_code(int code) { return code == HALO_F16 || code == HALO_BF16; }

// an operand's alignment for the GW = 4 route: 16 bytes of float32, 8 bytes of half
static bool dh_aligned(const void *p, int dtype) { return ((uintptr_t)p % (dtype == HALO_F32 ? 16 : 8)) == 0; }

// f(DT, X32, GW, D1) with the run-time choices as types; route 0: <4, true>, 1: <4, false>, 2: <1, false>
template <class F> static void dh_dispatch(int half_dtype, bool x32, bool vec, int64_t d, F f)
{
    auto r = [&](auto DT, auto X32) {
        if (vec && d == 1) f(DT, X32, std::integral_constant<int, 4>(), std::true_type());
        else if (vec) f(DT, X32, std::integral_constant<int, 4>(), std::false_type());
        else f(DT, X32, std::integral_constant<int, 1>(), std::false_type());
    };
    auto t = [&](auto DT) {
        if (x32) r(DT, std::true_type());
        else r(DT, std::false_type());
    };
    if (half_dtype == HALO_BF16) t(std::integral_constant<int, HALO_BF16>());
    else t(std::integral_constant<int, HALO_F16>());
}

}  // namespace halo

using namespace halo;

extern "C" size_t halo_dwconv_workspace_bytes(int64_t B, int64_t C, int64_t H, int64_t W, int64_t d)
{
    if (dw_check("halo_dwconv_workspace_bytes", B, C, H, W, d) != HALO_OK) return 0;
    const int b1 = dw_geom(C, H, W, d, 1).bpp, b4 = W % 4 == 0 ? dw_geom(C, H, W, d, 4).bpp : 0;
    return (size_t)(B * C) * (size_t)(b1 > b4 ? b1 : b4) * 9 * sizeof(double);
}

extern "C" int halo_dwconv3x3_affine_relu_fwd(const float *x, const float *w, const float *scale, const float *shift, float *y, int64_t B,
                                              int64_t C, int64_t H, int64_t W, int64_t d, void *stream)
{
    const char *who = "halo_dwconv3x3_affine_relu_fwd";
    if (int rc = dw_check(who, B, C, H, W, d)) return rc;
    if (!x || !w || !scale || !shift || !y) return fail(HALO_E_ARG, "%s: null argument", who);
    const bool vec = dw_vec(W, x, y, nullptr, nullptr);
    const DwGeom G = dw_geom(C, H, W, d, vec ? 4 : 1);
    unsigned grid;
    if (int rc = dw_grid(who, B * C, G, grid)) return rc;
    dw_launch_apply<DW_FWD>(vec, grid, (hipStream_t)stream, x, nullptr, w, scale, shift, y, G);
    return check_launch(who);
}

extern "C" int halo_dwconv3x3_affine_relu_bwd_data(const float *g, const float *y, const float *w, const float *scale, float *g_x, int64_t B,
                                                   int64_t C, int64_t H, int64_t W, int64_t d, void *stream)
{
    const char *who = "halo_dwconv3x3_affine_relu_bwd_data";
    if (int rc = dw_check(who, B, C, H, W, d)) return rc;
    if (!g || !y || !w || !scale || !g_x) return fail(HALO_E_ARG, "%s: null argument", who);
    const bool vec = dw_vec(W, g, y, g_x, nullptr);
    const DwGeom G = dw_geom(C, H, W, d, vec ? 4 : 1);
    unsigned grid;
    if (int rc = dw_grid(who, B * C, G, grid)) return rc;
    dw_launch_apply<DW_BWD>(vec, grid, (hipStream_t)stream, g, y, w, scale, nullptr, g_x, G);
    return check_launch(who);
}

extern "C" int halo_dwconv3x3_affine_relu_bwd_weight(const float *g, const float *y, const float *x, const float *scale, float *g_w, int64_t B,
                                                     int64_t C, int64_t H, int64_t W, int64_t d, void *workspace, size_t workspace_bytes,
                                                     void *stream)
{
    const char *who = "halo_dwconv3x3_affine_relu_bwd_weight";
    if (int rc = dw_check(who, B, C, H, W, d)) return rc;
    if (!g || !y || !x || !scale || !g_w) return fail(HALO_E_ARG, "%s: null argument", who);
    const size_t need = halo_dwconv_workspace_bytes(B, C, H, W, d);
    if (!workspace || workspace_bytes < need || ((uintptr_t)workspace % 8) != 0)
        return fail(HALO_E_WORKSPACE, "%s: workspace of %zu bytes, %zu needed (8-byte aligned)", who, workspace_bytes, need);
    const bool vec = dw_vec(W, g, y, x, nullptr);
    const DwGeom G = dw_geom(C, H, W, d, vec ? 4 : 1);
    unsigned grid;
    if (int rc = dw_grid(who, B * C, G, grid)) return rc;
    hipStream_t st = (hipStream_t)stream;
    double *part = (double *)workspace;
    const dim3 gr(grid), bl(DW_TPB);
    if (vec && d == 1) hipLaunchKernelGGL((k_dw_wpart<4, true>), gr, bl, 0, st, g, y, x, scale, part, G);
    else if (vec) hipLaunchKernelGGL((k_dw_wpart<4, false>), gr, bl, 0, st, g, y, x, scale, part, G);
    else hipLaunchKernelGGL((k_dw_wpart<1, false>), gr, bl, 0, st, g, y, x, scale, part, G);
    hipLaunchKernelGGL(k_dw_wsum, dim3((unsigned)cdiv(C * 9, DW_TPB)), bl, 0, st, (const double *)part, g_w, (int)B, (int)C, G.bpp);
    return check_launch(who);
}

extern "C" int halo_upcat_dwconv3x3_affine_relu_fwd(const float *a, const float *s, const float *w, const float *scale, const float *shift,
                                                    float *y, int64_t B, int64_t Ca, int64_t Cs, int64_t h, int64_t w_in, int64_t H, int64_t W,
                                                    void *stream)
{
    const char *who = "halo_upcat_dwconv3x3_affine_relu_fwd";
    if (int rc = upcat_check(who, B, Ca, Cs, h, w_in, H, W)) return rc;
    if ((Ca > 0 && !a) || (Cs > 0 && !s) || !w || !scale || !shift || !y) return fail(HALO_E_ARG, "%s: null argument", who);
    const bool vec = dw_vec(W, s, y, nullptr, nullptr);
    const DwGeom G = dw_geom(Ca + Cs, H, W, 1, vec ? 4 : 1);
    unsigned grid;
    if (int rc = dw_grid(who, B * (Ca + Cs), G, grid)) return rc;
    const DwCat K = upcat_operands(Ca, Cs, h, w_in, H, W);
    const dim3 gr(grid), bl(DW_TPB);
    hipStream_t st = (hipStream_t)stream;
    if (vec) hipLaunchKernelGGL((k_dw_upcat_fwd<4>), gr, bl, 0, st, a, s, w, scale, shift, y, G, K);
    else hipLaunchKernelGGL((k_dw_upcat_fwd<1>), gr, bl, 0, st, a, s, w, scale, shift, y, G, K);
    return check_launch(who);
}

extern "C" int halo_upcat_dwconv3x3_affine_relu_bwd_data(const float *g, const float *y, const float *w, const float *scale, float *g_up,
                                                         float *g_s, int64_t B, int64_t Ca, int64_t Cs, int64_t H, int64_t W, void *stream)
{
    const char *who = "halo_upcat_dwconv3x3_affine_relu_bwd_data";
    if (int rc = upcat_check(who, B, Ca, Cs, 1, 1, H, W)) return rc;
    if (!g || !y || !w || !scale) return fail(HALO_E_ARG, "%s: null argument", who);
    DwCat K = upcat_operands(Ca, Cs, 1, 1, H, W);
    K.c_lo = g_up ? 0 : (int)Ca;
    K.c_n = (int)((g_up ? Ca : 0) + (g_s ? Cs : 0));
    if (K.c_n == 0) return HALO_OK;                                // no gradient wanted (or none of the wanted half's channels exist)
    const bool vec = dw_vec(W, g, y, g_up, g_s);
    const DwGeom G = dw_geom(Ca + Cs, H, W, 1, vec ? 4 : 1);
    unsigned grid;
    if (int rc = dw_grid(who, B * K.c_n, G, grid)) return rc;
    const dim3 gr(grid), bl(DW_TPB);
    hipStream_t st = (hipStream_t)stream;
    if (vec) hipLaunchKernelGGL((k_dw_upcat_bwd<4>), gr, bl, 0, st, g, y, w, scale, g_up, g_s, G, K);
    else hipLaunchKernelGGL((k_dw_upcat_bwd<1>), gr, bl, 0, st, g, y, w, scale, g_up, g_s, G, K);
    return check_launch(who);
}

extern "C" int halo_upcat_dwconv3x3_affine_relu_bwd_weight(const float *g, const float *y, const float *a, const float *s, const float *scale,
                                                           float *g_w, int64_t B, int64_t Ca, int64_t Cs, int64_t h, int64_t w_in, int64_t H,
                                                           int64_t W, void *workspace, size_t workspace_bytes, void *stream)
{
    const char *who = "halo_upcat_dwconv3x3_affine_relu_bwd_weight";
    if (int rc = upcat_check(who, B, Ca, Cs, h, w_in, H, W)) return rc;
    if (!g || !y || (Ca > 0 && !a) || (Cs > 0 && !s) || !scale || !g_w) return fail(HALO_E_ARG, "%s: null argument", who);
    const int64_t C = Ca + Cs;
    const size_t need = halo_dwconv_workspace_bytes(B, C, H, W, 1);
    if (!workspace || workspace_bytes < need || ((uintptr_t)workspace % 8) != 0)
        return fail(HALO_E_WORKSPACE, "%s: workspace of %zu bytes, %zu needed (8-byte aligned)", who, workspace_bytes, need);
    const bool vec = dw_vec(W, g, y, s, nullptr);
    const DwGeom G = dw_geom(C, H, W, 1, vec ? 4 : 1);
    unsigned grid;
    if (int rc = dw_grid(who, B * C, G, grid)) return rc;
    const DwCat K = upcat_operands(Ca, Cs, h, w_in, H, W);
    hipStream_t st = (hipStream_t)stream;
    double *part = (double *)workspace;
    const dim3 gr(grid), bl(DW_TPB);
    if (vec) hipLaunchKernelGGL((k_dw_upcat_wpart<4>), gr, bl, 0, st, g, y, a, s, scale, part, G, K);
    else hipLaunchKernelGGL((k_dw_upcat_wpart<1>), gr, bl, 0, st, g, y, a, s, scale, part, G, K);
    hipLaunchKernelGGL(k_dw_wsum, dim3((unsigned)cdiv(C * 9, DW_TPB)), bl, 0, st, (const double *)part, g_w, (int)B, (int)C, G.bpp);
    return check_launch(who);
}

extern "C" int halo_joint_dwconv3x3_affine_relu_bwd(const float *g, const float *y, const float *x, const float *w, const float *scale,
                                                    float *g_x, float *g_w, int64_t B, int64_t C, int64_t H, int64_t W, int64_t d,
                                                    void *workspace, size_t workspace_bytes, void *stream)
{
    const char *who = "halo_joint_dwconv3x3_affine_relu_bwd";
    if (int rc = dw_check(who, B, C, H, W, d)) return rc;
    if (!g || !y || !x || !w || !scale || !g_x || !g_w) return fail(HALO_E_ARG, "%s: null argument", who);
    const size_t need = halo_dwconv_workspace_bytes(B, C, H, W, d);
    if (!workspace || workspace_bytes < need || ((uintptr_t)workspace % 8) != 0)
        return fail(HALO_E_WORKSPACE, "%s: workspace of %zu bytes, %zu needed (8-byte aligned)", who, workspace_bytes, need);
    const bool vec = dw_vec(W, g, y, x, g_x);
    const DwGeom G = dw_geom(C, H, W, d, vec ? 4 : 1);
    unsigned grid;
    if (int rc = dw_grid(who, B * C, G, grid)) return rc;
    hipStream_t st = (hipStream_t)stream;
    double *part = (double *)workspace;
    const dim3 gr(grid), bl(DW_TPB);
    if (vec && d == 1) hipLaunchKernelGGL((k_dw_joint<4, true>), gr, bl, 0, st, g, y, x, w, scale, g_x, part, G);
    else if (vec) hipLaunchKernelGGL((k_dw_joint<4, false>), gr, bl, 0, st, g, y, x, w, scale, g_x, part, G);
    else hipLaunchKernelGGL((k_dw_joint<1, false>), gr, bl, 0, st, g, y, x, w, scale, g_x, part, G);
    hipLaunchKernelGGL(k_dw_wsum, dim3((unsigned)cdiv(C * 9, DW_TPB)), bl, 0, st, (const double *)part, g_w, (int)B, (int)C, G.bpp);
    return check_launch(who);
}

extern "C" int halo_joint_upcat_dwconv3x3_affine_relu_bwd(const float *g, const float *y, const float *a, const float *s, const float *w,
                                                          const float *scale, float *g_up, float *g_s, float *g_w, int64_t B, int64_t Ca,
                                                          int64_t Cs, int64_t h, int64_t w_in, int64_t H, int64_t W, void *workspace,
                                                          size_t workspace_bytes, void *stream)
{
    const char *who = "halo_joint_upcat_dwconv3x3_affine_relu_bwd";
    if (int rc = upcat_check(who, B, Ca, Cs, h, w_in, H, W)) return rc;
    if (!g || !y || (Ca > 0 && (!a || !g_up)) || (Cs > 0 && (!s || !g_s)) || !w || !scale || !g_w) return fail(HALO_E_ARG, "%s: null argument", who);
    const int64_t C = Ca + Cs;
    const size_t need = halo_dwconv_workspace_bytes(B, C, H, W, 1);
    if (!workspace || workspace_bytes < need || ((uintptr_t)workspace % 8) != 0)
        return fail(HALO_E_WORKSPACE, "%s: workspace of %zu bytes, %zu needed (8-byte aligned)", who, workspace_bytes, need);
    const bool vec = dw_vec(W, g, y, s, (const void *)((uintptr_t)g_up | (uintptr_t)g_s));
    const DwGeom G = dw_geom(C, H, W, 1, vec ? 4 : 1);
    unsigned grid;
    if (int rc = dw_grid(who, B * C, G, grid)) return rc;
    const DwCat K = upcat_operands(Ca, Cs, h, w_in, H, W);
    hipStream_t st = (hipStream_t)stream;
    double *part = (double *)workspace;
    const dim3 gr(grid), bl(DW_TPB);
    if (vec) hipLaunchKernelGGL((k_dw_upcat_joint<4>), gr, bl, 0, st, g, y, a, s, w, scale, g_up, g_s, part, G, K);
    else hipLaunchKernelGGL((k_dw_upcat_joint<1>), gr, bl, 0, st, g, y, a, s, w, scale, g_up, g_s, part, G, K);
    hipLaunchKernelGGL(k_dw_wsum, dim3((unsigned)cdiv(C * 9, DW_TPB)), bl, 0, st, (const double *)part, g_w, (int)B, (int)C, G.bpp);
    return check_launch(who);
}

extern "C" int64_t halo_multi_dwconv_max_plane(void) { return DWM_MAX_PLANE; }

extern "C" int halo_multi_dwconv3x3_affine_relu_fwd(const float *x, const float *w, const float *scale, const float *shift, float *y, int64_t B,
                                                    int64_t C, int64_t H, int64_t W, int64_t n, const int64_t *d, void *stream)
{
    const char *who = "halo_multi_dwconv3x3_affine_relu_fwd";
    if (int rc = dwm_check(who, B, C, H, W, n, d)) return rc;
    if (!x || !w || !scale || !shift || !y) return fail(HALO_E_ARG, "%s: null argument", who);
    if (int rc = dwm_plane_check(who, H, W)) return rc;
    const bool vec = dw_vec(W, x, y, nullptr, nullptr);
    const DwMulti P = dwm_operands(C, H, W, n, d, vec ? 4 : 1);
    const int64_t planes = B * C;
    const dim3 gr((unsigned)(planes < DWM_MAX_GRID ? planes : DWM_MAX_GRID)), bl(DWM_FWD_TPB);
    const size_t lds = (size_t)(H * W) * sizeof(float);
    hipStream_t st = (hipStream_t)stream;
    static LdsLimitSeen seen4, seen1;
    if (vec) {
        if (int rc = dwm_raise_lds(who, seen4, (const void *)k_dwm_fwd<4>, lds)) return rc;
        hipLaunchKernelGGL((k_dwm_fwd<4>), gr, bl, lds, st, x, w, scale, shift, y, P, (long long)planes);
    } else {
        if (int rc = dwm_raise_lds(who, seen1, (const void *)k_dwm_fwd<1>, lds)) return rc;
        hipLaunchKernelGGL((k_dwm_fwd<1>), gr, bl, lds, st, x, w, scale, shift, y, P, (long long)planes);
    }
    return check_launch(who);
}

extern "C" int halo_multi_dwconv3x3_affine_relu_bwd_data(const float *const *g, const float *y, const float *w, const float *scale, float *g_x,
                                                         int64_t B, int64_t C, int64_t H, int64_t W, int64_t n, const int64_t *d, void *stream)
{
    const char *who = "halo_multi_dwconv3x3_affine_relu_bwd_data";
    if (int rc = dwm_check(who, B, C, H, W, n, d)) return rc;
    if (!g || !y || !w || !scale || !g_x) return fail(HALO_E_ARG, "%s: null argument", who);
    uintptr_t bits = 0;
    bool any = false;
    for (int64_t i = 0; i < n; ++i) any = any || g[i], bits |= (uintptr_t)g[i];
    if (!any) return fail(HALO_E_ARG, "%s: every gradient is null", who);
    if (int rc = dwm_plane_check(who, H, W)) return rc;
    const bool vec = dw_vec(W, (const void *)bits, y, g_x, nullptr);
    DwMulti P = dwm_operands(C, H, W, n, d, vec ? 4 : 1);
    for (int64_t i = 0; i < n; ++i) P.g[i] = g[i];
    const int64_t planes = B * C;
    const dim3 gr((unsigned)(planes < DWM_MAX_GRID ? planes : DWM_MAX_GRID)), bl(DWM_BWD_TPB);
    const size_t lds = (size_t)(H * W) * 2 * sizeof(float);
    hipStream_t st = (hipStream_t)stream;
    static LdsLimitSeen seen4, seen1;
    if (vec) {
        if (int rc = dwm_raise_lds(who, seen4, (const void *)k_dwm_bwd<4>, lds)) return rc;
        hipLaunchKernelGGL((k_dwm_bwd<4>), gr, bl, lds, st, y, w, scale, g_x, P, (long long)planes);
    } else {
        if (int rc = dwm_raise_lds(who, seen1, (const void *)k_dwm_bwd<1>, lds)) return rc;
        hipLaunchKernelGGL((k_dwm_bwd<1>), gr, bl, lds, st, y, w, scale, g_x, P, (long long)planes);
    }
    return check_launch(who);
}

extern "C" int halo_fan_dwconv3x3_affine_relu_bwd_data(const float *const *g, const float *y, const float *w, const float *scale, float *g_x,
                                                       int64_t B, int64_t C, int64_t H, int64_t W, int64_t n, const int64_t *d, int64_t m,
                                                       const float *const *e, const int32_t *e_plane, void *stream)
{
    const char *who = "halo_fan_dwconv3x3_affine_relu_bwd_data";
    if (int rc = dwm_check(who, B, C, H, W, n, d)) return rc;
    if (!g || !y || !w || !scale || !g_x) return fail(HALO_E_ARG, "%s: null argument", who);
    if (m < 0 || m > DWM_MAX_FAN) return fail(HALO_E_ARG, "%s: %lld extra addends, 0 to %d are served", who, (long long)m, DWM_MAX_FAN);
    if (m > 0 && (!e || !e_plane)) return fail(HALO_E_ARG, "%s: null argument", who);
    uintptr_t bits = 0;
    bool any = false;
    for (int64_t i = 0; i < n; ++i) any = any || g[i], bits |= (uintptr_t)g[i];
    if (!any) return fail(HALO_E_ARG, "%s: every gradient is null", who);
    if (int rc = dwm_plane_check(who, H, W)) return rc;
    DwFan F;
    for (int j = 0; j < DWM_MAX_FAN; ++j) {
        F.e[j] = j < m ? e[j] : nullptr;
        F.dense[j] = j < m ? e_plane[j] == 0 : 0;
        if (F.dense[j]) bits |= (uintptr_t)F.e[j];         // a per-plane addend is read one float at a time on either route
    }
    const bool vec = dw_vec(W, (const void *)bits, y, g_x, nullptr);
    DwMulti P = dwm_operands(C, H, W, n, d, vec ? 4 : 1);
    for (int64_t i = 0; i < n; ++i) P.g[i] = g[i];
    const int64_t planes = B * C;
    const dim3 gr((unsigned)(planes < DWM_MAX_GRID ? planes : DWM_MAX_GRID)), bl(DWM_BWD_TPB);
    const size_t lds = (size_t)(H * W) * 2 * sizeof(float);
    hipStream_t st = (hipStream_t)stream;
    static LdsLimitSeen seen4, seen1;
    if (vec) {
        if (int rc = dwm_raise_lds(who, seen4, (const void *)k_dwm_fan_bwd<4>, lds)) return rc;
        hipLaunchKernelGGL((k_dwm_fan_bwd<4>), gr, bl, lds, st, y, w, scale, g_x, P, F, (long long)planes);
    } else {
        if (int rc = dwm_raise_lds(who, seen1, (const void *)k_dwm_fan_bwd<1>, lds)) return rc;
        hipLaunchKernelGGL((k_dwm_fan_bwd<1>), gr, bl, lds, st, y, w, scale, g_x, P, F, (long long)planes);
    }
    return check_launch(who);
}

extern "C" int halo_half_dwconv3x3_affine_relu_fwd(const void *x, int x_dtype, const float *w, const float *scale, const float *shift, void *y16,
                                                   int half_dtype, int64_t B, int64_t C, int64_t H, int64_t W, int64_t d, void *stream)
{
    const char *who = "halo_half_dwconv3x3_affine_relu_fwd";
    if (!x || !w || !scale || !shift || !y16) return fail(HALO_E_ARG, "%s: null argument", who);
    if (!dh_half_code(half_dtype)) return fail(HALO_E_ARG, "%s: half_dtype %d is neither HALO_F16 nor HALO_BF16", who, half_dtype);
    if (x_dtype != HALO_F32 && x_dtype != half_dtype) return fail(HALO_E_ARG, "%s: x_dtype %d is neither HALO_F32 nor half_dtype", who, x_dtype);
    if (int rc = dw_check(who, B, C, H, W, d)) return rc;
    const bool vec = W % 4 == 0 && dh_aligned(x, x_dtype) && dh_aligned(y16, half_dtype);
    const DwGeom G = dw_geom(C, H, W, d, vec ? 4 : 1);
    unsigned grid;
    if (int rc = dw_grid(who, B * C, G, grid)) return rc;
    dh_dispatch(half_dtype, x_dtype == HALO_F32, vec, d, [&](auto DT, auto X32, auto GW, auto D1) {
        using XT = std::conditional_t<decltype(X32)::value, float, ac_half>;
        hipLaunchKernelGGL((k_dh_fwd<decltype(DT)::value, XT, decltype(GW)::value, decltype(D1)::value>), dim3(grid), dim3(DW_TPB), 0,
                           (hipStream_t)stream, (const XT *)x, w, scale, shift, (ac_half *)y16, G);
    });
    return check_launch(who);
}

extern "C" int halo_half_dwconv3x3_affine_relu_bwd_data(const void *g16, const void *y16, const float *w, const float *scale, void *g_x,
                                                        int gx_dtype, int half_dtype, int64_t B, int64_t C, int64_t H, int64_t W, int64_t d,
                                                        void *stream)
{
    const char *who = "halo_half_dwconv3x3_affine_relu_bwd_data";
    if (!g16 || !y16 || !w || !scale || !g_x) return fail(HALO_E_ARG, "%s: null argument", who);
    if (!dh_half_code(half_dtype)) return fail(HALO_E_ARG, "%s: half_dtype %d is neither HALO_F16 nor HALO_BF16", who, half_dtype);
    if (gx_dtype != HALO_F32 && gx_dtype != half_dtype) return fail(HALO_E_ARG, "%s: gx_dtype %d is neither HALO_F32 nor half_dtype", who, gx_dtype);
    if (int rc = dw_check(who, B, C, H, W, d)) return rc;
    const bool vec = W % 4 == 0 && dh_aligned(g16, half_dtype) && dh_aligned(y16, half_dtype) && dh_aligned(g_x, gx_dtype);
    const DwGeom G = dw_geom(C, H, W, d, vec ? 4 : 1);
    unsigned grid;
    if (int rc = dw_grid(who, B * C, G, grid)) return rc;
    dh_dispatch(half_dtype, gx_dtype == HALO_F32, vec, d, [&](auto DT, auto X32, auto GW, auto D1) {
        using OT = std::conditional_t<decltype(X32)::value, float, ac_half>;
        hipLaunchKernelGGL((k_dh_bwd<decltype(DT)::value, OT, decltype(GW)::value, decltype(D1)::value>), dim3(grid), dim3(DW_TPB), 0,
                           (hipStream_t)stream, (const ac_half *)g16, (const ac_half *)y16, w, scale, (OT *)g_x, G);
    });
    return check_launch(who);
}

extern "C" int halo_half_dwconv3x3_affine_relu_bwd_weight(const void *g16, const void *y16, const void *x, int x_dtype, const float *scale,
                                                          float *g_w, int half_dtype, int64_t B, int64_t C, int64_t H, int64_t W, int64_t d,
                                                          void *workspace, size_t workspace_bytes, void *stream)
{
    const char *who = "halo_half_dwconv3x3_affine_relu_bwd_weight";
    if (!g16 || !y16 || !x || !scale || !g_w) return fail(HALO_E_ARG, "%s: null argument", who);
    if (!dh_half_code(half_dtype)) return fail(HALO_E_ARG, "%s: half_dtype %d is neither HALO_F16 nor HALO_BF16", who, half_dtype);
    if (x_dtype != HALO_F32 && x_dtype != half_dtype) return fail(HALO_E_ARG, "%s: x_dtype %d is neither HALO_F32 nor half_dtype", who, x_dtype);
    if (int rc = dw_check(who, B, C, H, W, d)) return rc;
    const size_t need = halo_dwconv_workspace_bytes(B, C, H, W, d);
    if (!workspace || workspace_bytes < need || ((uintptr_t)workspace % 8) != 0)
        return fail(HALO_E_WORKSPACE, "%s: workspace of %zu bytes, %zu needed (8-byte aligned)", who, workspace_bytes, need);
    const bool vec = W % 4 == 0 && dh_aligned(g16, half_dtype) && dh_aligned(y16, half_dtype) && dh_aligned(x, x_dtype);
    const DwGeom G = dw_geom(C, H, W, d, vec ? 4 : 1);
    unsigned grid;
    if (int rc = dw_grid(who, B * C, G, grid)) return rc;
    hipStream_t st = (hipStream_t)stream;
    double *part = (double *)workspace;
    dh_dispatch(half_dtype, x_dtype == HALO_F32, vec, d, [&](auto DT, auto X32, auto GW, auto D1) {
        using XT = std::conditional_t<decltype(X32)::value, float, ac_half>;
        hipLaunchKernelGGL((k_dh_wpart<decltype(DT)::value, XT, decltype(GW)::value, decltype(D1)::value>), dim3(grid), dim3(DW_TPB), 0, st,
                           (const ac_half *)g16, (const ac_half *)y16, (const XT *)x, scale, part, G);
        hipLaunchKernelGGL((k_dh_wsum<decltype(DT)::value>), dim3((unsigned)cdiv(C * 9, DW_TPB)), dim3(DW_TPB), 0, st, (const double *)part, g_w,
                           (int)B, (int)C, G.bpp);
    });
    return check_launch(who);
}
