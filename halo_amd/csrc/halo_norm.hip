// A frozen norm, the residual add and the ReLU of a ResNet block (core/models/resnet.py:53-69, 92-112 with the FrozenBatchNorm2d of
// core/models/layers.py) in one pass over dense NCHW float32 planes:
//
//   pre = fl(fl(x * scale[c]) + shift[c])                  two roundings, never an fma (the build sets -ffp-contract=off)
//   id  = r   or   fl(fl(r * r_scale[c]) + r_shift[c])     the block's identity, or its downsample norm folded in
//   s   = pre   or   fl(pre + id)
//   y   = s <= 0 ? 0 : s                                   a NaN stays a NaN
//
//   gp  = y <= 0 ? 0 : g                                   a NaN y lets g through
//   g_x = fl(gp * scale[c]);   g_r = gp   or   fl(gp * r_scale[c])
//
// These are the statements and roundings of the torch chain `x * scale + bias; out += identity; relu_(out)` and of its autograd
// backward, element by element, so the results are the chain's bits.  There is no sum over elements: no order to fix, no LDS, no
// atomics, and the two routes below run the same statements.
//
// Tiling: a workgroup works inside one plane, so scale, shift, r_scale and r_shift are block-uniform scalar loads.  A plane of
// HW elements is cut into chunks of AN_TPB * AN_U groups of GW elements (GW = 4: 16-byte loads and stores, HW % 4 == 0 and
// every operand 16-byte aligned; GW = 1: any HW and any alignment).  A lane issues its AN_U loads of every operand before it
// computes (AN_U x 16 bytes per operand in flight), lanes of a wave take consecutive groups.  The grid is planes x chunks in one
// dimension; element offsets are 64-bit.  Chunks that lie wholly inside the plane take a branch without bounds tests.
#include "halo_common.hpp"

namespace halo {

constexpr int AN_TPB = 256;
constexpr int AN_U = 4;                        // groups per lane, all loaded before the first use
constexpr int AN_CHUNK = AN_TPB * AN_U;        // groups per workgroup
enum { AN_NONE = 0, AN_PLAIN = 1, AN_AFFINE = 2 };

typedef float an_f4 __attribute__((ext_vector_type(4)));

template <int GW> __device__ __forceinline__ void an_load(const float *p, float *v)
{
    if constexpr (GW == 4) {
        const an_f4 t = *reinterpret_cast<const an_f4 *>(p);
        v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
    } else {
        v[0] = *p;
    }
}

template <int GW> __device__ __forceinline__ void an_store(float *p, const float *v)
{
    if constexpr (GW == 4) {
        an_f4 t;
        t.x = v[0], t.y = v[1], t.z = v[2], t.w = v[3];
        *reinterpret_cast<an_f4 *>(p) = t;
    } else {
        *p = v[0];
    }
}

struct AnGeom {
    int C;
    int n;        // groups of GW elements per plane
    int cpp;      // chunks per plane
};

template <int GW, int RES, bool FULL>
__device__ __forceinline__ void an_fwd_chunk(const float *__restrict__ x, const float *__restrict__ r, float *__restrict__ y, int g0, int n,
                                             float sc, float sh, float rsc, float rsh)
{
    float xv[AN_U][GW], rv[AN_U][GW];
#pragma unroll
    for (int u = 0; u < AN_U; ++u) {
        const int g = g0 + u * AN_TPB;
        if (FULL || g < n) {
            an_load<GW>(x + (size_t)g * GW, xv[u]);
            if constexpr (RES != AN_NONE) an_load<GW>(r + (size_t)g * GW, rv[u]);
        }
    }
#pragma unroll
    for (int u = 0; u < AN_U; ++u) {
        const int g = g0 + u * AN_TPB;
        if (FULL || g < n) {
            float out[GW];
#pragma unroll
            for (int e = 0; e < GW; ++e) {
                float s = xv[u][e] * sc;
                s = s + sh;
                if constexpr (RES == AN_PLAIN) s = s + rv[u][e];
                if constexpr (RES == AN_AFFINE) {
                    float id = rv[u][e] * rsc;
                    id = id + rsh;
                    s = s + id;
                }
                out[e] = s <= 0.0f ? 0.0f : s;
            }
            an_store<GW>(y + (size_t)g * GW, out);
        }
    }
}

template <int GW, int RES>
__global__ void __launch_bounds__(AN_TPB) k_affine_relu_fwd(const float *__restrict__ x, const float *__restrict__ scale,
                                                            const float *__restrict__ shift, const float *__restrict__ r,
                                                            const float *__restrict__ r_scale, const float *__restrict__ r_shift,
                                                            float *__restrict__ y, AnGeom G)
{
    const unsigned plane = blockIdx.x / (unsigned)G.cpp;         // 32-bit: the grid has at most 2^31 - 1 workgroups
    const int chunk = (int)(blockIdx.x - plane * (unsigned)G.cpp), c = (int)(plane % (unsigned)G.C);
    const size_t po = (size_t)plane * G.n * GW;
    const float sc = scale[c], sh = shift[c];
    const float rsc = RES == AN_AFFINE ? r_scale[c] : 0.0f, rsh = RES == AN_AFFINE ? r_shift[c] : 0.0f;
    const float *rp = RES != AN_NONE ? r + po : nullptr;
    const int base = chunk * AN_CHUNK, g0 = base + (int)threadIdx.x;
    if (G.n - base >= AN_CHUNK) an_fwd_chunk<GW, RES, true>(x + po, rp, y + po, g0, G.n, sc, sh, rsc, rsh);
    else an_fwd_chunk<GW, RES, false>(x + po, rp, y + po, g0, G.n, sc, sh, rsc, rsh);
}

template <int GW, bool GX, bool GR, bool RAFF, bool FULL>
__device__ __forceinline__ void an_bwd_chunk(const float *__restrict__ g, const float *__restrict__ y, float *__restrict__ gx,
                                             float *__restrict__ gr, int g0, int n, float sc, float rsc)
{
    float gv[AN_U][GW], yv[AN_U][GW];
#pragma unroll
    for (int u = 0; u < AN_U; ++u) {
        const int q = g0 + u * AN_TPB;
        if (FULL || q < n) {
            an_load<GW>(g + (size_t)q * GW, gv[u]);
            an_load<GW>(y + (size_t)q * GW, yv[u]);
        }
    }
#pragma unroll
    for (int u = 0; u < AN_U; ++u) {
        const int q = g0 + u * AN_TPB;
        if (FULL || q < n) {
            float ox[GW], orr[GW];
#pragma unroll
            for (int e = 0; e < GW; ++e) {
                const float gp = yv[u][e] <= 0.0f ? 0.0f : gv[u][e];
                ox[e] = gp * sc;
                orr[e] = RAFF ? gp * rsc : gp;
            }
            if constexpr (GX) an_store<GW>(gx + (size_t)q * GW, ox);
            if constexpr (GR) an_store<GW>(gr + (size_t)q * GW, orr);
        }
    }
}

template <int GW, bool GX, bool GR, bool RAFF>
__global__ void __launch_bounds__(AN_TPB) k_affine_relu_bwd(const float *__restrict__ g, const float *__restrict__ y,
                                                            const float *__restrict__ scale, const float *__restrict__ r_scale,
                                                            float *__restrict__ gx, float *__restrict__ gr, AnGeom G)
{
    const unsigned plane = blockIdx.x / (unsigned)G.cpp;         // 32-bit: the grid has at most 2^31 - 1 workgroups
    const int chunk = (int)(blockIdx.x - plane * (unsigned)G.cpp), c = (int)(plane % (unsigned)G.C);
    const size_t po = (size_t)plane * G.n * GW;
    const float sc = GX ? scale[c] : 0.0f, rsc = RAFF ? r_scale[c] : 0.0f;
    float *xp = GX ? gx + po : nullptr, *rp = GR ? gr + po : nullptr;
    const int base = chunk * AN_CHUNK, g0 = base + (int)threadIdx.x;
    if (G.n - base >= AN_CHUNK) an_bwd_chunk<GW, GX, GR, RAFF, true>(g + po, y + po, xp, rp, g0, G.n, sc, rsc);
    else an_bwd_chunk<GW, GX, GR, RAFF, false>(g + po, y + po, xp, rp, g0, G.n, sc, rsc);
}

static int an_plan(const char *who, int64_t B, int64_t C, int64_t HW, bool vec, AnGeom &G, unsigned &grid)
{
    if (B < 1 || C < 1 || HW < 1) return fail(HALO_E_ARG, "%s: empty shape", who);
    if (HW > 0x7fffffffLL - AN_CHUNK || C > 0x7fffffffLL || B > 0x7fffffffLL || B * C > ((int64_t)1 << 40))
        return fail(HALO_E_UNSUPPORTED, "%s: %lld x %lld planes of %lld elements", who, (long long)B, (long long)C, (long long)HW);
    const int gw = vec ? 4 : 1;
    G.C = (int)C, G.n = (int)(HW / gw), G.cpp = (int)cdiv(HW / gw, AN_CHUNK);
    const int64_t blocks = B * C * G.cpp;
    if (blocks > 0x7fffffffLL) return fail(HALO_E_UNSUPPORTED, "%s: %lld blocks", who, (long long)blocks);
    grid = (unsigned)blocks;
    return HALO_OK;
}

static bool an_vec(int64_t HW, const void *p0, const void *p1, const void *p2, const void *p3)
{
    return HW % 4 == 0 && (((uintptr_t)p0 | (uintptr_t)p1 | (uintptr_t)p2 | (uintptr_t)p3) % 16) == 0;
}

template <int GW>
static void an_launch_fwd(int res, unsigned grid, hipStream_t st, const float *x, const float *scale, const float *shift, const float *r,
                          const float *r_scale, const float *r_shift, float *y, const AnGeom &G)
{
    const dim3 g(grid), b(AN_TPB);
    if (res == AN_NONE) hipLaunchKernelGGL((k_affine_relu_fwd<GW, AN_NONE>), g, b, 0, st, x, scale, shift, r, r_scale, r_shift, y, G);
    else if (res == AN_PLAIN) hipLaunchKernelGGL((k_affine_relu_fwd<GW, AN_PLAIN>), g, b, 0, st, x, scale, shift, r, r_scale, r_shift, y, G);
    else hipLaunchKernelGGL((k_affine_relu_fwd<GW, AN_AFFINE>), g, b, 0, st, x, scale, shift, r, r_scale, r_shift, y, G);
}

template <int GW>
static void an_launch_bwd(bool want_x, bool want_r, bool raff, unsigned grid, hipStream_t st, const float *g, const float *y,
                          const float *scale, const float *r_scale, float *gx, float *gr, const AnGeom &G)
{
    const dim3 gd(grid), b(AN_TPB);
    if (want_x && !want_r) hipLaunchKernelGGL((k_affine_relu_bwd<GW, true, false, false>), gd, b, 0, st, g, y, scale, r_scale, gx, gr, G);
    else if (!want_x && !raff) hipLaunchKernelGGL((k_affine_relu_bwd<GW, false, true, false>), gd, b, 0, st, g, y, scale, r_scale, gx, gr, G);
    else if (!want_x) hipLaunchKernelGGL((k_affine_relu_bwd<GW, false, true, true>), gd, b, 0, st, g, y, scale, r_scale, gx, gr, G);
    else if (!raff) hipLaunchKernelGGL((k_affine_relu_bwd<GW, true, true, false>), gd, b, 0, st, g, y, scale, r_scale, gx, gr, G);
    else hipLaunchKernelGGL((k_affine_relu_bwd<GW, true, true, true>), gd, b, 0, st, g, y, scale, r_scale, gx, gr, G);
}

}  // namespace halo

using namespace halo;

extern "C" int halo_affine_relu_fwd(const float *x, const float *scale, const float *shift, const float *r, const float *r_scale,
                                    const float *r_shift, float *y, int64_t B, int64_t C, int64_t HW, void *stream)
{
    const char *who = "halo_affine_relu_fwd";
    if (!x || !scale || !shift || !y) return fail(HALO_E_ARG, "%s: null argument", who);
    if ((r_scale == nullptr) != (r_shift == nullptr)) return fail(HALO_E_ARG, "%s: r_scale and r_shift are given together or not at all", who);
    if (r_scale && !r) return fail(HALO_E_ARG, "%s: r_scale without a residual operand", who);
    const bool vec = an_vec(HW, x, y, r, nullptr);
    AnGeom G;
    unsigned grid;
    if (int rc = an_plan(who, B, C, HW, vec, G, grid)) return rc;
    const int res = !r ? AN_NONE : r_scale ? AN_AFFINE : AN_PLAIN;
    if (vec) an_launch_fwd<4>(res, grid, (hipStream_t)stream, x, scale, shift, r, r_scale, r_shift, y, G);
    else an_launch_fwd<1>(res, grid, (hipStream_t)stream, x, scale, shift, r, r_scale, r_shift, y, G);
    return check_launch(who);
}

extern "C" int halo_affine_relu_bwd(const float *g, const float *y, const float *scale, const float *r_scale, float *g_x, float *g_r,
                                    int64_t B, int64_t C, int64_t HW, void *stream)
{
    const char *who = "halo_affine_relu_bwd";
    if (!g || !y) return fail(HALO_E_ARG, "%s: null argument", who);
    if (!g_x && !g_r) return fail(HALO_E_ARG, "%s: neither g_x nor g_r is asked for", who);
    if (g_x && !scale) return fail(HALO_E_ARG, "%s: g_x needs scale", who);
    const bool vec = an_vec(HW, g, y, g_x, g_r);
    AnGeom G;
    unsigned grid;
    if (int rc = an_plan(who, B, C, HW, vec, G, grid)) return rc;
    const bool raff = g_r && r_scale;
    if (vec) an_launch_bwd<4>(g_x != nullptr, g_r != nullptr, raff, grid, (hipStream_t)stream, g, y, scale, r_scale, g_x, g_r, G);
    else an_launch_bwd<1>(g_x != nullptr, g_r != nullptr, raff, grid, (hipStream_t)stream, g, y, scale, r_scale, g_x, g_r, G);
    return check_launch(who);
}
