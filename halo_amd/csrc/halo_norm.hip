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
// halo_fork_affine_relu_bwd is the same backward for a y that two consumers read (the next block's conv1 and its identity):
// g = fl(g_a + g_b), the one float32 add with which autograd accumulates two gradients, taken inside the pass.
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
#include "halo_norm_dev.hpp"

namespace halo {

constexpr int AN_TPB = 256;
constexpr int AN_U = 4;                        // groups per lane, all loaded before the first use
constexpr int AN_CHUNK = AN_TPB * AN_U;        // groups per workgroup
enum { AN_NONE = 0, AN_PLAIN = 1, AN_AFFINE = 2 };

// an_f4, an_load, an_store, an_affine and an_relu live in halo_norm_dev.hpp (halo_maxpool.hip runs the same statements)

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
                float s = an_affine(xv[u][e], sc, sh);
                if constexpr (RES == AN_PLAIN) s = s + rv[u][e];
                if constexpr (RES == AN_AFFINE) s = s + an_affine(rv[u][e], rsc, rsh);
                out[e] = an_relu(s);
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

// FORK: two gradients arrive at y (a block output that the next block reads twice); their sum is autograd's accumulation, one
// float32 add, and the statements behind it are the same
template <int GW, bool GX, bool GR, bool RAFF, bool FORK, bool FULL>
__device__ __forceinline__ void an_bwd_chunk(const float *__restrict__ g, const float *__restrict__ g2, const float *__restrict__ y,
                                             float *__restrict__ gx, float *__restrict__ gr, int g0, int n, float sc, float rsc)
{
    float gv[AN_U][GW], hv[AN_U][GW], yv[AN_U][GW];
#pragma unroll
    for (int u = 0; u < AN_U; ++u) {
        const int q = g0 + u * AN_TPB;
        if (FULL || q < n) {
            an_load<GW>(g + (size_t)q * GW, gv[u]);
            if constexpr (FORK) an_load<GW>(g2 + (size_t)q * GW, hv[u]);
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
                float gs = gv[u][e];
                if constexpr (FORK) gs = gs + hv[u][e];
                const float gp = yv[u][e] <= 0.0f ? 0.0f : gs;
                ox[e] = gp * sc;
                orr[e] = RAFF ? gp * rsc : gp;
            }
            if constexpr (GX) an_store<GW>(gx + (size_t)q * GW, ox);
            if constexpr (GR) an_store<GW>(gr + (size_t)q * GW, orr);
        }
    }
}

template <int GW, bool GX, bool GR, bool RAFF, bool FORK>
__global__ void __launch_bounds__(AN_TPB) k_affine_relu_bwd(const float *__restrict__ g, const float *__restrict__ g2, const float *__restrict__ y,
                                                            const float *__restrict__ scale, const float *__restrict__ r_scale,
                                                            float *__restrict__ gx, float *__restrict__ gr, AnGeom G)
{
    const unsigned plane = blockIdx.x / (unsigned)G.cpp;         // 32-bit: the grid has at most 2^31 - 1 workgroups
    const int chunk = (int)(blockIdx.x - plane * (unsigned)G.cpp), c = (int)(plane % (unsigned)G.C);
    const size_t po = (size_t)plane * G.n * GW;
    const float sc = GX ? scale[c] : 0.0f, rsc = RAFF ? r_scale[c] : 0.0f;
    const float *hp = FORK ? g2 + po : nullptr;
    float *xp = GX ? gx + po : nullptr, *rp = GR ? gr + po : nullptr;
    const int base = chunk * AN_CHUNK, g0 = base + (int)threadIdx.x;
    if (G.n - base >= AN_CHUNK) an_bwd_chunk<GW, GX, GR, RAFF, FORK, true>(g + po, hp, y + po, xp, rp, g0, G.n, sc, rsc);
    else an_bwd_chunk<GW, GX, GR, RAFF, FORK, false>(g + po, hp, y + po, xp, rp, g0, G.n, sc, rsc);
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

template <int GW, bool FORK>
static void an_launch_bwd(bool want_x, bool want_r, bool raff, unsigned grid, hipStream_t st, const float *g, const float *g2, const float *y,
                          const float *scale, const float *r_scale, float *gx, float *gr, const AnGeom &G)
{
    const dim3 gd(grid), b(AN_TPB);
    if (want_x && !want_r) hipLaunchKernelGGL((k_affine_relu_bwd<GW, true, false, false, FORK>), gd, b, 0, st, g, g2, y, scale, r_scale, gx, gr, G);
    else if (!want_x && !raff) hipLaunchKernelGGL((k_affine_relu_bwd<GW, false, true, false, FORK>), gd, b, 0, st, g, g2, y, scale, r_scale, gx, gr, G);
    else if (!want_x) hipLaunchKernelGGL((k_affine_relu_bwd<GW, false, true, true, FORK>), gd, b, 0, st, g, g2, y, scale, r_scale, gx, gr, G);
    else if (!raff) hipLaunchKernelGGL((k_affine_relu_bwd<GW, true, true, false, FORK>), gd, b, 0, st, g, g2, y, scale, r_scale, gx, gr, G);
    else hipLaunchKernelGGL((k_affine_relu_bwd<GW, true, true, true, FORK>), gd, b, 0, st, g, g2, y, scale, r_scale, gx, gr, G);
}


// ---------------------------------------------------------------- norm + ReLU + Dropout2d: the tail of a separable block behind a dropout
// nn.Dropout2d multiplies every plane (b, c) by one number m = mask[b * C + c], 0 or fl32(1 / (1 - p)), drawn by the caller.  The
// same plane / chunk walk with that one more block-uniform operand:
//
//   y   = fl(relu(fl(fl(x * scale[c]) + shift[c])) * m)         a NaN stays a NaN; inf * 0 is the stock chain's NaN
//   g_x = y <= 0 ? 0 : fl(fl(g * m) * scale[c])                 a NaN y lets g through
//
// m >= 0, so in a kept plane y > 0 exactly where the ReLU's output is, and the saved y stands in for it.  In a dropped plane y is 0
// or NaN and either branch gives a zero for a finite g: such a plane's workgroups write zeros and read neither g nor y.  That is
// the one deviation from autograd, which computes fl(fl(g * 0) * scale) there: a NaN for a non-finite g.

template <int GW, bool FULL>
__device__ __forceinline__ void an_mask_fwd_chunk(const float *__restrict__ x, float *__restrict__ y, int g0, int n, float sc, float sh, float m)
{
    float xv[AN_U][GW];
#pragma unroll
    for (int u = 0; u < AN_U; ++u) {
        const int g = g0 + u * AN_TPB;
        if (FULL || g < n) an_load<GW>(x + (size_t)g * GW, xv[u]);
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
                s = s <= 0.0f ? 0.0f : s;
                out[e] = s * m;
            }
            an_store<GW>(y + (size_t)g * GW, out);
        }
    }
}

template <int GW>
__global__ void __launch_bounds__(AN_TPB) k_affine_relu_mask_fwd(const float *__restrict__ x, const float *__restrict__ scale,
                                                                 const float *__restrict__ shift, const float *__restrict__ mask,
                                                                 float *__restrict__ y, AnGeom G)
{
    const unsigned plane = blockIdx.x / (unsigned)G.cpp;         // 32-bit: the grid has at most 2^31 - 1 workgroups
    const int chunk = (int)(blockIdx.x - plane * (unsigned)G.cpp), c = (int)(plane % (unsigned)G.C);
    const size_t po = (size_t)plane * G.n * GW;
    const float sc = scale[c], sh = shift[c], m = mask[plane];
    const int base = chunk * AN_CHUNK, g0 = base + (int)threadIdx.x;
    if (G.n - base >= AN_CHUNK) an_mask_fwd_chunk<GW, true>(x + po, y + po, g0, G.n, sc, sh, m);
    else an_mask_fwd_chunk<GW, false>(x + po, y + po, g0, G.n, sc, sh, m);
}

template <int GW, bool KEPT, bool FULL>
__device__ __forceinline__ void an_mask_bwd_chunk(const float *__restrict__ g, const float *__restrict__ y, float *__restrict__ gx, int g0, int n,
                                                  float sc, float m)
{
    float gv[AN_U][GW], yv[AN_U][GW];
    if constexpr (KEPT) {
#pragma unroll
        for (int u = 0; u < AN_U; ++u) {
            const int q = g0 + u * AN_TPB;
            if (FULL || q < n) {
                an_load<GW>(g + (size_t)q * GW, gv[u]);
                an_load<GW>(y + (size_t)q * GW, yv[u]);
            }
        }
    }
#pragma unroll
    for (int u = 0; u < AN_U; ++u) {
        const int q = g0 + u * AN_TPB;
        if (FULL || q < n) {
            float ox[GW];
#pragma unroll
            for (int e = 0; e < GW; ++e) {
                if constexpr (KEPT) {
                    float t = gv[u][e] * m;
                    t = t * sc;
                    ox[e] = yv[u][e] <= 0.0f ? 0.0f : t;
                } else {
                    ox[e] = 0.0f;
                }
            }
            an_store<GW>(gx + (size_t)q * GW, ox);
        }
    }
}

template <int GW>
__global__ void __launch_bounds__(AN_TPB) k_affine_relu_mask_bwd(const float *__restrict__ g, const float *__restrict__ y,
                                                                 const float *__restrict__ scale, const float *__restrict__ mask,
                                                                 float *__restrict__ gx, AnGeom G)
{
    const unsigned plane = blockIdx.x / (unsigned)G.cpp;         // 32-bit: the grid has at most 2^31 - 1 workgroups
    const int chunk = (int)(blockIdx.x - plane * (unsigned)G.cpp), c = (int)(plane % (unsigned)G.C);
    const size_t po = (size_t)plane * G.n * GW;
    const float sc = scale[c], m = mask[plane];
    const int base = chunk * AN_CHUNK, g0 = base + (int)threadIdx.x;
    const bool full = G.n - base >= AN_CHUNK;
    if (m != 0.0f) {                                             // block-uniform: the whole workgroup lies in one plane
        if (full) an_mask_bwd_chunk<GW, true, true>(g + po, y + po, gx + po, g0, G.n, sc, m);
        else an_mask_bwd_chunk<GW, true, false>(g + po, y + po, gx + po, g0, G.n, sc, m);
    } else {
        if (full) an_mask_bwd_chunk<GW, false, true>(g + po, y + po, gx + po, g0, G.n, sc, m);
        else an_mask_bwd_chunk<GW, false, false>(g + po, y + po, gx + po, g0, G.n, sc, m);
    }
}


// ---------------------------------------------------------------- norm + ReLU + Dropout2d with BOTH tensors kept
// The Euclidean v3+ head's old decoder layout returns the tensor in front of its nn.Dropout2d and feeds the one behind it to the
// classifier conv, so the pass has two outputs and its backward two incoming gradients, either of which may be absent:
//
//   y   = relu(fl(fl(x * scale[c]) + shift[c]))                 halo_affine_relu_fwd's statements
//   z   = fl(y * m)                                             m = mask[b * C + c]; inf * 0 is the stock chain's NaN
//   g   = g_y,  fl(g_z * m)  or  fl(g_y + fl(g_z * m))          the product first, then autograd's accumulation
//   g_x = fl((y <= 0 ? 0 : g) * scale[c])                       a NaN y lets g through
//
// y is the ReLU's own output here, so the gate is autograd's in every plane.  In a dropped plane (m == 0) g_z is not read: its term
// is taken as 0, which it is for a finite g_z (autograd has a NaN for a non-finite one: section 18's deviation).  With g_y absent
// such a plane's workgroups write zeros and read nothing.

template <int GW, bool FULL>
__device__ __forceinline__ void an_pair_fwd_chunk(const float *__restrict__ x, float *__restrict__ y, float *__restrict__ z, int g0, int n,
                                                  float sc, float sh, float m)
{
    float xv[AN_U][GW];
#pragma unroll
    for (int u = 0; u < AN_U; ++u) {
        const int g = g0 + u * AN_TPB;
        if (FULL || g < n) an_load<GW>(x + (size_t)g * GW, xv[u]);
    }
#pragma unroll
    for (int u = 0; u < AN_U; ++u) {
        const int g = g0 + u * AN_TPB;
        if (FULL || g < n) {
            float oy[GW], oz[GW];
#pragma unroll
            for (int e = 0; e < GW; ++e) {
                float s = xv[u][e] * sc;
                s = s + sh;
                oy[e] = s <= 0.0f ? 0.0f : s;
                oz[e] = oy[e] * m;
            }
            an_store<GW>(y + (size_t)g * GW, oy);
            an_store<GW>(z + (size_t)g * GW, oz);
        }
    }
}

template <int GW>
__global__ void __launch_bounds__(AN_TPB) k_affine_relu_pair_fwd(const float *__restrict__ x, const float *__restrict__ scale,
                                                                 const float *__restrict__ shift, const float *__restrict__ mask,
                                                                 float *__restrict__ y, float *__restrict__ z, AnGeom G)
{
    const unsigned plane = blockIdx.x / (unsigned)G.cpp;         // 32-bit: the grid has at most 2^31 - 1 workgroups
    const int chunk = (int)(blockIdx.x - plane * (unsigned)G.cpp), c = (int)(plane % (unsigned)G.C);
    const size_t po = (size_t)plane * G.n * GW;
    const float sc = scale[c], sh = shift[c], m = mask[plane];
    const int base = chunk * AN_CHUNK, g0 = base + (int)threadIdx.x;
    if (G.n - base >= AN_CHUNK) an_pair_fwd_chunk<GW, true>(x + po, y + po, z + po, g0, G.n, sc, sh, m);
    else an_pair_fwd_chunk<GW, false>(x + po, y + po, z + po, g0, G.n, sc, sh, m);
}

// GY / GZ: which of the two gradients this workgroup reads (neither: it writes zeros)
template <int GW, bool GY, bool GZ, bool FULL>
__device__ __forceinline__ void an_pair_bwd_chunk(const float *__restrict__ gy, const float *__restrict__ gz, const float *__restrict__ y,
                                                  float *__restrict__ gx, int g0, int n, float sc, float m)
{
    float av[AN_U][GW], bv[AN_U][GW], yv[AN_U][GW];
    if constexpr (GY || GZ) {
#pragma unroll
        for (int u = 0; u < AN_U; ++u) {
            const int q = g0 + u * AN_TPB;
            if (FULL || q < n) {
                if constexpr (GY) an_load<GW>(gy + (size_t)q * GW, av[u]);
                if constexpr (GZ) an_load<GW>(gz + (size_t)q * GW, bv[u]);
                an_load<GW>(y + (size_t)q * GW, yv[u]);
            }
        }
    }
#pragma unroll
    for (int u = 0; u < AN_U; ++u) {
        const int q = g0 + u * AN_TPB;
        if (FULL || q < n) {
            float ox[GW];
#pragma unroll
            for (int e = 0; e < GW; ++e) {
                if constexpr (GY || GZ) {
                    float t;
                    if constexpr (GZ) {
                        t = bv[u][e] * m;
                        if constexpr (GY) t = av[u][e] + t;
                    } else {
                        t = av[u][e];
                    }
                    t = yv[u][e] <= 0.0f ? 0.0f : t;
                    ox[e] = t * sc;
                } else {
                    ox[e] = 0.0f;
                }
            }
            an_store<GW>(gx + (size_t)q * GW, ox);
        }
    }
}

template <int GW, bool GY, bool GZ>
__global__ void __launch_bounds__(AN_TPB) k_affine_relu_pair_bwd(const float *__restrict__ gy, const float *__restrict__ gz,
                                                                 const float *__restrict__ y, const float *__restrict__ scale,
                                                                 const float *__restrict__ mask, float *__restrict__ gx, AnGeom G)
{
    const unsigned plane = blockIdx.x / (unsigned)G.cpp;         // 32-bit: the grid has at most 2^31 - 1 workgroups
    const int chunk = (int)(blockIdx.x - plane * (unsigned)G.cpp), c = (int)(plane % (unsigned)G.C);
    const size_t po = (size_t)plane * G.n * GW;
    const float sc = scale[c], m = GZ ? mask[plane] : 1.0f;
    const float *ap = GY ? gy + po : nullptr, *bp = GZ ? gz + po : nullptr;
    const int base = chunk * AN_CHUNK, g0 = base + (int)threadIdx.x;
    const bool full = G.n - base >= AN_CHUNK;
    if (!GZ || m != 0.0f) {                                      // block-uniform: the whole workgroup lies in one plane
        if (full) an_pair_bwd_chunk<GW, GY, GZ, true>(ap, bp, y + po, gx + po, g0, G.n, sc, m);
        else an_pair_bwd_chunk<GW, GY, GZ, false>(ap, bp, y + po, gx + po, g0, G.n, sc, m);
    } else {                                                     // a dropped plane: g_z's term is 0
        if (full) an_pair_bwd_chunk<GW, GY, false, true>(ap, bp, y + po, gx + po, g0, G.n, sc, m);
        else an_pair_bwd_chunk<GW, GY, false, false>(ap, bp, y + po, gx + po, g0, G.n, sc, m);
    }
}

template <int GW>
static void an_launch_pair_bwd(bool has_y, bool has_z, unsigned grid, hipStream_t st, const float *gy, const float *gz, const float *y,
                               const float *scale, const float *mask, float *gx, const AnGeom &G)
{
    const dim3 gd(grid), b(AN_TPB);
    if (has_y && has_z) hipLaunchKernelGGL((k_affine_relu_pair_bwd<GW, true, true>), gd, b, 0, st, gy, gz, y, scale, mask, gx, G);
    else if (has_z) hipLaunchKernelGGL((k_affine_relu_pair_bwd<GW, false, true>), gd, b, 0, st, gy, gz, y, scale, mask, gx, G);
    else hipLaunchKernelGGL((k_affine_relu_pair_bwd<GW, true, false>), gd, b, 0, st, gy, gz, y, scale, mask, gx, G);
}


// ---------------------------------------------------------------- the image-pooling branch of the v3+ bottleneck as a border-aware bias
// The last Cg input channels of the bottleneck's 3x3 zero-padded conv are constant planes v[b,c] (the pooled branch, broadcast), so
// their share of the conv output takes 9 values per (image, output channel): 3 row classes (top row, interior, bottom row) x 3
// column classes, by which taps fall inside the map.
//
//   S[b,o,k]       = sum_c Wg[o,c,k] v[b,c]                                float64 products and sums, a fixed reduction shape
//   T[b,o,rc,cc]   = fl32(sum_{ky in R(rc)} sum_{kx in C(cc)} S[b,o,ky,kx])  float64, ky then kx ascending, rounded once
//                    R(top) = {1,2}, R(interior) = {0,1,2}, R(bottom) = {0,1}; C likewise
//   y              = relu(fl(fl(fl(z + T[b,o,rc(i),cc(j)]) scale[o]) + shift[o]))
//   gp = y <= 0 ? 0 : g;   g_z = fl(gp scale[o]);   g_T[b,o,rc,cc] = sum over the class's pixels of g_z   (float64)
//
// The epilogue is k_affine_relu's plane / chunk walk; scale, shift and the plane's table of 9 entries are block-uniform.  The 16-byte
// route needs W % 4 == 0, so that a group of four lies in one row.  The class sums: every lane adds its elements into 9 float64
// accumulators in element order, a workgroup adds its lanes in a fixed LDS tree and writes its own row of the slab, and
// k_pool_fold_finish adds a plane's rows in ascending order: no atomics, the same bits on every call and every stream.

constexpr int PF_TPB = 256;                    // lanes of the fold pass: channel c goes to lane c % PF_TPB

struct PfGeom {
    AnGeom a;
    int H, W;
};

// the LDS tree of both reductions: 9 float64 per lane, halving strides
__device__ __forceinline__ void pf_tree(double (*red)[PF_TPB], const double *acc, int t)
{
#pragma unroll
    for (int k = 0; k < 9; ++k) red[k][t] = acc[k];
    __syncthreads();
    for (int s = PF_TPB / 2; s > 0; s >>= 1) {
        if (t < s) {
#pragma unroll
            for (int k = 0; k < 9; ++k) red[k][t] += red[k][t + s];
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(PF_TPB) k_pool_fold_table(const float *__restrict__ w, const float *__restrict__ v, float *__restrict__ T,
                                                            int Co, int Cg, int64_t c_off, int64_t row_stride)
{
    __shared__ double red[9][PF_TPB];
    const int b = (int)(blockIdx.x / (unsigned)Co), o = (int)(blockIdx.x - (unsigned)b * (unsigned)Co), t = (int)threadIdx.x;
    const float *wr = w + (size_t)o * (size_t)row_stride + (size_t)c_off * 9;
    const float *vb = v + (size_t)b * Cg;
    double acc[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int c = t; c < Cg; c += PF_TPB) {
        const double vc = (double)vb[c];
#pragma unroll
        for (int k = 0; k < 9; ++k) acc[k] += (double)wr[(size_t)c * 9 + k] * vc;
    }
    pf_tree(red, acc, t);
    if (t < 9) {
        const int rc = t / 3, cc = t - rc * 3;
        const int y0 = rc == 0 ? 1 : 0, y1 = rc == 2 ? 1 : 2, x0 = cc == 0 ? 1 : 0, x1 = cc == 2 ? 1 : 2;
        double s = 0.0;
        for (int ky = y0; ky <= y1; ++ky)
            for (int kx = x0; kx <= x1; ++kx) s += red[ky * 3 + kx][0];
        T[(size_t)blockIdx.x * 9 + t] = (float)s;
    }
}

// row class of a row: 0 top, 1 interior, 2 bottom
__device__ __forceinline__ int pf_rc(int row, int H) { return row == 0 ? 0 : row == H - 1 ? 2 : 1; }

template <int GW, bool FULL>
__device__ __forceinline__ void pf_fwd_chunk(const float *__restrict__ z, float *__restrict__ y, int g0, int n, int H, int W, float sc, float sh,
                                             const float *__restrict__ t)
{
    float zv[AN_U][GW];
#pragma unroll
    for (int u = 0; u < AN_U; ++u) {
        const int g = g0 + u * AN_TPB;
        if (FULL || g < n) an_load<GW>(z + (size_t)g * GW, zv[u]);
    }
#pragma unroll
    for (int u = 0; u < AN_U; ++u) {
        const int g = g0 + u * AN_TPB;
        if (FULL || g < n) {
            const unsigned e0 = (unsigned)g * GW, row = e0 / (unsigned)W, col = e0 - row * (unsigned)W;
            const float *tr = t + pf_rc((int)row, H) * 3;      // the plane's 36-byte table stays in the cache; a copy in registers
            const float t0 = tr[0], t1 = tr[1], t2 = tr[2];    // picked by selects comes back from the compiler as an LDS array
            float out[GW];
#pragma unroll
            for (int e = 0; e < GW; ++e) {
                const int c = (int)col + e;
                float s = zv[u][e] + (c == 0 ? t0 : c == W - 1 ? t2 : t1);
                s = s * sc;
                s = s + sh;
                out[e] = s <= 0.0f ? 0.0f : s;
            }
            an_store<GW>(y + (size_t)g * GW, out);
        }
    }
}

template <int GW>
__global__ void __launch_bounds__(AN_TPB) k_pool_fold_fwd(const float *__restrict__ z, const float *__restrict__ T, const float *__restrict__ scale,
                                                          const float *__restrict__ shift, float *__restrict__ y, PfGeom G)
{
    const unsigned plane = blockIdx.x / (unsigned)G.a.cpp;
    const int chunk = (int)(blockIdx.x - plane * (unsigned)G.a.cpp), c = (int)(plane % (unsigned)G.a.C);
    const size_t po = (size_t)plane * G.a.n * GW;
    const float sc = scale[c], sh = shift[c];
    const float *t = T + (size_t)plane * 9;
    const int base = chunk * AN_CHUNK, g0 = base + (int)threadIdx.x;
    if (G.a.n - base >= AN_CHUNK) pf_fwd_chunk<GW, true>(z + po, y + po, g0, G.a.n, G.H, G.W, sc, sh, t);
    else pf_fwd_chunk<GW, false>(z + po, y + po, g0, G.a.n, G.H, G.W, sc, sh, t);
}

template <int GW, bool GZ, bool SUMS, bool FULL>
__device__ __forceinline__ void pf_bwd_chunk(const float *__restrict__ g, const float *__restrict__ y, float *__restrict__ gz, int g0, int n, int H,
                                             int W, float sc, double *acc)
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
            const unsigned e0 = (unsigned)q * GW, row = e0 / (unsigned)W, col = e0 - row * (unsigned)W;
            const int rc = pf_rc((int)row, H);
            float ox[GW];
#pragma unroll
            for (int e = 0; e < GW; ++e) {
                const float gp = yv[u][e] <= 0.0f ? 0.0f : gv[u][e];
                ox[e] = gp * sc;
                if constexpr (SUMS) {
                    const int c = (int)col + e, cls = rc * 3 + (c == 0 ? 0 : c == W - 1 ? 2 : 1);
                    const double d = (double)ox[e];
#pragma unroll
                    for (int k = 0; k < 9; ++k) acc[k] += cls == k ? d : 0.0;
                }
            }
            if constexpr (GZ) an_store<GW>(gz + (size_t)q * GW, ox);
        }
    }
}

template <int GW, bool GZ, bool SUMS>
__global__ void __launch_bounds__(AN_TPB) k_pool_fold_bwd(const float *__restrict__ g, const float *__restrict__ y, const float *__restrict__ scale,
                                                          float *__restrict__ gz, double *__restrict__ slab, PfGeom G)
{
    static_assert(AN_TPB == PF_TPB, "pf_tree is sized for the plane walk's workgroup");
    __shared__ double red[SUMS ? 9 : 1][PF_TPB];
    const unsigned plane = blockIdx.x / (unsigned)G.a.cpp;
    const int chunk = (int)(blockIdx.x - plane * (unsigned)G.a.cpp), c = (int)(plane % (unsigned)G.a.C);
    const size_t po = (size_t)plane * G.a.n * GW;
    const float sc = scale[c];
    float *zp = GZ ? gz + po : nullptr;
    double acc[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const int base = chunk * AN_CHUNK, g0 = base + (int)threadIdx.x;
    if (G.a.n - base >= AN_CHUNK) pf_bwd_chunk<GW, GZ, SUMS, true>(g + po, y + po, zp, g0, G.a.n, G.H, G.W, sc, acc);
    else pf_bwd_chunk<GW, GZ, SUMS, false>(g + po, y + po, zp, g0, G.a.n, G.H, G.W, sc, acc);
    if constexpr (SUMS) {
        pf_tree(red, acc, (int)threadIdx.x);
        if (threadIdx.x < 9) slab[(size_t)blockIdx.x * 9 + threadIdx.x] = red[threadIdx.x][0];
    }
}

// g_T[plane][k] = the plane's slab rows added in ascending chunk order
__global__ void __launch_bounds__(PF_TPB) k_pool_fold_finish(const double *__restrict__ slab, double *__restrict__ gT, int64_t entries, int cpp)
{
    const int64_t i = (int64_t)blockIdx.x * PF_TPB + threadIdx.x;
    if (i >= entries) return;
    const int64_t plane = i / 9;
    const int k = (int)(i - plane * 9);
    double s = 0.0;
    for (int ch = 0; ch < cpp; ++ch) s += slab[((size_t)plane * cpp + ch) * 9 + k];
    gT[i] = s;
}

static int pf_plan(const char *who, int64_t B, int64_t Co, int64_t H, int64_t W, bool vec, PfGeom &G, unsigned &grid)
{
    if (B < 1 || Co < 1 || H < 1 || W < 1) return fail(HALO_E_ARG, "%s: empty shape", who);
    if (H < 2 || W < 2) return fail(HALO_E_ARG, "%s: a %lld x %lld map has no separate border classes (H, W >= 2)", who, (long long)H, (long long)W);
    if (H > 0x7fffffffLL || W > 0x7fffffffLL || H * W > 0x7fffffffLL - AN_CHUNK)
        return fail(HALO_E_UNSUPPORTED, "%s: %lld x %lld planes of %lld x %lld", who, (long long)B, (long long)Co, (long long)H, (long long)W);
    if (int rc = an_plan(who, B, Co, H * W, vec, G.a, grid)) return rc;
    G.H = (int)H, G.W = (int)W;
    return HALO_OK;
}

static bool pf_vec(int64_t W, const void *p0, const void *p1, const void *p2)
{
    return W % 4 == 0 && (((uintptr_t)p0 | (uintptr_t)p1 | (uintptr_t)p2) % 16) == 0;
}

// rows of the slab per plane: sized for the one-element route, which cuts a plane into the most chunks
static int64_t pf_slab_rows(int64_t H, int64_t W) { return cdiv(H * W, AN_CHUNK); }

template <int GW>
static void pf_launch_bwd(bool want_z, bool sums, unsigned grid, hipStream_t st, const float *g, const float *y, const float *scale, float *gz,
                          double *slab, const PfGeom &G)
{
    const dim3 gd(grid), b(AN_TPB);
    if (want_z && sums) hipLaunchKernelGGL((k_pool_fold_bwd<GW, true, true>), gd, b, 0, st, g, y, scale, gz, slab, G);
    else if (want_z) hipLaunchKernelGGL((k_pool_fold_bwd<GW, true, false>), gd, b, 0, st, g, y, scale, gz, slab, G);
    else hipLaunchKernelGGL((k_pool_fold_bwd<GW, false, true>), gd, b, 0, st, g, y, scale, gz, slab, G);
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

// both entries of the block tail's backward: g_b is the second gradient of halo_fork_affine_relu_bwd, null for the single one
static int an_bwd_entry(const char *who, const float *g, const float *g_b, const float *y, const float *scale, const float *r_scale, float *g_x,
                        float *g_r, int64_t B, int64_t C, int64_t HW, void *stream)
{
    if (!g_x && !g_r) return fail(HALO_E_ARG, "%s: neither g_x nor g_r is asked for", who);
    if (g_x && !scale) return fail(HALO_E_ARG, "%s: g_x needs scale", who);
    const bool vec = an_vec(HW, g, y, g_x, g_r) && (uintptr_t)g_b % 16 == 0;
    AnGeom G;
    unsigned grid;
    if (int rc = an_plan(who, B, C, HW, vec, G, grid)) return rc;
    const bool raff = g_r && r_scale, wx = g_x != nullptr, wr = g_r != nullptr;
    hipStream_t st = (hipStream_t)stream;
    if (g_b) {
        if (vec) an_launch_bwd<4, true>(wx, wr, raff, grid, st, g, g_b, y, scale, r_scale, g_x, g_r, G);
        else an_launch_bwd<1, true>(wx, wr, raff, grid, st, g, g_b, y, scale, r_scale, g_x, g_r, G);
    } else {
        if (vec) an_launch_bwd<4, false>(wx, wr, raff, grid, st, g, g_b, y, scale, r_scale, g_x, g_r, G);
        else an_launch_bwd<1, false>(wx, wr, raff, grid, st, g, g_b, y, scale, r_scale, g_x, g_r, G);
    }
    return check_launch(who);
}

extern "C" int halo_affine_relu_bwd(const float *g, const float *y, const float *scale, const float *r_scale, float *g_x, float *g_r,
                                    int64_t B, int64_t C, int64_t HW, void *stream)
{
    const char *who = "halo_affine_relu_bwd";
    if (!g || !y) return fail(HALO_E_ARG, "%s: null argument", who);
    return an_bwd_entry(who, g, nullptr, y, scale, r_scale, g_x, g_r, B, C, HW, stream);
}

extern "C" int halo_fork_affine_relu_bwd(const float *g_a, const float *g_b, const float *y, const float *scale, const float *r_scale,
                                         float *g_x, float *g_r, int64_t B, int64_t C, int64_t HW, void *stream)
{
    const char *who = "halo_fork_affine_relu_bwd";
    if (!g_a || !g_b || !y) return fail(HALO_E_ARG, "%s: null argument", who);
    return an_bwd_entry(who, g_a, g_b, y, scale, r_scale, g_x, g_r, B, C, HW, stream);
}

extern "C" int halo_masked_affine_relu_fwd(const float *x, const float *scale, const float *shift, const float *mask, float *y, int64_t B,
                                           int64_t C, int64_t HW, void *stream)
{
    const char *who = "halo_masked_affine_relu_fwd";
    if (!x || !scale || !shift || !mask || !y) return fail(HALO_E_ARG, "%s: null argument", who);
    const bool vec = an_vec(HW, x, y, nullptr, nullptr);
    AnGeom G;
    unsigned grid;
    if (int rc = an_plan(who, B, C, HW, vec, G, grid)) return rc;
    if (vec) hipLaunchKernelGGL((k_affine_relu_mask_fwd<4>), dim3(grid), dim3(AN_TPB), 0, (hipStream_t)stream, x, scale, shift, mask, y, G);
    else hipLaunchKernelGGL((k_affine_relu_mask_fwd<1>), dim3(grid), dim3(AN_TPB), 0, (hipStream_t)stream, x, scale, shift, mask, y, G);
    return check_launch(who);
}

extern "C" int halo_masked_affine_relu_bwd(const float *g, const float *y, const float *scale, const float *mask, float *g_x, int64_t B,
                                           int64_t C, int64_t HW, void *stream)
{
    const char *who = "halo_masked_affine_relu_bwd";
    if (!g || !y || !scale || !mask || !g_x) return fail(HALO_E_ARG, "%s: null argument", who);
    const bool vec = an_vec(HW, g, y, g_x, nullptr);
    AnGeom G;
    unsigned grid;
    if (int rc = an_plan(who, B, C, HW, vec, G, grid)) return rc;
    if (vec) hipLaunchKernelGGL((k_affine_relu_mask_bwd<4>), dim3(grid), dim3(AN_TPB), 0, (hipStream_t)stream, g, y, scale, mask, g_x, G);
    else hipLaunchKernelGGL((k_affine_relu_mask_bwd<1>), dim3(grid), dim3(AN_TPB), 0, (hipStream_t)stream, g, y, scale, mask, g_x, G);
    return check_launch(who);
}

extern "C" int halo_dropout_pair_fwd(const float *x, const float *scale, const float *shift, const float *mask, float *y, float *z, int64_t B,
                                     int64_t C, int64_t HW, void *stream)
{
    const char *who = "halo_dropout_pair_fwd";
    if (!x || !scale || !shift || !mask || !y || !z) return fail(HALO_E_ARG, "%s: null argument", who);
    const bool vec = an_vec(HW, x, y, z, nullptr);
    AnGeom G;
    unsigned grid;
    if (int rc = an_plan(who, B, C, HW, vec, G, grid)) return rc;
    if (vec) hipLaunchKernelGGL((k_affine_relu_pair_fwd<4>), dim3(grid), dim3(AN_TPB), 0, (hipStream_t)stream, x, scale, shift, mask, y, z, G);
    else hipLaunchKernelGGL((k_affine_relu_pair_fwd<1>), dim3(grid), dim3(AN_TPB), 0, (hipStream_t)stream, x, scale, shift, mask, y, z, G);
    return check_launch(who);
}

extern "C" int halo_dropout_pair_bwd(const float *g_y, const float *g_z, const float *y, const float *scale, const float *mask, float *g_x,
                                     int64_t B, int64_t C, int64_t HW, void *stream)
{
    const char *who = "halo_dropout_pair_bwd";
    if (!y || !scale || !mask || !g_x) return fail(HALO_E_ARG, "%s: null argument", who);
    if (!g_y && !g_z) return fail(HALO_E_ARG, "%s: null argument: neither g_y nor g_z is given", who);
    const bool vec = an_vec(HW, g_y, g_z, y, g_x);
    AnGeom G;
    unsigned grid;
    if (int rc = an_plan(who, B, C, HW, vec, G, grid)) return rc;
    if (vec) an_launch_pair_bwd<4>(g_y != nullptr, g_z != nullptr, grid, (hipStream_t)stream, g_y, g_z, y, scale, mask, g_x, G);
    else an_launch_pair_bwd<1>(g_y != nullptr, g_z != nullptr, grid, (hipStream_t)stream, g_y, g_z, y, scale, mask, g_x, G);
    return check_launch(who);
}

extern "C" size_t halo_pool_fold_workspace_bytes(int64_t B, int64_t Co, int64_t H, int64_t W)
{
    // the shapes pf_plan accepts, each factor bounded before it enters a product: 0 for anything a launch would refuse
    if (B < 1 || Co < 1 || H < 2 || W < 2 || H > 0x7fffffffLL || W > 0x7fffffffLL || B > 0x7fffffffLL || Co > 0x7fffffffLL) return 0;
    if (H * W > 0x7fffffffLL - AN_CHUNK || B * Co > 0x7fffffffLL) return 0;
    const int64_t rows = pf_slab_rows(H, W);                                  // at most 2^21
    if (B * Co > 0x7fffffffLL / rows) return 0;                                // more rows than a grid has workgroups
    return align_up((size_t)(B * Co * rows) * 9 * sizeof(double), 256);
}

extern "C" int halo_pool_fold_table(const float *w, const float *v, float *T, int64_t B, int64_t Co, int64_t Cg, int64_t c_off,
                                    int64_t row_stride, void *stream)
{
    const char *who = "halo_pool_fold_table";
    if (!w || !v || !T) return fail(HALO_E_ARG, "%s: null argument", who);
    if (B < 1 || Co < 1 || Cg < 1) return fail(HALO_E_ARG, "%s: empty shape", who);
    if (c_off < 0 || row_stride < (c_off + Cg) * 9) return fail(HALO_E_ARG, "%s: channels %lld..%lld do not fit a row of %lld elements", who,
                                                                (long long)c_off, (long long)(c_off + Cg), (long long)row_stride);
    if (Cg > 0x7fffffffLL / 9 || Co > 0x7fffffffLL || B * Co > 0x7fffffffLL)
        return fail(HALO_E_UNSUPPORTED, "%s: %lld x %lld tables over %lld channels", who, (long long)B, (long long)Co, (long long)Cg);
    hipLaunchKernelGGL(k_pool_fold_table, dim3((unsigned)(B * Co)), dim3(PF_TPB), 0, (hipStream_t)stream, w, v, T, (int)Co, (int)Cg, c_off,
                       row_stride);
    return check_launch(who);
}

extern "C" int halo_pool_fold_affine_relu_fwd(const float *z, const float *T, const float *scale, const float *shift, float *y, int64_t B,
                                              int64_t Co, int64_t H, int64_t W, void *stream)
{
    const char *who = "halo_pool_fold_affine_relu_fwd";
    if (!z || !T || !scale || !shift || !y) return fail(HALO_E_ARG, "%s: null argument", who);
    const bool vec = pf_vec(W, z, y, nullptr);
    PfGeom G;
    unsigned grid;
    if (int rc = pf_plan(who, B, Co, H, W, vec, G, grid)) return rc;
    if (vec) hipLaunchKernelGGL((k_pool_fold_fwd<4>), dim3(grid), dim3(AN_TPB), 0, (hipStream_t)stream, z, T, scale, shift, y, G);
    else hipLaunchKernelGGL((k_pool_fold_fwd<1>), dim3(grid), dim3(AN_TPB), 0, (hipStream_t)stream, z, T, scale, shift, y, G);
    return check_launch(who);
}

extern "C" int halo_pool_fold_affine_relu_bwd(const float *g, const float *y, const float *scale, float *g_z, double *g_T, int64_t B, int64_t Co,
                                              int64_t H, int64_t W, void *workspace, size_t workspace_bytes, void *stream)
{
    const char *who = "halo_pool_fold_affine_relu_bwd";
    if (!g || !y || !scale) return fail(HALO_E_ARG, "%s: null argument", who);
    const bool vec = pf_vec(W, g, y, g_z);
    PfGeom G;
    unsigned grid;
    if (int rc = pf_plan(who, B, Co, H, W, vec, G, grid)) return rc;
    if (!g_z && !g_T) return HALO_OK;                             // nothing is asked for: nothing is launched
    double *slab = nullptr;
    if (g_T) {
        Arena ar(workspace, workspace ? workspace_bytes : 0);
        slab = ar.take<double>((size_t)grid * 9);
        if (!slab) return fail(HALO_E_WORKSPACE, "%s: workspace of %zu bytes, halo_pool_fold_workspace_bytes gives %zu", who, workspace_bytes,
                               halo_pool_fold_workspace_bytes(B, Co, H, W));
    }
    if (vec) pf_launch_bwd<4>(g_z != nullptr, g_T != nullptr, grid, (hipStream_t)stream, g, y, scale, g_z, slab, G);
    else pf_launch_bwd<1>(g_z != nullptr, g_T != nullptr, grid, (hipStream_t)stream, g, y, scale, g_z, slab, G);
    if (g_T) {
        const int64_t entries = B * Co * 9;
        hipLaunchKernelGGL(k_pool_fold_finish, dim3((unsigned)cdiv(entries, PF_TPB)), dim3(PF_TPB), 0, (hipStream_t)stream, slab, g_T, entries,
                           G.a.cpp);
    }
    return check_launch(who);
}
