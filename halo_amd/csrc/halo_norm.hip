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
// Tiling, the same for every pass of this file (an_place, an_walk): a workgroup works inside one plane, so scale, shift, r_scale,
// r_shift and a plane's mask or table are block-uniform scalar loads.  A plane of HW elements is cut into chunks of AN_TPB * AN_U
// groups of GW elements (GW = 4: 16-byte loads and stores, HW % 4 == 0 and every operand 16-byte aligned; GW = 1: any HW and any
// alignment).  A lane issues its AN_U loads of every operand before it computes (AN_U x 16 bytes per operand in flight), lanes of
// a wave take consecutive groups.  The grid is planes x chunks in one dimension; element offsets are 64-bit.  Chunks that lie
// wholly inside the plane take a branch without bounds tests.  What a pass computes is its op: a struct that says which of the
// walk's operands it reads and writes, holds the block-uniform scalars, and turns one loaded group into one group to store.
#include <type_traits>

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

// where a workgroup and its lane work: one chunk of one plane
struct AnPlace {
    unsigned plane;   // b * C + c: indexes what there is one of per plane (the dropout mask, the fold table)
    int c;            // the channel: indexes scale, shift, r_scale, r_shift
    size_t po;        // the plane's element offset in every activation operand
    int g0;           // the lane's first group; its other AN_U - 1 follow at strides of AN_TPB
    int n;            // groups per plane
    bool full;        // the chunk lies wholly inside the plane
};

template <int GW> __device__ __forceinline__ AnPlace an_place(const AnGeom &G)
{
    const unsigned plane = blockIdx.x / (unsigned)G.cpp;         // 32-bit: the grid has at most 2^31 - 1 workgroups
    const int chunk = (int)(blockIdx.x - plane * (unsigned)G.cpp), base = chunk * AN_CHUNK;
    return {plane, (int)(plane % (unsigned)G.C), (size_t)plane * G.n * GW, base + (int)threadIdx.x, G.n, G.n - base >= AN_CHUNK};
}

// One chunk.  An op has
//   IN[3], OUT[2]                      which of i0..i2 it reads and of o0, o1 it writes; the others may be null and are not touched
//   group<GW>(g, in, out)              in[k][e] -> out[k][e] for the GW elements of group g of the plane (element g * GW + e), one
//                                      rounding per statement; per-lane state that outlives the walk sits behind a pointer in the op
// All loads of all AN_U groups are issued before the first group() runs.  An op that reads nothing issues no load.  The operands
// stay separate __restrict__ parameters down to the loads, and the registers are laid out operand by operand: group by group
// (in[u][k]) the one-element route takes 4 to 6 more VGPRs in every kernel.
template <int GW, bool FULL, class Op>
__device__ __forceinline__ void an_chunk(Op &op, const AnPlace &P, const float *__restrict__ i0, const float *__restrict__ i1,
                                         const float *__restrict__ i2, float *__restrict__ o0, float *__restrict__ o1)
{
    float in[3][AN_U][GW];
#pragma unroll
    for (int u = 0; u < AN_U; ++u) {
        const int g = P.g0 + u * AN_TPB;
        if (FULL || g < P.n) {
            if constexpr (Op::IN[0]) an_load<GW>(i0 + P.po + (size_t)g * GW, in[0][u]);
            if constexpr (Op::IN[1]) an_load<GW>(i1 + P.po + (size_t)g * GW, in[1][u]);
            if constexpr (Op::IN[2]) an_load<GW>(i2 + P.po + (size_t)g * GW, in[2][u]);
        }
    }
#pragma unroll
    for (int u = 0; u < AN_U; ++u) {
        const int g = P.g0 + u * AN_TPB;
        if (FULL || g < P.n) {
            float out[2][GW];
            const float *const v[3] = {in[0][u], in[1][u], in[2][u]};
            op.template group<GW>(g, v, out);
            if constexpr (Op::OUT[0]) an_store<GW>(o0 + P.po + (size_t)g * GW, out[0]);
            if constexpr (Op::OUT[1]) an_store<GW>(o1 + P.po + (size_t)g * GW, out[1]);
        }
    }
}

template <int GW, class Op>
__device__ __forceinline__ void an_walk(Op &op, const AnPlace &P, const float *__restrict__ i0, const float *__restrict__ i1,
                                        const float *__restrict__ i2, float *__restrict__ o0, float *__restrict__ o1)
{
    if (P.full) an_chunk<GW, true>(op, P, i0, i1, i2, o0, o1);
    else an_chunk<GW, false>(op, P, i0, i1, i2, o0, o1);
}

// in: x, r  out: y
template <int RES> struct AnFwd {
    static constexpr bool IN[3] = {true, RES != AN_NONE, false}, OUT[2] = {true, false};
    float sc, sh, rsc, rsh;
    template <int GW> __device__ __forceinline__ void group(int, const float *const *in, float (*out)[GW]) const
    {
#pragma unroll
        for (int e = 0; e < GW; ++e) {
            float s = an_affine(in[0][e], sc, sh);
            if constexpr (RES == AN_PLAIN) s = s + in[1][e];
            if constexpr (RES == AN_AFFINE) s = s + an_affine(in[1][e], rsc, rsh);
            out[0][e] = an_relu(s);
        }
    }
};

template <int GW, int RES>
__global__ void __launch_bounds__(AN_TPB) k_affine_relu_fwd(const float *__restrict__ x, const float *__restrict__ scale,
                                                            const float *__restrict__ shift, const float *__restrict__ r,
                                                            const float *__restrict__ r_scale, const float *__restrict__ r_shift,
                                                            float *__restrict__ y, AnGeom G)
{
    const AnPlace P = an_place<GW>(G);
    AnFwd<RES> op{scale[P.c], shift[P.c], RES == AN_AFFINE ? r_scale[P.c] : 0.0f, RES == AN_AFFINE ? r_shift[P.c] : 0.0f};
    an_walk<GW>(op, P, x, r, nullptr, y, nullptr);
}

// in: g, g2, y  out: g_x, g_r.  FORK: two gradients arrive at y (a block output that the next block reads twice); their sum is
// autograd's accumulation, one float32 add, and the statements behind it are the same
template <bool GX, bool GR, bool RAFF, bool FORK> struct AnBwd {
    static constexpr bool IN[3] = {true, FORK, true}, OUT[2] = {GX, GR};
    float sc, rsc;
    template <int GW> __device__ __forceinline__ void group(int, const float *const *in, float (*out)[GW]) const
    {
#pragma unroll
        for (int e = 0; e < GW; ++e) {
            float gs = in[0][e];
            if constexpr (FORK) gs = gs + in[1][e];
            const float gp = in[2][e] <= 0.0f ? 0.0f : gs;
            out[0][e] = gp * sc;
            out[1][e] = RAFF ? gp * rsc : gp;
        }
    }
};

template <int GW, bool GX, bool GR, bool RAFF, bool FORK>
__global__ void __launch_bounds__(AN_TPB) k_affine_relu_bwd(const float *__restrict__ g, const float *__restrict__ g2, const float *__restrict__ y,
                                                            const float *__restrict__ scale, const float *__restrict__ r_scale,
                                                            float *__restrict__ gx, float *__restrict__ gr, AnGeom G)
{
    const AnPlace P = an_place<GW>(G);
    AnBwd<GX, GR, RAFF, FORK> op{GX ? scale[P.c] : 0.0f, RAFF ? r_scale[P.c] : 0.0f};
    an_walk<GW>(op, P, g, g2, y, gx, gr);
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

// the route as a type: launch(std::integral_constant<int, GW>) with GW = 4 for the 16-byte route, 1 for the one-element route
template <class L> static void an_route(bool vec, L launch)
{
    if (vec) launch(std::integral_constant<int, 4>());
    else launch(std::integral_constant<int, 1>());
}

// run-time flags as types: f(std::bool_constant<flag>...), in the order given.  An entry rules out the combinations it cannot
// reach with `if constexpr`, so that no kernel is built for them.
template <class F> static void an_flags(F f) { f(); }
template <class F, class... Rest> static void an_flags(F f, bool flag, Rest... rest)
{
    if (flag) an_flags([&](auto... more) { f(std::true_type(), more...); }, rest...);
    else an_flags([&](auto... more) { f(std::false_type(), more...); }, rest...);
}

// an entry behind its null checks: plans the walk of B x C planes of HW elements on the route `vec`, has launch(GW, G, grid) enqueue
// the kernel, and reports
template <class L> static int an_run(const char *who, int64_t B, int64_t C, int64_t HW, bool vec, L launch)
{
    AnGeom G;
    unsigned grid;
    if (int rc = an_plan(who, B, C, HW, vec, G, grid)) return rc;
    an_route(vec, [&](auto GW) { launch(GW, G, dim3(grid)); });
    return check_launch(who);
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

// in: x  out: y
struct AnMaskFwd {
    static constexpr bool IN[3] = {true, false, false}, OUT[2] = {true, false};
    float sc, sh, m;
    template <int GW> __device__ __forceinline__ void group(int, const float *const *in, float (*out)[GW]) const
    {
#pragma unroll
        for (int e = 0; e < GW; ++e) {
            float s = in[0][e] * sc;
            s = s + sh;
            s = s <= 0.0f ? 0.0f : s;
            out[0][e] = s * m;
        }
    }
};

template <int GW>
__global__ void __launch_bounds__(AN_TPB) k_affine_relu_mask_fwd(const float *__restrict__ x, const float *__restrict__ scale,
                                                                 const float *__restrict__ shift, const float *__restrict__ mask,
                                                                 float *__restrict__ y, AnGeom G)
{
    const AnPlace P = an_place<GW>(G);
    AnMaskFwd op{scale[P.c], shift[P.c], mask[P.plane]};
    an_walk<GW>(op, P, x, nullptr, nullptr, y, nullptr);
}

// in: g, y  out: g_x.  KEPT = false, a dropped plane: reads nothing, writes zeros
template <bool KEPT> struct AnMaskBwd {
    static constexpr bool IN[3] = {KEPT, KEPT, false}, OUT[2] = {true, false};
    float sc, m;
    template <int GW> __device__ __forceinline__ void group(int, const float *const *in, float (*out)[GW]) const
    {
#pragma unroll
        for (int e = 0; e < GW; ++e) {
            if constexpr (KEPT) {
                float t = in[0][e] * m;
                t = t * sc;
                out[0][e] = in[1][e] <= 0.0f ? 0.0f : t;
            } else {
                out[0][e] = 0.0f;
            }
        }
    }
};

template <int GW>
__global__ void __launch_bounds__(AN_TPB) k_affine_relu_mask_bwd(const float *__restrict__ g, const float *__restrict__ y,
                                                                 const float *__restrict__ scale, const float *__restrict__ mask,
                                                                 float *__restrict__ gx, AnGeom G)
{
    const AnPlace P = an_place<GW>(G);
    const float sc = scale[P.c], m = mask[P.plane];
    if (m != 0.0f) {                                             // block-uniform: the whole workgroup lies in one plane
        AnMaskBwd<true> op{sc, m};
        an_walk<GW>(op, P, g, y, nullptr, gx, nullptr);
    } else {
        AnMaskBwd<false> op{sc, m};
        an_walk<GW>(op, P, g, y, nullptr, gx, nullptr);
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

// in: x  out: y, z
struct AnPairFwd {
    static constexpr bool IN[3] = {true, false, false}, OUT[2] = {true, true};
    float sc, sh, m;
    template <int GW> __device__ __forceinline__ void group(int, const float *const *in, float (*out)[GW]) const
    {
#pragma unroll
        for (int e = 0; e < GW; ++e) {
            float s = in[0][e] * sc;
            s = s + sh;
            out[0][e] = s <= 0.0f ? 0.0f : s;
            out[1][e] = out[0][e] * m;
        }
    }
};

template <int GW>
__global__ void __launch_bounds__(AN_TPB) k_affine_relu_pair_fwd(const float *__restrict__ x, const float *__restrict__ scale,
                                                                 const float *__restrict__ shift, const float *__restrict__ mask,
                                                                 float *__restrict__ y, float *__restrict__ z, AnGeom G)
{
    const AnPlace P = an_place<GW>(G);
    AnPairFwd op{scale[P.c], shift[P.c], mask[P.plane]};
    an_walk<GW>(op, P, x, nullptr, nullptr, y, z);
}

// in: g_y, g_z, y  out: g_x.  GY / GZ: which of the two gradients this workgroup reads (neither: it reads nothing and writes zeros)
template <bool GY, bool GZ> struct AnPairBwd {
    static constexpr bool IN[3] = {GY, GZ, GY || GZ}, OUT[2] = {true, false};
    float sc, m;
    template <int GW> __device__ __forceinline__ void group(int, const float *const *in, float (*out)[GW]) const
    {
#pragma unroll
        for (int e = 0; e < GW; ++e) {
            if constexpr (GY || GZ) {
                float t;
                if constexpr (GZ) {
                    t = in[1][e] * m;
                    if constexpr (GY) t = in[0][e] + t;
                } else {
                    t = in[0][e];
                }
                t = in[2][e] <= 0.0f ? 0.0f : t;
                out[0][e] = t * sc;
            } else {
                out[0][e] = 0.0f;
            }
        }
    }
};

template <int GW, bool GY, bool GZ>
__global__ void __launch_bounds__(AN_TPB) k_affine_relu_pair_bwd(const float *__restrict__ gy, const float *__restrict__ gz,
                                                                 const float *__restrict__ y, const float *__restrict__ scale,
                                                                 const float *__restrict__ mask, float *__restrict__ gx, AnGeom G)
{
    const AnPlace P = an_place<GW>(G);
    const float sc = scale[P.c], m = GZ ? mask[P.plane] : 1.0f;
    if (!GZ || m != 0.0f) {                                      // block-uniform: the whole workgroup lies in one plane
        AnPairBwd<GY, GZ> op{sc, m};
        an_walk<GW>(op, P, gy, gz, y, gx, nullptr);
    } else {                                                     // a dropped plane: g_z's term is 0
        AnPairBwd<GY, false> op{sc, m};
        an_walk<GW>(op, P, gy, gz, y, gx, nullptr);
    }
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

// in: z  out: y.  Row and column come from the group index: a group lies in one row on both routes
struct PfFwd {
    static constexpr bool IN[3] = {true, false, false}, OUT[2] = {true, false};
    int H, W;
    float sc, sh;
    const float *t;                                             // the plane's table
    template <int GW> __device__ __forceinline__ void group(int g, const float *const *in, float (*out)[GW]) const
    {
        const unsigned e0 = (unsigned)g * GW, row = e0 / (unsigned)W, col = e0 - row * (unsigned)W;
        const float *tr = t + pf_rc((int)row, H) * 3;          // the plane's 36-byte table stays in the cache; a copy in registers
        const float t0 = tr[0], t1 = tr[1], t2 = tr[2];        // picked by selects comes back from the compiler as an LDS array
#pragma unroll
        for (int e = 0; e < GW; ++e) {
            const int c = (int)col + e;
            float s = in[0][e] + (c == 0 ? t0 : c == W - 1 ? t2 : t1);
            s = s * sc;
            s = s + sh;
            out[0][e] = s <= 0.0f ? 0.0f : s;
        }
    }
};

template <int GW>
__global__ void __launch_bounds__(AN_TPB) k_pool_fold_fwd(const float *__restrict__ z, const float *__restrict__ T, const float *__restrict__ scale,
                                                          const float *__restrict__ shift, float *__restrict__ y, PfGeom G)
{
    const AnPlace P = an_place<GW>(G.a);
    PfFwd op{G.H, G.W, scale[P.c], shift[P.c], T + (size_t)P.plane * 9};
    an_walk<GW>(op, P, z, nullptr, nullptr, y, nullptr);
}

// in: g, y  out: g_z.  SUMS: the lane's class sums of g_z, in element order, go to the kernel's acc (held in the op itself, the
// 16-byte route's two SUMS kernels take 66 and 68 VGPRs instead of 56 and 62: 7 waves per SIMD)
template <bool GZ, bool SUMS> struct PfBwd {
    static constexpr bool IN[3] = {true, true, false}, OUT[2] = {GZ, false};
    int H, W;
    float sc;
    double *acc;
    template <int GW> __device__ __forceinline__ void group(int g, const float *const *in, float (*out)[GW]) const
    {
        const unsigned e0 = (unsigned)g * GW, row = e0 / (unsigned)W, col = e0 - row * (unsigned)W;
        const int rc = pf_rc((int)row, H);
#pragma unroll
        for (int e = 0; e < GW; ++e) {
            const float gv = in[0][e];                       // read in front of the gate: as the gate's own operand the first group's
            const float gp = in[1][e] <= 0.0f ? 0.0f : gv;     // load of g is moved under it and issued when y has arrived
            out[0][e] = gp * sc;
            if constexpr (SUMS) {
                const int c = (int)col + e, cls = rc * 3 + (c == 0 ? 0 : c == W - 1 ? 2 : 1);
                const double d = (double)out[0][e];
#pragma unroll
                for (int k = 0; k < 9; ++k) acc[k] += cls == k ? d : 0.0;
            }
        }
    }
};

template <int GW, bool GZ, bool SUMS>
__global__ void __launch_bounds__(AN_TPB) k_pool_fold_bwd(const float *__restrict__ g, const float *__restrict__ y, const float *__restrict__ scale,
                                                          float *__restrict__ gz, double *__restrict__ slab, PfGeom G)
{
    static_assert(AN_TPB == PF_TPB, "pf_tree is sized for the plane walk's workgroup");
    __shared__ double red[SUMS ? 9 : 1][PF_TPB];
    const AnPlace P = an_place<GW>(G.a);
    double acc[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    PfBwd<GZ, SUMS> op{G.H, G.W, scale[P.c], acc};
    an_walk<GW>(op, P, g, y, nullptr, gz, nullptr);
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

}  // namespace halo

using namespace halo;

extern "C" int halo_affine_relu_fwd(const float *x, const float *scale, const float *shift, const float *r, const float *r_scale,
                                    const float *r_shift, float *y, int64_t B, int64_t C, int64_t HW, void *stream)
{
    const char *who = "halo_affine_relu_fwd";
    if (!x || !scale || !shift || !y) return fail(HALO_E_ARG, "%s: null argument", who);
    if ((r_scale == nullptr) != (r_shift == nullptr)) return fail(HALO_E_ARG, "%s: r_scale and r_shift are given together or not at all", who);
    if (r_scale && !r) return fail(HALO_E_ARG, "%s: r_scale without a residual operand", who);
    return an_run(who, B, C, HW, an_vec(HW, x, y, r, nullptr), [&](auto GW, const AnGeom &G, dim3 grid) {
        an_flags([&](auto R, auto RAFF) {
            constexpr int RES = !R() ? AN_NONE : RAFF() ? AN_AFFINE : AN_PLAIN;
            hipLaunchKernelGGL((k_affine_relu_fwd<GW(), RES>), grid, dim3(AN_TPB), 0, (hipStream_t)stream, x, scale, shift, r, r_scale, r_shift, y, G);
        }, r != nullptr, r_scale != nullptr);
    });
}

// both entries of the block tail's backward: g_b is the second gradient of halo_fork_affine_relu_bwd, null for the single one
static int an_bwd_entry(const char *who, const float *g, const float *g_b, const float *y, const float *scale, const float *r_scale, float *g_x,
                        float *g_r, int64_t B, int64_t C, int64_t HW, void *stream)
{
    if (!g_x && !g_r) return fail(HALO_E_ARG, "%s: neither g_x nor g_r is asked for", who);
    if (g_x && !scale) return fail(HALO_E_ARG, "%s: g_x needs scale", who);
    const bool vec = an_vec(HW, g, y, g_x, g_r) && (uintptr_t)g_b % 16 == 0;
    return an_run(who, B, C, HW, vec, [&](auto GW, const AnGeom &G, dim3 grid) {
        an_flags([&](auto GX, auto GR, auto RAFF, auto FORK) {
            if constexpr ((GX() || GR()) && (GR() || !RAFF()))       // r_scale counts only where g_r is asked for
                hipLaunchKernelGGL((k_affine_relu_bwd<GW(), GX(), GR(), RAFF(), FORK()>), grid, dim3(AN_TPB), 0, (hipStream_t)stream, g, g_b, y,
                                   scale, r_scale, g_x, g_r, G);
        }, g_x != nullptr, g_r != nullptr, g_r && r_scale, g_b != nullptr);
    });
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
    return an_run(who, B, C, HW, an_vec(HW, x, y, nullptr, nullptr), [&](auto GW, const AnGeom &G, dim3 grid) {
        hipLaunchKernelGGL((k_affine_relu_mask_fwd<GW()>), grid, dim3(AN_TPB), 0, (hipStream_t)stream, x, scale, shift, mask, y, G);
    });
}

extern "C" int halo_masked_affine_relu_bwd(const float *g, const float *y, const float *scale, const float *mask, float *g_x, int64_t B,
                                           int64_t C, int64_t HW, void *stream)
{
    const char *who = "halo_masked_affine_relu_bwd";
    if (!g || !y || !scale || !mask || !g_x) return fail(HALO_E_ARG, "%s: null argument", who);
    return an_run(who, B, C, HW, an_vec(HW, g, y, g_x, nullptr), [&](auto GW, const AnGeom &G, dim3 grid) {
        hipLaunchKernelGGL((k_affine_relu_mask_bwd<GW()>), grid, dim3(AN_TPB), 0, (hipStream_t)stream, g, y, scale, mask, g_x, G);
    });
}

extern "C" int halo_dropout_pair_fwd(const float *x, const float *scale, const float *shift, const float *mask, float *y, float *z, int64_t B,
                                     int64_t C, int64_t HW, void *stream)
{
    const char *who = "halo_dropout_pair_fwd";
    if (!x || !scale || !shift || !mask || !y || !z) return fail(HALO_E_ARG, "%s: null argument", who);
    return an_run(who, B, C, HW, an_vec(HW, x, y, z, nullptr), [&](auto GW, const AnGeom &G, dim3 grid) {
        hipLaunchKernelGGL((k_affine_relu_pair_fwd<GW()>), grid, dim3(AN_TPB), 0, (hipStream_t)stream, x, scale, shift, mask, y, z, G);
    });
}

extern "C" int halo_dropout_pair_bwd(const float *g_y, const float *g_z, const float *y, const float *scale, const float *mask, float *g_x,
                                     int64_t B, int64_t C, int64_t HW, void *stream)
{
    const char *who = "halo_dropout_pair_bwd";
    if (!y || !scale || !mask || !g_x) return fail(HALO_E_ARG, "%s: null argument", who);
    if (!g_y && !g_z) return fail(HALO_E_ARG, "%s: null argument: neither g_y nor g_z is given", who);
    return an_run(who, B, C, HW, an_vec(HW, g_y, g_z, y, g_x), [&](auto GW, const AnGeom &G, dim3 grid) {
        an_flags([&](auto GY, auto GZ) {
            if constexpr (GY() || GZ())
                hipLaunchKernelGGL((k_affine_relu_pair_bwd<GW(), GY(), GZ()>), grid, dim3(AN_TPB), 0, (hipStream_t)stream, g_y, g_z, y, scale, mask,
                                   g_x, G);
        }, g_y != nullptr, g_z != nullptr);
    });
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
    an_route(vec, [&](auto GW) {
        hipLaunchKernelGGL((k_pool_fold_fwd<GW()>), dim3(grid), dim3(AN_TPB), 0, (hipStream_t)stream, z, T, scale, shift, y, G);
    });
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
    an_route(vec, [&](auto GW) {
        an_flags([&](auto GZ, auto SUMS) {
            if constexpr (GZ() || SUMS())
                hipLaunchKernelGGL((k_pool_fold_bwd<GW(), GZ(), SUMS()>), dim3(grid), dim3(AN_TPB), 0, (hipStream_t)stream, g, y, scale, g_z, slab, G);
        }, g_z != nullptr, g_T != nullptr);
    });
    if (g_T) {
        const int64_t entries = B * Co * 9;
        hipLaunchKernelGGL(k_pool_fold_finish, dim3((unsigned)cdiv(entries, PF_TPB)), dim3(PF_TPB), 0, (hipStream_t)stream, slab, g_T, entries,
                           G.a.cpp);
    }
    return check_launch(who);
}
