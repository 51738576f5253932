// The frozen-norm passes of halo_norm.hip under torch.autocast: the convolution in front hands over float16 or bfloat16, the stock
// chain `x * scale + bias; out += identity; relu_(out)` promotes to float32, and the next convolution has autocast round that
// float32 tensor back to half.  One pass over dense NCHW planes with every operand in its own element type:
//
//   pre = fl(fl(float(x) * scale[c]) + shift[c])             x half; two roundings, never an fma (the build sets -ffp-contract=off)
//   id  = r32   or   fl(fl(float(r16) * r_scale[c]) + r_shift[c])     the block's float32 identity, or the half output of its
//                                                            downsample convolution with that norm folded in
//   s   = pre   or   fl(pre + id)
//   y32 = s <= 0 ? 0 : s                                     a NaN stays a NaN
//   y16 = rne_half(y32)                                      what autocast's cast hands the next convolution
//
//   g   = g32,  float(g16)  or  fl(g32 + float(g16))         the gradients that arrived at y32 and y16; autograd's accumulation
//   gp  = s <= 0 ? 0 : g                                     a NaN s lets g through.  The gate is read off the saved y32, or -- for
//                                                            a pass that wrote y16 alone -- off pre recomputed from the saved x:
//                                                            y16 cannot stand in, a small positive y32 rounds to a half zero
//   g_x = rne_half(fl(gp * scale[c]))
//   g_r = gp (float32)   or   rne_half(fl(gp * r_scale[c]))
//
// half -> float is exact; float -> half rounds to nearest even, overflows to +-inf and keeps a NaN a NaN.  These are the statements
// and roundings of the torch chain under autocast and of its autograd backward, element by element: the chain's bits.
//
// Tiling: halo_norm.hip's plane / chunk walk.  A workgroup works inside one plane, so the per-channel scalars are block-uniform
// loads; a plane of HW elements is cut into chunks of AC_TPB * AC_U<GW> groups of GW elements.  GW = 8, the wide route: one
// 16-byte access of a half operand and two of a float32 operand per group, HW % 8 == 0 and every operand 16-byte aligned.  GW = 1:
// any HW and any alignment.  A lane issues the loads of all its groups of every operand before the first use; lanes of a wave take
// consecutive groups; the grid is planes x chunks in one dimension; element offsets are 64-bit; chunks that lie wholly inside the
// plane take a branch without bounds tests.
#include <type_traits>

#include "halo_common.hpp"
#include "halo_half_dev.hpp"
#include "halo_norm_dev.hpp"

namespace halo {

constexpr int AC_TPB = 256;
// groups per lane, all loaded before the first use: 2 x (32 + 16) bytes per float32 / half operand on the wide route, 4 elements on
// the one-element route (halo_norm.hip's count)
template <int GW> constexpr int AC_U = GW == 8 ? 2 : 4;
enum { AC_NONE = 0, AC_PLAIN = 1, AC_AFFINE = 2 };

typedef unsigned short ac_h8 __attribute__((ext_vector_type(8)));

template <int GW> __device__ __forceinline__ void ac_load(const float *p, float *v)
{
    if constexpr (GW == 8) {
        an_load<4>(p, v);
        an_load<4>(p + 4, v + 4);
    } else {
        v[0] = *p;
    }
}

template <int GW> __device__ __forceinline__ void ac_load(const ac_half *p, ac_half *v)
{
    if constexpr (GW == 8) {
        const ac_h8 t = *reinterpret_cast<const ac_h8 *>(p);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = t[e];
    } else {
        v[0] = *p;
    }
}

template <int GW> __device__ __forceinline__ void ac_store(float *p, const float *v)
{
    if constexpr (GW == 8) {
        an_store<4>(p, v);
        an_store<4>(p + 4, v + 4);
    } else {
        *p = v[0];
    }
}

template <int GW> __device__ __forceinline__ void ac_store(ac_half *p, const ac_half *v)
{
    if constexpr (GW == 8) {
        ac_h8 t;
#pragma unroll
        for (int e = 0; e < 8; ++e) t[e] = v[e];
        *reinterpret_cast<ac_h8 *>(p) = t;
    } else {
        *p = v[0];
    }
}

struct AcGeom {
    int C;
    int n;        // groups of GW elements per plane
    int cpp;      // chunks per plane
};

// where a workgroup and its lane work: one chunk of one plane
struct AcPlace {
    int c;            // the channel
    size_t po;        // the plane's element offset in every activation operand
    int g0;           // the lane's first group; its others follow at strides of AC_TPB
    int n;            // groups per plane
    bool full;        // the chunk lies wholly inside the plane
};

template <int GW> __device__ __forceinline__ AcPlace ac_place(const AcGeom &G)
{
    constexpr int CHUNK = AC_TPB * AC_U<GW>;
    const unsigned plane = blockIdx.x / (unsigned)G.cpp;         // 32-bit: the grid has at most 2^31 - 1 workgroups
    const int chunk = (int)(blockIdx.x - plane * (unsigned)G.cpp), base = chunk * CHUNK;
    return {(int)(plane % (unsigned)G.C), (size_t)plane * G.n * GW, base + (int)threadIdx.x, G.n, G.n - base >= CHUNK};
}

// ---------------------------------------------------------------- forward
// RES: AC_NONE, AC_PLAIN (r is float32) or AC_AFFINE (r is half, its norm folded in); Y32 / Y16: which outputs are written
template <int DT, int GW, int RES, bool Y32, bool Y16, bool FULL>
__device__ __forceinline__ void ac_fwd_chunk(const AcPlace &P, const ac_half *__restrict__ x, const float *__restrict__ r32,
                                             const ac_half *__restrict__ r16, float *__restrict__ y32, ac_half *__restrict__ y16, float sc,
                                             float sh, float rsc, float rsh)
{
    constexpr int U = AC_U<GW>;
    ac_half xv[U][GW], rh[U][GW];
    float rf[U][GW];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int g = P.g0 + u * AC_TPB;
        if (FULL || g < P.n) {
            const size_t o = P.po + (size_t)g * GW;
            ac_load<GW>(x + o, xv[u]);
            if constexpr (RES == AC_PLAIN) ac_load<GW>(r32 + o, rf[u]);
            if constexpr (RES == AC_AFFINE) ac_load<GW>(r16 + o, rh[u]);
        }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int g = P.g0 + u * AC_TPB;
        if (FULL || g < P.n) {
            const size_t o = P.po + (size_t)g * GW;
            float yf[GW];
            ac_half yh[GW];
#pragma unroll
            for (int e = 0; e < GW; ++e) {
                float s = an_affine(ac_float<DT>(xv[u][e]), sc, sh);
                if constexpr (RES == AC_PLAIN) s = s + rf[u][e];
                if constexpr (RES == AC_AFFINE) s = s + an_affine(ac_float<DT>(rh[u][e]), rsc, rsh);
                yf[e] = an_relu(s);
            }
            if constexpr (Y16) ac_round_group<DT, GW>(yf, yh);
            if constexpr (Y32) ac_store<GW>(y32 + o, yf);
            if constexpr (Y16) ac_store<GW>(y16 + o, yh);
        }
    }
}

template <int DT, int GW, int RES, bool Y32, bool Y16>
__global__ void __launch_bounds__(AC_TPB) k_ac_affine_relu_fwd(const ac_half *__restrict__ x, const float *__restrict__ scale,
                                                               const float *__restrict__ shift, const void *__restrict__ r,
                                                               const float *__restrict__ r_scale, const float *__restrict__ r_shift,
                                                               float *__restrict__ y32, ac_half *__restrict__ y16, AcGeom G)
{
    const AcPlace P = ac_place<GW>(G);
    const float sc = scale[P.c], sh = shift[P.c];
    const float rsc = RES == AC_AFFINE ? r_scale[P.c] : 0.0f, rsh = RES == AC_AFFINE ? r_shift[P.c] : 0.0f;
    const float *r32 = static_cast<const float *>(r);
    const ac_half *r16 = static_cast<const ac_half *>(r);
    if (P.full) ac_fwd_chunk<DT, GW, RES, Y32, Y16, true>(P, x, r32, r16, y32, y16, sc, sh, rsc, rsh);
    else ac_fwd_chunk<DT, GW, RES, Y32, Y16, false>(P, x, r32, r16, y32, y16, sc, sh, rsc, rsh);
}

// ---------------------------------------------------------------- backward
// G32 / G16: which gradients arrived; MX: the gate is pre recomputed from x (else the saved y32); GX / GR: which gradients are
// written; RAFF: g_r is the half gradient of a downsample convolution's output (else the float32 identity's)
template <int DT, int GW, bool G32, bool G16, bool MX, bool GX, bool GR, bool RAFF, bool FULL>
__device__ __forceinline__ void ac_bwd_chunk(const AcPlace &P, const float *__restrict__ g32, const ac_half *__restrict__ g16,
                                             const float *__restrict__ y32, const ac_half *__restrict__ x, ac_half *__restrict__ gx,
                                             float *__restrict__ gr32, ac_half *__restrict__ gr16, float sc, float sh, float rsc)
{
    constexpr int U = AC_U<GW>;
    float gf[U][GW], yf[U][GW];
    ac_half gh[U][GW], xv[U][GW];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int g = P.g0 + u * AC_TPB;
        if (FULL || g < P.n) {
            const size_t o = P.po + (size_t)g * GW;
            if constexpr (G32) ac_load<GW>(g32 + o, gf[u]);
            if constexpr (G16) ac_load<GW>(g16 + o, gh[u]);
            if constexpr (MX) ac_load<GW>(x + o, xv[u]);
            else ac_load<GW>(y32 + o, yf[u]);
        }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int g = P.g0 + u * AC_TPB;
        if (FULL || g < P.n) {
            const size_t o = P.po + (size_t)g * GW;
            ac_half ox[GW], orh[GW];
            float orf[GW], px[GW], pr[GW];                     // the float32 products, each rounded before its conversion
#pragma unroll
            for (int e = 0; e < GW; ++e) {
                float gs;
                if constexpr (G32 && G16) gs = gf[u][e] + ac_float<DT>(gh[u][e]);
                else if constexpr (G32) gs = gf[u][e];
                else gs = ac_float<DT>(gh[u][e]);
                float m;
                if constexpr (MX) m = an_affine(ac_float<DT>(xv[u][e]), sc, sh);
                else m = yf[u][e];
                const float gp = m <= 0.0f ? 0.0f : gs;
                if constexpr (GX) px[e] = gp * sc;
                if constexpr (GR && RAFF) pr[e] = gp * rsc;
                if constexpr (GR && !RAFF) orf[e] = gp;
            }
            if constexpr (GX) ac_round_group<DT, GW>(px, ox);
            if constexpr (GR && RAFF) ac_round_group<DT, GW>(pr, orh);
            if constexpr (GX) ac_store<GW>(gx + o, ox);
            if constexpr (GR && RAFF) ac_store<GW>(gr16 + o, orh);
            if constexpr (GR && !RAFF) ac_store<GW>(gr32 + o, orf);
        }
    }
}

template <int DT, int GW, bool G32, bool G16, bool MX, bool GX, bool GR, bool RAFF>
__global__ void __launch_bounds__(AC_TPB) k_ac_affine_relu_bwd(const float *__restrict__ g32, const ac_half *__restrict__ g16,
                                                               const float *__restrict__ y32, const ac_half *__restrict__ x,
                                                               const float *__restrict__ scale, const float *__restrict__ shift,
                                                               const float *__restrict__ r_scale, ac_half *__restrict__ gx,
                                                               void *__restrict__ gr, AcGeom G)
{
    const AcPlace P = ac_place<GW>(G);
    const float sc = (GX || MX) ? scale[P.c] : 0.0f, sh = MX ? shift[P.c] : 0.0f, rsc = RAFF ? r_scale[P.c] : 0.0f;
    float *gr32 = static_cast<float *>(gr);
    ac_half *gr16 = static_cast<ac_half *>(gr);
    if (P.full) ac_bwd_chunk<DT, GW, G32, G16, MX, GX, GR, RAFF, true>(P, g32, g16, y32, x, gx, gr32, gr16, sc, sh, rsc);
    else ac_bwd_chunk<DT, GW, G32, G16, MX, GX, GR, RAFF, false>(P, g32, g16, y32, x, gx, gr32, gr16, sc, sh, rsc);
}

// ---------------------------------------------------------------- host side
static int ac_plan(const char *who, int64_t B, int64_t C, int64_t HW, bool wide, AcGeom &G, unsigned &grid)
{
    if (B < 1 || C < 1 || HW < 1) return fail(HALO_E_ARG, "%s: empty shape", who);
    if (HW > 0x7fffffffLL - 1024 || C > 0x7fffffffLL || B > 0x7fffffffLL || B * C > ((int64_t)1 << 40))
        return fail(HALO_E_UNSUPPORTED, "%s: %lld x %lld planes of %lld elements", who, (long long)B, (long long)C, (long long)HW);
    const int gw = wide ? 8 : 1, chunk = AC_TPB * (wide ? AC_U<8> : AC_U<1>);
    G.C = (int)C, G.n = (int)(HW / gw), G.cpp = (int)cdiv(HW / gw, chunk);
    const int64_t blocks = B * C * G.cpp;
    if (blocks > 0x7fffffffLL) return fail(HALO_E_UNSUPPORTED, "%s: %lld blocks", who, (long long)blocks);
    grid = (unsigned)blocks;
    return HALO_OK;
}

template <class... P> static bool ac_wide(int64_t HW, P... p) { return HW % 8 == 0 && ((... | (uintptr_t)p) % 16) == 0; }

// run-time flags as types: f(std::bool_constant<flag>...), in the order given; an entry rules out the combinations it cannot reach
// with `if constexpr`, so that no kernel is built for them.  What is built, per half dtype and route (x 2 x 2):
//   forward    residual {none, float32, half + norm} x outputs {y32, y16, both}                              9 kernels
//   backward   arrived {g32, g16, both} x [ gate off x: g_x ]                                                  3
//              arrived {g32, g16, both} x [ gate off y32: g_x | g_r | g_r(half) | g_x+g_r | g_x+g_r(half) ]   15
template <class F> static void ac_flags(F f) { f(); }
template <class F, class... Rest> static void ac_flags(F f, bool flag, Rest... rest)
{
    if (flag) ac_flags([&](auto... more) { f(std::true_type(), more...); }, rest...);
    else ac_flags([&](auto... more) { f(std::false_type(), more...); }, rest...);
}

}  // namespace halo

using namespace halo;

extern "C" int halo_autocast_norm_relu_fwd(const void *x, const float *scale, const float *shift, const void *r, const float *r_scale,
                                           const float *r_shift, float *y32, void *y16, int half_dtype, int64_t B, int64_t C, int64_t HW,
                                           void *stream)
{
    const char *who = "halo_autocast_norm_relu_fwd";
    if (!x || !scale || !shift) return fail(HALO_E_ARG, "%s: null argument", who);
    if (!y32 && !y16) return fail(HALO_E_ARG, "%s: neither y32 nor y16 is asked for", who);
    if ((r_scale == nullptr) != (r_shift == nullptr)) return fail(HALO_E_ARG, "%s: r_scale and r_shift are given together or not at all", who);
    if (r_scale && !r) return fail(HALO_E_ARG, "%s: r_scale without a residual operand", who);
    if (half_dtype != HALO_F16 && half_dtype != HALO_BF16) return fail(HALO_E_ARG, "%s: half_dtype %d is neither HALO_F16 nor HALO_BF16", who, half_dtype);
    const bool wide = ac_wide(HW, x, r, y32, y16);
    AcGeom G;
    unsigned grid;
    if (int rc = ac_plan(who, B, C, HW, wide, G, grid)) return rc;
    ac_flags([&](auto BF, auto WIDE, auto R, auto RAFF, auto Y32, auto Y16) {
        if constexpr ((Y32() || Y16()) && (R() || !RAFF())) {
            constexpr int DT = BF() ? HALO_BF16 : HALO_F16, GW = WIDE() ? 8 : 1, RES = !R() ? AC_NONE : RAFF() ? AC_AFFINE : AC_PLAIN;
            hipLaunchKernelGGL((k_ac_affine_relu_fwd<DT, GW, RES, Y32(), Y16()>), dim3(grid), dim3(AC_TPB), 0, (hipStream_t)stream,
                               (const ac_half *)x, scale, shift, r, r_scale, r_shift, y32, (ac_half *)y16, G);
        }
    }, half_dtype == HALO_BF16, wide, r != nullptr, r_scale != nullptr, y32 != nullptr, y16 != nullptr);
    return check_launch(who);
}

extern "C" int halo_autocast_norm_relu_bwd(const float *g32, const void *g16, const float *y32, const void *x, const float *scale,
                                           const float *shift, const float *r_scale, void *g_x, void *g_r, int half_dtype, int64_t B,
                                           int64_t C, int64_t HW, void *stream)
{
    const char *who = "halo_autocast_norm_relu_bwd";
    if (!g32 && !g16) return fail(HALO_E_ARG, "%s: null argument: neither g32 nor g16 is given", who);
    if ((y32 == nullptr) == (x == nullptr)) return fail(HALO_E_ARG, "%s: the gate is read off y32 or off x, one of the two", who);
    if (!g_x && !g_r) return fail(HALO_E_ARG, "%s: neither g_x nor g_r is asked for", who);
    if (g_x && !scale) return fail(HALO_E_ARG, "%s: g_x needs scale", who);
    if (x && (!scale || !shift)) return fail(HALO_E_ARG, "%s: the gate off x needs scale and shift", who);
    if (x && g_r) return fail(HALO_E_ARG, "%s: the gate off x is that of a pass without a residual, g_r is asked for", who);
    if (half_dtype != HALO_F16 && half_dtype != HALO_BF16) return fail(HALO_E_ARG, "%s: half_dtype %d is neither HALO_F16 nor HALO_BF16", who, half_dtype);
    const bool wide = ac_wide(HW, g32, g16, y32, x, g_x, g_r);
    AcGeom G;
    unsigned grid;
    if (int rc = ac_plan(who, B, C, HW, wide, G, grid)) return rc;
    ac_flags([&](auto BF, auto WIDE, auto G32, auto G16, auto MX, auto GX, auto GR, auto RAFF) {
        if constexpr ((G32() || G16()) && (GX() || GR()) && !(MX() && GR()) && (GR() || !RAFF())) {      // r_scale counts only where g_r is asked for
            constexpr int DT = BF() ? HALO_BF16 : HALO_F16, GW = WIDE() ? 8 : 1;
            hipLaunchKernelGGL((k_ac_affine_relu_bwd<DT, GW, G32(), G16(), MX(), GX(), GR(), RAFF()>), dim3(grid), dim3(AC_TPB), 0,
                               (hipStream_t)stream, g32, (const ac_half *)g16, y32, (const ac_half *)x, scale, shift, r_scale, (ac_half *)g_x, g_r, G);
        }
    }, half_dtype == HALO_BF16, wide, g32 != nullptr, g16 != nullptr, x != nullptr, g_x != nullptr, g_r != nullptr, g_r && r_scale);
    return check_launch(who);
}
