// Hyperbolic head ops for gfx950: HyperMapper.{expmap,logmap,poincare_distance[_origin]} and
// HyperMLR._hyper_logits (core/utils/hyperbolic.py:16-188; arithmetic = geoopt's
// stereographic/math.py with k = -c), plus the align_corners bilinear resize the head tails and
// RegionSelection apply (core/models/classifier.py:375-377,556-557; core/active/build.py:123-135).
//
// Tensors are viewed as (outer, C, inner) with the reduction over C, so the NCHW dim=1 case
// (inner = H*W: consecutive lanes read consecutive pixels of one channel plane, coalesced) and
// the last-dim case (inner = 1) share one kernel.
#include "halo_common.hpp"
#include "halo_devmath.hpp"
#include <stdlib.h>

namespace halo {

constexpr int HTPB = 256;
typedef double d2_h __attribute__((ext_vector_type(2)));
typedef float f4_t __attribute__((ext_vector_type(4)));

template <typename T> __device__ __forceinline__ double ld_as_f64(const T *p) { return (double)*p; }

// ---------------------------------------------------------------- expmap0 + project  (hyperbolic.py:37-38)
template <typename TIN>
__global__ void __launch_bounds__(HTPB) k_expmap0_project(const TIN *__restrict__ x, double *__restrict__ y, long long outer,
                                                          int C, long long inner, double ks, double rks, double maxnorm)
{
    const long long idx = (long long)blockIdx.x * HTPB + threadIdx.x;
    if (idx >= outer * inner) return;
    const long long o = idx / inner, i = idx % inner;
    const TIN *xp = x + (size_t)o * C * inner + i;
    double *yp = y + (size_t)o * C * inner + i;
    double ssq = 0.0;
    for (int ch = 0; ch < C; ++ch) { const double v = ld_as_f64(xp + (size_t)ch * inner); ssq = __builtin_fma(v, v, ssq); }
    double n = __builtin_sqrt(ssq);
    n = n < 1e-15 ? 1e-15 : n;                               // clamp_min(1e-15)
    double a = n * ks;
    a = a > 15.0 ? 15.0 : (a < -15.0 ? -15.0 : a);           // geoopt tanh clamp
    const double g = rks * tanh(a);                          // tan_k(u_norm, k)
    double s2 = 0.0;
    for (int ch = 0; ch < C; ++ch) {
        const double v = g * (ld_as_f64(xp + (size_t)ch * inner) / n);
        yp[(size_t)ch * inner] = v;
        s2 = __builtin_fma(v, v, s2);
    }
    double ny = __builtin_sqrt(s2);
    ny = ny < 1e-15 ? 1e-15 : ny;
    if (ny > maxnorm)                                        // project: eps = 1e-5 for float64
        for (int ch = 0; ch < C; ++ch) yp[(size_t)ch * inner] = yp[(size_t)ch * inner] / ny * maxnorm;
}

// The same map through an LDS tile: a workgroup stages P consecutive pixels x all C channels (float32 input,
// 32-64 KiB) with 16-byte non-temporal loads issued back to back -- x is read from HBM ONCE (the kernel above walks
// the channel planes twice with a handful of loads in flight) -- then one lane per pixel runs the norm's fma chain
// over the tile, and all lanes write y as 16-byte non-temporal stores (the output is twice the input and written
// once).  Arithmetic and its order are exactly the kernel's above (one sequential fma chain per pixel in channel
// order, v = g * (x / n)), so the results are bit-identical.  project() can only act when g = tanh(.)/sqrt(c) is
// within 1e-9 of maxnorm (||y|| <= g (1 + C 2^-52)), so the second norm is computed only for such pixels.
typedef float f2_t __attribute__((ext_vector_type(2)));
// x / n for many x and one n: the division sequence hipcc emits for f64 is  v_div_scale (no-op for operands in the
// normal range), r = v_rcp_f64(n) refined by two Newton steps, q = x r, rem = fma(-n, q, x), q = fma(rem, r, q)
// (v_div_fmas without scaling), v_div_fixup (specials).  With n in [1e-15, 1e25] and |x| a float32 value the
// quotient is in the normal range, so the sequence below returns the identical bits with r computed once per pixel.
__device__ __forceinline__ double exact_rcp(double n)
{
    double r = __builtin_amdgcn_rcp(n);
    r = __builtin_fma(__builtin_fma(-n, r, 1.0), r, r);
    r = __builtin_fma(__builtin_fma(-n, r, 1.0), r, r);
    return r;
}
__device__ __forceinline__ double div_by(float x, double n, double r)
{
    const double xd = (double)x, q = xd * r;
    return __builtin_fma(__builtin_fma(-n, q, xd), r, q);
}

constexpr int EXP_LD = 8;      // 16-byte loads in flight per lane while staging

// A block walks tiles blockIdx.x, blockIdx.x + gridDim.x, ... (the host launches one block per tile) and requests the first
// EXP_LD 16-byte groups per thread of its NEXT tile before it touches the current one, so that a block walking several tiles has
// those loads in flight during the serial part of a tile -- one lane per pixel running the norm's fma chain over C channels while
// the other lanes of the block have nothing to do -- and during its write phase.
__global__ void __launch_bounds__(HTPB, 4) k_expmap0_project_tile(const float *__restrict__ x, double *__restrict__ y, long long outer,
                                                               int C, long long inner, int pshift, double ks, double rks,
                                                               double maxnorm)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_e[];
    const int P = 1 << pshift, tid = threadIdx.x;
    float *tile = reinterpret_cast<float *>(smem_e);                         // [C][P]
    double *s_n = reinterpret_cast<double *>(smem_e + (size_t)C * P * 4);    // per pixel: n, g, projection norm (0 = none)
    double *s_g = s_n + P, *s_pr = s_g + P;
    const long long tiles = (inner + P - 1) >> pshift, ntiles = outer * tiles;
    const int gsh = pshift - 2, gmask = (1 << gsh) - 1, ngroups = C << gsh;
    // element e of a tile = (channel e >> (pshift-2), 4-pixel group e & (P/4-1)); the first EXP_LD * HTPB of them are prefetched
    auto fetch = [&](long long t, f4_t (&q)[EXP_LD]) {
        const long long o = t / tiles, i0 = (t % tiles) << pshift;
        const int np = inner - i0 < P ? (int)(inner - i0) : P;
        const float *xp = x + (size_t)o * C * inner + i0;
#pragma unroll
        for (int u = 0; u < EXP_LD; ++u) {
            const int e = tid + u * HTPB, c = e >> gsh, px = (e & gmask) << 2;
            q[u] = (f4_t){0.f, 0.f, 0.f, 0.f};
            if (e < ngroups && px < np) q[u] = __builtin_nontemporal_load(reinterpret_cast<const f4_t *>(xp + (size_t)c * inner + px));
        }
    };
    f4_t q[EXP_LD];
    long long t = blockIdx.x;
    if (t < ntiles) fetch(t, q);
    for (; t < ntiles; t += gridDim.x) {
        const long long o = t / tiles, i0 = (t % tiles) << pshift;
        const int np = inner - i0 < P ? (int)(inner - i0) : P;                   // pixels of this tile (a multiple of 4)
        const float *xp = x + (size_t)o * C * inner + i0;
        double *yp = y + (size_t)o * C * inner + i0;
        // ---- stage: the prefetched groups, then whatever a larger tile has beyond them
#pragma unroll
        for (int u = 0; u < EXP_LD; ++u) {
            const int e = tid + u * HTPB;
            if (e < ngroups) *reinterpret_cast<f4_t *>(tile + ((size_t)(e >> gsh) << pshift) + ((e & gmask) << 2)) = q[u];
        }
        for (int e0 = tid + EXP_LD * HTPB; e0 < ngroups; e0 += HTPB * EXP_LD) {
            f4_t r[EXP_LD];
#pragma unroll
            for (int u = 0; u < EXP_LD; ++u) {
                const int e = e0 + u * HTPB, c = e >> gsh, px = (e & gmask) << 2;
                r[u] = (f4_t){0.f, 0.f, 0.f, 0.f};
                if (e < ngroups && px < np) r[u] = __builtin_nontemporal_load(reinterpret_cast<const f4_t *>(xp + (size_t)c * inner + px));
            }
#pragma unroll
            for (int u = 0; u < EXP_LD; ++u) {
                const int e = e0 + u * HTPB;
                if (e < ngroups) *reinterpret_cast<f4_t *>(tile + ((size_t)(e >> gsh) << pshift) + ((e & gmask) << 2)) = r[u];
            }
        }
        if (t + gridDim.x < ntiles) fetch(t + gridDim.x, q);                     // in flight during the rest of this tile
        __syncthreads();
        // ---- one lane per pixel: ||x||, the tanh gain, and (rarely) the projection norm
        if (tid < np) {
            double ssq = 0.0;
#pragma unroll 4
            for (int c = 0; c < C; ++c) { const double v = (double)tile[((size_t)c << pshift) + tid]; ssq = __builtin_fma(v, v, ssq); }
            double n = __builtin_sqrt(ssq);
            n = n < 1e-15 ? 1e-15 : n;
            double a = n * ks;
            a = a > 15.0 ? 15.0 : (a < -15.0 ? -15.0 : a);
            const double g = rks * tanh(a);
            double pr = 0.0;
            if (g >= maxnorm * (1.0 - 1e-9)) {
                double s2 = 0.0;
#pragma unroll 1
                for (int c = 0; c < C; ++c) { const double v = g * ((double)tile[((size_t)c << pshift) + tid] / n); s2 = __builtin_fma(v, v, s2); }
                double ny = __builtin_sqrt(s2);
                ny = ny < 1e-15 ? 1e-15 : ny;
                pr = ny > maxnorm ? ny : 0.0;
            }
            s_n[tid] = n; s_g[tid] = g; s_pr[tid] = pr;
        }
        __syncthreads();
        // ---- write: a thread keeps ONE pixel pair and walks the channels (pair, n, g and the reciprocal of n hoisted).
        // x / n is formed exactly as the hardware's own division sequence forms it for operands in the normal range
        // (v_rcp_f64, two Newton steps, q = x r, one fma correction): same bits as `x / n`, a third of the instructions.
        const int psh = pshift - 1, px = (tid & ((1 << psh) - 1)) << 1, cstep = HTPB >> psh;
        if (px < np) {
            const double n0 = s_n[px], n1 = s_n[px + 1], g0 = s_g[px], g1 = s_g[px + 1], p0 = s_pr[px], p1 = s_pr[px + 1];
            const double r0 = exact_rcp(n0), r1 = exact_rcp(n1);
            for (int c = tid >> psh; c < C; c += cstep) {
                const f2_t xv = *reinterpret_cast<const f2_t *>(tile + ((size_t)c << pshift) + px);
                double v0 = g0 * div_by(xv.x, n0, r0), v1 = g1 * div_by(xv.y, n1, r1);
                if (p0 != 0.0) v0 = v0 / p0 * maxnorm;
                if (p1 != 0.0) v1 = v1 / p1 * maxnorm;
                __builtin_nontemporal_store((d2_h){v0, v1}, reinterpret_cast<d2_h *>(yp + (size_t)c * inner + px));
            }
        }
        __syncthreads();                                                         // the tile may be overwritten
    }
}

// ---------------------------------------------------------------- expmap0 + project, register-resident (C <= CC)
// The head's own channel count is small (MODEL.HYPER_DIM = 64, defaults.py:14): a lane can hold ALL channels of its two pixels in
// registers (CC float2 values).  So: every plane load of the lane is issued up front (CC 8-byte non-temporal loads in flight, 512
// contiguous bytes per wave and plane), the norm's fma chain runs over registers in channel order, and the lane writes its CC
// 16-byte non-temporal stores -- x is read once, no LDS tile, no barrier, no lane idles while one lane per pixel runs the chain
// (k_expmap0_project_tile above: 0.32-0.35 of the HBM spec at 160x320x64, 0.59-0.63 at 640x1280x64).  Same operations in the same
// order per pixel as the two kernels above (sequential fma chain, v = g * (x / n) through the division sequence's own
// refinement, the projection only where it can act): bit-identical results.
template <int CC, bool EXACT>       // EXACT: C == CC, no per-channel test -- NOT instantiated: as one basic block the compiler schedules it into 255 registers + scratch
__global__ void __launch_bounds__(64, CC > 32 ? 3 : 4) k_expmap0_project_regs(const float *__restrict__ x, double *__restrict__ y, long long outer, int Crt,
                                                             long long inner, double ks, double rks, double maxnorm)
{
    const int C = EXACT ? CC : Crt;
    // grid (pixel pairs, outer): the plane bases are block-uniform (scalar registers), a lane's offset inside a plane is ONE 32-bit
    // register for all CC loads and stores (per-lane 64-bit pointers cost 2 x CC registers: 255 allocated, two waves per SIMD)
    const unsigned i0 = (blockIdx.x * 64u + threadIdx.x) * 2u;
    if ((long long)i0 >= inner) return;
    const float *xp = x + (size_t)blockIdx.y * C * inner;
    double *yp = y + (size_t)blockIdx.y * C * inner;
    f2_t v[CC];
#pragma unroll
    for (int c = 0; c < CC; ++c) {
        v[c] = (f2_t){0.f, 0.f};
        if (c < C) v[c] = __builtin_nontemporal_load(reinterpret_cast<const f2_t *>(xp + (size_t)c * inner + i0));
    }
    double s0 = 0.0, s1 = 0.0;
#pragma unroll
    for (int c = 0; c < CC; ++c)
        if (c < C) {
            const double a = (double)v[c].x, b = (double)v[c].y;
            s0 = __builtin_fma(a, a, s0); s1 = __builtin_fma(b, b, s1);
            if ((c & 7) == 7) __builtin_amdgcn_sched_barrier(0);
        }
    // keep the channels as the float32 values they are: without this the compiler holds their float64 conversions (made for the
    // chain above) across to the write phase -- 2 x 2 x CC registers, 255 allocated at CC = 64
#pragma unroll
    for (int c = 0; c < CC; ++c) asm volatile("" : "+v"(v[c]));
    double n[2] = {__builtin_sqrt(s0), __builtin_sqrt(s1)}, g[2], pr[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        n[k] = n[k] < 1e-15 ? 1e-15 : n[k];
        double a = n[k] * ks;
        a = a > 15.0 ? 15.0 : (a < -15.0 ? -15.0 : a);
        g[k] = rks * tanh(a);
        pr[k] = 0.0;
        if (g[k] >= maxnorm * (1.0 - 1e-9)) {                   // rare: only here can project() act
            double s2 = 0.0;
#pragma unroll 1
            for (int c = 0; c < C; ++c) {                      // rare: re-read the pixel's channels (no indexed access into v, and no
                const double w = g[k] * ((double)xp[(size_t)c * inner + i0 + k] / n[k]);       // 2 x CC unrolled divisions kept live)
                s2 = __builtin_fma(w, w, s2);
            }
            double ny = __builtin_sqrt(s2);
            ny = ny < 1e-15 ? 1e-15 : ny;
            pr[k] = ny > maxnorm ? ny : 0.0;
        }
    }
    const double r0 = exact_rcp(n[0]), r1 = exact_rcp(n[1]);
    if (!__any(pr[0] != 0.0 || pr[1] != 0.0)) {                 // (wave-uniform) nothing to project: the common case, from registers
#pragma unroll
        for (int c = 0; c < CC; ++c) {
            if (c < C) {
                const double w0 = g[0] * div_by(v[c].x, n[0], r0), w1 = g[1] * div_by(v[c].y, n[1], r1);
                __builtin_nontemporal_store((d2_h){w0, w1}, reinterpret_cast<d2_h *>(yp + (size_t)c * inner + i0));
                if ((c & 3) == 3) __builtin_amdgcn_sched_barrier(0);      // four channels' conversions live at a time, not CC
            }
        }
    } else {                                                    // a projected pixel in the wave: rolled loop, channels re-read
#pragma unroll 1
        for (int c = 0; c < C; ++c) {
            const f2_t xv = *reinterpret_cast<const f2_t *>(xp + (size_t)c * inner + i0);
            double w0 = g[0] * div_by(xv.x, n[0], r0), w1 = g[1] * div_by(xv.y, n[1], r1);
            if (pr[0] != 0.0) w0 = w0 / pr[0] * maxnorm;
            if (pr[1] != 0.0) w1 = w1 / pr[1] * maxnorm;
            __builtin_nontemporal_store((d2_h){w0, w1}, reinterpret_cast<d2_h *>(yp + (size_t)c * inner + i0));
        }
    }
}

// ---------------------------------------------------------------- logmap0 + project  (hyperbolic.py:60)
__global__ void __launch_bounds__(HTPB) k_logmap0_project(const double *__restrict__ x, double *__restrict__ y, long long outer,
                                                          int C, long long inner, double ks, double rks, double maxnorm)
{
    const long long idx = (long long)blockIdx.x * HTPB + threadIdx.x;
    if (idx >= outer * inner) return;
    const long long o = idx / inner, i = idx % inner;
    const double *xp = x + (size_t)o * C * inner + i;
    double *yp = y + (size_t)o * C * inner + i;
    double ssq = 0.0;
    for (int ch = 0; ch < C; ++ch) { const double v = xp[(size_t)ch * inner]; ssq = __builtin_fma(v, v, ssq); }
    double n = __builtin_sqrt(ssq);
    n = n < 1e-15 ? 1e-15 : n;
    const double g = rks * artanh_clamped(n * ks);
    double s2 = 0.0;
    for (int ch = 0; ch < C; ++ch) {
        const double v = (xp[(size_t)ch * inner] / n) * g;
        yp[(size_t)ch * inner] = v;
        s2 = __builtin_fma(v, v, s2);
    }
    double ny = __builtin_sqrt(s2);
    ny = ny < 1e-15 ? 1e-15 : ny;
    if (ny > maxnorm)
        for (int ch = 0; ch < C; ++ch) yp[(size_t)ch * inner] = yp[(size_t)ch * inner] / ny * maxnorm;
}

// ---------------------------------------------------------------- dist0  (hyperbolic.py:83)
template <typename T>
__global__ void __launch_bounds__(HTPB) k_dist0(const T *__restrict__ x, T *__restrict__ out, long long outer, int C,
                                                long long inner, double ks, double rks)
{
    const long long idx = (long long)blockIdx.x * HTPB + threadIdx.x;
    if (idx >= outer * inner) return;
    const long long o = idx / inner, i = idx % inner;
    const T *xp = x + (size_t)o * C * inner + i;
    T ssq = (T)0;
    for (int ch = 0; ch < C; ++ch) {
        const T v = xp[(size_t)ch * inner];
        if constexpr (sizeof(T) == 8) ssq = __builtin_fma(v, v, ssq); else ssq = __builtin_fmaf(v, v, ssq);
    }
    out[idx] = dist0_from_ssq(ssq, ks, rks);
}

// ---------------------------------------------------------------- dist(x, y) over the last dim  (hyperbolic.py:72)
__global__ void __launch_bounds__(HTPB) k_pdist(const double *__restrict__ x, const double *__restrict__ y,
                                                double *__restrict__ out, long long n, int d, double k, double ks, double rks)
{
    const long long r = (long long)blockIdx.x * HTPB + threadIdx.x;
    if (r >= n) return;
    const double *a = x + (size_t)r * d, *b = y + (size_t)r * d;
    double x2 = 0, y2 = 0, xy = 0;
    for (int j = 0; j < d; ++j) {
        const double u = -a[j], v = b[j];
        x2 = __builtin_fma(u, u, x2); y2 = __builtin_fma(v, v, y2); xy = __builtin_fma(u, v, xy);
    }
    const double ca = 1.0 - 2.0 * k * xy - k * y2, cb = 1.0 + k * x2;
    double den = 1.0 - 2.0 * k * xy + k * k * x2 * y2;
    den = den < 1e-15 ? 1e-15 : den;
    double s2 = 0;
    for (int j = 0; j < d; ++j) { const double m = (ca * (-a[j]) + cb * b[j]) / den; s2 = __builtin_fma(m, m, s2); }
    out[r] = 2.0 * (rks * artanh_clamped(__builtin_sqrt(s2) * ks));
}

// ---------------------------------------------------------------- HyperMLR  (hyperbolic.py:120-184)
// prep: per class  pp = ||P||^2 (as sqrt then square), anorm = ||A||, An = A / max(anorm,1e-12), pa = <-P, An>
// consts layout: [O] pp | [O] anorm | [O] pa | [O*C] An | [O*C] negP
// One wave per class (round 5; rounds 1-4 ran one LANE per class: 19 lanes walking 2 x C uncoalesced doubles each in three
// dependent passes took 78 us at C = 256 -- as long as the contraction it prepares at the head's own shape).  The rows of P and A
// are staged in LDS with coalesced loads, lane 0 runs the three fma chains IN CHANNEL ORDER from there (the same sums as before,
// bit for bit), the element-wise parts (A / ||A||, -P) are spread over the lanes.
__global__ void __launch_bounds__(64) k_mlr_prep(const double *__restrict__ P, const double *__restrict__ A, int O, int C,
                                                 double *__restrict__ consts, double *__restrict__ Wt = nullptr, int wt_half = 0)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_p[];
    double *sP = reinterpret_cast<double *>(smem_p), *sA = sP + C;     // P row | A row, then A^ row in place of A
    __shared__ double s_dn;
    const int o = blockIdx.x, lane = threadIdx.x;
    if (o >= O) return;
    for (int j = lane; j < C; j += 64) { sP[j] = P[(size_t)o * C + j]; sA[j] = A[(size_t)o * C + j]; }
    __syncthreads();
    if (lane == 0) {
        double sp = 0, sa = 0;
        for (int j = 0; j < C; ++j) { sp = __builtin_fma(sP[j], sP[j], sp); sa = __builtin_fma(sA[j], sA[j], sa); }
        const double np_ = __builtin_sqrt(sp), an = __builtin_sqrt(sa);
        consts[o] = np_ * np_;
        consts[O + o] = an;
        s_dn = an < 1e-12 ? 1e-12 : an;
    }
    __syncthreads();
    const double dn = s_dn;
    double *An = consts + 3 * O, *nP = consts + 3 * O + (size_t)O * C;
    for (int j = lane; j < C; j += 64) {
        const double v = sA[j] / dn;
        sA[j] = v;
        An[(size_t)o * C + j] = v;
        nP[(size_t)o * C + j] = -sP[j];
        if (Wt) {                                                        // channel-major image for the fused backward: row j = [-P of classes 0..half-1 | A^ ...]
            Wt[(size_t)j * 2 * wt_half + o] = -sP[j];
            Wt[(size_t)j * 2 * wt_half + wt_half + o] = v;
            if (o == 0)
                for (int q = O; q < wt_half; ++q) { Wt[(size_t)j * 2 * wt_half + q] = 0.0; Wt[(size_t)j * 2 * wt_half + wt_half + q] = 0.0; }
        }
    }
    __syncthreads();
    if (lane == 0) {
        double s_ = 0;
        for (int j = 0; j < C; ++j) s_ = __builtin_fma(-sP[j], sA[j], s_);
        consts[2 * O + o] = s_;
    }
}

__device__ __forceinline__ double clamp_min_nanprop(double v, double lo) { return (v != v) ? v : (v < lo ? lo : v); }

// One pixel per lane; the 2*O prototype rows are read as wave-uniform (scalar) loads; OB classes per pass.
template <int OB, typename TOUT>
__global__ void __launch_bounds__(HTPB) k_hypermlr(const double *__restrict__ x, const double *__restrict__ consts, int O, int C,
                                                   long long hw, double K, TOUT *__restrict__ out)
{
    const int b = blockIdx.y;
    const long long i = (long long)blockIdx.x * HTPB + threadIdx.x;
    if (i >= hw) return;
    const double *xb = x + (size_t)b * C * hw + i;
    const double *pp = consts, *anorm = consts + O, *pa = consts + 2 * O, *An = consts + 3 * O, *nP = consts + 3 * O + (size_t)O * C;
    double ssq = 0.0;
    for (int j = 0; j < C; ++j) { const double v = xb[(size_t)j * hw]; ssq = __builtin_fma(v, v, ssq); }
    const double nx = __builtin_sqrt(ssq), xx = nx * nx;
    const double sqK = __builtin_sqrt(K), maxnorm = (1.0 - 1e-3) / sqK;
    for (int o0 = 0; o0 < O; o0 += OB) {
        double px[OB], xa[OB];
#pragma unroll
        for (int q = 0; q < OB; ++q) { px[q] = 0.0; xa[q] = 0.0; }
        for (int j = 0; j < C; ++j) {
            const double v = xb[(size_t)j * hw];
#pragma unroll
            for (int q = 0; q < OB; ++q) {
                const int o = o0 + q < O ? o0 + q : O - 1;
                px[q] = __builtin_fma(v, nP[(size_t)o * C + j], px[q]);
                xa[q] = __builtin_fma(v, An[(size_t)o * C + j], xa[q]);
            }
        }
#pragma unroll
        for (int q = 0; q < OB; ++q) {
            const int o = o0 + q;
            if (o >= O) break;
            const double ppo = pp[o];
            const double sqsq = ((K * xx) * K) * ppo;
            const double Aa = (1.0 + (2.0 * K) * px[q]) + K * xx;
            const double Bb = 1.0 - K * ppo;
            const double D = clamp_min_nanprop((1.0 + (2.0 * K) * px[q]) + sqsq, 1e-12);
            const double al = Aa / D, be = Bb / D;
            const double mob = ((al * al) * ppo + (be * be) * xx) + ((2.0 * al) * be) * px[q];
            const double sq = __builtin_sqrt(mob);
            const double pn = sq > maxnorm ? maxnorm / clamp_min_nanprop(sq, 1e-12) : 1.0;
            const double mp = sq < maxnorm ? mob : maxnorm * maxnorm;
            const double md = (be * xa[q] + al * pa[o]) * pn;
            const double lamb = 2.0 / clamp_min_nanprop(1.0 - K * mp, 1e-12);
            const double sine = (sqK * md) * lamb;
            out[((size_t)b * O + o) * hw + i] = (TOUT)(((2.0 / sqK) * anorm[o]) * asinh(sine));
        }
    }
}


// ---------------------------------------------------------------- HyperMLR on the f64 matrix cores
// The two feature x prototype contractions  px = <x,-P>  and  xa = <x,A^>  ([Npix x C] . [C x 2O]) run on
// v_mfma_f64_16x16x4_f64:
//   A operand (16 pixels x 4 channels): lane l holds x[channel 4s + (l>>4)][pixel (l&15)]
//   B operand (4 channels x 16 columns): lane l holds Wt[channel 4s + (l>>4)][column (l&15)]
//   D (16 x 16): lane l holds column (l&15), rows (l>>4) + 4r, r = 0..3
// Column tiles (NT of them, 16 columns each) keep the -P and A^ column of a class in ONE lane:
//   NT = 2 (O <= 16): [-P 0..15 | A^ 0..15]
//   NT = 3 (O <= 24): [-P 0..15 | A^ 0..15 | -P 16..23, A^ 16..23]   (the last tile pairs lane j with lane j+8)
//   NT = 4 (O <= 32): [-P 0..15 | A^ 0..15 | -P 16..31 | A^ 16..31]
// so 19 classes cost 3 MFMAs per 16 pixels x 4 channels (38 of 48 columns useful).  ||x||^2 is accumulated
// on the VALU beside the matrix pipe (lane (l&15, l>>4) sums channels = l>>4 mod 4, combined at the end).
// Weight chunks (MLR_KC channels) are staged in LDS; x is read once, straight from its NCHW planes
// (16 consecutive pixels = one 128-byte line per 16 lanes); results leave through an LDS transpose as
// contiguous class rows.
typedef double v4d_t __attribute__((ext_vector_type(4)));
constexpr int MLR_KC = 32, MLR_MT = 2, MLR_WPAD = 1;

template <typename TOUT, int NT>
__global__ void __launch_bounds__(HTPB) k_hypermlr_mfma(const double *__restrict__ x, const double *__restrict__ consts, int O,
                                                        int C, long long hw, double K, TOUT *__restrict__ out)
{
    __shared__ double wts[NT * 16][MLR_KC + MLR_WPAD];
    __shared__ double xx_s[HTPB / 64][MLR_MT][16];
    __shared__ TOUT out_s[HTPB / 64][NT == 2 ? 16 : (NT == 3 ? 24 : 32)][MLR_MT * 16 + 1];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lc = lane & 15, lk = lane >> 4;
    const long long p_base = ((long long)blockIdx.x * (HTPB / 64) + wave) * (MLR_MT * 16);
    const double *xb = x + (size_t)b * C * hw;
    const double *pp = consts, *anorm = consts + O, *pa = consts + 2 * O, *An = consts + 3 * O, *nP = consts + 3 * O + (size_t)O * C;
    v4d_t acc[MLR_MT][NT];
    double ss[MLR_MT];
#pragma unroll
    for (int m = 0; m < MLR_MT; ++m) {
        ss[m] = 0.0;
#pragma unroll
        for (int n = 0; n < NT; ++n) acc[m][n] = (v4d_t){0, 0, 0, 0};
    }
    long long pix[MLR_MT];
#pragma unroll
    for (int m = 0; m < MLR_MT; ++m) pix[m] = p_base + m * 16 + lc;
    // x operands of a whole chunk (MLR_KC/4 k-steps x MLR_MT tiles) are requested up front and one chunk
    // ahead, so their HBM latency hides behind the previous chunk's MFMAs and the weight staging
    auto load_chunk = [&](int c0, double (&dst)[MLR_KC / 4][MLR_MT]) {
#pragma unroll
        for (int kk = 0; kk < MLR_KC / 4; ++kk) {
            const int c = c0 + kk * 4 + lk;
#pragma unroll
            for (int m = 0; m < MLR_MT; ++m) dst[kk][m] = (c < C && pix[m] < hw) ? xb[(size_t)c * hw + pix[m]] : 0.0;
        }
    };
    double a_cur[MLR_KC / 4][MLR_MT], a_nxt[MLR_KC / 4][MLR_MT];
    load_chunk(0, a_cur);
    for (int c0 = 0; c0 < C; c0 += MLR_KC) {
        if (c0 + MLR_KC < C) load_chunk(c0 + MLR_KC, a_nxt);
        __syncthreads();
        for (int e = tid; e < NT * 16 * MLR_KC; e += HTPB) {
            const int j = e / MLR_KC, k = e % MLR_KC, c = c0 + k;
            const int tile = j >> 4, col = j & 15;
            int cls;
            bool isA;
            if (tile == 0) { cls = col; isA = false; }
            else if (tile == 1) { cls = col; isA = true; }
            else if (NT == 3) { cls = 16 + (col & 7); isA = col >= 8; }
            else { cls = 16 + col; isA = tile == 3; }
            double v = 0.0;
            if (cls < O && c < C) v = isA ? An[(size_t)cls * C + c] : nP[(size_t)cls * C + c];
            wts[j][k] = v;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < MLR_KC / 4; ++kk) {
#pragma unroll
            for (int n = 0; n < NT; ++n) {
                const double bf = wts[n * 16 + lc][kk * 4 + lk];
#pragma unroll
                for (int m = 0; m < MLR_MT; ++m) acc[m][n] = __builtin_amdgcn_mfma_f64_16x16x4f64(a_cur[kk][m], bf, acc[m][n], 0, 0, 0);
            }
#pragma unroll
            for (int m = 0; m < MLR_MT; ++m) ss[m] = __builtin_fma(a_cur[kk][m], a_cur[kk][m], ss[m]);
        }
#pragma unroll
        for (int kk = 0; kk < MLR_KC / 4; ++kk)
#pragma unroll
            for (int m = 0; m < MLR_MT; ++m) a_cur[kk][m] = a_nxt[kk][m];
    }
    // ||x||^2 of pixel lc: the four channel-residue partial sums live in lanes lc, lc+16, lc+32, lc+48
#pragma unroll
    for (int m = 0; m < MLR_MT; ++m) {
        double t = ss[m] + __shfl_xor(ss[m], 16);
        t = t + __shfl_xor(t, 32);
        if (lk == 0) xx_s[wave][m][lc] = t;
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0): this wave's LDS writes before its own reads
    __builtin_amdgcn_wave_barrier();
    const double sqK = __builtin_sqrt(K), maxnorm = (1.0 - 1e-3) / sqK;
    auto logit_of = [&](double px, double xa, double ssq, int o) -> double {
        const double ppo = pp[o], ano = anorm[o], pao = pa[o];
        const double nx = __builtin_sqrt(ssq), xx = nx * nx;          // torch.norm(x)**2, hyperbolic.py:136
        const double sqsq = ((K * xx) * K) * ppo;
        const double Aa = (1.0 + (2.0 * K) * px) + K * xx;
        const double Bb = 1.0 - K * ppo;
        const double D = clamp_min_nanprop((1.0 + (2.0 * K) * px) + sqsq, 1e-12);
        const double al = Aa / D, be = Bb / D;
        const double mob = ((al * al) * ppo + (be * be) * xx) + ((2.0 * al) * be) * px;
        const double sq = __builtin_sqrt(mob);
        const double pn = sq > maxnorm ? maxnorm / clamp_min_nanprop(sq, 1e-12) : 1.0;
        const double mp = sq < maxnorm ? mob : maxnorm * maxnorm;
        const double md = (be * xa + al * pao) * pn;
        const double lamb = 2.0 / clamp_min_nanprop(1.0 - K * mp, 1e-12);
        const double sine = (sqK * md) * lamb;
        return ((2.0 / sqK) * ano) * asinh(sine);
    };
#pragma unroll
    for (int m = 0; m < MLR_MT; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = lk + 4 * r;
            const double ssq = xx_s[wave][m][row];
            if (lc < O) out_s[wave][lc][m * 16 + row] = (TOUT)logit_of(acc[m][0][r], acc[m][1][r], ssq, lc);
            if constexpr (NT == 3) {
                const double xa_hi = __shfl(acc[m][2][r], (lane + 8) & 63);      // A^ column of class 16 + lc sits 8 lanes up
                const int o = 16 + lc;
                if (lc < 8 && o < O) out_s[wave][o][m * 16 + row] = (TOUT)logit_of(acc[m][2][r], xa_hi, ssq, o);
            } else if constexpr (NT == 4) {
                const int o = 16 + lc;
                if (o < O) out_s[wave][o][m * 16 + row] = (TOUT)logit_of(acc[m][2][r], acc[m][3][r], ssq, o);
            }
        }
    __builtin_amdgcn_s_waitcnt(0xc07f);
    __builtin_amdgcn_wave_barrier();
    // coalesced store: each class row of this wave's 32 pixels is contiguous in the (B,O,hw) output
    for (int e = lane; e < O * (MLR_MT * 16); e += 64) {
        const int o = e / (MLR_MT * 16), q = e % (MLR_MT * 16);
        const long long p = p_base + q;
        if (p < hw) out[((size_t)b * O + o) * hw + p] = out_s[wave][o][q];
    }
}

// ---------------------------------------------------------------- HyperMLR, weights resident in LDS
// Same operand layout and contraction as k_hypermlr_mfma, restructured around what that kernel waits for:
//   * ALL of [-P | A^] (NT*16 rows x C channels, 98 KiB at C = 256) is staged in LDS once per workgroup, and the
//     workgroup's 8 waves then walk pixel tiles on their own -- no barrier and no weight traffic inside the loop
//     (the chunked kernel re-staged 12 KiB behind two barriers for every 32 channels);
//   * 8 waves = two per SIMD sharing that one weight image: while one wave runs its VALU epilogue the other keeps
//     the SIMD's matrix pipe busy (the f64 epilogue costs about as many issue cycles as the contraction);
//   * a lane's two row tiles are the EVEN and ODD pixel of a pair, so one 16-byte load feeds both MFMA operands;
//   * the epilogue shares one reciprocal of D between alpha and beta, and evaluates the projection quotient only
//     in waves that hold a pixel beyond maxnorm.
// Row stride of the weight image = C + pad doubles with (C + pad) mod 32 == 2: the 16 x 4 (row, channel) operand
// fetch of a wave is then conflict-free on the 64 LDS banks.
// ---- asinh / reciprocal for the matrix-core HyperMLR epilogue, where no bit-level contract exists (kept out of halo_devmath.hpp: that
// header holds the bit-exact recipes and is also compiled on the host by tests/native/devmath_host_check.cpp)
// -- no bit-level contract (the logits are within 1e-10 of the
// reference's; the acquisition's parity starts FROM the logits): every quotient a / b is a * rcp(b) with the reciprocal refined by
// two Newton steps from v_rcp_f64 (<= 1 ulp; 5 instructions where the IEEE division sequence takes 12-15: scaling, fixup), valid
// for finite b of ordinary magnitude -- the epilogue's denominators are clamped to >= 1e-12 or lie in [1, 1e150].
__device__ __forceinline__ double fast_rcp(double b)
{
    const double r0 = __builtin_amdgcn_rcp(b);
    double r = __builtin_fma(__builtin_fma(-b, r0, 1.0), r0, r0);
    r = __builtin_fma(__builtin_fma(-b, r, 1.0), r, r);
    return __builtin_fabs(b) == __builtin_inf() ? r0 : r;       // 1 / inf = 0 (the refinement would make it NaN); NaN stays NaN
}
// log of a double in [1, 1e300): log_core_ with its one quotient through fast_rcp
__device__ __forceinline__ double log_ge1_fast(double x)
{
    const double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10,
                 Lg1 = 6.666666666666735130e-01, Lg2 = 3.999999999940941908e-01,
                 Lg3 = 2.857142874366239149e-01, Lg4 = 2.222219843214978396e-01,
                 Lg5 = 1.818357216161805012e-01, Lg6 = 1.531383769920937332e-01,
                 Lg7 = 1.479819860511658591e-01;
    uint64_t u = (uint64_t)__double_as_longlong(x);
    uint32_t hx = (uint32_t)(u >> 32);
    hx += 0x3ff00000u - 0x3fe6a09eu;
    const int k = (int)(hx >> 20) - 0x3ff;
    hx = (hx & 0x000fffffu) + 0x3fe6a09eu;
    u = ((uint64_t)hx << 32) | (u & 0xffffffffull);
    const double f = __longlong_as_double((long long)u) - 1.0;
    const double hfsq = (0.5 * f) * f;
    const double s = f * fast_rcp(2.0 + f);
    const double z = s * s, w = z * z;
    const double t1 = w * __builtin_fma(w, __builtin_fma(w, Lg6, Lg4), Lg2);
    const double t2 = z * __builtin_fma(w, __builtin_fma(w, __builtin_fma(w, Lg7, Lg5), Lg3), Lg1);
    const double R = t2 + t1, dk = (double)k;
    return __builtin_fma(dk, ln2_hi, (f - (hfsq - __builtin_fma(s, hfsq + R, dk * ln2_lo))));
}
__device__ __forceinline__ double asinh_fast(double x)
{
    const double a = __builtin_fabs(x), a2 = a * a;
    const double t = a + a2 * fast_rcp(1.0 + __builtin_sqrt(1.0 + a2));
    const double u = 1.0 + t;
    // |x| beyond ~1e150 (a2 overflows) or NaN: the exact-order statement handles it
    const double r = (a < 1e150) ? log_ge1_fast(u) + (t - (u - 1.0)) * fast_rcp(u) : __builtin_fabs(asinh_det(x));
    return x != x ? x : __builtin_copysign(r, x);
}

constexpr int MLRP_TPB = 512, MLRP_SK = 4, MLRP_RING = 4;
#ifndef HALO_MLR_EP
#define HALO_MLR_EP 2
#endif
constexpr int MLR_EP = HALO_MLR_EP;       // classes per epilogue trip.  v2 head / 1024x2048x256, same box: 1 -> 193 us / 1.156 ms, 2 -> 180 / 1.128, 3 -> 190 / 1.152 (256 VGPRs + scratch)
#ifdef HALO_MLR_IEEE            // variant build for A/B (HALO_LIB_PATH): the round-4 epilogue, IEEE divisions
#define MLR_RCP(x) (1.0 / (x))
#define MLR_ASINH(x) asinh_det(x)
#else
#define MLR_RCP(x) fast_rcp(x)
#define MLR_ASINH(x) asinh_fast(x)
#endif
// hyperbolic.py:146-181 in the reference's own order (alpha, beta, the norm of the Mobius sum, its projection, lambda) for one
// (pixel, class): returns asinh(sineterm).  The matrix-core kernel's epilogue until round 5; now its rare arm and its A/B twin.
__device__ __forceinline__ double mlr_epilogue_ref(double px, double xa, double ppo, double pao, double xx, double Kxx, double KxxK,
                                                   double K, double sqK, double maxnorm)
{
    const double sqsq = KxxK * ppo;
    const double base = 1.0 + (2.0 * K) * px;
    const double Aa = base + Kxx;
    const double Bb = 1.0 - K * ppo;
    const double rD = MLR_RCP(clamp_min_nanprop(base + sqsq, 1e-12));   // one reciprocal for alpha and beta
    const double al = Aa * rD, be = Bb * rD;
    const double mob = ((al * al) * ppo + (be * be) * xx) + ((2.0 * al) * be) * px;
    const double sq = __builtin_sqrt(mob);
    const double pn = sq > maxnorm ? maxnorm / clamp_min_nanprop(sq, 1e-12) : 1.0;
    const double mp = sq < maxnorm ? mob : maxnorm * maxnorm;
    const double md = (be * xa + al * pao) * pn;
    const double lamb = 2.0 * MLR_RCP(clamp_min_nanprop(1.0 - K * mp, 1e-12));
    return MLR_ASINH((sqK * md) * lamb);
}
// 1/b, 1/sqrt(b), sqrt(b) for b finite, positive and of ordinary magnitude (no specials: the callers test their operands): the
// hardware estimate (v_rcp_f64 / v_rsq_f64, relative error e0 <= 2^-23) corrected through the SECOND-order term of its own
// residual -- r0 (1 + e + e^2), y0 (1 + e/2 + 3 e^2 / 8) -- so that ONE step leaves O(e0^3) < 2^-64 and the result is the rounding
// of the last fma (<= 1 ulp); the IEEE sequences hipcc emits (scaling, two steps, fix-up) are 12-15 instructions each.
__device__ __forceinline__ double rcp_q(double b)
{
    const double r0 = __builtin_amdgcn_rcp(b);
    const double e = __builtin_fma(-b, r0, 1.0);
    return __builtin_fma(__builtin_fma(e, e, e), r0, r0);
}
__device__ __forceinline__ double rsqrt_q(double b)
{
    const double y0 = __builtin_amdgcn_rsq(b);
    const double e = __builtin_fma(-(b * y0), y0, 1.0);
    return __builtin_fma(y0 * e, __builtin_fma(0.375, e, 0.5), y0);
}
__device__ __forceinline__ double sqrt_q(double b) { return b * rsqrt_q(b); }
// log_ge1_fast with its quotient through rcp_q (2 + f in [2.41, 3.42))
__device__ __forceinline__ double log_ge1_q(double x)
{
    const double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10,
                 Lg1 = 6.666666666666735130e-01, Lg2 = 3.999999999940941908e-01,
                 Lg3 = 2.857142874366239149e-01, Lg4 = 2.222219843214978396e-01,
                 Lg5 = 1.818357216161805012e-01, Lg6 = 1.531383769920937332e-01,
                 Lg7 = 1.479819860511658591e-01;
    uint64_t u = (uint64_t)__double_as_longlong(x);
    uint32_t hx = (uint32_t)(u >> 32);
    hx += 0x3ff00000u - 0x3fe6a09eu;
    const int k = (int)(hx >> 20) - 0x3ff;
    hx = (hx & 0x000fffffu) + 0x3fe6a09eu;
    u = ((uint64_t)hx << 32) | (u & 0xffffffffull);
    const double f = __longlong_as_double((long long)u) - 1.0;
    const double hfsq = (0.5 * f) * f;
    const double s = f * rcp_q(2.0 + f);
    const double z = s * s, w = z * z;
    const double t1 = w * __builtin_fma(w, __builtin_fma(w, Lg6, Lg4), Lg2);
    const double t2 = z * __builtin_fma(w, __builtin_fma(w, __builtin_fma(w, Lg7, Lg5), Lg3), Lg1);
    const double R = t2 + t1, dk = (double)k;
    return __builtin_fma(dk, ln2_hi, (f - (hfsq - __builtin_fma(s, hfsq + R, dk * ln2_lo))));
}

// The epilogue of one 32-pixel tile, shared by the matrix-core kernels below: the wave's accumulators (px = <x,-P>, xa = <x,A^> per
// class, and the four channel-residue partial sums of ||x||^2) go through the wave's LDS staging rows into a flat (class, pixel)
// mapping, where the Moebius / projection / asinh algebra runs and the logits are stored.
template <typename TOUT, int NT>
__device__ __forceinline__ void mlr_tile_epilogue(v4d_t (&acc)[2][NT], double (&ss)[2], double *pxs, double *xas, double *xs, int lane, int lc,
                                                  int lk, int O, const double *pp, const double *anorm, const double *pa, double K, double K2,
                                                  double sqK, double maxnorm, double maxn2, double c_in, double c_out, double oscale, long long b,
                                                  long long p_base, long long hw, TOUT *__restrict__ out, int force_ref)
{
    // ---- hand the accumulators to a flat (class, pixel) mapping through LDS: in the MFMA layout a lane would run
    // the f64 epilogue 16 times per tile (8 rows x 2 class slots, the second slot 3/16 useful at 19 classes); flat,
    // 32 pixels x O classes over 64 lanes is O/2 evaluations.  Pixel q = 2 * row + m; slot of (class o, pixel q) is
    // o*32 + ((q + o) & 31): conflict-free for the column-wise writes and the row-wise reads alike.
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        double t_ = ss[m] + __shfl_xor(ss[m], 16);               // ||x||^2 of row lc: four channel-residue partial sums
        t_ = t_ + __shfl_xor(t_, 32);
        if (lk == 0) xs[2 * lc + m] = t_;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int q = 2 * (lk + 4 * r) + m;
            if (lc < O) {
                pxs[lc * 32 + ((q + lc) & 31)] = acc[m][0][r];
                xas[lc * 32 + ((q + lc) & 31)] = acc[m][1][r];
            }
            if constexpr (NT == 3) {
                const int o = 16 + (lc & 7);
                if (o < O) (lc < 8 ? pxs : xas)[o * 32 + ((q + o) & 31)] = acc[m][2][r];
            } else if constexpr (NT == 4) {
                const int o = 16 + lc;
                if (o < O) {
                    pxs[o * 32 + ((q + o) & 31)] = acc[m][2][r];
                    xas[o * 32 + ((q + o) & 31)] = acc[m][3][r];
                }
            }
        }
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0): this wave's LDS writes before its own reads
    __builtin_amdgcn_wave_barrier();
    // A lane's pixel is the same in every iteration (e advances by 64, q = e & 31): everything that depends on the pixel alone
    // -- torch.norm(x)**2 with its square root, K xx, K xx K -- is evaluated once per lane and tile, not once per class
    // (round 4 took the square root O/2 times per lane: VERDICT r4 #6)
    const int q = lane & 31;
    const double nx = __builtin_sqrt(xs[q]), xx = nx * nx;                // torch.norm(x)**2, hyperbolic.py:136
    const double Kxx = K * xx, KxxK = Kxx * K;
    const long long p_ = p_base + q;
    TOUT *outp = out + (size_t)b * O * hw + p_;
    // MLR_EP classes per trip (o, o + 2, ...: a half-wave owns every other class), each phase written for all of them before
    // the next so that their dependent chains interleave inside one basic block; the wave-uniform tests sit between phases.
#pragma unroll 1
    for (int o0 = lane >> 5; o0 < O; o0 += 2 * MLR_EP) {
        // ---- ONE quotient per logit (round 5).  With A = 1 + 2K px + K xx, B = 1 - K pp, D = 1 + 2K px + K^2 xx pp the reference's
        // alpha = A/D, beta = B/D give  mob = N / D^2,  N = A^2 pp + B^2 xx + 2AB px,  and  mobdota = M / D,  M = B xa + A pa:
        //   inside the ball (N < maxnorm^2 D^2):  sine = sqrt(K) (M/D) 2 / (1 - K N/D^2)           = 2 sqrt(K) M D / (D^2 - K N)
        //   beyond it (projected onto maxnorm):   sine = sqrt(K) (M/D) (maxnorm D / sqrt(N)) lamb_max = sqrt(K) lamb_max maxnorm M / sqrt(N)
        // -- the same real-number function as hyperbolic.py:146-181 (both arms are continuous across the boundary, so WHICH side a
        // pixel within an ulp of it lands on moves the logit by an ulp), evaluated with one refined reciprocal (or reciprocal
        // square root) instead of two reciprocals, a square root and a comparison of roots.  The clamps of the reference cannot
        // act here: D >= 1e-12 is tested (anything else -- NaN included -- takes the reference-order statement below), and
        // 1 - K mob > 1 - K maxnorm^2 = 2e-3 inside the ball.  asinh(s) = log(|s| + sqrt(1 + s^2)): absolute error <= 2 ulp(1)
        // (the logits carry no relative contract near zero: tolerance 1e-10 absolute, tests/test_gpu_parity.py).
        double px[MLR_EP], xa[MLR_EP], ppo[MLR_EP], ano[MLR_EP], pao[MLR_EP], N[MLR_EP], M[MLR_EP], D[MLR_EP], G[MLR_EP], res[MLR_EP], a[MLR_EP], sine[MLR_EP];
        bool inside[MLR_EP], all_in = true, all_ok = !force_ref;
#pragma unroll
        for (int j = 0; j < MLR_EP; ++j) {
            const int o = o0 + 2 * j < O ? o0 + 2 * j : o0;               // a trip's surplus slots repeat its first class (never stored)
            const int sl = o * 32 + ((q + o) & 31);
            px[j] = pxs[sl]; xa[j] = xas[sl];
            ppo[j] = pp[o]; ano[j] = anorm[o]; pao[j] = pa[o];
        }
#pragma unroll
        for (int j = 0; j < MLR_EP; ++j) {
            const double base = __builtin_fma(K2, px[j], 1.0);
            const double Aa = base + Kxx;
            D[j] = __builtin_fma(KxxK, ppo[j], base);
            const double Bb = __builtin_fma(-K, ppo[j], 1.0);
            N[j] = __builtin_fma(Aa * Aa, ppo[j], __builtin_fma(Bb * Bb, xx, ((2.0 * Aa) * Bb) * px[j]));
            M[j] = __builtin_fma(Bb, xa[j], Aa * pao[j]);
            const double D2 = D[j] * D[j];
            inside[j] = N[j] < maxn2 * D2;
            all_in = all_in && inside[j];
            G[j] = (c_in * D[j]) * rcp_q(__builtin_fma(-K, N[j], D2));
        }
        if (__any(!all_in)) {                                             // wave-uniform skip: no pixel of the wave beyond the ball
#pragma unroll
            for (int j = 0; j < MLR_EP; ++j) G[j] = inside[j] ? G[j] : c_out * rsqrt_q(N[j]);
        }
#pragma unroll
        for (int j = 0; j < MLR_EP; ++j) {
            sine[j] = M[j] * G[j]; a[j] = __builtin_fabs(sine[j]);
            all_ok = all_ok && (D[j] >= 1e-12 && a[j] < 1e150);
            res[j] = __builtin_copysign(log_ge1_q(a[j] + sqrt_q(__builtin_fma(a[j], a[j], 1.0))), sine[j]);
        }
        if (__any(!all_ok)) {                                             // never in a trained head: clamped D, NaN / inf, |sine| ~ 1e150
#pragma unroll
            for (int j = 0; j < MLR_EP; ++j) {
                const double ref = mlr_epilogue_ref(px[j], xa[j], ppo[j], pao[j], xx, Kxx, KxxK, K, sqK, maxnorm);
                res[j] = (force_ref || !(D[j] >= 1e-12 && a[j] < 1e150)) ? ref : res[j];
            }
        }
#pragma unroll
        for (int j = 0; j < MLR_EP; ++j)
            if (p_ < hw && o0 + 2 * j < O) outp[(size_t)(o0 + 2 * j) * hw] = (TOUT)((oscale * ano[j]) * res[j]);
    }
}

template <typename TOUT, int NT>
__global__ void __launch_bounds__(MLRP_TPB) k_hypermlr_mfma_res(const double *__restrict__ x, const double *__restrict__ consts,
                                                                int O, int C, int wstride, long long hw, long long tiles_per_img,
                                                                long long ntiles, double K, TOUT *__restrict__ out, int force_ref)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_m[];
    double *wts = reinterpret_cast<double *>(smem_m);                                        // [2*O][wstride]: rows -P 0..O-1, then A^ 0..O-1
    double *stage = wts + (size_t)2 * O * wstride;                                           // per wave: px [O][32] | xa [O][32] | ||x||^2 [32]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lc = lane & 15, lk = lane >> 4;
    const double *pp = consts, *anorm = consts + O, *pa = consts + 2 * O, *An = consts + 3 * O, *nP = consts + 3 * O + (size_t)O * C;
    for (int j = wave; j < 2 * O; j += MLRP_TPB / 64) {
        const double *srow = j < O ? nP + (size_t)j * C : An + (size_t)(j - O) * C;
        for (int k = lane; k < C; k += 64) wts[(size_t)j * wstride + k] = srow[k];
    }
    __syncthreads();
    // this lane's B-operand rows: column lc of tile n is (class, -P | A^) = tile 0: (lc, P)  tile 1: (lc, A)
    // tile 2 of NT = 3: (16 + (lc & 7), lc >= 8)   tiles 2 / 3 of NT = 4: (16 + lc, P / A); columns of classes >= O are zero
    int wrow[NT];
    bool wok[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        int cls = lc;
        bool isA = n == 1;
        if (n >= 2) {
            if (NT == 3) { cls = 16 + (lc & 7); isA = lc >= 8; }
            else { cls = 16 + lc; isA = n == 3; }
        }
        wok[n] = cls < O;
        wrow[n] = ((isA ? O : 0) + (cls < O ? cls : 0)) * wstride;
    }
    const double sqK = __builtin_sqrt(K), maxnorm = (1.0 - 1e-3) / sqK;
    const double K2 = 2.0 * K, maxn2 = maxnorm * maxnorm, c_in = 2.0 * sqK, oscale = 2.0 / sqK,
                 c_out = (sqK * maxnorm) * (2.0 / (1.0 - K * maxn2));      // sqrt(K) maxnorm lamb(maxnorm^2)
    double *pxs = stage + (size_t)wave * (2 * O * 32 + 32), *xas = pxs + O * 32, *xs = xas + O * 32;
    // x operands travel through a register ring of MLRP_RING stages of MLRP_SK k-steps (16 channels) each: the loads
    // of stage s + RING - 1 are issued before the MFMAs of stage s, and the stream of stages runs ACROSS tile
    // boundaries (the first stages of the wave's next tile are in flight during this tile's epilogue).
    const int nst = C / (4 * MLRP_SK);                               // stages per tile; host: C % (4*SK*RING) == 0
    const long long tile0 = (long long)blockIdx.x * (MLRP_TPB / 64) + wave, tstride = (long long)gridDim.x * (MLRP_TPB / 64);
    // Loads are unconditional 16-byte pairs (host: hw even): a lane whose pixel pair lies beyond the image, or a
    // look-ahead past the wave's last tile, reads a clamped valid address instead and its results are never stored.
    struct TileRef { const double *q; long long b, p_base; };
    auto tile_ref = [&](long long tile) {
        TileRef t_;
        const long long tl = tile < ntiles ? tile : ntiles - 1;
        t_.b = tl / tiles_per_img;
        t_.p_base = (tl % tiles_per_img) * 32;
        long long pix0 = t_.p_base + 2 * lc;                        // this lane's pixel pair: row lc of tile m = 0 (even) and m = 1 (odd)
        pix0 = pix0 + 1 < hw ? pix0 : hw - 2;
        t_.q = x + (size_t)t_.b * C * hw + pix0;
        return t_;
    };
    auto issue = [&](const TileRef &t_, int st, double (&dst)[MLRP_SK][2]) {
#pragma unroll
        for (int kk = 0; kk < MLRP_SK; ++kk) {
            const d2_h v = *reinterpret_cast<const d2_h *>(t_.q + (size_t)(st * (4 * MLRP_SK) + kk * 4 + lk) * hw);
            dst[kk][0] = v.x; dst[kk][1] = v.y;
        }
    };
    double ring[MLRP_RING][MLRP_SK][2];
    TileRef cur = tile_ref(tile0);
#pragma unroll
    for (int u = 0; u < MLRP_RING - 1; ++u) issue(cur, u, ring[u]);
    for (long long tile = tile0; tile < ntiles; tile += tstride) {
        const TileRef nxt = tile_ref(tile + tstride);
        const long long b = cur.b, p_base = cur.p_base;
        v4d_t acc[2][NT];
        double ss[2] = {0.0, 0.0};
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int n = 0; n < NT; ++n) acc[m][n] = (v4d_t){0, 0, 0, 0};
        for (int s0 = 0; s0 < nst; s0 += MLRP_RING) {
#pragma unroll
            for (int u = 0; u < MLRP_RING; ++u) {
                const int st = s0 + u, ahead = st + MLRP_RING - 1;  // stage `ahead` lives in slot ahead % RING = (u + RING - 1) % RING
                if (ahead < nst) issue(cur, ahead, ring[(u + MLRP_RING - 1) % MLRP_RING]);
                else issue(nxt, ahead - nst, ring[(u + MLRP_RING - 1) % MLRP_RING]);
#pragma unroll
                for (int kk = 0; kk < MLRP_SK; ++kk) {
                    const int k = st * (4 * MLRP_SK) + kk * 4 + lk;
#pragma unroll
                    for (int n = 0; n < NT; ++n) {
                        // unconditional read (wrow points at a valid row for padding columns too), then a select: a read under a lane
                        // condition is a branch region with its own lgkmcnt(0) in front of the MFMA that uses it -- and cost 37 registers
                        const double bfv = wts[wrow[n] + k];
                        const double bf = wok[n] ? bfv : 0.0;
#pragma unroll
                        for (int m = 0; m < 2; ++m) acc[m][n] = __builtin_amdgcn_mfma_f64_16x16x4f64(ring[u][kk][m], bf, acc[m][n], 0, 0, 0);
                    }
#pragma unroll
                    for (int m = 0; m < 2; ++m) ss[m] = __builtin_fma(ring[u][kk][m], ring[u][kk][m], ss[m]);
                }
            }
        }
        mlr_tile_epilogue<TOUT, NT>(acc, ss, pxs, xas, xs, lane, lc, lk, O, pp, anorm, pa, K, K2, sqK, maxnorm, maxn2, c_in, c_out, oscale, b, p_base,
                                    hw, out, force_ref);
        __builtin_amdgcn_wave_barrier();      // the next tile's accumulators reuse the staging rows
        cur = nxt;
    }
}

// ---------------------------------------------------------------- the head tail in one kernel (C == 64)
// embed = project(expmap0(feat)) and out = HyperMLR(embed) (classifier.py:364-379, 552-558) for the heads' own channel count
// (MODEL.HYPER_DIM = 64, defaults.py:14), inference only.  k_hypermlr_mfma_res with its x operand PRODUCED in place: a wave loads
// the float32 features of its 32-pixel tile in the matrix-core operand layout (a lane: 16 channels of one pixel pair), parks
// them in its LDS staging rows, lanes 0..31 run one pixel's norm chain each IN CHANNEL ORDER (the contract's sum, section 2 of
// bit for bit what k_expmap0_project_regs computes), every lane then forms its 32 embedding values -- g * (x / n)
// through the division sequence's own refinement, the projection where it acts -- stores them (the head returns the
// embedding) and feeds them to the MFMAs it would otherwise have loaded them for.  Same embedding and same logits, bit for bit,
// as the two-kernel path (tests/test_gpu_parity.py); the 8 bytes per channel and pixel that path re-reads never leave the chip,
// and the exponential map's ~6 float64 operations per channel ride on a kernel that the FP64 pipe bounds anyway.
constexpr int HT_C = 64, HT_TS = 34;      // channels; row stride (floats) of the per-wave feature tile: 8-byte aligned rows, lk rows on distinct banks

template <typename TOUT, int NT>
__global__ void __launch_bounds__(MLRP_TPB) k_head_tail_c64(const float *__restrict__ z, const double *__restrict__ consts, int O, int wstride,
                                                            int wave_doubles, long long hw, long long tiles_per_img, long long ntiles, double K,
                                                            double ks, double rks, double maxnorm_e, double *__restrict__ embed,
                                                            TOUT *__restrict__ out, int force_ref)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_h[];
    double *wts = reinterpret_cast<double *>(smem_h);                                        // [2*O][wstride]: rows -P 0..O-1, then A^ 0..O-1
    double *stage = wts + (size_t)2 * O * wstride;                                           // per wave: the feature tile + (n, g, projection norm), THEN px | xa | ||x||^2
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lc = lane & 15, lk = lane >> 4;
    const double *pp = consts, *anorm = consts + O, *pa = consts + 2 * O, *An = consts + 3 * O, *nP = consts + 3 * O + (size_t)O * HT_C;
    for (int j = wave; j < 2 * O; j += MLRP_TPB / 64) {
        const double *srow = j < O ? nP + (size_t)j * HT_C : An + (size_t)(j - O) * HT_C;
        wts[(size_t)j * wstride + lane] = srow[lane];
    }
    __syncthreads();
    int wrow[NT];
    bool wok[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        int cls = lc;
        bool isA = n == 1;
        if (n >= 2) {
            if (NT == 3) { cls = 16 + (lc & 7); isA = lc >= 8; }
            else { cls = 16 + lc; isA = n == 3; }
        }
        wok[n] = cls < O;
        wrow[n] = ((isA ? O : 0) + (cls < O ? cls : 0)) * wstride;
    }
    const double sqK = __builtin_sqrt(K), maxnorm = (1.0 - 1e-3) / sqK;
    const double K2 = 2.0 * K, maxn2 = maxnorm * maxnorm, c_in = 2.0 * sqK, oscale = 2.0 / sqK,
                 c_out = (sqK * maxnorm) * (2.0 / (1.0 - K * maxn2));
    double *wv = stage + (size_t)wave * wave_doubles;
    double *pxs = wv, *xas = pxs + O * 32, *xs = xas + O * 32;                               // the epilogue's view of the wave's rows
    float *tile = reinterpret_cast<float *>(wv);                                              // the expmap's view: [64][HT_TS] floats ...
    double *sn = wv + (HT_C * HT_TS) / 2, *sg = sn + 32, *spr = sg + 32;                      // ... then n, g, projection norm per pixel
    const long long tile0 = (long long)blockIdx.x * (MLRP_TPB / 64) + wave, tstride = (long long)gridDim.x * (MLRP_TPB / 64);
    // (Tried: the loads of tile t + 1 issued behind tile t's contraction into the registers the embedding frees -- 256 registers + scratch,
    // 240 against 223 us at the v2 head; two waves per SIMD hide a tile's load latency behind the other wave's contraction already.)
    for (long long tl = tile0; tl < ntiles; tl += tstride) {
        const long long b = tl / tiles_per_img, p_base = (tl % tiles_per_img) * 32;
        long long pix0 = p_base + 2 * lc;
        const bool pair_ok = pix0 + 1 < hw;                        // hw is even: a pair is inside the image or outside it
        pix0 = pair_ok ? pix0 : hw - 2;                            // clamped loads, results never stored
        const float *zq = z + (size_t)b * HT_C * hw + pix0;
        f2_t zr[16];
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) zr[kk] = *reinterpret_cast<const f2_t *>(zq + (size_t)(kk * 4 + lk) * hw);
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) *reinterpret_cast<f2_t *>(tile + (kk * 4 + lk) * HT_TS + 2 * lc) = zr[kk];
        __builtin_amdgcn_s_waitcnt(0xc07f);
        __builtin_amdgcn_wave_barrier();
        if (lane < 32) {                                           // one pixel per lane: the norm's fma chain in channel order
            double ssq = 0.0;
#pragma unroll 8
            for (int c = 0; c < HT_C; ++c) { const double v = (double)tile[c * HT_TS + lane]; ssq = __builtin_fma(v, v, ssq); }
            double n = __builtin_sqrt(ssq);
            n = n < 1e-15 ? 1e-15 : n;
            double a = n * ks;
            a = a > 15.0 ? 15.0 : (a < -15.0 ? -15.0 : a);
            const double g = rks * tanh(a);
            double pr = 0.0;
            if (g >= maxnorm_e * (1.0 - 1e-9)) {                   // rare: only here can project() act
                double s2 = 0.0;
#pragma unroll 1
                for (int c = 0; c < HT_C; ++c) { const double w = g * ((double)tile[c * HT_TS + lane] / n); s2 = __builtin_fma(w, w, s2); }
                double ny = __builtin_sqrt(s2);
                ny = ny < 1e-15 ? 1e-15 : ny;
                pr = ny > maxnorm_e ? ny : 0.0;
            }
            sn[lane] = n; sg[lane] = g; spr[lane] = pr;
        }
        __builtin_amdgcn_s_waitcnt(0xc07f);
        __builtin_amdgcn_wave_barrier();
        const double n0 = sn[2 * lc], n1 = sn[2 * lc + 1], g0 = sg[2 * lc], g1 = sg[2 * lc + 1], p0 = spr[2 * lc], p1 = spr[2 * lc + 1];
        const double r0 = exact_rcp(n0), r1 = exact_rcp(n1);
        double y[16][2];
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) { y[kk][0] = g0 * div_by(zr[kk].x, n0, r0); y[kk][1] = g1 * div_by(zr[kk].y, n1, r1); }
        if (__any(p0 != 0.0 || p1 != 0.0)) {                       // (wave-uniform) a projected pixel in the tile
#pragma unroll
            for (int kk = 0; kk < 16; ++kk) {
                if (p0 != 0.0) y[kk][0] = y[kk][0] / p0 * maxnorm_e;
                if (p1 != 0.0) y[kk][1] = y[kk][1] / p1 * maxnorm_e;
            }
        }
        if (pair_ok) {
            double *eq = embed + (size_t)b * HT_C * hw + pix0;
#pragma unroll
            for (int kk = 0; kk < 16; ++kk)
                __builtin_nontemporal_store((d2_h){y[kk][0], y[kk][1]}, reinterpret_cast<d2_h *>(eq + (size_t)(kk * 4 + lk) * hw));
        }
        __builtin_amdgcn_wave_barrier();                           // every lane has read n / g / pr: the rows may become px | xa
        v4d_t acc[2][NT];
        double ss[2] = {0.0, 0.0};
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int n = 0; n < NT; ++n) acc[m][n] = (v4d_t){0, 0, 0, 0};
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) {
            const int k = kk * 4 + lk;
#pragma unroll
            for (int n = 0; n < NT; ++n) {
                const double bfv = wts[wrow[n] + k];
                const double bf = wok[n] ? bfv : 0.0;
#pragma unroll
                for (int m = 0; m < 2; ++m) acc[m][n] = __builtin_amdgcn_mfma_f64_16x16x4f64(y[kk][m], bf, acc[m][n], 0, 0, 0);
            }
#pragma unroll
            for (int m = 0; m < 2; ++m) ss[m] = __builtin_fma(y[kk][m], y[kk][m], ss[m]);
        }
        mlr_tile_epilogue<TOUT, NT>(acc, ss, pxs, xas, xs, lane, lc, lk, O, pp, anorm, pa, K, K2, sqK, maxnorm, maxn2, c_in, c_out, oscale, b, p_base,
                                    hw, out, force_ref);
        __builtin_amdgcn_wave_barrier();                           // the next tile's features reuse the staging rows
    }
}

// ---------------------------------------------------------------- bilinear, align_corners=True
// out = bilerp (halo_devmath.hpp): columns first, rows second, fma(l0, a, l1*b) -- ATen's order; weights in the tensor's dtype
template <typename T>
__global__ void __launch_bounds__(HTPB) k_bilinear(const T *__restrict__ src, T *__restrict__ dst, long long planes, int h, int w,
                                                   int H, int W, T sh, T sw)
{
    const long long idx = (long long)blockIdx.x * HTPB + threadIdx.x;
    const long long per = (long long)H * W;
    if (idx >= planes * per) return;
    const long long p = idx / per;
    const int y = (int)((idx % per) / W), x = (int)(idx % W);
    const T fy = sh * (T)y, fx = sw * (T)x;
    int y0 = (int)fy, x0 = (int)fx;
    y0 = y0 > h - 1 ? h - 1 : y0;
    x0 = x0 > w - 1 ? w - 1 : x0;
    const int y1 = y0 + (y0 < h - 1 ? 1 : 0), x1 = x0 + (x0 < w - 1 ? 1 : 0);
    const T ly1 = fy - (T)y0, ly0 = (T)1 - ly1, lx1 = fx - (T)x0, lx0 = (T)1 - lx1;
    const T *r0 = src + ((size_t)p * h + y0) * w, *r1 = src + ((size_t)p * h + y1) * w;
    dst[idx] = bilerp<T>(r0[x0], r0[x1], r1[x0], r1[x1], lx0, lx1, ly0, ly1);
}


// The same resize with VEC consecutive outputs per lane (16-byte non-temporal stores: the output is written once
// and is 16-40x the input), one output row per blockIdx.y, and the row / column weights computed once per thread and
// reused over the planes it walks (no 64-bit divisions per element).  Same arithmetic, bit-identical results.
template <typename T, int VEC>
__global__ void __launch_bounds__(HTPB) k_bilinear_rows(const T *__restrict__ src, T *__restrict__ dst, int planes, int h, int w,
                                                        int H, int W, T sh, T sw)
{
    const int y = blockIdx.y, xb = (blockIdx.x * HTPB + threadIdx.x) * VEC;
    if (xb >= W) return;
    const T fy = sh * (T)y;
    int y0 = (int)fy;
    y0 = y0 > h - 1 ? h - 1 : y0;
    const int y1 = y0 + (y0 < h - 1 ? 1 : 0);
    const T ly1 = fy - (T)y0, ly0 = (T)1 - ly1;
    int x0[VEC], x1[VEC];
    T lx0[VEC], lx1[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
        const T fx = sw * (T)(xb + j);
        int a = (int)fx;
        a = a > w - 1 ? w - 1 : a;
        x0[j] = a;
        x1[j] = a + (a < w - 1 ? 1 : 0);
        lx1[j] = fx - (T)a;
        lx0[j] = (T)1 - lx1[j];
    }
    for (int p = blockIdx.z; p < planes; p += gridDim.z) {
        const T *r0 = src + ((size_t)p * h + y0) * w, *r1 = src + ((size_t)p * h + y1) * w;
        T o[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            o[j] = bilerp<T>(r0[x0[j]], r0[x1[j]], r1[x0[j]], r1[x1[j]], lx0[j], lx1[j], ly0, ly1);
        }
        T *q = dst + ((size_t)p * H + y) * W + xb;
        if constexpr (sizeof(T) == 8 && VEC == 2) __builtin_nontemporal_store((d2_h){o[0], o[1]}, reinterpret_cast<d2_h *>(q));
        else if constexpr (sizeof(T) == 4 && VEC == 4) __builtin_nontemporal_store((f4_t){o[0], o[1], o[2], o[3]}, reinterpret_cast<f4_t *>(q));
        else {
#pragma unroll
            for (int j = 0; j < VEC; ++j) q[j] = o[j];
        }
    }
}

// ================================================================ backward
// Gradients of the head tail for training (core/models/classifier.py:553-554 under autograd).  Only the
// parts that are not plain GEMMs are kernels here: the Jacobian-transpose product of expmap0+project,
// and the per-(pixel, class) reverse sweep through HyperMLR's scalar algebra.  The two remaining
// contractions of the HyperMLR backward (d x = W^T D, d W = D x^T) are plain dense GEMMs and go to the
// BLAS library through torch (halo_amd/core/utils/hyperbolic.py).

// y = project(expmap0(x.double()))  ->  gx = J^T gy,  gx in x's dtype.  Per pixel: gx = alpha*gy + beta*u.
template <typename TIN>
__global__ void __launch_bounds__(HTPB) k_expmap0_project_bwd(const TIN *__restrict__ x, const double *__restrict__ gy,
                                                              TIN *__restrict__ gx, long long outer, int C, long long inner,
                                                              double ks, double rks, double maxnorm)
{
    const long long idx = (long long)blockIdx.x * HTPB + threadIdx.x;
    if (idx >= outer * inner) return;
    const long long o = idx / inner, i = idx % inner;
    const size_t base = (size_t)o * C * inner + i;
    // (round 5: eight channels' loads in flight per trip -- the kernel was one dependent load pair per trip, 77 us for 105 MB at
    //  the training shape --, and the forward's own rule for the second norm: project() can only act when g is within 1e-9 of
    //  maxnorm, k_expmap0_project_tile, so the pass over x that recomputes ||y0|| runs for such pixels only)
    double ssq = 0.0, d = 0.0;
#pragma unroll 8
    for (int ch = 0; ch < C; ++ch) {
        const double u = ld_as_f64(x + base + (size_t)ch * inner);
        ssq = __builtin_fma(u, u, ssq);
        d = __builtin_fma(u, gy[base + (size_t)ch * inner], d);
    }
    const double n_raw = __builtin_sqrt(ssq);
    const bool clamped = n_raw < 1e-15;                       // norm.clamp_min(1e-15): no gradient through the norm
    const double n = clamped ? 1e-15 : n_raw;
    const double a_raw = n * ks;
    const double th = tanh(a_raw > 15.0 ? 15.0 : a_raw);
    const double g = rks * th, phi = g / n;
    const double gprime = a_raw < 15.0 ? (1.0 - th * th) : 0.0;   // d tan_k / d n (0 beyond the tanh clamp)
    // forward's own projection decision: ||y0|| from the same element-wise values
    double ny = 0.0;
    if (g >= maxnorm * (1.0 - 1e-9)) {
        double s2 = 0.0;
#pragma unroll 8
        for (int ch = 0; ch < C; ++ch) { const double v = g * (ld_as_f64(x + base + (size_t)ch * inner) / n); s2 = __builtin_fma(v, v, s2); }
        ny = __builtin_sqrt(s2);
        ny = ny < 1e-15 ? 1e-15 : ny;
    }
    const double radial = clamped ? 0.0 : (gprime - phi) / (n * n);
    double alpha, beta;
    if (ny > maxnorm) {
        const double sc = maxnorm / ny;
        const double k0 = sc * phi * phi * d / (ny * ny);     // gy0 = sc*gy - k0*u
        const double d0 = sc * d - k0 * ssq;                  // u . gy0
        alpha = phi * sc;
        beta = -phi * k0 + radial * d0;
    } else {
        alpha = phi;
        beta = radial * d;
    }
#pragma unroll 8
    for (int ch = 0; ch < C; ++ch) {
        const size_t a = base + (size_t)ch * inner;
        gx[a] = (TIN)(alpha * gy[a] + beta * ld_as_f64(x + a));
    }
}

// One (pixel, class) of the reverse sweep through _hyper_logits' scalar algebra (hyperbolic.py:146-183): the forward values are
// recomputed from px = <x,-P>, xa = <x,A^>, xx = ||x||^2 and the class constants, then differentiated statement by statement
// (clamps and the projection's where() pass no gradient on their inactive side, as autograd has it).
struct MlrGrad { double d_px, d_xa, d_pp, d_pa, d_an, d_xx; };
// IEEE division / sqrt / asinh throughout, every clamp and both sides of the projection's where(): the term-map kernel's statement and
// the fused backward's rare arm.
__device__ __forceinline__ MlrGrad mlr_reverse(double px, double xa, double gF, double ppo, double pao, double ano, double xx, double K,
                                               double sqK, double maxnorm)
{
    // ---- forward
    const double t = 1.0 + (2.0 * K) * px;
    const double Aa = t + K * xx, Bb = 1.0 - K * ppo;
    const double D0 = t + ((K * xx) * K) * ppo;
    const bool Dlive = D0 >= 1e-12;
    const double D = Dlive ? D0 : 1e-12;
    const double al = Aa / D, be = Bb / D;
    const double mob = ((al * al) * ppo + (be * be) * xx) + ((2.0 * al) * be) * px;
    const double sq = __builtin_sqrt(mob);
    const bool over = sq > maxnorm, under = sq < maxnorm;
    const double pn = over ? maxnorm / (sq < 1e-12 ? 1e-12 : sq) : 1.0;
    const double mp = under ? mob : maxnorm * maxnorm;
    const double inner = be * xa + al * pao;
    const double md = inner * pn;
    const double den = 1.0 - K * mp;
    const bool denlive = den >= 1e-12;
    const double denc = denlive ? den : 1e-12;
    const double lam = 2.0 / denc;
    const double s = (sqK * md) * lam;
    // ---- reverse
    const double two_sqK = 2.0 / sqK;
    const double d_an = gF * two_sqK * asinh(s);
    const double d_s = gF * two_sqK * ano / __builtin_sqrt(1.0 + s * s);
    const double d_md = d_s * sqK * lam;
    const double d_lam = d_s * sqK * md;
    const double d_den = denlive ? -d_lam * 2.0 / (denc * denc) : 0.0;
    double d_mob = under ? -K * d_den : 0.0;
    const double d_inner = d_md * pn, d_pn = d_md * inner;
    double d_be = d_inner * xa, d_al = d_inner * pao;
    const double d_xa = d_inner * be, d_pa = d_inner * al;
    const double d_sq = over ? -d_pn * maxnorm / (sq * sq) : 0.0;
    if (sq > 0.0) d_mob += d_sq / (2.0 * sq);
    d_al += d_mob * (2.0 * al * ppo + 2.0 * be * px);
    d_be += d_mob * (2.0 * be * xx + 2.0 * al * px);
    double d_pp = d_mob * al * al, d_xx = d_mob * be * be, d_px = d_mob * 2.0 * al * be;
    const double d_Aa = d_al / D, d_Bb = d_be / D;
    const double d_D0 = Dlive ? -(d_al * Aa + d_be * Bb) / (D * D) : 0.0;
    double d_t = d_D0;
    d_xx += d_D0 * K * K * ppo;
    d_pp += d_D0 * K * K * xx;
    d_pp += -K * d_Bb;
    d_t += d_Aa;
    d_xx += K * d_Aa;
    d_px += 2.0 * K * d_t;
    return MlrGrad{d_px, d_xa, d_pp, d_pa, d_an, d_xx};
}
// The same sweep for a pixel INSIDE the ball with no clamp active -- D >= 1e-12, 0 < ||mobadd|| < maxnorm (hence 1 - K mob > 2e-3),
// |sineterm| < 1e150: every trained head, every pixel -- as ONE straight line: two corrected reciprocals (1/D, 1/(1 - K mob)) and one
// reciprocal root (1/sqrt(1 + s^2)) through rcp_q / rsqrt_q (<= 1 ulp), every other quotient a product with them, asinh as
// log(|s| + sqrt(1 + s^2)).  `ok` says whether the conditions held (NaN operands fail them); the caller recomputes the others with
// mlr_reverse.  No branch inside: two classes' chains written back to back interleave in one basic block.
struct MlrFast { MlrGrad g; bool ok; };
__device__ __forceinline__ MlrFast mlr_reverse_inside(double px, double xa, double gF, double ppo, double pao, double ano, double xx, double K,
                                                      double sqK, double maxnorm)
{
    const double t = __builtin_fma(2.0 * K, px, 1.0);
    const double Kxx = K * xx;
    const double Aa = t + Kxx, Bb = __builtin_fma(-K, ppo, 1.0);
    const double D = __builtin_fma(Kxx * K, ppo, t);
    bool ok = D >= 1e-12;
    const double rD = rcp_q(D);
    const double al = Aa * rD, be = Bb * rD;
    const double mob = __builtin_fma(al * al, ppo, __builtin_fma(be * be, xx, ((2.0 * al) * be) * px));
    ok = ok && mob > 1e-300 && mob < 1e300;
    ok = ok && sqrt_q(mob) < maxnorm;
    const double inner = __builtin_fma(be, xa, al * pao);
    const double rden = rcp_q(__builtin_fma(-K, mob, 1.0));
    const double lam = 2.0 * rden;
    const double s = (sqK * inner) * lam;
    const double a_ = __builtin_fabs(s);
    ok = ok && a_ < 1e150;
    const double u = __builtin_fma(a_, a_, 1.0), rsq1 = rsqrt_q(u);
    const double asinh_s = __builtin_copysign(log_ge1_q(__builtin_fma(u, rsq1, a_)), s);
    // ---- reverse
    const double gs = gF * (2.0 / sqK);
    const double d_an = gs * asinh_s;
    const double d_s = (gs * ano) * rsq1;
    const double d_md = (d_s * sqK) * lam;                               // pn = 1: d inner = d md, no gradient through pn
    const double d_lam = (d_s * sqK) * inner;
    const double d_mob = (K * 2.0) * (d_lam * (rden * rden));            // -K * d_den, d_den = -d_lam 2 / den^2
    const double d_xa = d_md * be, d_pa = d_md * al;
    const double d_al = __builtin_fma(d_mob, 2.0 * __builtin_fma(al, ppo, be * px), d_md * pao);
    const double d_be = __builtin_fma(d_mob, 2.0 * __builtin_fma(be, xx, al * px), d_md * xa);
    const double d_Aa = d_al * rD, d_Bb = d_be * rD;
    const double d_D0 = -__builtin_fma(d_al, Aa, d_be * Bb) * (rD * rD);
    const double KK = K * K;
    const double d_xx = __builtin_fma(K, d_Aa, __builtin_fma(d_D0 * KK, ppo, (d_mob * be) * be));
    const double d_pp = __builtin_fma(-K, d_Bb, __builtin_fma(d_D0 * KK, xx, (d_mob * al) * al));
    const double d_px = __builtin_fma(2.0 * K, d_D0 + d_Aa, ((d_mob * 2.0) * al) * be);
    return MlrFast{MlrGrad{d_px, d_xa, d_pp, d_pa, d_an, d_xx}, ok};
}

// Reverse sweep through _hyper_logits' scalar algebra (hyperbolic.py:146-183) for every (pixel, class):
// given gout = dL/dlogit it writes dL/dpx, dL/dxa and the per-element contributions to dL/dpp, dL/dpa,
// dL/d||A|| (B,O,hw each; the caller sums the last three over pixels) and dL/dxx summed over classes (B,hw).
template <int OB>
__global__ void __launch_bounds__(HTPB) k_hypermlr_bwd_terms(const double *__restrict__ x, const double *__restrict__ consts,
                                                             const double *__restrict__ gout, int O, int C, long long hw,
                                                             double K, double *__restrict__ dpx, double *__restrict__ dxa,
                                                             double *__restrict__ dxx, double *__restrict__ dpp,
                                                             double *__restrict__ dpa, double *__restrict__ dan)
{
    const int b = blockIdx.y;
    const long long i = (long long)blockIdx.x * HTPB + threadIdx.x;
    if (i >= hw) return;
    const double *xb = x + (size_t)b * C * hw + i;
    const double *pp = consts, *anorm = consts + O, *pa = consts + 2 * O, *An = consts + 3 * O, *nP = consts + 3 * O + (size_t)O * C;
    double ssq = 0.0;
    for (int j = 0; j < C; ++j) { const double v = xb[(size_t)j * hw]; ssq = __builtin_fma(v, v, ssq); }
    const double nx = __builtin_sqrt(ssq), xx = nx * nx;
    const double sqK = __builtin_sqrt(K), maxnorm = (1.0 - 1e-3) / sqK;
    double dxx_acc = 0.0;
    for (int o0 = 0; o0 < O; o0 += OB) {
        double px[OB], xa[OB];
#pragma unroll
        for (int q = 0; q < OB; ++q) { px[q] = 0.0; xa[q] = 0.0; }
        for (int j = 0; j < C; ++j) {
            const double v = xb[(size_t)j * hw];
#pragma unroll
            for (int q = 0; q < OB; ++q) {
                const int o = o0 + q < O ? o0 + q : O - 1;
                px[q] = __builtin_fma(v, nP[(size_t)o * C + j], px[q]);
                xa[q] = __builtin_fma(v, An[(size_t)o * C + j], xa[q]);
            }
        }
#pragma unroll
        for (int q = 0; q < OB; ++q) {
            const int o = o0 + q;
            if (o < O) {
            const size_t oi = ((size_t)b * O + o) * hw + i;
            const MlrGrad g_ = mlr_reverse(px[q], xa[q], gout[oi], pp[o], pa[o], anorm[o], xx, K, sqK, maxnorm);
            dpx[oi] = g_.d_px; dxa[oi] = g_.d_xa; dpp[oi] = g_.d_pp; dpa[oi] = g_.d_pa; dan[oi] = g_.d_an;
            dxx_acc += g_.d_xx;
            }
        }
    }
    dxx[(size_t)b * hw + i] = dxx_acc;
}


// ---------------------------------------------------------------- HyperMLR backward, fused (round 5)
// Until round 5 the backward was k_hypermlr_bwd_terms (five (B,O,hw) term maps written to HBM) followed by ~45 library launches
// in halo_amd/core/utils/hyperbolic.py: three full-map sums, two einsums with their permuted copies, a padded / permuted batched
// GEMM for d W, and a dozen (O,C)-sized element-wise kernels -- 0.56 ms of the 0.81 ms the head tail's forward + backward took at
// the training shape (2 x 64 x 160 x 320; profiles/r05_head_bwd_kernels.txt), against 0.03 ms for the forward.  Now, behind k_mlr_prep:
//   k_mlr_bwd_pixels   one lane per pixel: ||x||^2 and the two contractions px / xa in ONE walk over the channels (weights broadcast
//                      from an LDS image of [-P | A^] laid out channel-major), the reverse sweep for every class; dpx / dxa (the
//                      matrix D, 2O x pixels) and dxx go to the workspace, the three per-class sums (dpp, dpa, d||A||) leave as one
//                      partial per workgroup (fixed shuffle tree, fixed order afterwards: deterministic);
//   k_mlr_bwd_dxw      gx = W^T D + 2 x dxx  and  d W = D x^T  in ONE pass over D and x on the f64 matrix cores, the tile transposed
//                      through LDS between the two products; one (2O x C) partial of d W per persistent workgroup;
//   k_mlr_bwd_final    sums the partials in a fixed order and applies the (O,C)-sized algebra (||P||^2, <-P,A^>, F.normalize).
// Serves O <= MLRB_OP classes and C a multiple of 64 up to 256 (the heads: 19 classes, 64 channels); anything else keeps the
// term-map path above.
constexpr int MLRB_OP = 20, MLRB_WS = 2 * MLRB_OP, MLRB_TPB = 256, MLRB_NWG = 256;

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m);
    return v;
}

template <bool SCALAR_W, typename TG>      // TG: dtype of gout (float32: the head's .float() under autograd hands a float32 gradient back)
__global__ void __launch_bounds__(MLRB_TPB, SCALAR_W ? 3 : 2) k_mlr_bwd_pixels(const double *__restrict__ x, const double *__restrict__ consts,
                                                             const double *__restrict__ Wg, const TG *__restrict__ gout, int O, int C,
                                                             long long hw, double K, double *__restrict__ Dws,
                                                             double *__restrict__ dxx_out, double *__restrict__ cls_part)
{
    // Wg [C][MLRB_WS]: -P of classes 0..OP-1 | A^ of classes 0..OP-1 (zero beyond O), written by k_mlr_prep.  Every lane of a wave
    // wants the SAME weight at the same time, and there are two ways to hand it over:
    //   SCALAR_W   the addresses are wave-uniform: the 40 doubles of a channel arrive through the scalar cache into SGPRs and feed
    //              v_fma_f64 as scalar operands (s_load_dwordx16 x 5 per channel in the emitted code);
    //   otherwise  broadcast from an LDS copy: 20 ds_read_b128 per channel and wave, 8 cycles each on the CU's ONE LDS pipe against
    //              41 x 4.5 cycles of fma on each of its four SIMDs -- LDS-bound by a factor of 3.5 once the chip is full.
    // Measured (pixels kernel alone): 819 200 pixels (the v2 head) 366 us from LDS, 296 us scalar; 102 400 pixels (the training shape:
    // 1.5 waves per SIMD, nothing to hide an s_load's latency behind) 57 us from LDS, 64 us scalar -- the host picks by pixel count.
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_b[];
    __shared__ double s_red[MLRB_TPB / 64][3 * MLRB_OP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.y;
    const double *pp = consts, *anorm = consts + O, *pa = consts + 2 * O;
    const double *Wt = Wg;
    if constexpr (!SCALAR_W) {
        double *Wl = reinterpret_cast<double *>(smem_b);
        const d2_h *src = reinterpret_cast<const d2_h *>(Wg);
        for (int e = tid; e < C * MLRB_WS / 2; e += MLRB_TPB) reinterpret_cast<d2_h *>(Wl)[e] = src[e];
        __syncthreads();
        Wt = Wl;
    }
    const long long i_raw = (long long)blockIdx.x * MLRB_TPB + tid;
    const bool live = i_raw < hw;
    const long long i = live ? i_raw : hw - 1;                           // idle lanes repeat the last pixel (loads stay valid, nothing stored, zero summed)
    const double *xb = x + (size_t)b * C * hw + i;
    // ONE walk over the pixel's channels: ||x||^2 and all 2 x OP contraction chains together, eight channels per trip, the next
    // trip's eight loads issued before this trip's arithmetic.  (The first version walked x four times -- norm, two class passes
    // with dpx / dxa parked in 80 registers, d x -- at 252 registers and 1.5 waves per SIMD: every trip was an exposed L2 round trip.)
    constexpr int UN = 8;                                                // C % 64 == 0
    auto load8 = [&](double (&d)[UN], int j0) {
#pragma unroll
        for (int u = 0; u < UN; ++u) d[u] = xb[(size_t)(j0 + u) * hw];
    };
    double ssq = 0.0, px[MLRB_OP], xa[MLRB_OP];
#pragma unroll
    for (int q = 0; q < MLRB_OP; ++q) { px[q] = 0.0; xa[q] = 0.0; }
    {
        double cur[UN], nxt[UN];
        load8(cur, 0);
        for (int j0 = 0; j0 < C; j0 += UN) {
            if (j0 + UN < C) load8(nxt, j0 + UN);
#pragma unroll
            for (int u = 0; u < UN; ++u) {
                const double *wr = Wt + (size_t)(j0 + u) * MLRB_WS;            // wave-uniform address
                ssq = __builtin_fma(cur[u], cur[u], ssq);
#pragma unroll
                for (int q = 0; q < MLRB_OP; ++q) {
                    px[q] = __builtin_fma(cur[u], wr[q], px[q]);
                    xa[q] = __builtin_fma(cur[u], wr[MLRB_OP + q], xa[q]);
                }
            }
#pragma unroll
            for (int u = 0; u < UN; ++u) cur[u] = nxt[u];
        }
    }
    const double nx = __builtin_sqrt(ssq), xx = nx * nx;                  // torch.norm(x)**2, hyperbolic.py:136
    const double sqK = __builtin_sqrt(K), maxnorm = (1.0 - 1e-3) / sqK;
    double dxx_acc = 0.0;
    double *d0 = Dws + (size_t)b * 2 * O * hw + i;
    // Two classes per trip, both straight-line sweeps written back to back (one basic block: their dependent chains interleave),
    // then ONE wave-uniform test for the rare arm.  Class O of an odd O is padding (zero weights, constants read in bounds, nothing
    // stored or summed).
    const TG *gb = gout + (size_t)b * O * hw + i;
#pragma unroll
    for (int o = 0; o < MLRB_OP; o += 2) {
        if (o < O) {                                                     // wave-uniform
            const bool has1 = o + 1 < O;                                 // wave-uniform
            const double gF0 = (double)gb[(size_t)o * hw], gF1 = has1 ? (double)gb[(size_t)(o + 1) * hw] : 0.0;
            MlrFast f0 = mlr_reverse_inside(px[o], xa[o], gF0, pp[o], pa[o], anorm[o], xx, K, sqK, maxnorm);
            MlrFast f1 = mlr_reverse_inside(px[o + 1], xa[o + 1], gF1, pp[o + 1], pa[o + 1], anorm[o + 1], xx, K, sqK, maxnorm);
            if (__any(!f0.ok || (has1 && !f1.ok))) {                     // clamped D, on / beyond the ball, NaN / inf: never in a trained head
                if (!f0.ok) f0.g = mlr_reverse(px[o], xa[o], gF0, pp[o], pa[o], anorm[o], xx, K, sqK, maxnorm);
                if (has1 && !f1.ok) f1.g = mlr_reverse(px[o + 1], xa[o + 1], gF1, pp[o + 1], pa[o + 1], anorm[o + 1], xx, K, sqK, maxnorm);
            }
            if (live) { d0[(size_t)o * hw] = f0.g.d_px; d0[(size_t)(O + o) * hw] = f0.g.d_xa; }
            dxx_acc += f0.g.d_xx;
            // the three per-class sums: fixed shuffle trees (their ds_bpermute latency hides behind the other chains and waves)
            const double s0 = wave_sum(live ? f0.g.d_pp : 0.0), s1 = wave_sum(live ? f0.g.d_pa : 0.0), s2 = wave_sum(live ? f0.g.d_an : 0.0);
            if (lane == 0) { s_red[wave][o] = s0; s_red[wave][MLRB_OP + o] = s1; s_red[wave][2 * MLRB_OP + o] = s2; }
            if (has1) {
                if (live) { d0[(size_t)(o + 1) * hw] = f1.g.d_px; d0[(size_t)(O + o + 1) * hw] = f1.g.d_xa; }
                dxx_acc += f1.g.d_xx;
                const double t0 = wave_sum(live ? f1.g.d_pp : 0.0), t1 = wave_sum(live ? f1.g.d_pa : 0.0), t2 = wave_sum(live ? f1.g.d_an : 0.0);
                if (lane == 0) { s_red[wave][o + 1] = t0; s_red[wave][MLRB_OP + o + 1] = t1; s_red[wave][2 * MLRB_OP + o + 1] = t2; }
            }
        }
    }
    if (live) dxx_out[(size_t)b * hw + i] = dxx_acc;
    __syncthreads();
    if (tid < 3 * MLRB_OP) {                                             // the workgroup's partial: waves added in wave order
        const int k = tid / MLRB_OP, o = tid % MLRB_OP;
        if (o < O) {
            double t = 0.0;
#pragma unroll
            for (int w = 0; w < MLRB_TPB / 64; ++w) t += s_red[w][tid];
            cls_part[((size_t)(blockIdx.y * gridDim.x + blockIdx.x) * 3 + k) * O + o] = t;
        }
    }
}

// d x = W^T D + 2 x dxx  AND  d W = D x^T  in one pass over D and x on the f64 matrix cores (as two kernels they read x twice and D
// three times between them, and were HBM-bound at large pixel counts).  d x: out[channel][pixel] = sum_k W^T[channel][k] D[k][pixel],
// k over the 2O rows of D; the A operand (16 channels x 4 rows of D) is the weights, constant over the launch, the B operand (4 rows of
// D x 16 pixels) comes from lane (pixel = lane & 15, k = lane >> 4), which loads D[4 ks + k][pixel] -- 128 contiguous bytes per row --
// and x[16 ct + k + 4 q][pixel]; the result lane holds pixel (lane & 15) of channels (lane >> 4) + 4 q of each 16-channel tile, so x
// is read and d x written in 128-byte row segments as well.  A wave walks 16-pixel tiles; blockIdx.y is the 64-channel block.  After
// the d x MFMAs (weights from an LDS image) the wave parks D and x of the tile in its own LDS slab and reads them back TRANSPOSED for
// the d W MFMAs, whose k slot is the pixel (the k slot of an MFMA is ANY pixel as long as both operands agree on it): lane (row =
// lane & 15, slot = lane >> 4) takes D[16 rt + row][4 e + slot] and x[16 ct + row][4 e + slot].  48 x 64 d W accumulators stay in
// registers over the wave's tiles.
constexpr int MLRX_KS = (2 * MLRB_OP + 3) / 4;                           // k steps covering 2O <= 40 rows
constexpr int MLRZ_RS = 17, MLRZ_WS = 66;                                // row strides (doubles) of the per-wave slabs / of the weight image
__global__ void __launch_bounds__(256, 2) k_mlr_bwd_dxw(const double *__restrict__ x, const double *__restrict__ consts, const double *__restrict__ Dws,
                                                        const double *__restrict__ dxx, int O, int C, long long hw, int Bn, double *__restrict__ gx,
                                                        double *__restrict__ w_part)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_z[];
    double *Wl = reinterpret_cast<double *>(smem_z);                      // [40][MLRZ_WS]: row kk = -P of class kk (< O) | A^ of class kk - O | zero
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 15, k = lane >> 4, cb = blockIdx.y;
    double *Dt = Wl + 4 * MLRX_KS * MLRZ_WS + (size_t)wave * (4 * MLRX_KS + 64) * MLRZ_RS, *Xt = Dt + 4 * MLRX_KS * MLRZ_RS;
    const double *An = consts + 3 * O, *nP = consts + 3 * O + (size_t)O * C;
    for (int e = tid; e < 4 * MLRX_KS * 64; e += 256) {
        const int kk = e >> 6, c = e & 63;
        Wl[kk * MLRZ_WS + c] = kk < O ? nP[(size_t)kk * C + cb * 64 + c] : (kk < 2 * O ? An[(size_t)(kk - O) * C + cb * 64 + c] : 0.0);
    }
    __syncthreads();
    const long long tpi = (hw + 15) / 16, ntiles = tpi * Bn, tstride = (long long)gridDim.x * 4;
    // the D operand of the wave's NEXT tile is requested before this tile's MFMAs (a tile's 40 d x MFMAs last about as long as an HBM
    // round trip under load: unpipelined, two waves per SIMD left the matrix pipe idle half the time)
    auto load_d = [&](long long t_, double (&d)[MLRX_KS]) {
        const long long tl = t_ < ntiles ? t_ : ntiles - 1;
        const int b = (int)(tl / tpi);
        const long long p = (tl % tpi) * 16 + col, pc = p < hw ? p : hw - 1;
#pragma unroll
        for (int ks = 0; ks < MLRX_KS; ++ks) {
            const int kk = 4 * ks + k;
            // unconditional (the two padding rows of the last step read row 0) + select: under a lane condition this load is a
            // branch region whose merge waits for EVERY load in flight -- the prefetch it belongs to included
            const double v = Dws[((size_t)b * 2 * O + (kk < 2 * O ? kk : 0)) * hw + pc];
            d[ks] = kk < 2 * O ? v : 0.0;
        }
    };
    v4d_t accw[3][4];
#pragma unroll
    for (int rt = 0; rt < 3; ++rt)
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) accw[rt][ct] = (v4d_t){0, 0, 0, 0};
    double bd[MLRX_KS], bn[MLRX_KS];
    long long t_ = (long long)blockIdx.x * 4 + wave;
    load_d(t_, bd);
    for (; t_ < ntiles; t_ += tstride) {
        const int b = (int)(t_ / tpi);
        const long long p = (t_ % tpi) * 16 + col;
        const bool in = p < hw;
        const long long pc = in ? p : hw - 1;
        load_d(t_ + tstride, bn);
        const double two_dxx = 2.0 * dxx[(size_t)b * hw + pc];
        double xv[4][4];
#pragma unroll
        for (int ct = 0; ct < 4; ++ct)
#pragma unroll
            for (int q = 0; q < 4; ++q) xv[ct][q] = x[((size_t)b * C + cb * 64 + ct * 16 + k + 4 * q) * hw + pc];
        // ---- d x = W^T D (+ 2 x dxx)
        v4d_t acc[4];
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) acc[ct] = (v4d_t){0, 0, 0, 0};
#pragma unroll
        for (int ks = 0; ks < MLRX_KS; ++ks)
#pragma unroll
            for (int ct = 0; ct < 4; ++ct)
                acc[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(Wl[(4 * ks + k) * MLRZ_WS + ct * 16 + col], bd[ks], acc[ct], 0, 0, 0);
        // ---- the tile's D and x to the slab (pixels beyond the image contribute nothing to d W)
#pragma unroll
        for (int ks = 0; ks < MLRX_KS; ++ks) Dt[(4 * ks + k) * MLRZ_RS + col] = in ? bd[ks] : 0.0;
#pragma unroll
        for (int ct = 0; ct < 4; ++ct)
#pragma unroll
            for (int q = 0; q < 4; ++q) Xt[(ct * 16 + k + 4 * q) * MLRZ_RS + col] = xv[ct][q];
        if (in)
#pragma unroll
            for (int ct = 0; ct < 4; ++ct)
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    gx[((size_t)b * C + cb * 64 + ct * 16 + k + 4 * q) * hw + p] = __builtin_fma(two_dxx, xv[ct][q], acc[ct][q]);
        __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0): this wave's slab writes before its own transposed reads
        __builtin_amdgcn_wave_barrier();
        // ---- d W += D x^T over the tile's 16 pixels: slot = lane >> 4 is pixel 4 e + slot
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            double aw_[3], bw_[4];
#pragma unroll
            for (int rt = 0; rt < 3; ++rt) {
                const int j = rt * 16 + col;                             // row of D (col doubles as the row index here)
                const double v = Dt[(j < 4 * MLRX_KS ? j : 0) * MLRZ_RS + 4 * e + k];
                aw_[rt] = j < 4 * MLRX_KS ? v : 0.0;                     // rows 40..47 do not exist (rows 2O..39 hold zeros)
            }
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) bw_[ct] = Xt[(ct * 16 + col) * MLRZ_RS + 4 * e + k];
#pragma unroll
            for (int rt = 0; rt < 3; ++rt)
#pragma unroll
                for (int ct = 0; ct < 4; ++ct) accw[rt][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(aw_[rt], bw_[ct], accw[rt][ct], 0, 0, 0);
        }
        __builtin_amdgcn_s_waitcnt(0xc07f);   // the transposed reads before the next tile's writes
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int ks = 0; ks < MLRX_KS; ++ks) bd[ks] = bn[ks];
    }
    // ---- the workgroup's partial of d W: waves combined as (0 + 1) + (2 + 3) through the (now free) slabs
    __syncthreads();
    double *s_acc = Wl + 4 * MLRX_KS * MLRZ_WS;                           // two areas of 48 x 64 doubles inside the four slabs' space
    auto publish = [&](double *dst) {
#pragma unroll
        for (int rt = 0; rt < 3; ++rt)
#pragma unroll
            for (int ct = 0; ct < 4; ++ct)
#pragma unroll
                for (int q = 0; q < 4; ++q) dst[(rt * 16 + k + 4 * q) * 64 + ct * 16 + col] = accw[rt][ct][q];
    };
    auto absorb = [&](const double *src) {
#pragma unroll
        for (int rt = 0; rt < 3; ++rt)
#pragma unroll
            for (int ct = 0; ct < 4; ++ct)
#pragma unroll
                for (int q = 0; q < 4; ++q) accw[rt][ct][q] += src[(rt * 16 + k + 4 * q) * 64 + ct * 16 + col];
    };
    if (wave & 1) publish(s_acc + (wave >> 1) * 48 * 64);
    __syncthreads();
    if (!(wave & 1)) absorb(s_acc + (wave >> 1) * 48 * 64);
    __syncthreads();
    if (wave == 2) publish(s_acc);
    __syncthreads();
    if (wave == 0) {
        absorb(s_acc);
#pragma unroll
        for (int rt = 0; rt < 3; ++rt)
#pragma unroll
            for (int ct = 0; ct < 4; ++ct)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int j = rt * 16 + k + 4 * q;
                    if (j < 2 * O) w_part[((size_t)blockIdx.x * 2 * O + j) * C + cb * 64 + ct * 16 + col] = accw[rt][ct][q];
                }
    }
}

// One workgroup per class: the partial sums in a fixed order, then hyperbolic.py's own parameter algebra differentiated --
//   pp = ||P||^2 -> 2 P dpp;  pa = <-P, A^> -> -A^ dpa (to P), -P dpa (to A^);  A^ = A / max(||A||, 1e-12) (F.normalize);  ||A|| -> A / ||A|| dan.
constexpr int MLRF_TPB = 1024, MLRF_NW = MLRF_TPB / 64;
__global__ void __launch_bounds__(MLRF_TPB) k_mlr_bwd_final(const double *__restrict__ A, const double *__restrict__ consts,
                                                            const double *__restrict__ w_part, int n_wpart, const double *__restrict__ cls_part,
                                                            int n_cpart, int O, int C, double *__restrict__ gP, double *__restrict__ gA)
{
    __shared__ double s_red[MLRF_NW][3], s_dot, s_w[MLRF_NW][2][64], s_gan[256];          // C <= 256
    const int o = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double *anorm = consts + O, *An = consts + 3 * O, *nP = consts + 3 * O + (size_t)O * C;
    // the three class sums: thread t adds workgroup partials t, t + 1024, ...; then the fixed shuffle tree and the waves in order
    double c3[3] = {0.0, 0.0, 0.0};
    for (int g = tid; g < n_cpart; g += MLRF_TPB)
#pragma unroll
        for (int k = 0; k < 3; ++k) c3[k] += cls_part[((size_t)g * 3 + k) * O + o];
#pragma unroll
    for (int k = 0; k < 3; ++k) { const double t = wave_sum(c3[k]); if (lane == 0) s_red[wave][k] = t; }
    __syncthreads();
    double dpp = 0.0, dpa = 0.0, dan = 0.0;
#pragma unroll
    for (int w = 0; w < MLRF_NW; ++w) { dpp += s_red[w][0]; dpa += s_red[w][1]; dan += s_red[w][2]; }
    const double an = anorm[o], dn = an < 1e-12 ? 1e-12 : an;
    double dot_acc = 0.0;
    for (int c0 = 0; c0 < C; c0 += 64) {                                  // 64 columns at a time: wave w adds weight partials w, w + 16, ...
        const int c = c0 + lane;
        double gp = 0.0, ga = 0.0;
        if (c < C)
#pragma unroll 16                                                            // 256 partials / 16 waves: every load of the wave in flight at once
            for (int g = wave; g < n_wpart; g += MLRF_NW) {
                gp += w_part[((size_t)g * 2 * O + o) * C + c];
                ga += w_part[((size_t)g * 2 * O + O + o) * C + c];
            }
        s_w[wave][0][lane] = gp; s_w[wave][1][lane] = ga;
        __syncthreads();
        if (wave == 0 && c < C) {
            double g_negP = 0.0, g_xa = 0.0;
#pragma unroll
            for (int w = 0; w < MLRF_NW; ++w) { g_negP += s_w[w][0][lane]; g_xa += s_w[w][1][lane]; }
            const double np_ = nP[(size_t)o * C + c], ah = An[(size_t)o * C + c];
            const double g_An = g_xa + dpa * np_;                        // through xa and pa = <-P, A^>
            gP[(size_t)o * C + c] = (-g_negP + dpp * (2.0 * -np_)) - dpa * ah;
            s_gan[c] = g_An;                                              // finished below, once <g_An, A^> is known
            dot_acc = __builtin_fma(g_An, ah, dot_acc);
        }
        __syncthreads();
    }
    if (wave == 0) { const double t = wave_sum(dot_acc); if (lane == 0) s_dot = t; }
    __syncthreads();
    const double dot = s_dot;
    for (int c = tid; c < C; c += MLRF_TPB) {
        const double ah = An[(size_t)o * C + c];
        gA[(size_t)o * C + c] = (s_gan[c] - dot * ah) / dn + dan * A[(size_t)o * C + c] / an;
    }
}

}  // namespace halo

using namespace halo;

static inline unsigned nblocks(long long n) { return (unsigned)cdiv(n, HTPB); }

// Test hook, read at every launch of the one-quotient HyperMLR epilogue (halo_hypermlr_logits' resident kernel, halo_head_tail):
// HALO_MLR_EPI_REF set = the reference-order epilogue for every logit, the independent reference that tests/test_gpu_parity.py,
// tests/fuzz_head.py and tools/ab_mlr_epilogue.py compare the default against.  Not a user option.
static inline int mlr_epi_ref() { return getenv("HALO_MLR_EPI_REF") != nullptr; }

extern "C" int halo_expmap0_project(const void *x, int x_dtype, double *y, int64_t outer, int64_t C, int64_t inner, double c,
                                    void *stream)
{
    if (!x || !y || outer <= 0 || C <= 0 || inner <= 0) return fail(HALO_E_ARG, "halo_expmap0_project: null/empty argument");
    if (c <= 0) return fail(HALO_E_UNSUPPORTED, "halo_expmap0_project: curvature must be > 0 (Poincare ball)");
    const double ks = sqrt(fabs(-c) + 1e-15), rks = 1.0 / ks, maxnorm = (1.0 - 1e-5) / sqrt(fabs(-c) + 1e-15);
    hipStream_t st = (hipStream_t)stream;
    // float32 planes (the head's case): LDS-tiled single-read kernel.  P pixels x C channels per workgroup, 32 KiB where
    // that leaves P >= 32 (a full 128-byte line per channel row), up to 96 KiB otherwise
    int pshift = 0;
    size_t lds = 0;
    if (x_dtype == HALO_F32 && inner >= 4 && inner % 4 == 0 && ((uintptr_t)x % 16) == 0 && ((uintptr_t)y % 16) == 0) {
        pshift = 8;                                             // P = 256
        while (pshift > 5 && ((size_t)C << pshift) * 4 > 32 * 1024) --pshift;
        while (pshift > 2 && (1ll << (pshift - 1)) >= inner) --pshift;      // tiny planes: no wider than needed
        lds = ((size_t)C << pshift) * 4 + 3 * ((size_t)8 << pshift);
        if (lds > 96 * 1024) pshift = 0;
    }
    // the head's channel counts (<= 64): every channel of a lane's pixel pair lives in registers -- no tile
    if (x_dtype == HALO_F32 && C <= 64 && inner % 2 == 0 && inner < (1ll << 31) && outer <= 65535 && ((uintptr_t)x % 8) == 0 &&
        ((uintptr_t)y % 16) == 0) {
        const dim3 gr((unsigned)cdiv(inner / 2, 64), (unsigned)outer);
#define HALO_EXPR(CC_, EX_) hipLaunchKernelGGL((k_expmap0_project_regs<CC_, EX_>), gr, dim3(64), 0, st, (const float *)x, y, (long long)outer, (int)C, (long long)inner, ks, rks, maxnorm)
        if (C <= 16) HALO_EXPR(16, false);
        else if (C <= 32) HALO_EXPR(32, false);
        else HALO_EXPR(64, false);
#undef HALO_EXPR
    }
    else if (pshift) {
        static LdsLimitSeen seen;
        if (lds > 64 * 1024 && !raise_lds_limit(seen, (const void *)k_expmap0_project_tile, 96 * 1024))
            return fail(HALO_E_LAUNCH, "halo_expmap0_project: cannot raise the dynamic LDS limit");
        const long long tiles = (inner + (1ll << pshift) - 1) >> pshift, ntiles = outer * tiles;
        // One block per tile (round 3: a persistent launch, as many blocks as the CUs hold, each walking its tiles with the next
        // tile's loads in flight, gained nothing at these sizes -- 0.096 vs 0.098 ms at C=256 256x512, 0.136 vs 0.122 ms at C=64
        // 640x1280: the whole kernel is ~100 us, a block sees only 4 tiles)
        hipLaunchKernelGGL(k_expmap0_project_tile, dim3((unsigned)ntiles), dim3(HTPB), lds, st, (const float *)x, y,
                           (long long)outer, (int)C, (long long)inner, pshift, ks, rks, maxnorm);
    }
    else if (x_dtype == HALO_F32)
        hipLaunchKernelGGL((k_expmap0_project<float>), dim3(nblocks(outer * inner)), dim3(HTPB), 0, st, (const float *)x, y, (long long)outer, (int)C, (long long)inner, ks, rks, maxnorm);
    else if (x_dtype == HALO_F64)
        hipLaunchKernelGGL((k_expmap0_project<double>), dim3(nblocks(outer * inner)), dim3(HTPB), 0, st, (const double *)x, y, (long long)outer, (int)C, (long long)inner, ks, rks, maxnorm);
    else return fail(HALO_E_ARG, "halo_expmap0_project: bad dtype");
    return check_launch("halo_expmap0_project");
}

extern "C" int halo_logmap0_project(const double *x, double *y, int64_t outer, int64_t C, int64_t inner, double c, void *stream)
{
    if (!x || !y || outer <= 0 || C <= 0 || inner <= 0) return fail(HALO_E_ARG, "halo_logmap0_project: null/empty argument");
    if (c <= 0) return fail(HALO_E_UNSUPPORTED, "halo_logmap0_project: curvature must be > 0");
    const double ks = sqrt(fabs(-c) + 1e-15), rks = 1.0 / ks, maxnorm = (1.0 - 1e-5) / sqrt(fabs(-c) + 1e-15);
    hipLaunchKernelGGL(k_logmap0_project, dim3(nblocks(outer * inner)), dim3(HTPB), 0, (hipStream_t)stream, x, y, (long long)outer, (int)C, (long long)inner, ks, rks, maxnorm);
    return check_launch("halo_logmap0_project");
}

extern "C" int halo_dist0(const void *x, int dtype, void *out, int64_t outer, int64_t C, int64_t inner, double c, void *stream)
{
    if (!x || !out || outer <= 0 || C <= 0 || inner <= 0) return fail(HALO_E_ARG, "halo_dist0: null/empty argument");
    if (c <= 0) return fail(HALO_E_UNSUPPORTED, "halo_dist0: curvature must be > 0");
    const double ks = sqrt(fabs(-c) + 1e-15), rks = 1.0 / ks;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == HALO_F64)
        hipLaunchKernelGGL((k_dist0<double>), dim3(nblocks(outer * inner)), dim3(HTPB), 0, st, (const double *)x, (double *)out, (long long)outer, (int)C, (long long)inner, ks, rks);
    else if (dtype == HALO_F32)
        hipLaunchKernelGGL((k_dist0<float>), dim3(nblocks(outer * inner)), dim3(HTPB), 0, st, (const float *)x, (float *)out, (long long)outer, (int)C, (long long)inner, ks, rks);
    else return fail(HALO_E_ARG, "halo_dist0: bad dtype");
    return check_launch("halo_dist0");
}

extern "C" int halo_pdist(const double *x, const double *y, double *out, int64_t n, int64_t d, double c, void *stream)
{
    if (!x || !y || !out || n <= 0 || d <= 0) return fail(HALO_E_ARG, "halo_pdist: null/empty argument");
    if (c <= 0) return fail(HALO_E_UNSUPPORTED, "halo_pdist: curvature must be > 0");
    const double ks = sqrt(fabs(-c) + 1e-15), rks = 1.0 / ks;
    hipLaunchKernelGGL(k_pdist, dim3(nblocks(n)), dim3(HTPB), 0, (hipStream_t)stream, x, y, out, (long long)n, (int)d, -c, ks, rks);
    return check_launch("halo_pdist");
}

extern "C" size_t halo_hypermlr_workspace_bytes(int64_t O, int64_t C)
{
    if (O <= 0 || C <= 0) return 0;
    return (size_t)(3 * O + 2 * O * C) * sizeof(double) + 256;
}

extern "C" int halo_hypermlr_logits(const double *x, const double *P, const double *A, void *out, int out_dtype, int64_t B,
                                    int64_t C, int64_t O, int64_t hw, double c, void *workspace, size_t workspace_bytes,
                                    void *stream)
{
    if (!x || !P || !A || !out || B <= 0 || C <= 0 || O <= 0 || hw <= 0) return fail(HALO_E_ARG, "halo_hypermlr_logits: null/empty argument");
    if (c <= 0) return fail(HALO_E_UNSUPPORTED, "halo_hypermlr_logits: curvature must be > 0");
    if (!workspace || workspace_bytes < halo_hypermlr_workspace_bytes(O, C)) return fail(HALO_E_WORKSPACE, "halo_hypermlr_logits: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    double *consts = (double *)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
    if (C > 3968) return fail(HALO_E_UNSUPPORTED, "HyperMLR: more than 3968 channels (the class rows are staged in 64 KiB of LDS)");
    hipLaunchKernelGGL(k_mlr_prep, dim3((unsigned)O), dim3(64), (size_t)2 * C * sizeof(double), st, P, A, (int)O, (int)C, consts);
    // matrix-core path: up to 32 classes (two 16-column tiles per operand); anything else takes the VALU kernel
    if (out_dtype != HALO_F32 && out_dtype != HALO_F64) return fail(HALO_E_ARG, "halo_hypermlr_logits: bad out dtype");
    // weights-resident matrix-core kernel when the [-P | A^] image plus the per-wave staging fits LDS
    if (O <= 32) {
        const int NT = O <= 16 ? 2 : (O <= 24 ? 3 : 4);
        const int wstride = (int)C + (int)(((2 - C) % 32 + 32) % 32);            // (C + pad) mod 32 == 2
        const size_t lds = ((size_t)2 * O * wstride + (size_t)(MLRP_TPB / 64) * (2 * O * 32 + 32)) * 8;
        if (lds <= 160 * 1024 && C % (4 * MLRP_SK * MLRP_RING) == 0 && hw % 2 == 0 && hw >= 2 &&      // the stage ring must line up across tiles
            ((uintptr_t)x % 16) == 0) {
            const long long tiles_per_img = cdiv(hw, 32), ntiles = tiles_per_img * B;
            long long gx = cdiv(ntiles, MLRP_TPB / 64);
            gx = gx > 256 ? 256 : gx;                                              // one resident workgroup per CU, persistent over tiles
            const int force_ref = mlr_epi_ref();
#define HALO_MLRP(T, NT_)                                                                                                          \
    {                                                                                                                             \
        static LdsLimitSeen seen;                                                                                                 \
        if (!raise_lds_limit(seen, (const void *)k_hypermlr_mfma_res<T, NT_>, 160 * 1024))                                        \
            return fail(HALO_E_LAUNCH, "halo_hypermlr_logits: cannot raise the dynamic LDS limit");                               \
        hipLaunchKernelGGL((k_hypermlr_mfma_res<T, NT_>), dim3((unsigned)gx), dim3(MLRP_TPB), lds, st, x, (const double *)consts, (int)O, \
                           (int)C, wstride, (long long)hw, tiles_per_img, ntiles, c, (T *)out, force_ref);                        \
    }
            if (out_dtype == HALO_F32) { if (NT == 2) HALO_MLRP(float, 2) else if (NT == 3) HALO_MLRP(float, 3) else HALO_MLRP(float, 4) }
            else { if (NT == 2) HALO_MLRP(double, 2) else if (NT == 3) HALO_MLRP(double, 3) else HALO_MLRP(double, 4) }
#undef HALO_MLRP
            return check_launch("halo_hypermlr_logits");
        }
    }
    // the chunked matrix-core kernel: a C the resident kernel's stage ring does not divide, an odd pixel count, unaligned x
    if (O <= 32) {
        dim3 gridm((unsigned)cdiv(hw, (HTPB / 64) * MLR_MT * 16), (unsigned)B);
#define HALO_MLR(T, NT_) hipLaunchKernelGGL((k_hypermlr_mfma<T, NT_>), gridm, dim3(HTPB), 0, st, x, (const double *)consts, (int)O, (int)C, (long long)hw, c, (T *)out)
        if (out_dtype == HALO_F32) { if (O <= 16) HALO_MLR(float, 2); else if (O <= 24) HALO_MLR(float, 3); else HALO_MLR(float, 4); }
        else { if (O <= 16) HALO_MLR(double, 2); else if (O <= 24) HALO_MLR(double, 3); else HALO_MLR(double, 4); }
#undef HALO_MLR
        return check_launch("halo_hypermlr_logits");
    }
    dim3 grid(nblocks(hw), (unsigned)B);
    constexpr int OB = 10;
    if (out_dtype == HALO_F32)
        hipLaunchKernelGGL((k_hypermlr<OB, float>), grid, dim3(HTPB), 0, st, x, (const double *)consts, (int)O, (int)C, (long long)hw, c, (float *)out);
    else if (out_dtype == HALO_F64)
        hipLaunchKernelGGL((k_hypermlr<OB, double>), grid, dim3(HTPB), 0, st, x, (const double *)consts, (int)O, (int)C, (long long)hw, c, (double *)out);
    else return fail(HALO_E_ARG, "halo_hypermlr_logits: bad out dtype");
    return check_launch("halo_hypermlr_logits");
}

// The head tail of classifier.py:364-379 / 552-558 in ONE launch behind the per-class constants: embed = project(expmap0(feat)),
// out = HyperMLR(embed) [.float()].  Returns 1 -- nothing enqueued -- when the shape is not served (C != 64, more than 32 classes, an odd
// pixel count, unaligned bases: the caller then makes the two calls halo_expmap0_project + halo_hypermlr_logits, whose results this
// call reproduces bit for bit); 0 on success; < 0 on an error.  Workspace: halo_hypermlr_workspace_bytes(O, C).
extern "C" int halo_head_tail(const float *feat, const double *P, const double *A, double *embed, void *out, int out_dtype, int64_t B,
                              int64_t C, int64_t O, int64_t hw, double c, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!feat || !P || !A || !embed || !out || B <= 0 || C <= 0 || O <= 0 || hw <= 0) return fail(HALO_E_ARG, "halo_head_tail: null/empty argument");
    if (c <= 0) return fail(HALO_E_UNSUPPORTED, "halo_head_tail: curvature must be > 0");
    if (out_dtype != HALO_F32 && out_dtype != HALO_F64) return fail(HALO_E_ARG, "halo_head_tail: bad out dtype");
    if (!workspace || workspace_bytes < halo_hypermlr_workspace_bytes(O, C)) return fail(HALO_E_WORKSPACE, "halo_head_tail: workspace too small");
    if (C != HT_C || O > 32 || hw % 2 != 0 || hw < 2 || ((uintptr_t)feat % 8) != 0 || ((uintptr_t)embed % 16) != 0)
        return 1;
    hipStream_t st = (hipStream_t)stream;
    double *consts = (double *)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
    const int NT = O <= 16 ? 2 : (O <= 24 ? 3 : 4);
    const int wstride = (int)C + (int)(((2 - C) % 32 + 32) % 32);                // (C + pad) mod 32 == 2
    const int stage_d = (int)(2 * O * 32 + 32), tile_d = (HT_C * HT_TS) / 2 + 96;
    const int wave_doubles = stage_d > tile_d ? stage_d : tile_d;
    const size_t lds = ((size_t)2 * O * wstride + (size_t)(MLRP_TPB / 64) * wave_doubles) * 8;
    if (lds > 160 * 1024) return 1;
    hipLaunchKernelGGL(k_mlr_prep, dim3((unsigned)O), dim3(64), (size_t)2 * C * sizeof(double), st, P, A, (int)O, (int)C, consts);
    const double ks = sqrt(fabs(-c) + 1e-15), rks = 1.0 / ks, maxnorm_e = (1.0 - 1e-5) / sqrt(fabs(-c) + 1e-15);
    const long long tiles_per_img = cdiv(hw, 32), ntiles = tiles_per_img * B;
    long long gx = cdiv(ntiles, MLRP_TPB / 64);
    gx = gx > 256 ? 256 : gx;
    const int force_ref = mlr_epi_ref();
#define HALO_HT(T, NT_)                                                                                                            \
    {                                                                                                                             \
        static LdsLimitSeen seen;                                                                                                 \
        if (!raise_lds_limit(seen, (const void *)k_head_tail_c64<T, NT_>, 160 * 1024))                                            \
            return fail(HALO_E_LAUNCH, "halo_head_tail: cannot raise the dynamic LDS limit");                                     \
        hipLaunchKernelGGL((k_head_tail_c64<T, NT_>), dim3((unsigned)gx), dim3(MLRP_TPB), lds, st, feat, (const double *)consts, (int)O, wstride, \
                           wave_doubles, (long long)hw, tiles_per_img, ntiles, c, ks, rks, maxnorm_e, embed, (T *)out, force_ref);   \
    }
    if (out_dtype == HALO_F32) { if (NT == 2) HALO_HT(float, 2) else if (NT == 3) HALO_HT(float, 3) else HALO_HT(float, 4) }
    else { if (NT == 2) HALO_HT(double, 2) else if (NT == 3) HALO_HT(double, 3) else HALO_HT(double, 4) }
#undef HALO_HT
    return check_launch("halo_head_tail");
}

// Upsampling (the head tails' x1.6 ... x6.4): the per-lane source taps of the kernel above are gathers (4 per output),
// and at 16 bytes stored per lane the texture-address path, not HBM, sets its pace.  Here a block first stages the
// two source rows of BL_PC planes, restricted to the columns its 256*VEC outputs touch, in LDS with coalesced
// loads, and the taps become LDS reads.  Same arithmetic, bit-identical results.
constexpr int BL_PC = 4;

template <typename T, int VEC>
__global__ void __launch_bounds__(HTPB) k_bilinear_lds(const T *__restrict__ src, T *__restrict__ dst, int planes, int h, int w,
                                                       int H, int W, T sh, T sw, int span)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_b[];
    T *tile = reinterpret_cast<T *>(smem_b);                       // [BL_PC][2][span]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int y = blockIdx.y, xb0 = blockIdx.x * HTPB * VEC, xb = xb0 + tid * VEC;
    const T fy = sh * (T)y;
    int y0 = (int)fy;
    y0 = y0 > h - 1 ? h - 1 : y0;
    const int y1 = y0 + (y0 < h - 1 ? 1 : 0);
    const T ly1 = fy - (T)y0, ly0 = (T)1 - ly1;
    // source columns this block needs
    const int xl = xb0 + HTPB * VEC - 1 < W - 1 ? xb0 + HTPB * VEC - 1 : W - 1;
    int sx0 = (int)(sw * (T)xb0), sx1 = (int)(sw * (T)xl);
    sx0 = sx0 > w - 1 ? w - 1 : sx0;
    sx1 = sx1 > w - 1 ? w - 1 : sx1;
    sx1 += sx1 < w - 1 ? 1 : 0;
    const int ncol = sx1 - sx0 + 1;                                // <= span (host bound)
    int x0[VEC], x1[VEC];
    T lx0[VEC], lx1[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
        const int x = xb + j < W ? xb + j : W - 1;
        const T fx = sw * (T)x;
        int a = (int)fx;
        a = a > w - 1 ? w - 1 : a;
        x0[j] = a - sx0;
        x1[j] = a + (a < w - 1 ? 1 : 0) - sx0;
        lx1[j] = fx - (T)a;
        lx0[j] = (T)1 - lx1[j];
    }
    for (int p0 = blockIdx.z * BL_PC; p0 < planes; p0 += gridDim.z * BL_PC) {
        __syncthreads();                                           // the previous chunk's taps have been read
        // wave wv stages tile rows wv and wv + 4 (row = plane-in-chunk * 2 + {y0, y1})
#pragma unroll
        for (int rr = 0; rr < 2; ++rr) {
            const int row = wave + 4 * rr, pl = row >> 1;
            if (p0 + pl < planes) {
                const T *sp = src + ((size_t)(p0 + pl) * h + ((row & 1) ? y1 : y0)) * w + sx0;
                for (int c0 = lane; c0 < ncol; c0 += 64 * 8) {               // all loads of the segment first (see k_bilinear_lds_rows)
                    T reg[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) { const int col = c0 + 64 * u; reg[u] = sp[col < ncol ? col : ncol - 1]; }
#pragma unroll
                    for (int u = 0; u < 8; ++u) { const int col = c0 + 64 * u; if (col < ncol) tile[row * span + col] = reg[u]; }
                }
            }
        }
        __syncthreads();
        if (xb < W) {
#pragma unroll
            for (int pl = 0; pl < BL_PC; ++pl) {
                if (p0 + pl >= planes) break;
                const T *r0 = tile + (pl * 2) * span, *r1 = r0 + span;
                T o[VEC];
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    o[j] = bilerp<T>(r0[x0[j]], r0[x1[j]], r1[x0[j]], r1[x1[j]], lx0[j], lx1[j], ly0, ly1);
                }
                T *q = dst + ((size_t)(p0 + pl) * H + y) * W + xb;
                if constexpr (sizeof(T) == 8 && VEC == 2) __builtin_nontemporal_store((d2_h){o[0], o[1]}, reinterpret_cast<d2_h *>(q));
                else if constexpr (sizeof(T) == 4 && VEC == 4) __builtin_nontemporal_store((f4_t){o[0], o[1], o[2], o[3]}, reinterpret_cast<f4_t *>(q));
                else if constexpr (sizeof(T) == 4 && VEC == 2) __builtin_nontemporal_store((f2_t){o[0], o[1]}, reinterpret_cast<f2_t *>(q));
                else {
#pragma unroll
                    for (int j = 0; j < VEC; ++j) q[j] = o[j];
                }
            }
        }
    }
}

// Round 3: BL_RO output rows per block.  Up-sampling by f reuses every source row for f output rows, so a block that owns
// one output row (above) stages two source rows and synchronises twice for every 16 bytes it stores per lane and plane; here
// a block owns BL_RO consecutive output rows: the <= BL_SR source rows they touch are staged once per plane chunk, and a
// thread has BL_PC * BL_RO 16-byte stores in flight per pair of barriers instead of BL_PC.  Same arithmetic (bilerp), same bits.
constexpr int BL_RO = 4, BL_SR = 6, BL_PCR = 4;     // output rows per block, source rows staged at most, planes per chunk

// (float32 with 4 pixels per lane: four rows of taps and weights need ~180 registers -- two blocks per CU instead of four; round 4
// kept that case on the one-row kernel, 0.40 of the HBM spec at the v2 head's 640x1280 -> 1024x2048)
template <typename T, int VEC>
__global__ void __launch_bounds__(HTPB, (sizeof(T) == 4 && VEC == 4) ? 2 : 4) k_bilinear_lds_rows(const T *__restrict__ src, T *__restrict__ dst, int planes, int h, int w,
                                                            int H, int W, T sh, T sw, int span, int pcr)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_b[];
    T *tile = reinterpret_cast<T *>(smem_b);                       // [pcr][nsr][span]: pcr <= BL_PCR planes per chunk
    const int tid = threadIdx.x;
    const int yb = blockIdx.y * BL_RO, xb0 = blockIdx.x * HTPB * VEC, xb = xb0 + tid * VEC;
    // source rows of this block's output rows: [sy0, sy0 + nsr)
    const int ylast = yb + BL_RO - 1 < H - 1 ? yb + BL_RO - 1 : H - 1;
    int sy0 = (int)(sh * (T)yb), sy1 = (int)(sh * (T)ylast);
    sy0 = sy0 > h - 1 ? h - 1 : sy0;
    sy1 = sy1 > h - 1 ? h - 1 : sy1;
    sy1 += sy1 < h - 1 ? 1 : 0;
    const int nsr = sy1 - sy0 + 1;                                 // <= BL_SR (host bound)
    int ry0[BL_RO], ry1[BL_RO];
    T ly0[BL_RO], ly1[BL_RO];
#pragma unroll
    for (int r = 0; r < BL_RO; ++r) {
        const int y = yb + r < H ? yb + r : H - 1;
        const T fy = sh * (T)y;
        int a = (int)fy;
        a = a > h - 1 ? h - 1 : a;
        ry0[r] = (a - sy0) * span;
        ry1[r] = (a + (a < h - 1 ? 1 : 0) - sy0) * span;
        ly1[r] = fy - (T)a;
        ly0[r] = (T)1 - ly1[r];
    }
    const int xl = xb0 + HTPB * VEC - 1 < W - 1 ? xb0 + HTPB * VEC - 1 : W - 1;
    int sx0 = (int)(sw * (T)xb0), sx1 = (int)(sw * (T)xl);
    sx0 = sx0 > w - 1 ? w - 1 : sx0;
    sx1 = sx1 > w - 1 ? w - 1 : sx1;
    sx1 += sx1 < w - 1 ? 1 : 0;
    const int ncol = sx1 - sx0 + 1;                                // <= span (host bound)
    int x0[VEC], x1[VEC];
    T lx0[VEC], lx1[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
        const int x = xb + j < W ? xb + j : W - 1;
        const T fx = sw * (T)x;
        int a = (int)fx;
        a = a > w - 1 ? w - 1 : a;
        x0[j] = a - sx0;
        x1[j] = a + (a < w - 1 ? 1 : 0) - sx0;
        lx1[j] = fx - (T)a;
        lx0[j] = (T)1 - lx1[j];
    }
    const int plane_lds = nsr * span;
    for (int p0 = blockIdx.z * pcr; p0 < planes; p0 += gridDim.z * pcr) {
        __syncthreads();                                           // the previous chunk's taps have been read
        // wave wv stages the (plane, source row) pairs wv, wv + 4, ...: one coalesced row segment each.  All loads of a pair are
        // issued before its first LDS store (BL_ST in flight per lane; a segment of up to 64 * BL_ST columns): with one load per trip
        // the staging was a chain of ~20 dependent round trips per chunk at the v2 head's x1.6 geometry (324-column segments, 16
        // pairs), and the kernel ran at 0.43 of the HBM spec where the x4 geometry -- 9 trips -- reached 0.70
        constexpr int BL_ST = 8;
        for (int pr = tid >> 6, pl = 0, rr = tid >> 6; pr < pcr * nsr; pr += HTPB / 64, rr += HTPB / 64) {
            while (rr >= nsr) { rr -= nsr; ++pl; }
            if (p0 + pl < planes) {
                const T *sp = src + ((size_t)(p0 + pl) * h + sy0 + rr) * w + sx0;
                T *tq = tile + pl * plane_lds + rr * span;
                for (int c0 = tid & 63; c0 < ncol; c0 += 64 * BL_ST) {
                    T reg[BL_ST];
#pragma unroll
                    for (int u = 0; u < BL_ST; ++u) { const int col = c0 + 64 * u; reg[u] = sp[col < ncol ? col : ncol - 1]; }
#pragma unroll
                    for (int u = 0; u < BL_ST; ++u) { const int col = c0 + 64 * u; if (col < ncol) tq[col] = reg[u]; }
                }
            }
        }
        __syncthreads();
        if (xb < W) {
#pragma unroll 1
            for (int pl = 0; pl < pcr; ++pl) {                      // one plane's taps and outputs live at a time
                if (p0 + pl >= planes) break;
                const T *tp = tile + pl * plane_lds;
#pragma unroll
                for (int r = 0; r < BL_RO; ++r) {
                    if (yb + r >= H) break;
                    const T *r0 = tp + ry0[r], *r1 = tp + ry1[r];
                    // (the empty asm keeps the row's fractions from being hoisted and duplicated per plane)
                    T l0 = ly0[r], l1 = ly1[r];
                    asm volatile("" : "+v"(l0), "+v"(l1));
                    T o[VEC];
#pragma unroll
                    for (int j = 0; j < VEC; ++j) {
                        o[j] = bilerp<T>(r0[x0[j]], r0[x1[j]], r1[x0[j]], r1[x1[j]], lx0[j], lx1[j], l0, l1);
                    }
                    T *q = dst + ((size_t)(p0 + pl) * H + yb + r) * W + xb;
                    if constexpr (sizeof(T) == 8 && VEC == 2) __builtin_nontemporal_store((d2_h){o[0], o[1]}, reinterpret_cast<d2_h *>(q));
                    else if constexpr (sizeof(T) == 4 && VEC == 4) __builtin_nontemporal_store((f4_t){o[0], o[1], o[2], o[3]}, reinterpret_cast<f4_t *>(q));
                    else if constexpr (sizeof(T) == 4 && VEC == 2) __builtin_nontemporal_store((f2_t){o[0], o[1]}, reinterpret_cast<f2_t *>(q));
                    else {
#pragma unroll
                        for (int j = 0; j < VEC; ++j) q[j] = o[j];
                    }
                    __builtin_amdgcn_sched_barrier(0);             // one output row's taps live at a time (registers)
                }
            }
        }
    }
}

template <typename T, int VEC>
static void launch_bilinear_rows(const void *src, void *dst, int64_t planes, int64_t h, int64_t w, int64_t H, int64_t W, hipStream_t st)
{
    const T sh = H > 1 ? (T)(h - 1) / (T)(H - 1) : (T)0, sw = W > 1 ? (T)(w - 1) / (T)(W - 1) : (T)0;
    const unsigned gx = (unsigned)cdiv(W, (int64_t)HTPB * VEC);
    // enough blocks to fill the chip, each thread re-using its weights over the planes it walks
    int64_t gz = cdiv(8192, (int64_t)gx * H);
    gz = gz < 1 ? 1 : (gz > planes ? planes : gz);
    if (gz > 65535) gz = 65535;
    // source columns one block can touch: its 256*VEC outputs span sw*(256*VEC-1) source units, plus the +1 taps
    const int64_t span = (int64_t)((double)sw * (double)(HTPB * VEC - 1)) + 4;
    // BL_RO output rows per block where they touch at most BL_SR source rows (up-sampling by >= 0.8)
    const int64_t srows = (int64_t)((double)sh * (double)(BL_RO - 1)) + 3;
    // planes per chunk: BL_PCR where their taps fit 24 KiB of LDS (the x4 geometries: 6-7 blocks per CU), fewer for wide source
    // windows (x1.6: 10 KiB per plane -> 2 planes) so that as many blocks stay resident
    int pcr = BL_PCR;
    while (pcr > 1 && (size_t)pcr * srows * span * sizeof(T) > 24 * 1024) pcr >>= 1;
    const size_t lds_r = (size_t)pcr * srows * span * sizeof(T);
    // (float32 with 4 pixels per lane stays on the one-row kernel: on the four-row kernel it needs 178 registers -- two blocks per CU --
    // and measured no faster at the v2 head's 640x1280 -> 1024x2048, 0.066 against 0.069 ms, and slower at x4: 0.044 against 0.039)
    if constexpr (!(sizeof(T) == 4 && VEC == 4)) {
        if (srows <= BL_SR && lds_r <= 48 * 1024 && cdiv(H, BL_RO) <= 65535) {
            const unsigned gyr = (unsigned)cdiv(H, BL_RO);
            int64_t gzl = cdiv(8192, (int64_t)gx * gyr);
            const int64_t chunks = cdiv(planes, pcr);
            gzl = gzl < 1 ? 1 : (gzl > chunks ? chunks : gzl);
            if (gzl > 65535) gzl = 65535;
            hipLaunchKernelGGL((k_bilinear_lds_rows<T, VEC>), dim3(gx, gyr, (unsigned)gzl), dim3(HTPB), lds_r, st, (const T *)src, (T *)dst,
                               (int)planes, (int)h, (int)w, (int)H, (int)W, sh, sw, (int)span, pcr);
            return;
        }
    }
    const size_t lds = (size_t)BL_PC * 2 * span * sizeof(T);
    // float32 planes magnified >= 3x: the taps of a row come from a few hundred bytes that stay in the vector cache -- gathering them
    // from global memory measured FASTER than staging them (19 planes: 256x512 -> 1024x2048 29.9 against 35.2 us, 160x320 -> 640x1280
    // 16.9 against 21.0; at x1.6 the staged kernel wins, 66 against 73)
    const bool gather = sizeof(T) == 4 && (double)sw <= 1.0 / 3.0 && (double)sh <= 1.0 / 3.0;
    if (lds <= 32 * 1024 && !gather) {
        int64_t gzl = cdiv(8192, (int64_t)gx * H);
        const int64_t chunks = cdiv(planes, BL_PC);
        gzl = gzl < 1 ? 1 : (gzl > chunks ? chunks : gzl);
        if (gzl > 65535) gzl = 65535;
        hipLaunchKernelGGL((k_bilinear_lds<T, VEC>), dim3(gx, (unsigned)H, (unsigned)gzl), dim3(HTPB), lds, st, (const T *)src, (T *)dst,
                           (int)planes, (int)h, (int)w, (int)H, (int)W, sh, sw, (int)span);
        return;
    }
    hipLaunchKernelGGL((k_bilinear_rows<T, VEC>), dim3(gx, (unsigned)H, (unsigned)gz), dim3(HTPB), 0, st, (const T *)src, (T *)dst,
                       (int)planes, (int)h, (int)w, (int)H, (int)W, sh, sw);
}

extern "C" int halo_bilinear_upsample(const void *src, void *dst, int dtype, int64_t planes, int64_t h, int64_t w, int64_t H,
                                      int64_t W, void *stream)
{
    if (!src || !dst || planes <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0) return fail(HALO_E_ARG, "halo_bilinear_upsample: null/empty argument");
    if (dtype != HALO_F64 && dtype != HALO_F32) return fail(HALO_E_ARG, "halo_bilinear_upsample: bad dtype");
    hipStream_t st = (hipStream_t)stream;
    const bool rows = H <= 65535 && planes <= 0x7fffffff;     // otherwise one element per thread (k_bilinear)
    const bool a16 = ((uintptr_t)dst % 16) == 0;
    if (rows && dtype == HALO_F64) {
        if (W % 2 == 0 && a16) launch_bilinear_rows<double, 2>(src, dst, planes, h, w, H, W, st);
        else launch_bilinear_rows<double, 1>(src, dst, planes, h, w, H, W, st);
    } else if (rows) {
        // mild magnification (below x3: the v2 head's 640x1280 -> 1024x2048): two pixels per lane on the four-row kernel -- a source row
        // is staged once per four output rows; the one-row kernel that serves float32 x 4 stages two source rows for EVERY output row,
        // 3.2x the input at x1.6
        const bool mild = H > 1 && W > 1 && (double)(h - 1) / (double)(H - 1) > 1.0 / 3.0 && (double)(w - 1) / (double)(W - 1) > 1.0 / 3.0;
        if (W % 4 == 0 && a16 && !mild) launch_bilinear_rows<float, 4>(src, dst, planes, h, w, H, W, st);
        else if (W % 2 == 0 && ((uintptr_t)dst % 8) == 0) launch_bilinear_rows<float, 2>(src, dst, planes, h, w, H, W, st);
        else launch_bilinear_rows<float, 1>(src, dst, planes, h, w, H, W, st);
    } else {
        const long long n = (long long)planes * H * W;
        if (dtype == HALO_F64) {
            const double sh = H > 1 ? (double)(h - 1) / (double)(H - 1) : 0.0, sw = W > 1 ? (double)(w - 1) / (double)(W - 1) : 0.0;
            hipLaunchKernelGGL((k_bilinear<double>), dim3(nblocks(n)), dim3(HTPB), 0, st, (const double *)src, (double *)dst, (long long)planes, (int)h, (int)w, (int)H, (int)W, sh, sw);
        } else {
            const float sh = H > 1 ? (float)(h - 1) / (float)(H - 1) : 0.0f, sw = W > 1 ? (float)(w - 1) / (float)(W - 1) : 0.0f;
            hipLaunchKernelGGL((k_bilinear<float>), dim3(nblocks(n)), dim3(HTPB), 0, st, (const float *)src, (float *)dst, (long long)planes, (int)h, (int)w, (int)H, (int)W, sh, sw);
        }
    }
    return check_launch("halo_bilinear_upsample");
}

extern "C" int halo_expmap0_project_bwd(const void *x, int x_dtype, const double *gy, void *gx, int64_t outer, int64_t C,
                                        int64_t inner, double c, void *stream)
{
    if (!x || !gy || !gx || outer <= 0 || C <= 0 || inner <= 0) return fail(HALO_E_ARG, "halo_expmap0_project_bwd: null/empty argument");
    if (c <= 0) return fail(HALO_E_UNSUPPORTED, "halo_expmap0_project_bwd: curvature must be > 0");
    const double ks = sqrt(fabs(-c) + 1e-15), rks = 1.0 / ks, maxnorm = (1.0 - 1e-5) / sqrt(fabs(-c) + 1e-15);
    hipStream_t st = (hipStream_t)stream;
    if (x_dtype == HALO_F32)
        hipLaunchKernelGGL((k_expmap0_project_bwd<float>), dim3(nblocks(outer * inner)), dim3(HTPB), 0, st, (const float *)x, gy, (float *)gx, (long long)outer, (int)C, (long long)inner, ks, rks, maxnorm);
    else if (x_dtype == HALO_F64)
        hipLaunchKernelGGL((k_expmap0_project_bwd<double>), dim3(nblocks(outer * inner)), dim3(HTPB), 0, st, (const double *)x, gy, (double *)gx, (long long)outer, (int)C, (long long)inner, ks, rks, maxnorm);
    else return fail(HALO_E_ARG, "halo_expmap0_project_bwd: bad dtype");
    return check_launch("halo_expmap0_project_bwd");
}

// ---- fused HyperMLR backward (k_mlr_bwd_pixels / _dxw / _final).  Workspace: consts | D (B,2O,hw) | dxx (B,hw) | Wt (C,40) | class partials | weight partials.
static inline bool mlr_bwd_fused_ok(int64_t C, int64_t O) { return O >= 1 && O <= MLRB_OP && C % 64 == 0 && C >= 64 && C <= 256; }
static inline int64_t mlr_bwd_pix_blocks(int64_t B, int64_t hw) { return cdiv(hw, MLRB_TPB) * B; }
extern "C" size_t halo_hypermlr_backward_workspace_bytes(int64_t B, int64_t C, int64_t O, int64_t hw)
{
    if (B <= 0 || C <= 0 || O <= 0 || hw <= 0 || !mlr_bwd_fused_ok(C, O)) return 0;       // 0: shape not served (use halo_hypermlr_bwd_terms)
    return halo_hypermlr_workspace_bytes(O, C) + 256 + ((size_t)B * (2 * O + 1) * hw + (size_t)C * MLRB_WS + (size_t)mlr_bwd_pix_blocks(B, hw) * 3 * O +
                                                       (size_t)MLRB_NWG * 2 * O * C) * sizeof(double) + 5 * 256;
}

extern "C" int halo_hypermlr_backward(const double *x, const double *P, const double *A, const void *gout, int gout_dtype, int64_t B,
                                      int64_t C, int64_t O, int64_t hw, double c, double *gx, double *gP, double *gA, void *workspace,
                                      size_t workspace_bytes, void *stream)
{
    if (!x || !P || !A || !gout || !gx || !gP || !gA || B <= 0 || C <= 0 || O <= 0 || hw <= 0)
        return fail(HALO_E_ARG, "halo_hypermlr_backward: null/empty argument");
    if (c <= 0) return fail(HALO_E_UNSUPPORTED, "halo_hypermlr_backward: curvature must be > 0");
    if (gout_dtype != HALO_F32 && gout_dtype != HALO_F64) return fail(HALO_E_ARG, "halo_hypermlr_backward: bad gout dtype");
    if (!mlr_bwd_fused_ok(C, O))
        return fail(HALO_E_UNSUPPORTED, "halo_hypermlr_backward: serves at most %d classes and 64 | C <= 256 (got O = %lld, C = %lld): use halo_hypermlr_bwd_terms",
                    MLRB_OP, (long long)O, (long long)C);
    if (!workspace || workspace_bytes < halo_hypermlr_backward_workspace_bytes(B, C, O, hw)) return fail(HALO_E_WORKSPACE, "halo_hypermlr_backward: workspace too small");
    if (B > 65535) return fail(HALO_E_UNSUPPORTED, "halo_hypermlr_backward: more than 65535 images per call");
    hipStream_t st = (hipStream_t)stream;
    Arena ar(workspace, workspace_bytes);
    double *consts = ar.take<double>((size_t)(3 * O + 2 * O * C));
    double *Dws = ar.take<double>((size_t)B * 2 * O * hw);
    double *dxx = ar.take<double>((size_t)B * hw);
    double *Wt = ar.take<double>((size_t)C * MLRB_WS);
    const int64_t npb = mlr_bwd_pix_blocks(B, hw);
    double *cls_part = ar.take<double>((size_t)npb * 3 * O);
    double *w_part = ar.take<double>((size_t)MLRB_NWG * 2 * O * C);
    if (!ar.ok() || !consts || !Dws || !dxx || !Wt || !cls_part || !w_part) return fail(HALO_E_WORKSPACE, "halo_hypermlr_backward: workspace too small");
    hipLaunchKernelGGL(k_mlr_prep, dim3((unsigned)O), dim3(64), (size_t)2 * C * sizeof(double), st, P, A, (int)O, (int)C, consts, Wt, MLRB_OP);
    {
        const dim3 gp((unsigned)cdiv(hw, MLRB_TPB), (unsigned)B);
        // >= 2 resident waves on every SIMD: weights through the scalar cache, otherwise from an LDS image (same bits)
        const bool scalar_w = (long long)B * hw >= 400000;
#define HALO_MLRB_PIX(SW_, TG_, LDS_)                                                                                              \
    hipLaunchKernelGGL((k_mlr_bwd_pixels<SW_, TG_>), gp, dim3(MLRB_TPB), LDS_, st, x, (const double *)consts, (const double *)Wt, (const TG_ *)gout, \
                       (int)O, (int)C, (long long)hw, c, Dws, dxx, cls_part)
        if (scalar_w) {
            if (gout_dtype == HALO_F32) HALO_MLRB_PIX(true, float, 0); else HALO_MLRB_PIX(true, double, 0);
        } else {
            const size_t lds = (size_t)C * MLRB_WS * sizeof(double);     // 80 KiB at C = 256
            static LdsLimitSeen seen_f, seen_d;
            if (lds > 48 * 1024 && !(gout_dtype == HALO_F32 ? raise_lds_limit(seen_f, (const void *)k_mlr_bwd_pixels<false, float>, 96 * 1024)
                                                            : raise_lds_limit(seen_d, (const void *)k_mlr_bwd_pixels<false, double>, 96 * 1024)))
                return fail(HALO_E_LAUNCH, "halo_hypermlr_backward: cannot raise the dynamic LDS limit");
            if (gout_dtype == HALO_F32) HALO_MLRB_PIX(false, float, lds); else HALO_MLRB_PIX(false, double, lds);
        }
#undef HALO_MLRB_PIX
        // one pass for d x and d W (k_mlr_bwd_dxw): 2 x 64 x 160 x 320 123 us against 138 for the whole backward as two kernels,
        // 1 x 64 x 640 x 1280 607 against 736
        const long long ntiles = cdiv(hw, 16) * B;
        const unsigned g = (unsigned)(cdiv(ntiles, 4) < MLRB_NWG ? cdiv(ntiles, 4) : MLRB_NWG);
        const size_t lds = ((size_t)4 * MLRX_KS * MLRZ_WS + (size_t)4 * (4 * MLRX_KS + 64) * MLRZ_RS) * sizeof(double);
        static LdsLimitSeen seen;
        if (!raise_lds_limit(seen, (const void *)k_mlr_bwd_dxw, 96 * 1024))
            return fail(HALO_E_LAUNCH, "halo_hypermlr_backward: cannot raise the dynamic LDS limit");
        hipLaunchKernelGGL(k_mlr_bwd_dxw, dim3(g, (unsigned)(C / 64)), dim3(256), lds, st, x, (const double *)consts, (const double *)Dws, (const double *)dxx,
                           (int)O, (int)C, (long long)hw, (int)B, gx, w_part);
        hipLaunchKernelGGL(k_mlr_bwd_final, dim3((unsigned)O), dim3(MLRF_TPB), 0, st, A, (const double *)consts, (const double *)w_part, (int)g,
                           (const double *)cls_part, (int)npb, (int)O, (int)C, gP, gA);
    }
    return check_launch("halo_hypermlr_backward");
}

extern "C" int halo_hypermlr_bwd_terms(const double *x, const double *P, const double *A, const double *gout, int64_t B, int64_t C,
                                       int64_t O, int64_t hw, double c, double *dpx, double *dxa, double *dxx, double *dpp,
                                       double *dpa, double *dan, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!x || !P || !A || !gout || !dpx || !dxa || !dxx || !dpp || !dpa || !dan || B <= 0 || C <= 0 || O <= 0 || hw <= 0)
        return fail(HALO_E_ARG, "halo_hypermlr_bwd_terms: null/empty argument");
    if (c <= 0) return fail(HALO_E_UNSUPPORTED, "halo_hypermlr_bwd_terms: curvature must be > 0");
    if (!workspace || workspace_bytes < halo_hypermlr_workspace_bytes(O, C)) return fail(HALO_E_WORKSPACE, "halo_hypermlr_bwd_terms: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    double *consts = (double *)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
    if (C > 3968) return fail(HALO_E_UNSUPPORTED, "HyperMLR: more than 3968 channels (the class rows are staged in 64 KiB of LDS)");
    hipLaunchKernelGGL(k_mlr_prep, dim3((unsigned)O), dim3(64), (size_t)2 * C * sizeof(double), st, P, A, (int)O, (int)C, consts);
    dim3 grid(nblocks(hw), (unsigned)B);
    hipLaunchKernelGGL((k_hypermlr_bwd_terms<10>), grid, dim3(HTPB), 0, st, x, (const double *)consts, gout, (int)O, (int)C, (long long)hw, c, dpx, dxa, dxx, dpp, dpa, dan);
    return check_launch("halo_hypermlr_bwd_terms");
}
