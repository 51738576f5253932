// HFR, the weighted normalisation of the DeepLab-v3+ hyperbolic head, forward and backward (core/models/classifier.py:529-550).
//
// x = conv_reduce output (B, C, h, w) f32, P = h * w, wn_mlp = Sequential(Linear(C, C), BatchNorm1d(C), ReLU(), Linear(C, C)):
//
//   h_p = W1 x_p + b1      z_p = BN(h_p)      r_p = relu(z_p)      w_b = W2 (mean_p r_p) + b2      wc_b = clamp(w_b, min=1e-5)
//   n_bc = ||x_bc||_2 over p      y = (x / max(n, 1e-12)) * wc
//
// Forward, as passes over x (a block owns HT = 256 consecutive pixels of one image, one pixel per thread; h is recomputed
// from x in every pass and never stored):
//   k_hfr_stats       per-block (sum h, sum h^2) per channel, f64           --k_hfr_stats_merge--> (count, mean, M2) per channel
//   [the caller may merge the rows of several ranks here: halo_hfr_fwd_stats / halo_hfr_fwd_apply]
//   k_hfr_bn_prepare  scale / shift of the BN, the running-stat update
//   k_hfr_apply       per-block (sum r, sum x^2, #(z > 0), sum_{z>0} h) per (image, channel), f64     --k_hfr_colsum-->
//   k_hfr_weights     w = W2 mean_r + b2, the clamp, the norms
//   k_hfr_scale       y = (x / n) * wc
// Backward (g = dL/dy):
//   k_hfr_dot         A = sum_p g x per (image, channel)
//   k_hfr_bwd_small   g_W2, g_b2, g_gamma, g_beta and the two per-channel BN sums sum g_z, sum g_z zhat; g_z_p is
//                     [z_p > 0] (W2^T g_w_b) / P, one vector per image masked per pixel, so both sums follow from the forward's
//                     per-(image, channel) #(z > 0) and sum_{z>0} h without another pass over x
//   [the caller may all-reduce the two BN sums here: halo_hfr_bwd_reduce / halo_hfr_bwd_apply]
//   k_hfr_coef        per (image, channel): g_h_p = [z_p > 0] c1 + c0 + h_p c2 and g_x(normalize) = g e1 + x e2
//   k_hfr_bwd_out     g_x = W1^T g_h + the normalize branch, and per-block partials of g_W1 = sum g_h x^T, g_b1 = sum g_h
//                     --k_hfr_colsum--> g_W1, g_b1
//
// Determinism: every reduction runs in a fixed order (per-thread ascending loops, fixed shuffle trees, per-block slab rows
// added in ascending order by fixed segments).  No atomics anywhere, so repeated calls return identical bits.  z is
// recomputed with the same statements in every pass, so the ReLU mask of the backward is the forward's.
//
// C = 64 (REDUCED_CHANNELS) is templated: x of a pixel lives in registers and W1 / W2 are read with uniform addresses.
// The generic arm (any C <= 256) reads x from memory at every use and stages g_h in the workspace; it is the correctness route
// for other widths, not a tuned one.
#include "halo_common.hpp"

namespace halo {

constexpr int HT = 256;             // threads per block = pixels per tile
constexpr int HCW = 8;              // channels per LDS reduction chunk
constexpr int HSTR = HT + 1;        // LDS row stride (floats) of a chunk
constexpr int H_MAX_C = 256;
constexpr int HSEG = 16;            // row segments of k_hfr_colsum
constexpr int HSUB = 16;            // pixels per round of the g_W1 outer product (C = 64 arm)
constexpr int HGP = 64 + 4;         // LDS row stride of that round
constexpr int HDOT = 8;             // splits of a plane in k_hfr_dot
constexpr int HNQ = 4;              // per-(image, channel) forward sums: r, x^2, #(z > 0), sum_{z>0} h
constexpr int HNC = 5;              // per-(image, channel) backward coefficients: c1, c0, c2, e1, e2
constexpr float H_CLAMP = 1e-5f, H_NEPS = 1e-12f;

// the pixel's x column: registers for a templated width, memory for the generic arm
template <int CT> struct PixelX {
    float r[CT > 0 ? CT : 1];
    const float *xp;
    long long P;
    bool in;
    __device__ __forceinline__ void load(const float *__restrict__ col, long long P_, int C, bool in_)
    {
        xp = col, P = P_, in = in_;
        if constexpr (CT > 0) {
#pragma unroll
            for (int k = 0; k < CT; ++k) r[k] = in ? col[(size_t)k * P] : 0.0f;
        }
        (void)C;
    }
    __device__ __forceinline__ float operator()(int k) const
    {
        if constexpr (CT > 0) return r[k];
        else return in ? xp[(size_t)k * P] : 0.0f;
    }
};

// h_c = b1_c + sum_k W1[c, k] x_k, k ascending: the same statements in every pass
template <int CT>
__device__ __forceinline__ float hfr_h(const PixelX<CT> &X, const float *__restrict__ W1, const float *__restrict__ b1, int c, int C)
{
    const float *w = W1 + (size_t)c * C;
    float a = b1[c];
    if constexpr (CT > 0) {
#pragma unroll
        for (int k = 0; k < CT; ++k) a = fmaf(w[k], X.r[k], a);
    } else {
        for (int k = 0; k < C; ++k) a = fmaf(w[k], X(k), a);
    }
    return a;
}

__device__ __forceinline__ int tile_pixels(long long P, long long p0) { return (int)(P - p0 < HT ? P - p0 : HT); }

// ---------------------------------------------------------------- forward
// part row (b * gridDim.x + blockIdx.x): [sum h (C)][sum h^2 (C)] over the block's pixels, f64
template <int CT>
__global__ void __launch_bounds__(HT) k_hfr_stats(const float *__restrict__ x, long long P, int C_, const float *__restrict__ W1,
                                                  const float *__restrict__ b1, double *__restrict__ part)
{
    __shared__ float s_h[HCW][HSTR];
    const int C = CT > 0 ? CT : C_;
    const int b = blockIdx.y, tid = threadIdx.x;
    const long long p0 = (long long)blockIdx.x * HT, p = p0 + tid;
    const int nvalid = tile_pixels(P, p0);
    PixelX<CT> X;
    X.load(x + (size_t)b * C * P + (p < P ? p : 0), P, C, p < P);
    double *row = part + ((size_t)b * gridDim.x + blockIdx.x) * 2 * C;
    const int ci = tid >> 5, grp = tid & 31;
    for (int c0 = 0; c0 < C; c0 += HCW) {
#pragma unroll
        for (int i = 0; i < HCW; ++i)
            if (c0 + i < C) s_h[i][tid] = hfr_h(X, W1, b1, c0 + i, C);
        __syncthreads();
        double s = 0.0, s2 = 0.0;
        for (int j = 0; j < HT / 32; ++j) {
            const int px = j * 32 + grp;
            if (px < nvalid) {
                const double v = (double)s_h[ci][px];
                s += v;
                s2 += v * v;
            }
        }
#pragma unroll
        for (int off = 16; off > 0; off >>= 1) {
            s += __shfl_xor(s, off);
            s2 += __shfl_xor(s2, off);
        }
        if (grp == 0 && c0 + ci < C) {
            row[c0 + ci] = s;
            row[C + c0 + ci] = s2;
        }
        __syncthreads();
    }
}

__device__ __forceinline__ void chan_merge(double &n, double &m, double &M2, double nb, double mb, double M2b)
{
    if (nb == 0.0) return;
    if (n == 0.0) { n = nb, m = mb, M2 = M2b; return; }
    const double nn = n + nb, d = mb - m;
    m = m + d * (nb / nn);
    M2 = M2 + M2b + d * d * (n * nb / nn);
    n = nn;
}

// one block per channel: rows r = tid, tid + HT, ... merged in ascending order per thread, then a fixed tree; stats[c] =
// (count, mean, M2)
__global__ void __launch_bounds__(HT) k_hfr_stats_merge(const double *__restrict__ part, int R, int nblk, int C, long long P,
                                                        double *__restrict__ stats)
{
    __shared__ double sn[HT], sm[HT], sM[HT];
    const int c = blockIdx.x, tid = threadIdx.x;
    double n = 0.0, m = 0.0, M2 = 0.0;
    for (int r = tid; r < R; r += HT) {
        const double nr = (double)tile_pixels(P, (long long)(r % nblk) * HT);
        const double S = part[(size_t)r * 2 * C + c], S2 = part[(size_t)r * 2 * C + C + c];
        const double mr = S / nr;
        chan_merge(n, m, M2, nr, mr, fmax(S2 - S * mr, 0.0));
    }
    sn[tid] = n, sm[tid] = m, sM[tid] = M2;
    __syncthreads();
    for (int s = HT / 2; s > 0; s >>= 1) {
        if (tid < s) {
            double a = sn[tid], am = sm[tid], aM = sM[tid];
            chan_merge(a, am, aM, sn[tid + s], sm[tid + s], sM[tid + s]);
            sn[tid] = a, sm[tid] = am, sM[tid] = aM;
        }
        __syncthreads();
    }
    if (tid == 0) {
        stats[(size_t)c * 3 + 0] = sn[0];
        stats[(size_t)c * 3 + 1] = sm[0];
        stats[(size_t)c * 3 + 2] = sM[0];
    }
}

// thread c: aff = (scale, shift) f32 of z = h * scale + shift; bnp[c] = (mean, invstd, count) f64, count 0 for running stats.
// With stats, the running stats (when given) take F.batch_norm's update with the unbiased variance.
__global__ void k_hfr_bn_prepare(const double *__restrict__ stats, int C, float *__restrict__ rmean, float *__restrict__ rvar, double mom,
                                 double eps, const float *__restrict__ gamma, const float *__restrict__ beta, float *__restrict__ aff,
                                 double *__restrict__ bnp)
{
    const int c = threadIdx.x;
    if (c >= C) return;
    double mean, var, count;
    if (stats) {
        count = stats[(size_t)c * 3 + 0];
        mean = stats[(size_t)c * 3 + 1];
        const double M2 = stats[(size_t)c * 3 + 2];
        var = M2 / count;
        if (rmean) rmean[c] = (float)((1.0 - mom) * (double)rmean[c] + mom * mean);
        if (rvar) rvar[c] = (float)((1.0 - mom) * (double)rvar[c] + mom * (M2 / (count - 1.0)));
    } else {
        mean = (double)rmean[c];
        var = (double)rvar[c];
        count = 0.0;
    }
    const double inv = 1.0 / sqrt(var + eps);
    const double g = gamma ? (double)gamma[c] : 1.0, bt = beta ? (double)beta[c] : 0.0;
    aff[c] = (float)(g * inv);
    aff[C + c] = (float)(bt - mean * (g * inv));
    bnp[(size_t)c * 3 + 0] = mean;
    bnp[(size_t)c * 3 + 1] = inv;
    bnp[(size_t)c * 3 + 2] = count;
}

__device__ __forceinline__ float hfr_z(float h, float sc, float sh) { return fmaf(h, sc, sh); }

// part row (b * gridDim.x + blockIdx.x): HNQ x C sums over the block's pixels, f64
template <int CT>
__global__ void __launch_bounds__(HT) k_hfr_apply(const float *__restrict__ x, long long P, int C_, const float *__restrict__ W1,
                                                  const float *__restrict__ b1, const float *__restrict__ aff, double *__restrict__ part)
{
    __shared__ float s_h[HCW][HSTR], s_x[HCW][HSTR];
    const int C = CT > 0 ? CT : C_;
    const int b = blockIdx.y, tid = threadIdx.x;
    const long long p0 = (long long)blockIdx.x * HT, p = p0 + tid;
    const int nvalid = tile_pixels(P, p0);
    const float *xcol = x + (size_t)b * C * P + (p < P ? p : 0);
    PixelX<CT> X;
    X.load(xcol, P, C, p < P);
    double *row = part + ((size_t)b * gridDim.x + blockIdx.x) * HNQ * C;
    const int ci = tid >> 5, grp = tid & 31;
    for (int c0 = 0; c0 < C; c0 += HCW) {
#pragma unroll
        for (int i = 0; i < HCW; ++i)
            if (c0 + i < C) {
                s_h[i][tid] = hfr_h(X, W1, b1, c0 + i, C);
                s_x[i][tid] = p < P ? xcol[(size_t)(c0 + i) * P] : 0.0f;      // a cached reload: no dynamic register index
            }
        __syncthreads();
        const int c = c0 + ci;
        const float sc = c < C ? aff[c] : 0.0f, sh = c < C ? aff[C + c] : 0.0f;
        double sr = 0.0, sx = 0.0, sn = 0.0, smh = 0.0;
        for (int j = 0; j < HT / 32; ++j) {
            const int px = j * 32 + grp;
            if (px < nvalid) {
                const float h = s_h[ci][px];
                const float z = hfr_z(h, sc, sh);
                if (z > 0.0f) {
                    sr += (double)z;
                    sn += 1.0;
                    smh += (double)h;
                }
                const double xv = (double)s_x[ci][px];
                sx += xv * xv;
            }
        }
#pragma unroll
        for (int off = 16; off > 0; off >>= 1) {
            sr += __shfl_xor(sr, off);
            sx += __shfl_xor(sx, off);
            sn += __shfl_xor(sn, off);
            smh += __shfl_xor(smh, off);
        }
        if (grp == 0 && c < C) {
            row[c] = sr;
            row[C + c] = sx;
            row[2 * C + c] = sn;
            row[3 * C + c] = smh;
        }
        __syncthreads();
    }
}

// out[g][m] = sum_r part[g][r][m] (columns [0, M)): HSEG segments of consecutive rows, each summed in ascending order, then the
// segments in ascending order.  f64 into outd, or f32 into outf (m < msplit) / outf2 (m >= msplit).
template <typename T>
__global__ void __launch_bounds__(HT) k_hfr_colsum(const T *__restrict__ part, int R, int M, double *__restrict__ outd,
                                                   float *__restrict__ outf, int msplit, float *__restrict__ outf2)
{
    __shared__ double s[HSEG][16 + 1];
    const int g = blockIdx.y, col = threadIdx.x & 15, seg = threadIdx.x >> 4;
    const int m = blockIdx.x * 16 + col;
    const int r0 = (int)((long long)R * seg / HSEG), r1 = (int)((long long)R * (seg + 1) / HSEG);
    double a = 0.0;
    if (m < M)
        for (int r = r0; r < r1; ++r) a += (double)part[((size_t)g * R + r) * M + m];
    s[seg][col] = a;
    __syncthreads();
    if (threadIdx.x < 16 && m < M) {
        double t = s[0][col];
        for (int q = 1; q < HSEG; ++q) t += s[q][col];
        if (outd) outd[(size_t)g * M + m] = t;
        else if (m < msplit) outf[m] = (float)t;
        else outf2[m - msplit] = (float)t;
    }
}

// block b, thread c: mr[b][c] = mean_p r (f64); wv[b] = (w, wc, n, max(n, eps)) f32
__global__ void k_hfr_weights(const double *__restrict__ sums, int C, long long P, const float *__restrict__ W2, const float *__restrict__ b2,
                              double *__restrict__ mr, float *__restrict__ wv)
{
    __shared__ double sm[H_MAX_C];
    const int b = blockIdx.x, c = threadIdx.x;
    const double *s = sums + (size_t)b * HNQ * C;
    if (c < C) {
        sm[c] = s[c] / (double)P;
        mr[(size_t)b * C + c] = sm[c];
    }
    __syncthreads();
    if (c >= C) return;
    double w = (double)b2[c];
    for (int k = 0; k < C; ++k) w += (double)W2[(size_t)c * C + k] * sm[k];
    const float wr = (float)w;
    const float wc = wr < H_CLAMP ? H_CLAMP : wr;
    const float n = (float)sqrt(s[C + c]);
    const float nc = n < H_NEPS ? H_NEPS : n;
    float *o = wv + (size_t)b * 4 * C;
    o[c] = wr;
    o[C + c] = wc;
    o[2 * C + c] = n;
    o[3 * C + c] = nc;
}

// block (b * C + c, chunk): y = (x / max(n, eps)) * wc, F.normalize's division then the weight
__global__ void __launch_bounds__(HT) k_hfr_scale(const float *__restrict__ x, long long P, int C, const float *__restrict__ wv,
                                                  float *__restrict__ y)
{
    const int bc = blockIdx.x, b = bc / C, c = bc - b * C;
    const float wc = wv[(size_t)b * 4 * C + C + c], nc = wv[(size_t)b * 4 * C + 3 * C + c];
    const float *xr = x + (size_t)bc * P;
    float *yr = y + (size_t)bc * P;
    const long long base = (long long)blockIdx.y * HT * 4 + threadIdx.x;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long long i = base + (long long)j * HT;
        if (i < P) yr[i] = (xr[i] / nc) * wc;
    }
}

// ---------------------------------------------------------------- backward
__device__ __forceinline__ double block_sum(double v, double *s)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = s[0];
    for (int w = 1; w < HT / 64; ++w) t += s[w];
    return t;
}

// block (b * C + c, split): part[bc][split] = sum g x over the split's pixels, f64
__global__ void __launch_bounds__(HT) k_hfr_dot(const float *__restrict__ g, const float *__restrict__ x, long long P, double *__restrict__ part)
{
    __shared__ double s[HT / 64];
    const int bc = blockIdx.x, sp = blockIdx.y;
    const long long q0 = P * sp / HDOT, q1 = P * (sp + 1) / HDOT;
    const float *gr = g + (size_t)bc * P, *xr = x + (size_t)bc * P;
    double a = 0.0;
    for (long long i = q0 + threadIdx.x; i < q1; i += HT) a += (double)gr[i] * (double)xr[i];
    const double t = block_sum(a, s);
    if (threadIdx.x == 0) part[(size_t)bc * HDOT + sp] = t;
}

// one block.  bw = [A (B x C)][g_w (B x C)][g_r (B x C)] f64, g_r = (W2^T g_w) / P; gsums[c] = (sum g_z, sum g_z zhat) f64
__global__ void __launch_bounds__(HT) k_hfr_bwd_small(const double *__restrict__ dpart, const float *__restrict__ wv, const double *__restrict__ mr,
                                                      const double *__restrict__ sums, const double *__restrict__ bnp, const float *__restrict__ W2,
                                                      int B, int C, long long P, double *__restrict__ bw, float *__restrict__ gW2,
                                                      float *__restrict__ gb2, float *__restrict__ ggamma, float *__restrict__ gbeta,
                                                      double *__restrict__ gsums)
{
    const int tid = threadIdx.x, BC = B * C;
    double *A = bw, *gw = bw + BC, *gr = bw + 2 * BC;
    for (int i = tid; i < BC; i += HT) {
        const int b = i / C, c = i - b * C;
        double a = 0.0;
        for (int s = 0; s < HDOT; ++s) a += dpart[(size_t)i * HDOT + s];
        const float *o = wv + (size_t)b * 4 * C;
        A[i] = a;
        gw[i] = o[c] >= H_CLAMP ? a / (double)o[3 * C + c] : 0.0;     // sum_p g u, through the clamp
    }
    __syncthreads();
    for (int i = tid; i < BC; i += HT) {
        const int b = i / C, k = i - b * C;
        double a = 0.0;
        for (int c = 0; c < C; ++c) a += (double)W2[(size_t)c * C + k] * gw[(size_t)b * C + c];
        gr[i] = a / (double)P;
    }
    for (int e = tid; e < C * C; e += HT) {
        const int c = e / C, k = e - c * C;
        double a = 0.0;
        for (int b = 0; b < B; ++b) a += gw[(size_t)b * C + c] * mr[(size_t)b * C + k];
        gW2[e] = (float)a;
    }
    for (int c = tid; c < C; c += HT) {
        double a = 0.0;
        for (int b = 0; b < B; ++b) a += gw[(size_t)b * C + c];
        gb2[c] = (float)a;
    }
    __syncthreads();
    for (int k = tid; k < C; k += HT) {
        const double mean = bnp[(size_t)k * 3 + 0], inv = bnp[(size_t)k * 3 + 1];
        double sg = 0.0, sgz = 0.0;
        for (int b = 0; b < B; ++b) {
            const double *s = sums + (size_t)b * HNQ * C;
            const double cnt = s[2 * C + k], smh = s[3 * C + k], r = gr[(size_t)b * C + k];
            sg += r * cnt;
            sgz += r * (inv * (smh - mean * cnt));
        }
        gsums[(size_t)k * 2 + 0] = sg;
        gsums[(size_t)k * 2 + 1] = sgz;
        if (ggamma) ggamma[k] = (float)sgz;
        if (gbeta) gbeta[k] = (float)sg;
    }
}

// block b, thread c: coef[b] = (c1, c0, c2, e1, e2) f32.  Batch statistics (count > 0):
//   g_h = a ([z > 0] g_r - Sg / N - zhat Sgz / N),  a = gamma invstd,  zhat = (h - mean) invstd;  running statistics: g_h = a [z > 0] g_r.
//   normalize: g_x = g wc / nc - [n >= eps] x wc A / (nc^2 n)
__global__ void k_hfr_coef(const double *__restrict__ bw, const double *__restrict__ bnp, const double *__restrict__ gsums,
                           const float *__restrict__ gamma, const float *__restrict__ wv, int B, int C, float *__restrict__ coef)
{
    const int b = blockIdx.x, c = threadIdx.x;
    if (c >= C) return;
    const int BC = B * C;
    const double A = bw[(size_t)b * C + c], gr = bw[2 * (size_t)BC + (size_t)b * C + c];
    const double mean = bnp[(size_t)c * 3 + 0], inv = bnp[(size_t)c * 3 + 1], N = bnp[(size_t)c * 3 + 2];
    const double a = (gamma ? (double)gamma[c] : 1.0) * inv;
    double c0 = 0.0, c2 = 0.0;
    if (N > 0.0) {
        const double sg = gsums[(size_t)c * 2 + 0] / N, sgz = gsums[(size_t)c * 2 + 1] / N;
        c2 = -a * inv * sgz;
        c0 = -a * sg + a * mean * inv * sgz;
    }
    const float *o = wv + (size_t)b * 4 * C;
    const double wc = (double)o[C + c], n = (double)o[2 * C + c], nc = (double)o[3 * C + c];
    float *q = coef + (size_t)b * HNC * C;
    q[c] = (float)(a * gr);
    q[C + c] = (float)c0;
    q[2 * C + c] = (float)c2;
    q[3 * C + c] = (float)(wc / nc);
    q[4 * C + c] = n >= (double)H_NEPS ? (float)(-wc * A / (nc * nc * n)) : 0.0f;
}

__device__ __forceinline__ float hfr_gh(float h, float sc, float sh, float c1, float c0, float c2)
{
    float v = fmaf(h, c2, c0);
    if (hfr_z(h, sc, sh) > 0.0f) v += c1;
    return v;
}

// C = 64: g_h of the pixel in registers, g_x written, then HT / HSUB rounds of the outer product sum_p g_h x^T staged in LDS;
// thread (cb, kb) owns the 4 x 4 block (4 cb + i, 4 kb + j) and, for kb = 0, g_b1 of 4 cb + i.  wpart row = [g_W1 (C x C)][g_b1 (C)]
template <int CT>
__global__ void __launch_bounds__(HT) k_hfr_bwd_out(const float *__restrict__ x, const float *__restrict__ g, long long P, const float *__restrict__ W1,
                                                    const float *__restrict__ b1, const float *__restrict__ aff, const float *__restrict__ coef,
                                                    float *__restrict__ gx, float *__restrict__ wpart)
{
    static_assert(CT == 64, "the register arm is written for C = 64");
    __shared__ float s_g[HSUB][HGP], s_x[HSUB][HGP];
    constexpr int C = CT;
    const int b = blockIdx.y, tid = threadIdx.x;
    const long long p0 = (long long)blockIdx.x * HT, p = p0 + tid;
    const bool in = p < P;
    const size_t off = (size_t)b * C * P + (in ? p : 0);
    PixelX<CT> X;
    X.load(x + off, P, C, in);
    const float *q = coef + (size_t)b * HNC * C;
    float gh[C], acc[C];
#pragma unroll
    for (int k = 0; k < C; ++k) acc[k] = 0.0f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float h = hfr_h(X, W1, b1, c, C);
        const float v = hfr_gh(h, aff[c], aff[C + c], q[c], q[C + c], q[2 * C + c]);
        gh[c] = in ? v : 0.0f;
        const float *w = W1 + (size_t)c * C;
#pragma unroll
        for (int k = 0; k < C; ++k) acc[k] = fmaf(w[k], v, acc[k]);
    }
    if (in) {
#pragma unroll
        for (int k = 0; k < C; ++k) {
            const float gk = g[off + (size_t)k * P];
            gx[off + (size_t)k * P] = acc[k] + fmaf(X.r[k], q[4 * C + k], gk * q[3 * C + k]);
        }
    }
    const int cb = tid >> 4, kb = tid & 15;
    float o[4][4] = {}, ob[4] = {};
#pragma unroll 1
    for (int s = 0; s < HT / HSUB; ++s) {
        if ((tid >> 4) == s) {
            const int lp = tid & (HSUB - 1);
#pragma unroll
            for (int k = 0; k < C; ++k) {
                s_g[lp][k] = gh[k];
                s_x[lp][k] = X.r[k];
            }
        }
        __syncthreads();
#pragma unroll 4
        for (int lp = 0; lp < HSUB; ++lp) {
            const float4 a = *reinterpret_cast<const float4 *>(&s_g[lp][cb * 4]);
            const float4 xv = *reinterpret_cast<const float4 *>(&s_x[lp][kb * 4]);
            const float av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {xv.x, xv.y, xv.z, xv.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
#pragma unroll
                for (int j = 0; j < 4; ++j) o[i][j] = fmaf(av[i], bv[j], o[i][j]);
                ob[i] += av[i];
            }
        }
        __syncthreads();
    }
    float *row = wpart + ((size_t)b * gridDim.x + blockIdx.x) * (size_t)(C * C + C);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        *reinterpret_cast<float4 *>(&row[(size_t)(cb * 4 + i) * C + kb * 4]) = make_float4(o[i][0], o[i][1], o[i][2], o[i][3]);
        if (kb == 0) row[C * C + cb * 4 + i] = ob[i];
    }
}

// generic C: g_h staged in ghw (B, C, P), then the block's outer-product entries one per thread pass
__global__ void __launch_bounds__(HT) k_hfr_bwd_out_generic(const float *__restrict__ x, const float *__restrict__ g, long long P, int C,
                                                            const float *__restrict__ W1, const float *__restrict__ b1, const float *__restrict__ aff,
                                                            const float *__restrict__ coef, float *__restrict__ gx, float *__restrict__ wpart,
                                                            float *__restrict__ ghw)
{
    const int b = blockIdx.y, tid = threadIdx.x;
    const long long p0 = (long long)blockIdx.x * HT, p = p0 + tid;
    const bool in = p < P;
    const int nvalid = tile_pixels(P, p0);
    const size_t plane = (size_t)b * C * P;
    PixelX<0> X;
    X.load(x + plane + (in ? p : 0), P, C, in);
    const float *q = coef + (size_t)b * HNC * C;
    if (in) {
        for (int c = 0; c < C; ++c) {
            const float h = hfr_h(X, W1, b1, c, C);
            ghw[plane + (size_t)c * P + p] = hfr_gh(h, aff[c], aff[C + c], q[c], q[C + c], q[2 * C + c]);
        }
        for (int k = 0; k < C; ++k) {
            float a = 0.0f;
            for (int c = 0; c < C; ++c) a = fmaf(W1[(size_t)c * C + k], ghw[plane + (size_t)c * P + p], a);
            const size_t o = plane + (size_t)k * P + p;
            gx[o] = a + fmaf(x[o], q[4 * C + k], g[o] * q[3 * C + k]);
        }
    }
    __syncthreads();
    float *row = wpart + ((size_t)b * gridDim.x + blockIdx.x) * (size_t)(C * C + C);
    for (int e = tid; e < C * C + C; e += HT) {
        const int c = e < C * C ? e / C : e - C * C, k = e < C * C ? e - c * C : -1;
        const float *gr = ghw + plane + (size_t)c * P + p0;
        const float *xr = x + plane + (size_t)(k < 0 ? 0 : k) * P + p0;
        float a = 0.0f;
        for (int i = 0; i < nvalid; ++i) a = k < 0 ? a + gr[i] : fmaf(gr[i], xr[i], a);
        row[e] = a;
    }
}

// ---------------------------------------------------------------- host side
struct HfrLayout {
    double *part1, *part2, *sums, *bnp, *mr, *dpart, *bw, *gsums_local;
    float *aff, *wv, *coef, *wpart, *ghw;
    size_t bytes;
};

static int hfr_blocks(int64_t P) { return (int)cdiv(P, HT); }

static HfrLayout hfr_layout(void *ws, size_t cap, int64_t B, int64_t C, int64_t P)
{
    Arena a(ws, cap);
    HfrLayout L;
    const size_t R = (size_t)B * hfr_blocks(P);
    L.part1 = a.take<double>(R * 2 * C);
    L.part2 = a.take<double>(R * HNQ * C);
    L.sums = a.take<double>((size_t)B * HNQ * C);
    L.bnp = a.take<double>((size_t)C * 3);
    L.mr = a.take<double>((size_t)B * C);
    L.dpart = a.take<double>((size_t)B * C * HDOT);
    L.bw = a.take<double>((size_t)B * C * 3);
    L.gsums_local = a.take<double>((size_t)C * 2);
    L.aff = a.take<float>((size_t)C * 2);
    L.wv = a.take<float>((size_t)B * 4 * C);
    L.coef = a.take<float>((size_t)B * HNC * C);
    L.wpart = a.take<float>(R * (size_t)(C * C + C));
    L.ghw = C == 64 ? nullptr : a.take<float>((size_t)B * C * P);
    L.bytes = a.off + 256;
    return L;
}

static int hfr_check(const char *who, int64_t B, int64_t C, int64_t P)
{
    if (B < 1 || C < 1 || P < 1) return fail(HALO_E_ARG, "%s: empty shape B=%lld C=%lld P=%lld", who, (long long)B, (long long)C, (long long)P);
    if (C > H_MAX_C) return fail(HALO_E_UNSUPPORTED, "%s: C = %lld > %d", who, (long long)C, H_MAX_C);
    if (cdiv(P, HT * 4) > 65535 || B > 65535 || B * C > ((int64_t)1 << 31) - 1)
        return fail(HALO_E_UNSUPPORTED, "%s: shape B=%lld C=%lld P=%lld out of range", who, (long long)B, (long long)C, (long long)P);
    return HALO_OK;
}

static int hfr_ws(const char *who, void *ws, size_t bytes, int64_t B, int64_t C, int64_t P, HfrLayout &L)
{
    const size_t need = halo_hfr_workspace_bytes(B, C, P);
    if (!ws || bytes < need) return fail(HALO_E_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", who, bytes, need);
    L = hfr_layout(ws, bytes, B, C, P);
    return HALO_OK;
}

template <typename T>
static void colsum(hipStream_t st, const T *part, int G, int R, int M, double *outd, float *outf, int msplit, float *outf2)
{
    hipLaunchKernelGGL((k_hfr_colsum<T>), dim3((unsigned)cdiv(M, 16), (unsigned)G), dim3(HT), 0, st, part, R, M, outd, outf, msplit, outf2);
}

}  // namespace halo

using namespace halo;

extern "C" size_t halo_hfr_workspace_bytes(int64_t B, int64_t C, int64_t P)
{
    if (B < 1 || C < 1 || P < 1 || C > H_MAX_C) return 0;
    return hfr_layout(nullptr, (size_t)-1 / 2, B, C, P).bytes;
}

extern "C" int halo_hfr_fwd_stats(const float *x, int64_t B, int64_t C, int64_t P, const float *W1, const float *b1, double *stats,
                                  void *workspace, size_t workspace_bytes, void *stream)
{
    const char *who = "halo_hfr_fwd_stats";
    if (int rc = hfr_check(who, B, C, P)) return rc;
    if (!x || !W1 || !b1 || !stats) return fail(HALO_E_ARG, "%s: null argument", who);
    HfrLayout L;
    if (int rc = hfr_ws(who, workspace, workspace_bytes, B, C, P, L)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int nblk = hfr_blocks(P);
    const dim3 grid((unsigned)nblk, (unsigned)B);
    if (C == 64) hipLaunchKernelGGL((k_hfr_stats<64>), grid, dim3(HT), 0, st, x, (long long)P, (int)C, W1, b1, L.part1);
    else hipLaunchKernelGGL((k_hfr_stats<0>), grid, dim3(HT), 0, st, x, (long long)P, (int)C, W1, b1, L.part1);
    hipLaunchKernelGGL(k_hfr_stats_merge, dim3((unsigned)C), dim3(HT), 0, st, (const double *)L.part1, (int)(B * nblk), nblk, (int)C,
                       (long long)P, stats);
    return check_launch(who);
}

extern "C" int halo_hfr_fwd_apply(const float *x, int64_t B, int64_t C, int64_t P, const float *W1, const float *b1, const double *stats,
                                  float *running_mean, float *running_var, double momentum, double eps, const float *gamma, const float *beta,
                                  const float *W2, const float *b2, float *y, void *workspace, size_t workspace_bytes, void *stream)
{
    const char *who = "halo_hfr_fwd_apply";
    if (int rc = hfr_check(who, B, C, P)) return rc;
    if (!x || !W1 || !b1 || !W2 || !b2 || !y) return fail(HALO_E_ARG, "%s: null argument", who);
    if (!stats && (!running_mean || !running_var)) return fail(HALO_E_ARG, "%s: neither batch statistics nor running statistics", who);
    if (!stats && B * P < 1) return fail(HALO_E_ARG, "%s: empty batch", who);
    HfrLayout L;
    if (int rc = hfr_ws(who, workspace, workspace_bytes, B, C, P, L)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int nblk = hfr_blocks(P);
    const dim3 grid((unsigned)nblk, (unsigned)B);
    hipLaunchKernelGGL(k_hfr_bn_prepare, dim3(1), dim3(H_MAX_C), 0, st, stats, (int)C, running_mean, running_var, momentum, eps, gamma, beta,
                       L.aff, L.bnp);
    if (C == 64) hipLaunchKernelGGL((k_hfr_apply<64>), grid, dim3(HT), 0, st, x, (long long)P, (int)C, W1, b1, (const float *)L.aff, L.part2);
    else hipLaunchKernelGGL((k_hfr_apply<0>), grid, dim3(HT), 0, st, x, (long long)P, (int)C, W1, b1, (const float *)L.aff, L.part2);
    colsum<double>(st, L.part2, (int)B, nblk, (int)(HNQ * C), L.sums, nullptr, 0, nullptr);
    hipLaunchKernelGGL(k_hfr_weights, dim3((unsigned)B), dim3(H_MAX_C), 0, st, (const double *)L.sums, (int)C, (long long)P, W2, b2, L.mr, L.wv);
    hipLaunchKernelGGL(k_hfr_scale, dim3((unsigned)(B * C), (unsigned)cdiv(P, HT * 4)), dim3(HT), 0, st, x, (long long)P, (int)C,
                       (const float *)L.wv, y);
    return check_launch(who);
}

extern "C" int halo_hfr_bwd_reduce(const float *x, int64_t B, int64_t C, int64_t P, const float *W2, const float *g, float *g_W2, float *g_b2,
                                   float *g_gamma, float *g_beta, double *gsums, void *workspace, size_t workspace_bytes, void *stream)
{
    const char *who = "halo_hfr_bwd_reduce";
    if (int rc = hfr_check(who, B, C, P)) return rc;
    if (!x || !W2 || !g || !g_W2 || !g_b2 || !gsums) return fail(HALO_E_ARG, "%s: null argument", who);
    HfrLayout L;
    if (int rc = hfr_ws(who, workspace, workspace_bytes, B, C, P, L)) return rc;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_hfr_dot, dim3((unsigned)(B * C), HDOT), dim3(HT), 0, st, g, x, (long long)P, L.dpart);
    hipLaunchKernelGGL(k_hfr_bwd_small, dim3(1), dim3(HT), 0, st, (const double *)L.dpart, (const float *)L.wv, (const double *)L.mr,
                       (const double *)L.sums, (const double *)L.bnp, W2, (int)B, (int)C, (long long)P, L.bw, g_W2, g_b2, g_gamma, g_beta, gsums);
    return check_launch(who);
}

extern "C" int halo_hfr_bwd_apply(const float *x, int64_t B, int64_t C, int64_t P, const float *W1, const float *b1, const float *gamma,
                                  const float *g, const double *gsums, float *g_x, float *g_W1, float *g_b1, void *workspace,
                                  size_t workspace_bytes, void *stream)
{
    const char *who = "halo_hfr_bwd_apply";
    if (int rc = hfr_check(who, B, C, P)) return rc;
    if (!x || !W1 || !b1 || !g || !gsums || !g_x || !g_W1 || !g_b1) return fail(HALO_E_ARG, "%s: null argument", who);
    HfrLayout L;
    if (int rc = hfr_ws(who, workspace, workspace_bytes, B, C, P, L)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int nblk = hfr_blocks(P);
    const dim3 grid((unsigned)nblk, (unsigned)B);
    hipLaunchKernelGGL(k_hfr_coef, dim3((unsigned)B), dim3(H_MAX_C), 0, st, (const double *)L.bw, (const double *)L.bnp, gsums, gamma,
                       (const float *)L.wv, (int)B, (int)C, L.coef);
    if (C == 64)
        hipLaunchKernelGGL((k_hfr_bwd_out<64>), grid, dim3(HT), 0, st, x, g, (long long)P, W1, b1, (const float *)L.aff, (const float *)L.coef,
                           g_x, L.wpart);
    else
        hipLaunchKernelGGL(k_hfr_bwd_out_generic, grid, dim3(HT), 0, st, x, g, (long long)P, (int)C, W1, b1, (const float *)L.aff,
                           (const float *)L.coef, g_x, L.wpart, L.ghw);
    colsum<float>(st, L.wpart, 1, (int)(B * nblk), (int)(C * C + C), nullptr, g_W1, (int)(C * C), g_b1);
    return check_launch(who);
}
