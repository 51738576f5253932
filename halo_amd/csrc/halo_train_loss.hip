// The training criterion from the head's low-resolution logits, forward and backward (core/train_learners.py:224-243, 328-368,
// 404-463, 505-563; core/loss/negative_learning_loss.py:6-16).
//
// Every learner step upsamples the (B, K, h, w) logits to the input size with F.interpolate(align_corners=True), takes
// torch.softmax, nn.CrossEntropyLoss(ignore_index) and NegativeLearningLoss of the full-resolution maps, and autograd takes it
// all back through the resize.  Here the full-resolution maps never exist:
//
//   logit (B, K, h, w) f32 + label (B, H, W) --k_upl_fwd--> per-block partials (B * nblk, 5) f64 --k_upl_finalize--> sums[5]
//   sums = {ce_sum, ce_count, nl_sum, nl_count, bad_label_count}
//   logit + label + sums + g_ce + g_nl --k_upl_bwd--> grad_logit (B, K, h, w) f32
//
// Numerics: the taps and the softmax are halo_softmax.hpp's statements of ATen's CPU kernels, so p -- and with it
// the negative-learning mask p < threshold -- is torch's, bit for bit, where halo_eval.hip's p is.  CE is ATen's log_softmax at
// the label, (x_y - m) - log(sum exp(x - m)); NL is -log((1 - p) + 1e-6) over the masked classes.  A label outside [0, K) that is
// not ignore_index is counted and never used as an index.
//
// Determinism: each thread sums its pixels in a fixed order in float64, a block folds its threads with a fixed shuffle tree into
// its own slab row, and one block adds the rows in a fixed order.  The backward is the adjoint of the resize as a GATHER: a block
// owns 32 low-resolution cells of one row, recomputes the per-pixel gradient d at every full-resolution pixel whose taps reach
// them, sums each cell's contributions along x in ascending column order per thread, stages the row sums in LDS and adds them
// along y in ascending row order.  No atomics anywhere, so repeated calls return identical bits.
#include "halo_common.hpp"
#include "halo_devmath.hpp"
#include "halo_softmax.hpp"

namespace halo {

constexpr int UTPB = 256;
constexpr int UF_ITERS = 4;                      // pixels per thread in the forward: 1024 per block
constexpr int UF_PX = UTPB * UF_ITERS;
constexpr int U_MAX_K = 1024;                    // the bound of k_eval_confusion_generic
constexpr int U_NSUM = 5;                        // ce_sum, ce_count, nl_sum, nl_count, bad_label_count
constexpr int UB_X = 32, UB_Y = UTPB / UB_X;     // backward block: 32 low-res cells of one row x 8 full-res rows per pass
constexpr int UB_OUT = 3;                        // ceil(19 * 32 / 256): (class, cell) outputs a thread owns

template <typename TL>
__device__ __forceinline__ long long load_label(const TL *p) { return (long long)__builtin_nontemporal_load(p); }

__device__ __forceinline__ bool label_in_range(long long t, int K) { return t >= 0 && t < K; }

// smallest output coordinate o in [0, n_out] whose lower tap make_taps(o).i0 is >= i (n_out when there is none).  i0 is
// monotone in o, so the outputs whose taps reach the input cells [i - 1, i] are [first_at_least(i - 1), first_at_least(i + 1)).
__device__ __forceinline__ int tap0(int o, float scale, int n_in)
{
    const int i0 = (int)(scale * (float)o);
    return i0 > n_in - 1 ? n_in - 1 : i0;
}
__device__ __forceinline__ int first_at_least(int i, float scale, int n_in, int n_out)
{
    if (i <= 0) return 0;
    float est = scale > 0.0f ? (float)i / scale : (float)n_out;
    int o = est >= (float)n_out ? n_out : (int)est;
    o = o < 0 ? 0 : o;
    while (o > 0 && tap0(o - 1, scale, n_in) >= i) --o;
    while (o < n_out && tap0(o, scale, n_in) < i) ++o;
    return o;
}

// weight of input cell i in output coordinate o's interpolation (both taps count where they coincide at the border)
__device__ __forceinline__ float tap_weight(const Taps<float> &t, int i) { return (t.i0 == i ? t.l0 : 0.0f) + (t.i1 == i ? t.l1 : 0.0f); }

__device__ __forceinline__ void block_sum5(double (&v)[U_NSUM], double *__restrict__ out)
{
    __shared__ double s[U_NSUM][UTPB / 64];
#pragma unroll
    for (int q = 0; q < U_NSUM; ++q)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v[q] += __shfl_xor(v[q], off);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int q = 0; q < U_NSUM; ++q) s[q][wave] = v[q];
    __syncthreads();
    if (threadIdx.x == 0)
#pragma unroll
        for (int q = 0; q < U_NSUM; ++q) {
            double a = s[q][0];
            for (int w = 1; w < UTPB / 64; ++w) a += s[q][w];
            out[q] = a;
        }
}

// ---------------------------------------------------------------- forward
template <int K_T, typename TL>
__global__ void __launch_bounds__(UTPB) k_upl_fwd(const float *__restrict__ logit, long long bstride, int h, int w, const TL *__restrict__ label,
                                                  int H, int W, float sh, float sw, long long ignore, float thr, int terms,
                                                  double *__restrict__ part)
{
    const int b = blockIdx.y;
    const int hw = H * W;
    const size_t plane_bytes = (size_t)h * w * 4;
    const char *base = reinterpret_cast<const char *>(logit + (size_t)b * bstride);
    auto at = [](const char *p, unsigned off) { return *reinterpret_cast<const float *>(p + off); };
    double ce_s = 0.0, nl_s = 0.0;
    int ce_n = 0, nl_n = 0, bad_n = 0;
#pragma unroll 1
    for (int it = 0; it < UF_ITERS; ++it) {
        const int i_raw = (blockIdx.x * UF_ITERS + it) * UTPB + threadIdx.x;
        const bool in = i_raw < hw;
        const int i = in ? i_raw : hw - 1;              // tail lanes compute the last pixel (the lean-softmax vote is per wave) and count nothing
        const int y = i / W, x = i - y * W;
        const Taps<float> ty = make_taps<float>(y, sh, h), tx = make_taps<float>(x, sw, w);
        const unsigned a00 = (unsigned)(ty.i0 * w + tx.i0) * 4u, a01 = (unsigned)(ty.i0 * w + tx.i1) * 4u,
                       a10 = (unsigned)(ty.i1 * w + tx.i0) * 4u, a11 = (unsigned)(ty.i1 * w + tx.i1) * 4u;
        float p[1][K_T], xs[K_T];
        const char *pl = base;
#pragma unroll
        for (int c = 0; c < K_T; ++c, pl += plane_bytes)
            xs[c] = p[0][c] = bilerp<float>(at(pl, a00), at(pl, a01), at(pl, a10), at(pl, a11), tx.l0, tx.l1, ty.l0, ty.l1);
        const long long t = load_label(label + (size_t)b * hw + i);
        const bool labelled = in && t != ignore && label_in_range(t, K_T);
        bad_n += (in && t != ignore && !label_in_range(t, K_T)) ? 1 : 0;
        if (!softmax_lean<K_T, 1>(p)) softmax_general<K_T, 1>(p);
        if ((terms & HALO_LOSS_CE) && labelled) {
            // ATen's log_softmax at the label: (x_y - max) - log(sum exp(x - max)); the label selects, it never indexes
            float m = xs[0], xt = xs[0];
#pragma unroll
            for (int c = 1; c < K_T; ++c) { m = xs[c] > m ? xs[c] : m; xt = c == t ? xs[c] : xt; }
            float s = 0.0f;
#pragma unroll
            for (int c = 0; c < K_T; ++c) s = s + det_expf(xs[c] - m);
            ce_s += (double)(-((xt - m) - det_logf(s)));
        }
        ce_n += labelled ? 1 : 0;
        if ((terms & HALO_LOSS_NL) && in) {
#pragma unroll
            for (int c = 0; c < K_T; ++c)
                if (p[0][c] < thr) { nl_s += (double)(-det_logf((1.0f - p[0][c]) + 1e-6f)); ++nl_n; }
        }
    }
    double v[U_NSUM] = {ce_s, (double)ce_n, nl_s, (double)nl_n, (double)bad_n};
    block_sum5(v, part + ((size_t)b * gridDim.x + blockIdx.x) * U_NSUM);
}

// Any class count up to U_MAX_K: rolled loops over the class planes, softmax_general's order (max by `>`, running sum of
// det_expf(x - m) from +0, one division per class), the interpolation recomputed in each pass.
template <typename TL>
__global__ void __launch_bounds__(UTPB) k_upl_fwd_generic(const float *__restrict__ logit, long long bstride, int K, int h, int w,
                                                          const TL *__restrict__ label, int H, int W, float sh, float sw, long long ignore,
                                                          float thr, int terms, double *__restrict__ part)
{
    const int b = blockIdx.y;
    const int hw = H * W;
    const long long hwl = (long long)h * w;
    const float *base = logit + (size_t)b * bstride;
    double ce_s = 0.0, nl_s = 0.0;
    int ce_n = 0, nl_n = 0, bad_n = 0;
#pragma unroll 1
    for (int it = 0; it < UF_ITERS; ++it) {
        const int i_raw = (blockIdx.x * UF_ITERS + it) * UTPB + threadIdx.x;
        if (i_raw >= hw) break;
        const int y = i_raw / W, x = i_raw - y * W;
        const Taps<float> ty = make_taps<float>(y, sh, h), tx = make_taps<float>(x, sw, w);
        auto interp = [&](int c) {
            const float *pl = base + (size_t)c * hwl;
            return bilerp<float>(pl[ty.i0 * w + tx.i0], pl[ty.i0 * w + tx.i1], pl[ty.i1 * w + tx.i0], pl[ty.i1 * w + tx.i1], tx.l0, tx.l1,
                                 ty.l0, ty.l1);
        };
        const long long t = load_label(label + (size_t)b * hw + i_raw);
        const bool labelled = t != ignore && label_in_range(t, K);
        bad_n += (t != ignore && !label_in_range(t, K)) ? 1 : 0;
        ce_n += labelled ? 1 : 0;
        float m = interp(0);
#pragma unroll 1
        for (int c = 1; c < K; ++c) { const float q = interp(c); m = q > m ? q : m; }
        float s = 0.0f;
#pragma unroll 1
        for (int c = 0; c < K; ++c) s = s + det_expf(interp(c) - m);
        if ((terms & HALO_LOSS_CE) && labelled) ce_s += (double)(-((interp((int)t) - m) - det_logf(s)));
        if (terms & HALO_LOSS_NL) {
#pragma unroll 1
            for (int c = 0; c < K; ++c) {
                const float p = det_expf(interp(c) - m) / s;
                if (p < thr) { nl_s += (double)(-det_logf((1.0f - p) + 1e-6f)); ++nl_n; }
            }
        }
    }
    double v[U_NSUM] = {ce_s, (double)ce_n, nl_s, (double)nl_n, (double)bad_n};
    block_sum5(v, part + ((size_t)b * gridDim.x + blockIdx.x) * U_NSUM);
}

// partials (nrow, 5) -> sums[5] (overwritten), one block, fixed order
__global__ void __launch_bounds__(UTPB) k_upl_finalize(const double *__restrict__ part, int nrow, double *__restrict__ sums)
{
    double v[U_NSUM] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int r = threadIdx.x; r < nrow; r += UTPB)
#pragma unroll
        for (int q = 0; q < U_NSUM; ++q) v[q] += part[(size_t)r * U_NSUM + q];
    block_sum5(v, sums);
}

// ---------------------------------------------------------------- backward
// The two upstream scales: g_ce / ce_count and g_nl / nl_count, zero for a term that is off, has no upstream gradient or no
// element (torch's mean CE over nothing is NaN with a zero gradient).
struct UplScales { float a, b; };
__device__ __forceinline__ UplScales upl_scales(int terms, const double *__restrict__ sums, const float *__restrict__ g_ce,
                                                const float *__restrict__ g_nl)
{
    UplScales s;
    s.a = (terms & HALO_LOSS_CE) && g_ce && sums[1] > 0.0 ? (float)((double)g_ce[0] / sums[1]) : 0.0f;
    s.b = (terms & HALO_LOSS_NL) && g_nl && sums[3] > 0.0 ? (float)((double)g_nl[0] / sums[3]) : 0.0f;
    return s;
}

// d_k = a (p_k - [k = y]) [labelled] + b p_k (q_k - sum_c q_c p_c),  q_c = [p_c < thr] / ((1 - p_c) + 1e-6), p in place
template <int K_T>
__device__ __forceinline__ void pixel_grad(float (&p)[K_T], long long t, bool labelled, float thr, UplScales sc)
{
    float sig = 0.0f, q[K_T];
#pragma unroll
    for (int c = 0; c < K_T; ++c) {
        q[c] = p[c] < thr ? 1.0f / ((1.0f - p[c]) + 1e-6f) : 0.0f;
        sig = __builtin_fmaf(q[c], p[c], sig);
    }
    const float a = labelled ? sc.a : 0.0f;
#pragma unroll
    for (int c = 0; c < K_T; ++c) p[c] = a * (p[c] - (c == t ? 1.0f : 0.0f)) + sc.b * (p[c] * (q[c] - sig));
}

template <int K_T, typename TL>
__global__ void __launch_bounds__(UTPB) k_upl_bwd(const float *__restrict__ logit, long long bstride, int h, int w, const TL *__restrict__ label,
                                                  int H, int W, float sh, float sw, long long ignore, float thr, int terms,
                                                  const double *__restrict__ sums, const float *__restrict__ g_ce, const float *__restrict__ g_nl,
                                                  float *__restrict__ grad)
{
    __shared__ float red[UB_Y][K_T][UB_X];
    const int jl = threadIdx.x % UB_X, yl = threadIdx.x / UB_X;
    const int i = blockIdx.y, b = blockIdx.z;
    const int j = blockIdx.x * UB_X + jl;
    const bool jin = j < w;
    const UplScales sc = upl_scales(terms, sums, g_ce, g_nl);
    const int Ya = first_at_least(i - 1, sh, h, H), Yb = first_at_least(i + 1, sh, h, H);
    const int Xa = jin ? first_at_least(j - 1, sw, w, W) : 0, Xb = jin ? first_at_least(j + 1, sw, w, W) : 0;
    const size_t plane_bytes = (size_t)h * w * 4;
    const char *base = reinterpret_cast<const char *>(logit + (size_t)b * bstride);
    auto at = [](const char *p, unsigned off) { return *reinterpret_cast<const float *>(p + off); };
    float acc[UB_OUT];
#pragma unroll
    for (int r = 0; r < UB_OUT; ++r) acc[r] = 0.0f;
#pragma unroll 1
    for (int y0 = Ya; y0 < Yb; y0 += UB_Y) {
        const int Y = y0 + yl;
        float rx[K_T];
#pragma unroll
        for (int c = 0; c < K_T; ++c) rx[c] = 0.0f;
        if (Y < Yb && jin) {
            const Taps<float> ty = make_taps<float>(Y, sh, h);
            const float wy = tap_weight(ty, i);
            const TL *lrow = label + (size_t)b * H * W + (size_t)Y * W;
#pragma unroll 1
            for (int X = Xa; X < Xb; ++X) {
                const Taps<float> tx = make_taps<float>(X, sw, w);
                const float wx = tap_weight(tx, j);
                const unsigned a00 = (unsigned)(ty.i0 * w + tx.i0) * 4u, a01 = (unsigned)(ty.i0 * w + tx.i1) * 4u,
                               a10 = (unsigned)(ty.i1 * w + tx.i0) * 4u, a11 = (unsigned)(ty.i1 * w + tx.i1) * 4u;
                float p[1][K_T];
                const char *pl = base;
#pragma unroll
                for (int c = 0; c < K_T; ++c, pl += plane_bytes)
                    p[0][c] = bilerp<float>(at(pl, a00), at(pl, a01), at(pl, a10), at(pl, a11), tx.l0, tx.l1, ty.l0, ty.l1);
                if (!softmax_lean<K_T, 1>(p)) softmax_general<K_T, 1>(p);
                const long long t = load_label(lrow + X);
                pixel_grad<K_T>(p[0], t, t != ignore && label_in_range(t, K_T), thr, sc);
#pragma unroll
                for (int c = 0; c < K_T; ++c) rx[c] = __builtin_fmaf(wx, p[0][c], rx[c]);
            }
#pragma unroll
            for (int c = 0; c < K_T; ++c) rx[c] = wy * rx[c];
        }
#pragma unroll
        for (int c = 0; c < K_T; ++c) red[yl][c][jl] = rx[c];
        __syncthreads();
        const int ny = Yb - y0 < UB_Y ? Yb - y0 : UB_Y;
#pragma unroll
        for (int r = 0; r < UB_OUT; ++r) {
            const int o = threadIdx.x + r * UTPB;
            if (o < K_T * UB_X) {
                const int c = o / UB_X, jj = o % UB_X;
                for (int yy = 0; yy < ny; ++yy) acc[r] += red[yy][c][jj];
            }
        }
        __syncthreads();
    }
    float *gb = grad + (size_t)b * K_T * h * w + (size_t)i * w + (size_t)blockIdx.x * UB_X;
#pragma unroll
    for (int r = 0; r < UB_OUT; ++r) {
        const int o = threadIdx.x + r * UTPB;
        if (o < K_T * UB_X) {
            const int c = o / UB_X, jj = o % UB_X;
            if (blockIdx.x * UB_X + jj < w) gb[(size_t)c * h * w + jj] = acc[r];
        }
    }
}

// Any class count: one thread per (image, class, low-res cell); at every pixel the taps reach, the pixel's max, sum and
// sum_c q_c p_c are recomputed over all classes (cost quadratic in K: the arm serves the odd class counts, the templated ones
// the models' 19 and 16).  Same order as k_upl_bwd: along x in ascending columns per full-res row, then along y.
template <typename TL>
__global__ void __launch_bounds__(UTPB) k_upl_bwd_generic(const float *__restrict__ logit, long long bstride, int K, int h, int w,
                                                          const TL *__restrict__ label, int H, int W, float sh, float sw, long long ignore,
                                                          float thr, int terms, const double *__restrict__ sums, const float *__restrict__ g_ce,
                                                          const float *__restrict__ g_nl, float *__restrict__ grad, long long n_out)
{
    const long long e = (long long)blockIdx.x * UTPB + threadIdx.x;
    if (e >= n_out) return;
    const long long hwl = (long long)h * w;
    const int j = (int)(e % w), i = (int)((e / w) % h), k = (int)((e / hwl) % K);
    const long long b = e / (hwl * K);
    const UplScales sc = upl_scales(terms, sums, g_ce, g_nl);
    const float *base = logit + (size_t)b * bstride;
    const int Ya = first_at_least(i - 1, sh, h, H), Yb = first_at_least(i + 1, sh, h, H);
    const int Xa = first_at_least(j - 1, sw, w, W), Xb = first_at_least(j + 1, sw, w, W);
    float acc = 0.0f;
#pragma unroll 1
    for (int Y = Ya; Y < Yb; ++Y) {
        const Taps<float> ty = make_taps<float>(Y, sh, h);
        const TL *lrow = label + (size_t)b * H * W + (size_t)Y * W;
        float rx = 0.0f;
#pragma unroll 1
        for (int X = Xa; X < Xb; ++X) {
            const Taps<float> tx = make_taps<float>(X, sw, w);
            auto interp = [&](int c) {
                const float *pl = base + (size_t)c * hwl;
                return bilerp<float>(pl[ty.i0 * w + tx.i0], pl[ty.i0 * w + tx.i1], pl[ty.i1 * w + tx.i0], pl[ty.i1 * w + tx.i1], tx.l0,
                                     tx.l1, ty.l0, ty.l1);
            };
            float m = interp(0);
#pragma unroll 1
            for (int c = 1; c < K; ++c) { const float q = interp(c); m = q > m ? q : m; }
            float s = 0.0f;
#pragma unroll 1
            for (int c = 0; c < K; ++c) s = s + det_expf(interp(c) - m);
            float sig = 0.0f;
            if (sc.b != 0.0f) {
#pragma unroll 1
                for (int c = 0; c < K; ++c) {
                    const float p = det_expf(interp(c) - m) / s;
                    sig = __builtin_fmaf(p < thr ? 1.0f / ((1.0f - p) + 1e-6f) : 0.0f, p, sig);
                }
            }
            const float p = det_expf(interp(k) - m) / s;
            const float q = p < thr ? 1.0f / ((1.0f - p) + 1e-6f) : 0.0f;
            const long long t = load_label(lrow + X);
            const float a = (t != ignore && label_in_range(t, K)) ? sc.a : 0.0f;
            const float d = a * (p - (k == t ? 1.0f : 0.0f)) + sc.b * (p * (q - sig));
            rx = __builtin_fmaf(tap_weight(tx, j), d, rx);
        }
        acc = __builtin_fmaf(tap_weight(ty, i), rx, acc);
    }
    grad[e] = acc;
}

// ---------------------------------------------------------------- host side
static int upl_blocks(int64_t H, int64_t W) { return (int)cdiv(H * W, UF_PX); }

static int upl_check(const char *who, const float *logit, const void *label, int64_t bstride, int64_t B, int64_t K, int64_t h, int64_t w,
                     int label_dtype, int64_t H, int64_t W, int terms)
{
    if (!logit || !label) return fail(HALO_E_ARG, "%s: null argument", who);
    if (K < 1 || B < 1 || h < 1 || w < 1 || H < 1 || W < 1)
        return fail(HALO_E_ARG, "%s: empty shape (B=%lld, K=%lld, h=%lld, w=%lld, H=%lld, W=%lld)", who, (long long)B, (long long)K,
                    (long long)h, (long long)w, (long long)H, (long long)W);
    if (K > U_MAX_K) return fail(HALO_E_UNSUPPORTED, "%s: %lld classes (at most %d)", who, (long long)K, U_MAX_K);
    if (H < h || W < w)   // torch interpolates down as well; this path upsamples only (the adjoint's gather assumes it)
        return fail(HALO_E_UNSUPPORTED, "%s: output %lld x %lld is smaller than the logits' %lld x %lld (upsampling only)", who,
                    (long long)H, (long long)W, (long long)h, (long long)w);
    if (label_dtype != HALO_I64 && label_dtype != HALO_I32 && label_dtype != HALO_U8)
        return fail(HALO_E_UNSUPPORTED, "%s: label dtype code %d (int64, int32 or uint8)", who, label_dtype);
    if (terms & ~(HALO_LOSS_CE | HALO_LOSS_NL)) return fail(HALO_E_ARG, "%s: terms %d", who, terms);
    if (bstride < K * h * w || h * w * 4 > 0xffffffffLL)
        return fail(HALO_E_ARG, "%s: logit planes %lld x %lld with batch stride %lld for %lld classes", who, (long long)h, (long long)w,
                    (long long)bstride, (long long)K);
    // pixel indices stay in int: the forward's last block, the backward's rows and cells; grid dimensions
    if (H * W > 0x7fffffffLL - UF_PX || B > 65535 || h > 65535 || B * K * h * w > 0x7fffffffLL * (int64_t)UTPB)
        return fail(HALO_E_UNSUPPORTED, "%s: image of %lld pixels x %lld images", who, (long long)(H * W), (long long)B);
    return HALO_OK;
}

// F.interpolate(align_corners=True): the source step of one output step, in float32 (as halo_eval.hip)
static float upl_scale(int64_t in, int64_t out) { return out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.0f; }

template <typename TL>
static void launch_fwd(dim3 grid, hipStream_t st, const float *logit, long long bs, int K, int h, int w, const void *label, int H, int W,
                       float sh, float sw, long long ig, float thr, int terms, double *part)
{
    const TL *lab = (const TL *)label;
    if (K == 19) hipLaunchKernelGGL((k_upl_fwd<19, TL>), grid, dim3(UTPB), 0, st, logit, bs, h, w, lab, H, W, sh, sw, ig, thr, terms, part);
    else if (K == 16) hipLaunchKernelGGL((k_upl_fwd<16, TL>), grid, dim3(UTPB), 0, st, logit, bs, h, w, lab, H, W, sh, sw, ig, thr, terms, part);
    else hipLaunchKernelGGL((k_upl_fwd_generic<TL>), grid, dim3(UTPB), 0, st, logit, bs, K, h, w, lab, H, W, sh, sw, ig, thr, terms, part);
}

template <typename TL>
static void launch_bwd(hipStream_t st, const float *logit, long long bs, int B, int K, int h, int w, const void *label, int H, int W, float sh,
                       float sw, long long ig, float thr, int terms, const double *sums, const float *g_ce, const float *g_nl, float *grad)
{
    const TL *lab = (const TL *)label;
    const dim3 grid((unsigned)cdiv(w, UB_X), (unsigned)h, (unsigned)B);
    if (K == 19)
        hipLaunchKernelGGL((k_upl_bwd<19, TL>), grid, dim3(UTPB), 0, st, logit, bs, h, w, lab, H, W, sh, sw, ig, thr, terms, sums, g_ce, g_nl, grad);
    else if (K == 16)
        hipLaunchKernelGGL((k_upl_bwd<16, TL>), grid, dim3(UTPB), 0, st, logit, bs, h, w, lab, H, W, sh, sw, ig, thr, terms, sums, g_ce, g_nl, grad);
    else {
        const long long n = (long long)B * K * h * w;
        hipLaunchKernelGGL((k_upl_bwd_generic<TL>), dim3((unsigned)cdiv(n, UTPB)), dim3(UTPB), 0, st, logit, bs, K, h, w, lab, H, W, sh, sw,
                           ig, thr, terms, sums, g_ce, g_nl, grad, n);
    }
}

}  // namespace halo

using namespace halo;

extern "C" size_t halo_upsampled_loss_workspace_bytes(int64_t B, int64_t K, int64_t H, int64_t W)
{
    if (B < 1 || K < 1 || H < 1 || W < 1) return 0;
    return (size_t)B * upl_blocks(H, W) * U_NSUM * sizeof(double) + 256;
}

extern "C" int halo_upsampled_loss_fwd(const float *logit, int64_t logit_bstride, int64_t B, int64_t K, int64_t h, int64_t w, const void *label,
                                       int label_dtype, int64_t H, int64_t W, int64_t ignore_index, double threshold, int terms, double *sums,
                                       void *workspace, size_t workspace_bytes, void *stream)
{
    const char *who = "halo_upsampled_loss_fwd";
    if (int rc = upl_check(who, logit, label, logit_bstride, B, K, h, w, label_dtype, H, W, terms)) return rc;
    if (!sums) return fail(HALO_E_ARG, "%s: null argument", who);
    const size_t need = halo_upsampled_loss_workspace_bytes(B, K, H, W);
    if (!workspace || workspace_bytes < need) return fail(HALO_E_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, need);
    double *part = (double *)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
    hipStream_t st = (hipStream_t)stream;
    const int nblk = upl_blocks(H, W);
    const dim3 grid((unsigned)nblk, (unsigned)B);
    const float sh = upl_scale(h, H), sw = upl_scale(w, W), thr = (float)threshold;
    const long long bs = (long long)logit_bstride, ig = (long long)ignore_index;
    if (label_dtype == HALO_I64) launch_fwd<int64_t>(grid, st, logit, bs, (int)K, (int)h, (int)w, label, (int)H, (int)W, sh, sw, ig, thr, terms, part);
    else if (label_dtype == HALO_I32) launch_fwd<int32_t>(grid, st, logit, bs, (int)K, (int)h, (int)w, label, (int)H, (int)W, sh, sw, ig, thr, terms, part);
    else launch_fwd<uint8_t>(grid, st, logit, bs, (int)K, (int)h, (int)w, label, (int)H, (int)W, sh, sw, ig, thr, terms, part);
    hipLaunchKernelGGL(k_upl_finalize, dim3(1), dim3(UTPB), 0, st, (const double *)part, (int)(B * nblk), sums);
    return check_launch(who);
}

extern "C" int halo_upsampled_loss_bwd(const float *logit, int64_t logit_bstride, int64_t B, int64_t K, int64_t h, int64_t w, const void *label,
                                       int label_dtype, int64_t H, int64_t W, int64_t ignore_index, double threshold, int terms,
                                       const double *sums, const float *g_ce, const float *g_nl, float *grad_logit, void *stream)
{
    const char *who = "halo_upsampled_loss_bwd";
    if (int rc = upl_check(who, logit, label, logit_bstride, B, K, h, w, label_dtype, H, W, terms)) return rc;
    if (!sums || !grad_logit) return fail(HALO_E_ARG, "%s: null argument", who);
    hipStream_t st = (hipStream_t)stream;
    const float sh = upl_scale(h, H), sw = upl_scale(w, W), thr = (float)threshold;
    const long long bs = (long long)logit_bstride, ig = (long long)ignore_index;
    if (label_dtype == HALO_I64)
        launch_bwd<int64_t>(st, logit, bs, (int)B, (int)K, (int)h, (int)w, label, (int)H, (int)W, sh, sw, ig, thr, terms, sums, g_ce, g_nl, grad_logit);
    else if (label_dtype == HALO_I32)
        launch_bwd<int32_t>(st, logit, bs, (int)B, (int)K, (int)h, (int)w, label, (int)H, (int)W, sh, sw, ig, thr, terms, sums, g_ce, g_nl, grad_logit);
    else
        launch_bwd<uint8_t>(st, logit, bs, (int)B, (int)K, (int)h, (int)w, label, (int)H, (int)W, sh, sw, ig, thr, terms, sums, g_ce, g_nl, grad_logit);
    return check_launch(who);
}
