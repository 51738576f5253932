// The validation metric as HIP kernels for gfx950 (core/train_learners.py:57-128, core/utils/misc.py:35-47).
//
// Per image the reference upsamples the head's logits of [x, flip(x)] to label size, takes the softmax, averages the map with
// the flipped one, takes the arg-max and histograms prediction / label / agreement with torch.histc on the host.  Here one
// launch covers B images and the full-resolution maps never exist:
//
//   logit (B*views, K, h, w) f32 + label (B, H, W) --k_eval_confusion--> per-block partials (B, nblk, 3, K) u32 [+ pred (B,H,W) i64]
//   pred (B, H, W) + label                     --k_confusion_from_pred--> the same partials
//   partials --k_confusion_finalize--> counts (B, 3, K) i64 += [intersection, union, target]
//
// Numerics: the taps and the softmax are halo_softmax.hpp's statements of ATen's CPU kernels; view 1 is
// interpolated at column W-1-x with that column's own taps (the interpolation is not mirror-symmetric in float32), the two
// probability maps are averaged as (a + b) / 2, and the arg-max follows torch.max(dim) on the CPU: the first maximal class wins
// and a NaN counts as maximal.  The counts are integers: histc's float32 bins are exact below 2^24 per bin.
//
// The histogram (cdna guide, Guideline 12): a wave folds its 64 pixels into one (prediction, label) key per distinct pair with a
// ballot loop, its leader lane adds the pair's population to a 3*K u32 LDS histogram, and each block writes that histogram to
// its own slab row.  No global atomics; the finalize kernel adds the partials into the caller's int64 accumulator, so an epoch's
// sum stays on the device.
#include "halo_common.hpp"
#include "halo_devmath.hpp"
#include "halo_softmax.hpp"

namespace halo {

constexpr int ETPB = 256;
constexpr int EV_ITERS = 4;                       // pixels per thread: 1024 per block, 2048 blocks (8192 waves) per 1024 x 2048 image
constexpr int EV_PX = ETPB * EV_ITERS;
constexpr int EV_MAX_K = 1024;                    // (prediction, label) key packs two classes in 16 bits each; 12 KB of LDS

template <typename TL>
__device__ __forceinline__ long long load_nt(const TL *p) { return (long long)__builtin_nontemporal_load(p); }

// the reference's integer semantics (intersectionAndUnionGPU): o = ignore where the label is ignored, else the prediction;
// histc(bins=K, min=0, max=K-1) keeps exactly the integers 0..K-1.  Key: (o' << 16) | t' with K standing for "not counted";
// NONE is the key of a pixel that counts nowhere.
__device__ __forceinline__ int count_key(long long pred, long long t, long long ignore, int K)
{
    const long long o = t == ignore ? ignore : pred;
    const int oc = (o >= 0 && o < K) ? (int)o : K;
    const int tc = (t >= 0 && t < K) ? (int)t : K;
    return (oc << 16) | tc;
}
__device__ __forceinline__ int key_none(int K) { return (K << 16) | K; }

// Fold the wave's keys into the block histogram h = [intersection K | output K | target K].  Wave-uniform: every lane of the
// wave calls it; `valid` is false for tail lanes and for pixels that count nowhere.
__device__ __forceinline__ void wave_count(int key, bool valid, int K, unsigned *h)
{
    const int lane = threadIdx.x & 63;
    unsigned long long rem = __ballot(valid);
    while (rem) {
        const int leader = __builtin_ctzll(rem);
        const int k = __builtin_amdgcn_readlane(key, leader);
        const unsigned long long m = __ballot(key == k) & rem;
        if (lane == leader) {
            const unsigned n = (unsigned)__popcll(m);
            const int oc = k >> 16, tc = k & 0xffff;
            if (oc < K) atomicAdd(&h[K + oc], n);
            if (tc < K) atomicAdd(&h[2 * K + tc], n);
            if (oc == tc && oc < K) atomicAdd(&h[oc], n);
        }
        rem &= ~m;
    }
}

__device__ __forceinline__ void clear_hist(unsigned *h, int n)
{
    for (int j = threadIdx.x; j < n; j += ETPB) h[j] = 0u;
    __syncthreads();
}

__device__ __forceinline__ void store_hist(const unsigned *h, int n, unsigned *__restrict__ part)
{
    __syncthreads();
    unsigned *dst = part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * n;
    for (int j = threadIdx.x; j < n; j += ETPB) dst[j] = h[j];
}

// torch.max(dim) on the CPU (ATen compare_base_kernel): `if (!(v <= best)) { best = v; idx = c; if (isnan(v)) break; }`
template <int K_T>
__device__ __forceinline__ int argmax_torch(const float (&a)[K_T])
{
    float best = a[0];
    int am = 0;
    bool stop = a[0] != a[0];
#pragma unroll
    for (int c = 1; c < K_T; ++c) {
        const bool up = !stop && !(a[c] <= best);
        am = up ? c : am;
        best = up ? a[c] : best;
        stop = stop || (up && a[c] != a[c]);
    }
    return am;
}

// One output pixel per thread and iteration.  VIEWS = 2: view 1 is the flipped image's map, read at the mirrored column.
template <int K_T, int VIEWS, typename TL>
__global__ void __launch_bounds__(ETPB) k_eval_confusion(const float *__restrict__ logit, long long bstride, int h, int w,
                                                         const TL *__restrict__ label, int H, int W, float sh, float sw, long long ignore,
                                                         unsigned *__restrict__ part, long long *__restrict__ pred_out)
{
    __shared__ unsigned hist[3 * K_T];
    clear_hist(hist, 3 * K_T);
    const int b = blockIdx.y;
    const int hw = H * W;
    const size_t plane_bytes = (size_t)h * w * 4;
    auto at = [](const char *base, unsigned off) { return *reinterpret_cast<const float *>(base + off); };
#pragma unroll 1
    for (int it = 0; it < EV_ITERS; ++it) {
        const int i_raw = (blockIdx.x * EV_ITERS + it) * ETPB + threadIdx.x;
        const bool in = i_raw < hw;
        const int i = in ? i_raw : hw - 1;              // tail lanes compute the last pixel (the lean-softmax vote is per wave) and count nothing
        const int y = i / W, x = i - y * W;
        const Taps<float> ty = make_taps<float>(y, sh, h);
        float p[VIEWS][K_T];
#pragma unroll
        for (int v = 0; v < VIEWS; ++v) {
            const Taps<float> tx = make_taps<float>(v == 0 ? x : W - 1 - x, sw, w);
            const char *pl = reinterpret_cast<const char *>(logit + (size_t)(VIEWS * b + v) * bstride);
            const unsigned a00 = (unsigned)(ty.i0 * w + tx.i0) * 4u, a01 = (unsigned)(ty.i0 * w + tx.i1) * 4u,
                           a10 = (unsigned)(ty.i1 * w + tx.i0) * 4u, a11 = (unsigned)(ty.i1 * w + tx.i1) * 4u;
#pragma unroll
            for (int c = 0; c < K_T; ++c, pl += plane_bytes)
                p[v][c] = bilerp<float>(at(pl, a00), at(pl, a01), at(pl, a10), at(pl, a11), tx.l0, tx.l1, ty.l0, ty.l1);
        }
        const long long t = load_nt(label + (size_t)b * hw + i);
        if (!softmax_lean<K_T, VIEWS>(p)) softmax_general<K_T, VIEWS>(p);
        float a[K_T];
#pragma unroll
        for (int c = 0; c < K_T; ++c) a[c] = VIEWS == 2 ? (p[0][c] + p[VIEWS - 1][c]) / 2.0f : p[0][c];
        const int pr = argmax_torch<K_T>(a);
        if (pred_out && in) __builtin_nontemporal_store((long long)pr, pred_out + (size_t)b * hw + i);
        const int key = count_key(pr, t, ignore, K_T);
        wave_count(key, in && key != key_none(K_T), K_T, hist);
    }
    store_hist(hist, 3 * K_T, part);
}

// Any class count: the same arithmetic with rolled loops over the class planes (softmax_general's order: max by `>`, running sum
// of det_expf(x - m) from +0, one division per class), the interpolation recomputed in each of the three passes.
template <int VIEWS, typename TL>
__global__ void __launch_bounds__(ETPB) k_eval_confusion_generic(const float *__restrict__ logit, long long bstride, int K,
                                                                 int h, int w, const TL *__restrict__ label, int H, int W, float sh,
                                                                 float sw, long long ignore, unsigned *__restrict__ part,
                                                                 long long *__restrict__ pred_out)
{
    extern __shared__ unsigned hist_dyn[];
    clear_hist(hist_dyn, 3 * K);
    const int b = blockIdx.y;
    const int hw = H * W;
    const long long hwl = (long long)h * w;
#pragma unroll 1
    for (int it = 0; it < EV_ITERS; ++it) {
        const int i_raw = (blockIdx.x * EV_ITERS + it) * ETPB + threadIdx.x;
        const bool in = i_raw < hw;
        const int i = in ? i_raw : hw - 1;
        const int y = i / W, x = i - y * W;
        const Taps<float> ty = make_taps<float>(y, sh, h);
        Taps<float> tx[VIEWS];
        const float *base[VIEWS];
        float m[VIEWS], s[VIEWS];
#pragma unroll
        for (int v = 0; v < VIEWS; ++v) {
            tx[v] = make_taps<float>(v == 0 ? x : W - 1 - x, sw, w);
            base[v] = logit + (size_t)(VIEWS * b + v) * bstride;
        }
        auto interp = [&](int v, int c) {
            const float *pl = base[v] + (size_t)c * hwl;
            return bilerp<float>(pl[ty.i0 * w + tx[v].i0], pl[ty.i0 * w + tx[v].i1], pl[ty.i1 * w + tx[v].i0], pl[ty.i1 * w + tx[v].i1],
                                 tx[v].l0, tx[v].l1, ty.l0, ty.l1);
        };
#pragma unroll
        for (int v = 0; v < VIEWS; ++v) {
            float mv = interp(v, 0);
#pragma unroll 1
            for (int c = 1; c < K; ++c) { const float q = interp(v, c); mv = q > mv ? q : mv; }
            float sv = 0.0f;
#pragma unroll 1
            for (int c = 0; c < K; ++c) sv = sv + det_expf(interp(v, c) - mv);
            m[v] = mv;
            s[v] = sv;
        }
        float best = 0.0f;
        int am = 0;
        bool stop = false;
#pragma unroll 1
        for (int c = 0; c < K; ++c) {
            float q = det_expf(interp(0, c) - m[0]) / s[0];
            if constexpr (VIEWS == 2) q = (q + det_expf(interp(VIEWS - 1, c) - m[VIEWS - 1]) / s[VIEWS - 1]) / 2.0f;
            const bool up = c == 0 || (!stop && !(q <= best));
            am = up ? c : am;
            best = up ? q : best;
            stop = stop || (up && q != q);
        }
        const long long t = load_nt(label + (size_t)b * hw + i);
        if (pred_out && in) __builtin_nontemporal_store((long long)am, pred_out + (size_t)b * hw + i);
        const int key = count_key(am, t, ignore, K);
        wave_count(key, in && key != key_none(K), K, hist_dyn);
    }
    store_hist(hist_dyn, 3 * K, part);
}

// Counting only, for a prediction map that already exists (the drop-in for intersectionAndUnionGPU).
template <typename TP, typename TL>
__global__ void __launch_bounds__(ETPB) k_confusion_from_pred(const TP *__restrict__ pred, const TL *__restrict__ label, int K, int hw,
                                                              long long ignore, unsigned *__restrict__ part)
{
    extern __shared__ unsigned hist_dyn[];
    clear_hist(hist_dyn, 3 * K);
    const int b = blockIdx.y;
#pragma unroll 1
    for (int it = 0; it < EV_ITERS; ++it) {
        const int i_raw = (blockIdx.x * EV_ITERS + it) * ETPB + threadIdx.x;
        const bool in = i_raw < hw;
        const int i = in ? i_raw : hw - 1;
        const long long pv = load_nt(pred + (size_t)b * hw + i);
        const long long t = load_nt(label + (size_t)b * hw + i);
        const int key = count_key(pv, t, ignore, K);       // a prediction outside [0, K) counts as output nowhere, as in histc
        wave_count(key, in && key != key_none(K), K, hist_dyn);
    }
    store_hist(hist_dyn, 3 * K, part);
}

// partials (B, nblk, [I | O | T] x K) u32 -> counts (B, 3, K) i64 += [I, O + T - I, T].  One block per (class, image).
__global__ void __launch_bounds__(ETPB) k_confusion_finalize(const unsigned *__restrict__ part, int nblk, int K, long long *__restrict__ counts)
{
    const int c = blockIdx.x, b = blockIdx.y;
    unsigned long long I = 0, O = 0, T = 0;
    for (int j = threadIdx.x; j < nblk; j += ETPB) {
        const unsigned *p = part + ((size_t)b * nblk + j) * 3 * K;
        I += p[c];
        O += p[K + c];
        T += p[2 * K + c];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        I += __shfl_xor(I, off);
        O += __shfl_xor(O, off);
        T += __shfl_xor(T, off);
    }
    __shared__ unsigned long long s[3][ETPB / 64];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { s[0][wave] = I; s[1][wave] = O; s[2][wave] = T; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int q = 1; q < ETPB / 64; ++q) { I += s[0][q]; O += s[1][q]; T += s[2][q]; }
        long long *dst = counts + (size_t)b * 3 * K;
        dst[c] += (long long)I;
        dst[K + c] += (long long)(O + T - I);
        dst[2 * K + c] += (long long)T;
    }
}

// ---------------------------------------------------------------- host side
static int eval_blocks(int64_t H, int64_t W) { return (int)cdiv(H * W, EV_PX); }

static int check_dims(const char *who, int64_t K, int64_t H, int64_t W, int64_t B)
{
    if (K < 1 || H < 1 || W < 1 || B < 1) return fail(HALO_E_ARG, "%s: empty shape (K=%lld, H=%lld, W=%lld, B=%lld)", who, (long long)K,
                                                      (long long)H, (long long)W, (long long)B);
    if (K > EV_MAX_K) return fail(HALO_E_UNSUPPORTED, "%s: %lld classes (at most %d)", who, (long long)K, EV_MAX_K);
    // pixel indices of the last block stay in int
    if (H * W > 0x7fffffffLL - EV_PX || B > 65535) return fail(HALO_E_UNSUPPORTED, "%s: image of %lld pixels x %lld images", who, (long long)(H * W), (long long)B);
    return HALO_OK;
}

static bool label_code_ok(int code) { return code == HALO_I64 || code == HALO_I32 || code == HALO_U8; }

template <int K_T, int VIEWS>
static void launch_fused(dim3 grid, hipStream_t st, const float *logit, long long bstride, int h, int w, const void *label, int label_dtype,
                         int H, int W, float sh, float sw, long long ignore, unsigned *part, long long *pred)
{
    if (label_dtype == HALO_I64)
        hipLaunchKernelGGL((k_eval_confusion<K_T, VIEWS, int64_t>), grid, dim3(ETPB), 0, st, logit, bstride, h, w, (const int64_t *)label, H, W, sh, sw, ignore, part, pred);
    else if (label_dtype == HALO_I32)
        hipLaunchKernelGGL((k_eval_confusion<K_T, VIEWS, int32_t>), grid, dim3(ETPB), 0, st, logit, bstride, h, w, (const int32_t *)label, H, W, sh, sw, ignore, part, pred);
    else
        hipLaunchKernelGGL((k_eval_confusion<K_T, VIEWS, uint8_t>), grid, dim3(ETPB), 0, st, logit, bstride, h, w, (const uint8_t *)label, H, W, sh, sw, ignore, part, pred);
}

template <int VIEWS>
static void launch_generic(dim3 grid, hipStream_t st, const float *logit, long long bstride, int K, int h, int w, const void *label,
                           int label_dtype, int H, int W, float sh, float sw, long long ignore, unsigned *part, long long *pred)
{
    const size_t lds = (size_t)3 * K * sizeof(unsigned);
    if (label_dtype == HALO_I64)
        hipLaunchKernelGGL((k_eval_confusion_generic<VIEWS, int64_t>), grid, dim3(ETPB), lds, st, logit, bstride, K, h, w, (const int64_t *)label, H, W, sh, sw, ignore, part, pred);
    else if (label_dtype == HALO_I32)
        hipLaunchKernelGGL((k_eval_confusion_generic<VIEWS, int32_t>), grid, dim3(ETPB), lds, st, logit, bstride, K, h, w, (const int32_t *)label, H, W, sh, sw, ignore, part, pred);
    else
        hipLaunchKernelGGL((k_eval_confusion_generic<VIEWS, uint8_t>), grid, dim3(ETPB), lds, st, logit, bstride, K, h, w, (const uint8_t *)label, H, W, sh, sw, ignore, part, pred);
}

template <typename TP>
static void launch_from_pred(dim3 grid, size_t lds, hipStream_t st, const TP *pred, const void *label, int label_dtype, int K, int hw,
                             long long ignore, unsigned *part)
{
    if (label_dtype == HALO_I64)
        hipLaunchKernelGGL((k_confusion_from_pred<TP, int64_t>), grid, dim3(ETPB), lds, st, pred, (const int64_t *)label, K, hw, ignore, part);
    else if (label_dtype == HALO_I32)
        hipLaunchKernelGGL((k_confusion_from_pred<TP, int32_t>), grid, dim3(ETPB), lds, st, pred, (const int32_t *)label, K, hw, ignore, part);
    else
        hipLaunchKernelGGL((k_confusion_from_pred<TP, uint8_t>), grid, dim3(ETPB), lds, st, pred, (const uint8_t *)label, K, hw, ignore, part);
}

}  // namespace halo

using namespace halo;

extern "C" size_t halo_eval_workspace_bytes(int64_t B, int64_t K, int64_t H, int64_t W)
{
    if (B < 1 || K < 1 || H < 1 || W < 1) return 0;
    return (size_t)B * eval_blocks(H, W) * 3 * K * sizeof(unsigned) + 256;
}

extern "C" int halo_eval_confusion(const float *logit, int64_t logit_bstride, int views, int64_t K, int64_t h, int64_t w, const void *label,
                                   int label_dtype, int64_t H, int64_t W, int64_t B, int64_t ignore_index, int64_t *counts, int64_t *pred,
                                   void *workspace, size_t workspace_bytes, void *stream)
{
    const char *who = "halo_eval_confusion";
    if (!logit || !label || !counts) return fail(HALO_E_ARG, "%s: null argument", who);
    if (int rc = check_dims(who, K, H, W, B)) return rc;
    if (views != 1 && views != 2) return fail(HALO_E_UNSUPPORTED, "%s: %d views (1 or 2)", who, views);
    if (!label_code_ok(label_dtype)) return fail(HALO_E_UNSUPPORTED, "%s: label dtype code %d (int64, int32 or uint8)", who, label_dtype);
    if (h < 1 || w < 1 || logit_bstride < K * h * w || h * w * 4 > 0xffffffffLL)
        return fail(HALO_E_ARG, "%s: logit planes %lld x %lld with batch stride %lld for %lld classes", who, (long long)h, (long long)w,
                    (long long)logit_bstride, (long long)K);
    const size_t need = halo_eval_workspace_bytes(B, K, H, W);
    if (!workspace || workspace_bytes < need) return fail(HALO_E_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, need);
    unsigned *part = (unsigned *)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
    hipStream_t st = (hipStream_t)stream;
    const int nblk = eval_blocks(H, W);
    const dim3 grid((unsigned)nblk, (unsigned)B);
    // F.interpolate(align_corners=True): the source step of one output step, in float32 (as k_logit_maps_lr)
    const float sh = H > 1 ? (float)(h - 1) / (float)(H - 1) : 0.0f, sw = W > 1 ? (float)(w - 1) / (float)(W - 1) : 0.0f;
    const long long bs = (long long)logit_bstride, ig = (long long)ignore_index;
    long long *pr = (long long *)pred;
    if (K == 19 && views == 2) launch_fused<19, 2>(grid, st, logit, bs, (int)h, (int)w, label, label_dtype, (int)H, (int)W, sh, sw, ig, part, pr);
    else if (K == 19) launch_fused<19, 1>(grid, st, logit, bs, (int)h, (int)w, label, label_dtype, (int)H, (int)W, sh, sw, ig, part, pr);
    else if (K == 16 && views == 2) launch_fused<16, 2>(grid, st, logit, bs, (int)h, (int)w, label, label_dtype, (int)H, (int)W, sh, sw, ig, part, pr);
    else if (K == 16) launch_fused<16, 1>(grid, st, logit, bs, (int)h, (int)w, label, label_dtype, (int)H, (int)W, sh, sw, ig, part, pr);
    else {
        if (views == 2) launch_generic<2>(grid, st, logit, bs, (int)K, (int)h, (int)w, label, label_dtype, (int)H, (int)W, sh, sw, ig, part, pr);
        else launch_generic<1>(grid, st, logit, bs, (int)K, (int)h, (int)w, label, label_dtype, (int)H, (int)W, sh, sw, ig, part, pr);
    }
    hipLaunchKernelGGL(k_confusion_finalize, dim3((unsigned)K, (unsigned)B), dim3(ETPB), 0, st, (const unsigned *)part, nblk, (int)K, (long long *)counts);
    return check_launch(who);
}

extern "C" int halo_confusion_from_pred(const void *pred, int pred_dtype, const void *label, int label_dtype, int64_t K, int64_t H, int64_t W,
                                        int64_t B, int64_t ignore_index, int64_t *counts, void *workspace, size_t workspace_bytes, void *stream)
{
    const char *who = "halo_confusion_from_pred";
    if (!pred || !label || !counts) return fail(HALO_E_ARG, "%s: null argument", who);
    if (int rc = check_dims(who, K, H, W, B)) return rc;
    if (!label_code_ok(pred_dtype) || !label_code_ok(label_dtype))
        return fail(HALO_E_UNSUPPORTED, "%s: dtype codes %d / %d (int64, int32 or uint8)", who, pred_dtype, label_dtype);
    const size_t need = halo_eval_workspace_bytes(B, K, H, W);
    if (!workspace || workspace_bytes < need) return fail(HALO_E_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, need);
    unsigned *part = (unsigned *)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
    hipStream_t st = (hipStream_t)stream;
    const int nblk = eval_blocks(H, W);
    const dim3 grid((unsigned)nblk, (unsigned)B);
    const size_t lds = (size_t)3 * K * sizeof(unsigned);
    const int hw = (int)(H * W);
    if (pred_dtype == HALO_I64) launch_from_pred<int64_t>(grid, lds, st, (const int64_t *)pred, label, label_dtype, (int)K, hw, ignore_index, part);
    else if (pred_dtype == HALO_I32) launch_from_pred<int32_t>(grid, lds, st, (const int32_t *)pred, label, label_dtype, (int)K, hw, ignore_index, part);
    else launch_from_pred<uint8_t>(grid, lds, st, (const uint8_t *)pred, label, label_dtype, (int)K, hw, ignore_index, part);
    hipLaunchKernelGGL(k_confusion_finalize, dim3((unsigned)K, (unsigned)B), dim3(ETPB), 0, st, (const unsigned *)part, nblk, (int)K, (long long *)counts);
    return check_launch(who);
}
