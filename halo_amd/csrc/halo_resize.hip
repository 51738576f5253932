// Backward of the align_corners=True bilinear resize (halo_bilinear_upsample, halo_hyperbolic.hip): the adjoint as a GATHER.
//
//   grad_in[p, i, j] = sum_Y sum_X  wy(Y, i) * wx(X, j) * grad_out[p, Y, X]
//   wy(Y, i) = [t.i0 == i] t.l0 + [t.i1 == i] t.l1,  t = make_taps<T>(Y, sh, h)  (halo_softmax.hpp; the forward's sh, sw)
//
// ATen's device backward scatters four float atomic adds per grad_out element; here every grad_in element is written once, by
// one thread.  make_taps(o).i0 is monotone in o, so the grad_out rows whose taps reach the cell rows [i - 1, i] are ONE range
// [first_at_least(i - 1), first_at_least(i + 1)), and the same along x (the idea of k_upl_bwd, halo_train_loss.hip).
//
// Order of summation (both kernels below, whatever the tiling -- so the bits depend on the operands and the shape alone):
//   r(Y)  = fma(wx(X, j), g[Y, X], r) over the cell's columns X in ascending order, starting from 0, in the operand dtype;
//   grad  = fma(wy(Y, i), r(Y), grad) over the cell's rows Y in ascending order, starting from 0.
// No atomics, no cross-thread reduction of one element.
//
// k_bilinear_bwd_tiled: a block owns RB_TI x RB_TJ cells of one plane.  The grad_out rows of its footprint are staged in LDS
// once (coalesced 16-byte non-temporal loads: grad_out is read once, apart from the one-cell halo two neighbouring blocks
// share), in chunks of `rc` rows so that any magnification fits; stage A turns a chunk into row sums r(Y) per cell column
// (weights from a per-block table, one LDS read each), stage B adds the chunk's rows into the cells.  A chunk boundary does not
// change the order above.
// k_bilinear_bwd_cell: one thread per cell straight from global memory, 64-bit indexing -- every shape the tiled kernel's LDS
// budget or int range does not serve (a single source column under a very wide output, planes * h * w beyond 2^31, ...).
#include "halo_common.hpp"
#include "halo_devmath.hpp"
#include "halo_softmax.hpp"

namespace halo {

constexpr int RB_TPB = 256;
constexpr int RB_TJ = 32, RB_TI = RB_TPB / RB_TJ;      // cells per block: 8 rows x 32 columns
constexpr int RB_TILE_BYTES = 24 * 1024;                // staged grad_out rows of one chunk
constexpr int RB_LDS_BYTES = 48 * 1024;                 // all three LDS arrays; more -> k_bilinear_bwd_cell
constexpr int RB_ST = 4;                                // staging loads in flight per thread
constexpr int RB_MAX_DIM = 1 << 20;                     // tiled kernel: float32 holds every coordinate exactly (the LDS bounds rely on it)

typedef float rb_f4 __attribute__((ext_vector_type(4)));
typedef double rb_d2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float rb_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double rb_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }

// make_taps(o).i0, and the smallest output coordinate in [0, n_out] whose i0 is >= i (n_out when there is none)
template <typename T>
__host__ __device__ __forceinline__ int rb_tap0(int o, T scale, int n_in)
{
    const int i0 = (int)(scale * (T)o);
    return i0 > n_in - 1 ? n_in - 1 : i0;
}
template <typename T>
__host__ __device__ __forceinline__ int rb_first_at_least(int i, T scale, int n_in, int n_out)
{
    if (i <= 0) return 0;
    const T est = scale > (T)0 ? (T)i / scale : (T)n_out;
    int o = est >= (T)n_out ? n_out : (int)est;
    o = o < 0 ? 0 : o;
    while (o > 0 && rb_tap0<T>(o - 1, scale, n_in) >= i) --o;
    while (o < n_out && rb_tap0<T>(o, scale, n_in) < i) ++o;
    return o;
}

// weight of input cell i in output coordinate o (both taps count where they coincide at the border)
template <typename T>
__device__ __forceinline__ T rb_weight(int o, T scale, int n_in, int i)
{
    const Taps<T> t = make_taps<T>(o, scale, n_in);
    return (t.i0 == i ? t.l0 : (T)0) + (t.i1 == i ? t.l1 : (T)0);
}

template <typename T, int VEC> struct RbVec;
template <> struct RbVec<float, 4> { typedef rb_f4 type; };
template <> struct RbVec<double, 2> { typedef rb_d2 type; };
template <> struct RbVec<float, 1> { typedef float type; };
template <> struct RbVec<double, 1> { typedef double type; };

// span: staged columns per row (>= every block's footprint, a multiple of VEC); kmax: grad_out columns per cell at most;
// rc: rows per chunk.  LDS: tile [rc][span] | rsum [rc][RB_TJ] | wtab [kmax][RB_TJ].  VEC > 1 requires W % VEC == 0 and a
// 16-byte aligned grad_out (every staged row segment then starts on a 16-byte boundary).
template <typename T, int VEC>
__global__ void __launch_bounds__(RB_TPB) k_bilinear_bwd_tiled(const T *__restrict__ go, T *__restrict__ gi, long long nwork, int h, int w,
                                                               int H, int W, T sh, T sw, int tiles_x, int tiles_y, int span, int kmax, int rc)
{
    typedef typename RbVec<T, VEC>::type VT;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_rb[];
    T *tile = reinterpret_cast<T *>(smem_rb);
    T *rsum = tile + (size_t)rc * span;
    T *wtab = rsum + (size_t)rc * RB_TJ;
    const int tid = threadIdx.x, jl = tid % RB_TJ, il = tid / RB_TJ;
    const int tiles = tiles_x * tiles_y;
    for (long long wk = blockIdx.x; wk < nwork; wk += gridDim.x) {
        const long long p = wk / tiles;
        const int t = (int)(wk - p * tiles);
        const int i0 = (t / tiles_x) * RB_TI, j0 = (t % tiles_x) * RB_TJ;
        // cells outside the plane compute the last cell again and store nothing
        const int ic = i0 + il < h ? i0 + il : h - 1, jc = j0 + jl < w ? j0 + jl : w - 1;
        const int ilast = (i0 + RB_TI < h ? i0 + RB_TI : h) - 1, jlast = (j0 + RB_TJ < w ? j0 + RB_TJ : w) - 1;
        const int xa = rb_first_at_least<T>(jc - 1, sw, w, W), ya = rb_first_at_least<T>(ic - 1, sh, h, H);
        const int yb = rb_first_at_least<T>(ic + 1, sh, h, H);
        int n = rb_first_at_least<T>(jc + 1, sw, w, W) - xa;
        n = n < kmax ? n : kmax;                                   // (never cuts: the host's kmax bounds it; LDS indices stay inside whatever happens)
        const int Ya = rb_first_at_least<T>(i0 - 1, sh, h, H), Yb = rb_first_at_least<T>(ilast + 1, sh, h, H);
        int Xa = rb_first_at_least<T>(j0 - 1, sw, w, W), Xb = rb_first_at_least<T>(jlast + 1, sw, w, W);
        Xa = Xa / VEC * VEC;
        Xb = (Xb + VEC - 1) / VEC * VEC;                           // <= W: W % VEC == 0
        int ncol = Xb - Xa;
        ncol = ncol < span ? ncol : span;                          // (never cuts, as above)
        const int xo = xa - Xa < span - n ? xa - Xa : span - n;    // (never cuts)
        for (int k = il; k < n; k += RB_TI) wtab[k * RB_TJ + jl] = rb_weight<T>(xa + k, sw, w, jc);
        const T *gp = go + (size_t)p * H * W;
        const int nv = ncol / VEC;
        T acc = (T)0;
        for (int yc = Ya; yc < Yb; yc += rc) {
            const int nr = Yb - yc < rc ? Yb - yc : rc;
            // stage the chunk: RB_ST loads per thread first, addresses clamped instead of the loads predicated, then the LDS stores
            const int total = nr * nv;
            for (int e0 = tid; e0 < total; e0 += RB_TPB * RB_ST) {
                VT reg[RB_ST];
#pragma unroll
                for (int u = 0; u < RB_ST; ++u) {
                    int e = e0 + u * RB_TPB;
                    e = e < total ? e : total - 1;
                    const int r = e / nv, c = e - r * nv;
                    reg[u] = __builtin_nontemporal_load(reinterpret_cast<const VT *>(gp + (size_t)(yc + r) * W + Xa + c * VEC));
                }
#pragma unroll
                for (int u = 0; u < RB_ST; ++u) {
                    const int e = e0 + u * RB_TPB;
                    if (e < total) {
                        const int r = e / nv, c = e - r * nv;
                        *reinterpret_cast<VT *>(tile + r * span + c * VEC) = reg[u];
                    }
                }
            }
            __syncthreads();
            // A: row sums of this thread's cell column, ascending X
            for (int r = il; r < nr; r += RB_TI) {
                const T *row = tile + r * span + xo;
                T s = (T)0;
                for (int k = 0; k < n; ++k) s = rb_fma(wtab[k * RB_TJ + jl], row[k], s);
                rsum[r * RB_TJ + jl] = s;
            }
            __syncthreads();
            // B: the chunk's rows of this thread's cell, ascending Y.  (The next chunk's staging writes `tile` only, and its
            // stage A -- which writes rsum -- lies behind the barrier every thread reaches after this loop.)
            const int ylo = ya > yc ? ya : yc, yhi = yb < yc + nr ? yb : yc + nr;
            for (int Y = ylo; Y < yhi; ++Y) acc = rb_fma(rb_weight<T>(Y, sh, h, ic), rsum[(Y - yc) * RB_TJ + jl], acc);
        }
        if (i0 + il < h && j0 + jl < w) gi[((size_t)p * h + ic) * w + jc] = acc;
        __syncthreads();                                           // wtab and rsum are rewritten by the next work item
    }
}

template <typename T>
__global__ void __launch_bounds__(RB_TPB) k_bilinear_bwd_cell(const T *__restrict__ go, T *__restrict__ gi, long long n_in, int h, int w,
                                                              int H, int W, T sh, T sw)
{
    const long long hw = (long long)h * w;
    for (long long e = (long long)blockIdx.x * RB_TPB + threadIdx.x; e < n_in; e += (long long)gridDim.x * RB_TPB) {
        const long long p = e / hw;
        const long long q = e - p * hw;
        const int i = (int)(q / w), j = (int)(q - (long long)i * w);
        const int ya = rb_first_at_least<T>(i - 1, sh, h, H), yb = rb_first_at_least<T>(i + 1, sh, h, H);
        const int xa = rb_first_at_least<T>(j - 1, sw, w, W), xb = rb_first_at_least<T>(j + 1, sw, w, W);
        const T *gp = go + (size_t)p * H * W;
        T acc = (T)0;
        for (int Y = ya; Y < yb; ++Y) {
            const T *row = gp + (size_t)Y * W;
            T s = (T)0;
            for (int X = xa; X < xb; ++X) s = rb_fma(rb_weight<T>(X, sw, w, j), row[X], s);
            acc = rb_fma(rb_weight<T>(Y, sh, h, i), s, acc);
        }
        gi[e] = acc;
    }
}

// the most output coordinates whose lower tap falls on `cells + 1` consecutive input cells: fl(scale * o) lies in an interval of
// width cells + 1 (+ the rounding of the product, far below the 0.001), coordinates exact in T up to RB_MAX_DIM
static int64_t rb_reach(double scale, int cells, int64_t n_out)
{
    if (!(scale > 0.0)) return n_out;
    const double r = ((double)cells + 1.001) / scale + 2.0;
    return r >= (double)n_out ? n_out : (int64_t)r;
}

template <typename T, int VEC>
static bool launch_bwd_tiled(const T *go, T *gi, int64_t planes, int64_t h, int64_t w, int64_t H, int64_t W, T sh, T sw, hipStream_t st)
{
    if (H > RB_MAX_DIM || W > RB_MAX_DIM) return false;
    const int64_t span = (rb_reach((double)sw, RB_TJ, W) + 2 * (VEC - 1) + VEC - 1) / VEC * VEC;
    const int64_t kmax = rb_reach((double)sw, 1, W);
    int64_t rc = RB_TILE_BYTES / (span * (int64_t)sizeof(T));
    const int64_t rows = rb_reach((double)sh, RB_TI, H);
    rc = rc > rows ? rows : rc;
    const int64_t lds = (rc * span + rc * RB_TJ + kmax * RB_TJ) * (int64_t)sizeof(T);
    if (rc < 4 && rc < rows) return false;
    if (rc < 1 || lds > RB_LDS_BYTES) return false;
    const int64_t tiles_x = cdiv(w, RB_TJ), tiles_y = cdiv(h, RB_TI);
    if (tiles_x * tiles_y > 0x7fffffffLL) return false;
    const int64_t nwork = planes * tiles_x * tiles_y;
    const unsigned grid = (unsigned)(nwork < (1 << 22) ? nwork : (1 << 22));
    hipLaunchKernelGGL((k_bilinear_bwd_tiled<T, VEC>), dim3(grid), dim3(RB_TPB), (size_t)lds, st, go, gi, (long long)nwork, (int)h, (int)w, (int)H,
                       (int)W, sh, sw, (int)tiles_x, (int)tiles_y, (int)span, (int)kmax, (int)rc);
    return true;
}

template <typename T>
static void launch_bwd(const void *grad_out, void *grad_in, int64_t planes, int64_t h, int64_t w, int64_t H, int64_t W, hipStream_t st)
{
    // the forward's scales (launch_bilinear_rows)
    const T sh = H > 1 ? (T)(h - 1) / (T)(H - 1) : (T)0, sw = W > 1 ? (T)(w - 1) / (T)(W - 1) : (T)0;
    const T *go = (const T *)grad_out;
    T *gi = (T *)grad_in;
    constexpr int V = 16 / (int)sizeof(T);
    const bool wide = W % V == 0 && ((uintptr_t)grad_out % 16) == 0;
    if (wide ? launch_bwd_tiled<T, V>(go, gi, planes, h, w, H, W, sh, sw, st) : launch_bwd_tiled<T, 1>(go, gi, planes, h, w, H, W, sh, sw, st)) return;
    const long long n = (long long)planes * h * w;
    const int64_t blocks = cdiv(n, RB_TPB);
    hipLaunchKernelGGL((k_bilinear_bwd_cell<T>), dim3((unsigned)(blocks < (1 << 22) ? blocks : (1 << 22))), dim3(RB_TPB), 0, st, go, gi, n, (int)h,
                       (int)w, (int)H, (int)W, sh, sw);
}

}  // namespace halo

using namespace halo;

extern "C" int halo_bilinear_upsample_bwd(const void *grad_out, void *grad_in, int dtype, int64_t planes, int64_t h, int64_t w, int64_t H,
                                          int64_t W, void *stream)
{
    const char *who = "halo_bilinear_upsample_bwd";
    if (!grad_out || !grad_in || planes <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0) return fail(HALO_E_ARG, "%s: null/empty argument", who);
    if (dtype != HALO_F64 && dtype != HALO_F32) return fail(HALO_E_ARG, "%s: bad dtype", who);
    if (H < h || W < w)
        return fail(HALO_E_ARG, "%s: output %lld x %lld is smaller than the input's %lld x %lld (the adjoint of an upsampling only)", who,
                    (long long)H, (long long)W, (long long)h, (long long)w);
    if (H > 0x7fffffffLL || W > 0x7fffffffLL || planes > (int64_t)1 << 40)
        return fail(HALO_E_ARG, "%s: %lld planes of %lld x %lld", who, (long long)planes, (long long)H, (long long)W);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == HALO_F64) launch_bwd<double>(grad_out, grad_in, planes, h, w, H, W, st);
    else launch_bwd<float>(grad_out, grad_in, planes, h, w, H, W, st);
    return check_launch(who);
}
