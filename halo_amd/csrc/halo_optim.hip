// The optimiser step of one param group in one pass per launch: geoopt's RiemannianSGD on the Euclidean manifold (every parameter of
// the reference's models) and torch.optim.SGD, each with the bits of its stock chain of ATen kernels, in the parameter's dtype T
// (float32 or float64, mixed inside one group).  Scalars are cast to T once, as ATen casts a Python double.
//
//   HALO_SGD_GEOOPT  (geoopt/optim/rsgd.py, RiemannianSGD.step; egrad2rgrad = id, retr(x, u) = x + u, the buffer is transported as it is)
//     g1 = fma(wd, p, g)                                g.add_(p, alpha=wd): always, so wd = 0 with p = +-inf adds 0 * inf = NaN; stored to g
//     momentum > 0:  b0 = first ? g : buf               the clone of the RAW gradient, read where the buffer would be
//                    b1 = fma(1 - dampening, g1, fl(b0 * momentum))       buf.mul_(momentum).add_(g1, alpha=1 - dampening); stored to buf
//                    nesterov: g2 = fma(momentum, b1, g1), d = g2         g1.add_(buf, alpha=momentum): in place, g2 is what g keeps
//                    else:     d = b1
//     momentum <= 0: d = g1
//     p = fl(p + fl(-lr * d))                           two roundings: a multiply kernel, then an add kernel
//
//   HALO_SGD_TORCH  (torch/optim/sgd.py, maximize = False; its foreach and its single-tensor form run the same statements)
//     g1 = wd != 0 ? fma(wd, p, g) : g                  g.add(p, alpha=wd), not in place: g is never written
//     momentum != 0: b1 = first ? g1 : fma(1 - dampening, g1, fl(buf * momentum));  stored to buf
//                    d = nesterov ? fma(momentum, b1, g1) : b1
//     momentum == 0: d = g1
//     p = fma(-lr, d, p)                                p.add_(d, alpha=-lr): one rounding
//
// Every `a + alpha * b` of ATen's add kernels is one fma on the device (its functor is compiled with contraction on); the file is
// compiled with -ffp-contract=off and says fma where one is meant.  Denormals are kept.
//
// Layout: a workgroup of SGD_TPB lanes owns one chunk of SGD_CHUNK elements of one tensor.  The per-tensor table (pointers, element
// counts, first block of each tensor, flags) travels by value in the kernel arguments, SGD_CAP tensors per launch, so nothing has to
// outlive the call on a host that runs ahead; blockIdx -> (tensor, chunk) is a scalar binary search over the block prefix sums.
// A tensor whose three pointers are 16-byte aligned moves 16 bytes per lane and access, SGD_DEPTH accesses per array in flight; any
// other tensor moves one element per lane and access with the same statements.  Plain vector stores, no LDS, no atomics.
#include "halo_common.hpp"

namespace halo {

constexpr int SGD_TPB = 256;
constexpr int SGD_CHUNK = 4096;                // elements per workgroup, either dtype
constexpr int SGD_CAP = 96;                    // tensors per launch: the table below stays under the 4 KB of kernel arguments
constexpr int SGD_DEPTH = 4;                   // accesses per array a lane issues before the first use

constexpr unsigned SGD_F64 = 1, SGD_FIRST = 2, SGD_VEC = 4;          // SgdTable::flags

struct SgdTable {
    void *p[SGD_CAP];
    void *g[SGD_CAP];
    void *buf[SGD_CAP];
    int n[SGD_CAP];
    int start[SGD_CAP + 1];                    // first block of tensor i; start[count] = blocks of the launch
    unsigned char flags[SGD_CAP];
    int count;
};

struct SgdHyper {
    double neg_lr, momentum, one_minus_dampening, wd;
    int mode;                                  // HALO_SGD_*
    int use_momentum;                          // geoopt: momentum > 0; torch: momentum != 0
    int nesterov;
    int add_wd;                                // geoopt: always; torch: wd != 0
};

static_assert(sizeof(SgdTable) + sizeof(SgdHyper) <= 3584, "the table has to fit the kernel arguments");

template <typename T> struct SgdScalars { T neg_lr, momentum, omd, wd; };

// one element; g and b are updated to what the step leaves in p.grad and in the buffer
template <typename T, int MODE>
__device__ __forceinline__ void sgd_element(T &p, T &g, T &b, const SgdScalars<T> &s, bool first, bool use_momentum, bool nesterov, bool add_wd)
{
    if constexpr (MODE == HALO_SGD_GEOOPT) {
        T g1 = fma(s.wd, p, g);
        T d = g1;
        if (use_momentum) {
            const T b0 = first ? g : b;
            const T scaled = b0 * s.momentum;
            b = fma(s.omd, g1, scaled);
            d = b;
            if (nesterov) {
                g1 = fma(s.momentum, b, g1);
                d = g1;
            }
        }
        g = g1;
        const T u = s.neg_lr * d;
        p = p + u;
    } else {
        const T g1 = add_wd ? fma(s.wd, p, g) : g;
        T d = g1;
        if (use_momentum) {
            if (first) {
                b = g1;
            } else {
                const T scaled = b * s.momentum;
                b = fma(s.omd, g1, scaled);
            }
            d = nesterov ? fma(s.momentum, b, g1) : b;
        }
        p = fma(s.neg_lr, d, p);
    }
}

template <typename T> struct SgdVec;
template <> struct SgdVec<float> { typedef float4 type; };
template <> struct SgdVec<double> { typedef double2 type; };

// W elements per access: W = 16 / sizeof(T) on the aligned route (m a multiple of W here), W = 1 otherwise.  Items base .. base + m - 1
// of W elements each; a lane takes items tid, tid + TPB, ... SGD_DEPTH at a time.
template <typename T, int MODE, int W>
__device__ __forceinline__ void sgd_chunk(T *p, T *g, T *b, int items, const SgdScalars<T> &s, bool first, bool use_momentum, bool nesterov,
                                          bool add_wd)
{
    typedef typename SgdVec<T>::type V;
    const bool read_b = use_momentum && !first;                  // a first use reads no buffer (it may hold anything)
    const bool write_g = MODE == HALO_SGD_GEOOPT;
    for (int k0 = (int)threadIdx.x; k0 < items; k0 += SGD_TPB * SGD_DEPTH) {
        T vp[SGD_DEPTH][W], vg[SGD_DEPTH][W], vb[SGD_DEPTH][W];
#pragma unroll
        for (int j = 0; j < SGD_DEPTH; ++j) {
            const int k = k0 + j * SGD_TPB;
            if (k < items) {
                if constexpr (W == 1) {
                    vp[j][0] = p[k];
                    vg[j][0] = g[k];
                    vb[j][0] = read_b ? b[k] : T(0);
                } else {
                    *reinterpret_cast<V *>(vp[j]) = reinterpret_cast<const V *>(p)[k];
                    *reinterpret_cast<V *>(vg[j]) = reinterpret_cast<const V *>(g)[k];
                    if (read_b) *reinterpret_cast<V *>(vb[j]) = reinterpret_cast<const V *>(b)[k];
                    else
#pragma unroll
                        for (int e = 0; e < W; ++e) vb[j][e] = T(0);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < SGD_DEPTH; ++j) {
            const int k = k0 + j * SGD_TPB;
            if (k < items) {
#pragma unroll
                for (int e = 0; e < W; ++e) sgd_element<T, MODE>(vp[j][e], vg[j][e], vb[j][e], s, first, use_momentum, nesterov, add_wd);
                if constexpr (W == 1) {
                    p[k] = vp[j][0];
                    if (write_g) g[k] = vg[j][0];
                    if (use_momentum) b[k] = vb[j][0];
                } else {
                    reinterpret_cast<V *>(p)[k] = *reinterpret_cast<const V *>(vp[j]);
                    if (write_g) reinterpret_cast<V *>(g)[k] = *reinterpret_cast<const V *>(vg[j]);
                    if (use_momentum) reinterpret_cast<V *>(b)[k] = *reinterpret_cast<const V *>(vb[j]);
                }
            }
        }
    }
}

template <typename T, int MODE>
__device__ __forceinline__ void sgd_tensor_chunk(void *pp, void *gp, void *bp, int n, int chunk, unsigned flags, const SgdHyper &h)
{
    constexpr int W = 16 / (int)sizeof(T);
    SgdScalars<T> s;
    s.neg_lr = (T)h.neg_lr, s.momentum = (T)h.momentum, s.omd = (T)h.one_minus_dampening, s.wd = (T)h.wd;
    const bool first = (flags & SGD_FIRST) != 0, use_momentum = h.use_momentum != 0, nesterov = h.nesterov != 0, add_wd = h.add_wd != 0;
    const size_t base = (size_t)chunk * SGD_CHUNK;
    const int m = min(SGD_CHUNK, (int)((size_t)n - base));       // elements of this chunk, >= 1
    T *p = (T *)pp + base, *g = (T *)gp + base, *b = bp ? (T *)bp + base : nullptr;
    if (flags & SGD_VEC) {
        const int whole = m / W * W;                               // base is a multiple of W: the accesses stay 16-byte aligned
        sgd_chunk<T, MODE, W>(p, g, b, m / W, s, first, use_momentum, nesterov, add_wd);
        sgd_chunk<T, MODE, 1>(p + whole, g + whole, b ? b + whole : nullptr, m - whole, s, first, use_momentum, nesterov, add_wd);
    } else {
        sgd_chunk<T, MODE, 1>(p, g, b, m, s, first, use_momentum, nesterov, add_wd);
    }
}

template <int MODE>
__global__ void __launch_bounds__(SGD_TPB) k_sgd_step(SgdTable tab, SgdHyper h)
{
    // the tensor whose blocks hold this one: the last t with start[t] <= block (tensors of no blocks share a start and are passed over)
    const int block = (int)blockIdx.x;
    int lo = 0, hi = tab.count;                                  // start[lo] <= block < start[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (tab.start[mid] <= block) lo = mid;
        else hi = mid;
    }
    const int t = lo, chunk = block - tab.start[t];
    const unsigned flags = tab.flags[t];
    if (flags & SGD_F64) sgd_tensor_chunk<double, MODE>(tab.p[t], tab.g[t], tab.buf[t], tab.n[t], chunk, flags, h);
    else sgd_tensor_chunk<float, MODE>(tab.p[t], tab.g[t], tab.buf[t], tab.n[t], chunk, flags, h);
}

// The tensors of the launch that starts at tensor `next`: up to SGD_CAP tensors of at least one element, in order.  idx[j] is the
// j-th one's place in the caller's list, start[j] its first block, start[m] the launch's blocks.  Returns m and moves `next` on.
static int sgd_plan_launch(const int64_t *n, int64_t count, int64_t &next, int64_t *idx, int *start)
{
    int m = 0;
    int64_t blocks = 0;
    while (next < count && m < SGD_CAP) {
        if (n[next] > 0) {
            idx[m] = next;
            start[m] = (int)blocks;
            blocks += cdiv(n[next], SGD_CHUNK);                  // below 2^19 each: 96 of them stay far below 2^31
            ++m;
        }
        ++next;
    }
    start[m] = (int)blocks;
    return m;
}

static int sgd_check_sizes(const char *who, const int64_t *n, int64_t count)
{
    for (int64_t i = 0; i < count; ++i) {
        if (n[i] < 0) return fail(HALO_E_ARG, "%s: tensor %lld has %lld elements", who, (long long)i, (long long)n[i]);
        if (n[i] >= ((int64_t)1 << 31)) return fail(HALO_E_UNSUPPORTED, "%s: tensor %lld has %lld elements, 2^31 or more", who, (long long)i, (long long)n[i]);
    }
    return HALO_OK;
}

}  // namespace halo

using namespace halo;

extern "C" int halo_sgd_plan_limits(int64_t *chunk, int64_t *cap)
{
    if (!chunk || !cap) return fail(HALO_E_ARG, "halo_sgd_plan_limits: null argument");
    *chunk = SGD_CHUNK, *cap = SGD_CAP;
    return HALO_OK;
}

extern "C" int halo_sgd_plan(const int64_t *n, int64_t count, int64_t *launch_of, int64_t *first_block, int64_t *launches)
{
    const char *who = "halo_sgd_plan";
    if (count < 0 || (count > 0 && (!n || !launch_of || !first_block)) || !launches) return fail(HALO_E_ARG, "%s: null argument", who);
    if (int rc = sgd_check_sizes(who, n, count)) return rc;
    int64_t next = 0, made = 0, idx[SGD_CAP];
    int start[SGD_CAP + 1];
    for (int64_t i = 0; i < count; ++i) launch_of[i] = -1, first_block[i] = -1;
    while (next < count) {
        const int m = sgd_plan_launch(n, count, next, idx, start);
        if (m == 0) break;
        for (int j = 0; j < m; ++j) launch_of[idx[j]] = made, first_block[idx[j]] = start[j];
        ++made;
    }
    *launches = made;
    return HALO_OK;
}

extern "C" int halo_sgd_step(const halo_sgd_args *a, void *stream)
{
    const char *who = "halo_sgd_step";
    if (!a || a->struct_bytes != sizeof(halo_sgd_args)) return fail(HALO_E_ARG, "%s: descriptor missing or of another size", who);
    if (a->mode != HALO_SGD_GEOOPT && a->mode != HALO_SGD_TORCH) return fail(HALO_E_ARG, "%s: mode %d", who, a->mode);
    if (a->count < 0 || (a->count > 0 && !a->tensors)) return fail(HALO_E_ARG, "%s: %lld tensors without a list", who, (long long)a->count);
    SgdHyper h;
    h.neg_lr = -a->lr, h.momentum = a->momentum, h.one_minus_dampening = 1.0 - a->dampening, h.wd = a->weight_decay;
    h.mode = a->mode, h.nesterov = a->nesterov != 0;
    h.use_momentum = a->mode == HALO_SGD_GEOOPT ? a->momentum > 0 : a->momentum != 0;
    h.add_wd = a->mode == HALO_SGD_GEOOPT || a->weight_decay != 0;
    if (h.nesterov && !h.use_momentum) return fail(HALO_E_ARG, "%s: nesterov without momentum", who);
    // every check before the first launch
    for (int64_t i = 0; i < a->count; ++i) {
        const halo_sgd_tensor &t = a->tensors[i];
        if (t.n < 0) return fail(HALO_E_ARG, "%s: tensor %lld has %lld elements", who, (long long)i, (long long)t.n);
        if (t.n >= ((int64_t)1 << 31)) return fail(HALO_E_UNSUPPORTED, "%s: tensor %lld has %lld elements, 2^31 or more", who, (long long)i, (long long)t.n);
        if (t.dtype != HALO_F32 && t.dtype != HALO_F64) return fail(HALO_E_UNSUPPORTED, "%s: tensor %lld has dtype %d", who, (long long)i, t.dtype);
        if (t.n > 0 && (!t.p || !t.g || (h.use_momentum && !t.buf))) return fail(HALO_E_ARG, "%s: tensor %lld lacks a pointer", who, (long long)i);
    }
    int64_t next = 0, idx[SGD_CAP], n[SGD_CAP];
    while (next < a->count) {
        // sgd_plan_launch reads sizes from a plain list: the next SGD_CAP non-empty tensors are found on a window of it
        SgdTable tab;
        int m = 0;
        int64_t blocks = 0;
        while (next < a->count && m < SGD_CAP) {
            if (a->tensors[next].n > 0) idx[m] = next, n[m] = a->tensors[next].n, ++m;
            ++next;
        }
        if (m == 0) break;
        int64_t at = 0, where[SGD_CAP];
        const int got = sgd_plan_launch(n, m, at, where, tab.start);
        if (got != m) return fail(HALO_E_LAUNCH, "%s: plan of %d tensors for %d", who, got, m);
        blocks = tab.start[m];
        for (int j = 0; j < m; ++j) {
            const halo_sgd_tensor &t = a->tensors[idx[j]];
            void *buf = h.use_momentum ? t.buf : nullptr;
            tab.p[j] = t.p, tab.g[j] = t.g, tab.buf[j] = buf, tab.n[j] = (int)t.n;
            const bool vec = ((uintptr_t)t.p | (uintptr_t)t.g | (uintptr_t)buf) % 16 == 0;
            tab.flags[j] = (unsigned char)((t.dtype == HALO_F64 ? SGD_F64 : 0) | (t.first ? SGD_FIRST : 0) | (vec ? SGD_VEC : 0));
        }
        for (int j = m; j < SGD_CAP; ++j) tab.p[j] = tab.g[j] = tab.buf[j] = nullptr, tab.n[j] = 0, tab.flags[j] = 0, tab.start[j + 1] = (int)blocks;
        tab.count = m;
        const dim3 gd((unsigned)blocks), b(SGD_TPB);
        if (a->mode == HALO_SGD_GEOOPT) hipLaunchKernelGGL((k_sgd_step<HALO_SGD_GEOOPT>), gd, b, 0, (hipStream_t)stream, tab, h);
        else hipLaunchKernelGGL((k_sgd_step<HALO_SGD_TORCH>), gd, b, 0, (hipStream_t)stream, tab, h);
        if (int rc = check_launch(who)) return rc;
    }
    return HALO_OK;
}
