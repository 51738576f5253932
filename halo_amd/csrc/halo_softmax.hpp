// Per-pixel numerics shared by the scoring path (halo_score.hip) and the validation metric (halo_eval.hip): ATen's bilinear taps
// (align_corners=True) and ATen's softmax over the classes of a pixel held in registers.  One statement of each, so that the two
// translation units cannot drift apart; halo_score.hip's header comment on "logits -> entropy / prediction" explains the two
// softmax statements and when the lean one applies.
#pragma once
#include "halo_devmath.hpp"

namespace halo {

// bilinear taps of one output coordinate, weights in the tensor's dtype (align_corners=True)
template <typename T> struct Taps { int i0, i1; T l0, l1; };
template <typename T>
__device__ __forceinline__ Taps<T> make_taps(int o, T scale, int in_size)
{
    Taps<T> t;
    const T f = scale * (T)o;
    int i0 = (int)f;
    i0 = i0 > in_size - 1 ? in_size - 1 : i0;
    t.i0 = i0;
    t.i1 = i0 + (i0 < in_size - 1 ? 1 : 0);
    t.l1 = f - (T)i0;
    t.l0 = (T)1 - t.l1;
    return t;
}

__device__ __forceinline__ float vmax3(float a, float b, float c) { float r; asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r; }
__device__ __forceinline__ float vmin3(float a, float b, float c) { float r; asm("v_min3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r; }

// Lean softmax of NP pixels in registers.  Returns false -- p untouched -- when some lane of the wave needs the general
// statement.  NaN logits hide from the two running extrema (a comparison with NaN is false), hence the sum t: it is NaN
// iff a NaN (or both infinities) is among the classes; infinite logits make lo - m infinite or NaN.
template <int O_T, int NP>
__device__ __forceinline__ bool softmax_lean(float (&p)[NP][O_T])
{
    float m[NP], lo[NP], t[NP];
#pragma unroll
    for (int j = 0; j < NP; ++j) m[j] = lo[j] = t[j] = p[j][0];
    // the two extrema through v_max3_f32 / v_min3_f32, two classes per instruction (a compare + select pair per class and
    // extremum before: four 4-cycle instructions per class, now one).  They differ from the `>` / `<` scan only where it does
    // not matter: a NaN operand is skipped (t is NaN then and the wave takes the general statement) and max(-0, +0) is +0
    // (x - m is then +-0 either way and exp(+-0) = 1).
#pragma unroll
    for (int c = 1; c + 1 < O_T; c += 2) {
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            m[j] = vmax3(m[j], p[j][c], p[j][c + 1]);
            lo[j] = vmin3(lo[j], p[j][c], p[j][c + 1]);
            t[j] = (t[j] + p[j][c]) + p[j][c + 1];
        }
    }
    if constexpr ((O_T - 1) % 2 == 1) {
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            m[j] = vmax3(m[j], p[j][O_T - 1], p[j][O_T - 1]);
            lo[j] = vmin3(lo[j], p[j][O_T - 1], p[j][O_T - 1]);
            t[j] = t[j] + p[j][O_T - 1];
        }
    }
    bool general = false;
#pragma unroll
    for (int j = 0; j < NP; ++j) general = general || !(lo[j] - m[j] >= -64.0f) || t[j] != t[j];
    if (__any(general)) return false;
    float s[NP], r[NP];
#pragma unroll
    for (int j = 0; j < NP; ++j) s[j] = 0.0f;
#pragma unroll
    for (int c = 0; c < O_T; ++c) {
#pragma unroll
        for (int j = 0; j < NP; ++j) { p[j][c] = det_expf_core_small(p[j][c] - m[j]); s[j] = s[j] + p[j][c]; }
    }
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        r[j] = __builtin_amdgcn_rcpf(s[j]);
        r[j] = __builtin_fmaf(__builtin_fmaf(-s[j], r[j], 1.0f), r[j], r[j]);
    }
#pragma unroll
    for (int c = 0; c < O_T; ++c) {
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            float q = p[j][c] * r[j];
            q = __builtin_fmaf(__builtin_fmaf(-s[j], q, p[j][c]), r[j], q);
            p[j][c] = __builtin_fmaf(__builtin_fmaf(-s[j], q, p[j][c]), r[j], q);
        }
    }
    return true;
}

// General softmax in registers, for logits that exist nowhere in memory (the fused low-resolution path).
template <int O_T, int NP>
__device__ __forceinline__ void softmax_general(float (&p)[NP][O_T])
{
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        float m = p[j][0], s = 0.0f;
#pragma unroll
        for (int c = 1; c < O_T; ++c) m = p[j][c] > m ? p[j][c] : m;
#pragma unroll
        for (int c = 0; c < O_T; ++c) { p[j][c] = det_expf(p[j][c] - m); s = s + p[j][c]; }
#pragma unroll
        for (int c = 0; c < O_T; ++c) p[j][c] = p[j][c] / s;
    }
}

}  // namespace halo
