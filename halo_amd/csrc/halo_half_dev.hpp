// The half operands of the autocast passes (halo_norm_autocast.hip, the typed depthwise kernels of halo_dwconv.hip) on the device:
// the 16 bits of a float16 or a bfloat16, their exact widening, and the round-to-nearest-even conversions back.
#pragma once
#include "halo_common.hpp"
#include "halo_half_round.hpp"

namespace halo {

typedef unsigned short ac_half;                                  // the 16 bits of a float16 or a bfloat16; DT says which

template <int DT> __device__ __forceinline__ float ac_float(ac_half h)
{
    if constexpr (DT == HALO_F16) return (float)__builtin_bit_cast(_Float16, h);
    else return __builtin_bit_cast(float, (unsigned)h << 16);
}

typedef float ac_f2 __attribute__((ext_vector_type(2)));
typedef _Float16 ac_hh2 __attribute__((ext_vector_type(2)));
typedef unsigned short ac_h2 __attribute__((ext_vector_type(2)));

// round to nearest even; overflow gives +-inf; a NaN stays a NaN (quiet, sign kept).  Both in integer arithmetic
// (halo_half_round.hpp): written as `(_Float16)(a * b)` the conversion of one float is compiled into a multiply that converts its
// unrounded product (v_fma_mixlo_f16), one rounding where the torch chain has two.  The pairs of the wide route (ac_round_group)
// convert in hardware.
template <int DT> __device__ __forceinline__ ac_half ac_round(float f)
{
    if constexpr (DT == HALO_F16) return f16_round_bits(f);
    else return bf16_round_bits(f);
}

// a group's roundings: pairs for float16 (one conversion instruction per two elements)
template <int DT, int GW> __device__ __forceinline__ void ac_round_group(const float *f, ac_half *h)
{
    if constexpr (DT == HALO_F16 && GW % 2 == 0) {
#pragma unroll
        for (int e = 0; e < GW; e += 2) {
            const ac_f2 v = {f[e], f[e + 1]};
            const ac_h2 t = __builtin_bit_cast(ac_h2, __builtin_convertvector(v, ac_hh2));
            h[e] = t.x, h[e + 1] = t.y;
        }
    } else {
#pragma unroll
        for (int e = 0; e < GW; ++e) h[e] = ac_round<DT>(f[e]);
    }
}

}  // namespace halo
