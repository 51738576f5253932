// float -> float16 / bfloat16 bits, round to nearest even, in integer arithmetic: plain C++ that compiles for the host as well
// (tests/test_norm_autocast_host.py builds it into a small program and holds it to numpy's and torch's conversions).
// halo_norm_autocast.hip rounds with these where the compiler would otherwise fuse a product into its conversion.
#pragma once

#if defined(__HIPCC__)
#define HALO_HD __host__ __device__ __forceinline__
#else
#define HALO_HD inline
#endif

namespace halo {

HALO_HD unsigned hr_bits(float f)
{
    unsigned u;
    __builtin_memcpy(&u, &f, 4);
    return u;
}

HALO_HD float hr_float(unsigned u)
{
    float f;
    __builtin_memcpy(&f, &u, 4);
    return f;
}

// float16: overflow gives +-inf (65520 and above), a NaN stays a NaN (quiet, sign kept), subnormal results are kept
HALO_HD unsigned short f16_round_bits(float f)
{
    const unsigned u = hr_bits(f);
    const unsigned sign = (u >> 16) & 0x8000u;
    unsigned a = u & 0x7fffffffu;
    if (a > 0x7f800000u) return (unsigned short)(sign | 0x7e00u);
    if (a >= 0x477ff000u) return (unsigned short)(sign | 0x7c00u);          // 65520 and above round to inf
    if (a < 0x38800000u) {                                                  // below 2^-14: a half subnormal or zero
        const float t = hr_float(a) + 0.5f;                                 // the float32 add rounds to multiples of 2^-24
        return (unsigned short)(sign | (hr_bits(t) - 0x3f000000u));
    }
    a -= 0x38000000u;                                                       // the exponent bias, 127 -> 15
    a += 0xfffu + ((a >> 13) & 1u);
    return (unsigned short)(sign | (a >> 13));
}

// bfloat16: float32's upper half; overflow gives +-inf by the carry, a NaN stays a NaN (quiet, sign kept)
HALO_HD unsigned short bf16_round_bits(float f)
{
    unsigned u = hr_bits(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)((u >> 16) | 0x0040u);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (unsigned short)(u >> 16);
}

}  // namespace halo
