// Device functions shared by the frozen-norm passes (halo_norm.hip, halo_maxpool.hip): the 16-byte / one-element group access and
// the statements of a frozen norm and of the ReLU behind it, each rounding on its own.
#pragma once

namespace halo {

typedef float an_f4 __attribute__((ext_vector_type(4)));

template <int GW> __device__ __forceinline__ void an_load(const float *p, float *v)
{
    if constexpr (GW == 4) {
        const an_f4 t = *reinterpret_cast<const an_f4 *>(p);
        v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
    } else {
        v[0] = *p;
    }
}

template <int GW> __device__ __forceinline__ void an_store(float *p, const float *v)
{
    if constexpr (GW == 4) {
        an_f4 t;
        t.x = v[0], t.y = v[1], t.z = v[2], t.w = v[3];
        *reinterpret_cast<an_f4 *>(p) = t;
    } else {
        *p = v[0];
    }
}

// fl(fl(x * sc) + sh): the frozen norm's two statements, never an fma (the build sets -ffp-contract=off)
__device__ __forceinline__ float an_affine(float x, float sc, float sh)
{
    float s = x * sc;
    s = s + sh;
    return s;
}

// the ReLU of every pass: a NaN stays a NaN, everything else that is not positive becomes +0
__device__ __forceinline__ float an_relu(float s) { return s <= 0.0f ? 0.0f : s; }

}  // namespace halo
