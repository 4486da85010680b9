// Device bodies of the forward-process sample and the mask blend, shared by qsample.hip (mdx_q_sample_f32,
// mdx_vae_encode_noised_f32) and rng.hip (mdx_slot_blend_f32): every entry that promises the bits of another runs these.
#pragma once

#include "mdx_common.h"

// The q-sample statement, shared by every entry: one explicit fma, so all compile to the same two instructions whatever
// surrounds them (mdx_vae_encode_noised_f32's xt_out is bit for bit mdx_q_sample_f32 of its z0_out).  a = 1, b = 0 returns x0.
__device__ __forceinline__ float q_sample_f(float x0, float n, float a, float b) { return __builtin_fmaf(a, x0, b * n); }

// m q + (1 - m) img: m == 0 returns img and m == 1 returns q, bit for bit (finite q / img)
__device__ __forceinline__ float blend_f(float m, float q, float img) { return __builtin_fmaf(m, q, (1.0f - m) * img); }

template <int V>
__device__ __forceinline__ void load_v(const float* p, float (&v)[V]) {
    if constexpr (V == 4) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(p);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
        v[0] = *p;
    }
}

template <int V>
__device__ __forceinline__ void store_v(float* p, const float (&v)[V]) {
    if constexpr (V == 4) {
        f32x4 t;
        t.x = v[0]; t.y = v[1]; t.z = v[2]; t.w = v[3];
        *reinterpret_cast<f32x4*>(p) = t;
    } else {
        *p = v[0];
    }
}
