// Device bodies of the per-sample seeded generator (include/mdx.h has the counter layout and the uniform mapping), shared by
// rng.hip (mdx_philox_u32, mdx_randn_f32, mdx_randn_slots_f32, mdx_slot_blend_f32) and resample.hip (mdx_resample_noised_f32):
// every entry that promises the bits of mdx_randn_f32 takes its values from quad_values alone.
// No fast-math flag and no fast intrinsic here: logf / sqrtf / sincospif are the precise ones.
#pragma once

#include <math.h>

#include "mdx_common.h"

constexpr unsigned PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u;
constexpr unsigned PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;
constexpr unsigned DROPOUT_STREAM_BIT = 0x80000000u;

struct Quad {
    unsigned w[4];
};

// Philox4x32-10 of counter (c0, c1, c2, 0) under key (k0, k1)
__device__ __forceinline__ Quad philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned k0, unsigned k1) {
    unsigned c3 = 0;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(PHILOX_M0, c0), lo0 = PHILOX_M0 * c0;
        const unsigned hi1 = __umulhi(PHILOX_M1, c2), lo1 = PHILOX_M1 * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += PHILOX_W0;
        k1 += PHILOX_W1;
    }
    Quad q;
    q.w[0] = c0; q.w[1] = c1; q.w[2] = c2; q.w[3] = c3;
    return q;
}

// word -> uniform in the open interval (0, 1): ((w >> 9) + 1/2) * 2^-23.  The conversion of a 23-bit integer and the fma are
// both exact, so the value is (2 (w >> 9) + 1) * 2^-24 in every arithmetic: 2^-24 <= u <= 1 - 2^-24.
__device__ __forceinline__ float uniform_open(unsigned w) {
    return __builtin_fmaf((float)(w >> 9), 0x1p-23f, 0x1p-24f);
}

// Box-Muller on one word pair: the cosine branch is the even element's, the sine branch the odd one's
__device__ __forceinline__ void box_muller(unsigned wa, unsigned wb, float& z_even, float& z_odd) {
    const float r = sqrtf(-2.0f * logf(uniform_open(wa)));
    float s, c;
    sincospif(2.0f * uniform_open(wb), &s, &c);
    z_even = r * c;
    z_odd = r * s;
}

struct RngParams {
    const unsigned long long* seeds;
    void* out;              // [B][n] uint32 (MODE_U32) or fp32
    unsigned stream, draw;
    float scale, dropout_p, inv_keep;
    unsigned long long n;   // elements of one sample
    unsigned long long items;   // B * n / V
    // SLOTS only (mdx_randn_slots_f32): sample b draws with counter draw + pos_b, and only while its slot is active
    const int* slot_start;
    const int* slot_len;
    int tick;
};

enum { MODE_U32 = 0, MODE_NORMAL = 1, MODE_NORMAL_DROPOUT = 2 };

// The four elements 4 blk .. 4 blk + 3 of the sample with this seed; every launch form goes through here, so an element's bits
// do not depend on the form that wrote it.
template <int MODE>
__device__ __forceinline__ void quad_values(const RngParams& p, unsigned long long seed, unsigned draw, unsigned blk,
                                            unsigned (&bits)[4]) {
    const unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
    const Quad q = philox4x32_10(blk, draw, p.stream, k0, k1);
    if constexpr (MODE == MODE_U32) {
#pragma unroll
        for (int e = 0; e < 4; ++e) bits[e] = q.w[e];
    } else {
        float z[4], v[4];
        box_muller(q.w[0], q.w[1], z[0], z[1]);
        box_muller(q.w[2], q.w[3], z[2], z[3]);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = p.scale * z[e];
        if constexpr (MODE == MODE_NORMAL_DROPOUT) {
            const Quad d = philox4x32_10(blk, draw, p.stream | DROPOUT_STREAM_BIT, k0, k1);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = uniform_open(d.w[e]) >= p.dropout_p ? v[e] * p.inv_keep : 0.0f;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) bits[e] = __float_as_uint(v[e]);
    }
}

constexpr long RNG_MAX_N = 1L << 34;    // element >> 2 is the counter's 32-bit word 0
