// Per-sample seeded noise: Philox4x32-10 (Salmon et al., "Parallel Random Numbers: As Easy as 1, 2, 3", SC'11; the Random123
// constants) as a counter-based generator, and Box-Muller normals on its words.  Every output element is a pure function of
// (its sample's seed, stream, draw, its index inside the sample): the batch size, the row, the launch geometry and the
// alignment of `out` do not enter (include/mdx.h has the counter layout and the uniform mapping).
// One Philox call is ~40 integer instructions (ten rounds of two 32 x 32 -> 64 multiplies) for four elements, next to one
// 16-byte store: the kernel stays bound by its stores.  Launch shape as qsample.hip: one-wave workgroups, a grid-stride loop,
// one float4 per lane and iteration where n % 4 == 0 and `out` is 16-byte aligned, one float otherwise.
// No fast-math flag and no fast intrinsic in this file: logf / sqrtf / sincospif are the precise ones, and the restatement in
// tests/_seeded_util.py holds the result to 1e-5.
#include <math.h>

#include "mdx_common.h"
#include "qsample_device.h"
#include "rng_device.h"

namespace {

constexpr int RNG_THREADS = 64;
constexpr int RNG_MAX_BLOCKS = 4096;    // 256 CUs x 16 waves; larger tensors take further passes of the grid-stride loop

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// V == 4: item j is quad j % (n / 4) of sample j / (n / 4) (n % 4 == 0, out 16-byte aligned: the host decides);
// V == 1: item j is element j % n of sample j / n, lane (element & 3) of its quad.
// SLOTS: the draw counter is per sample, p.draw + pos of the sample's session slot (mdx_common.h: mdx_slot_pos), and the items
// of an inactive slot are skipped -- nothing of its span is written.  The values still come from quad_values alone.
template <int MODE, int V, bool SLOTS = false>
__global__ __launch_bounds__(RNG_THREADS) void rng_kernel(const RngParams p) {
    const unsigned long long per = p.n / V;
    unsigned* out = reinterpret_cast<unsigned*>(p.out);     // fp32 results travel as their bit patterns
    for (unsigned long long j = (unsigned long long)blockIdx.x * RNG_THREADS + threadIdx.x; j < p.items;
         j += (unsigned long long)gridDim.x * RNG_THREADS) {
        const unsigned long long b = j / per, i = j - b * per;
        unsigned draw = p.draw;
        if constexpr (SLOTS) {
            const int pos = mdx_slot_pos(p.slot_start, p.slot_len, (int)b, 0x7fffffff, p.tick);
            if (pos < 0) continue;
            draw += (unsigned)pos;
        }
        const unsigned long long seed = p.seeds[b];
        unsigned v[4];
        if constexpr (V == 4) {
            quad_values<MODE>(p, seed, draw, (unsigned)i, v);
            u32x4 t;
            t.x = v[0]; t.y = v[1]; t.z = v[2]; t.w = v[3];
            *reinterpret_cast<u32x4*>(out + j * 4) = t;
        } else {
            quad_values<MODE>(p, seed, draw, (unsigned)(i >> 2), v);
            const int lane = (int)(i & 3);
            out[j] = lane == 0 ? v[0] : lane == 1 ? v[1] : lane == 2 ? v[2] : v[3];
        }
    }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

inline int rng_blocks(unsigned long long items) {
    const unsigned long long blocks = (items + RNG_THREADS - 1) / RNG_THREADS;
    return (int)(blocks < (unsigned long long)RNG_MAX_BLOCKS ? blocks : (unsigned long long)RNG_MAX_BLOCKS);
}

template <int MODE, bool SLOTS = false>
void rng_launch(RngParams p, int B, hipStream_t s) {
    if (p.n % 4 == 0 && aligned16(p.out)) {
        p.items = (unsigned long long)B * (p.n / 4);
        hipLaunchKernelGGL((rng_kernel<MODE, 4, SLOTS>), dim3(rng_blocks(p.items)), dim3(RNG_THREADS), 0, s, p);
    } else {
        p.items = (unsigned long long)B * p.n;
        hipLaunchKernelGGL((rng_kernel<MODE, 1, SLOTS>), dim3(rng_blocks(p.items)), dim3(RNG_THREADS), 0, s, p);
    }
}

// ------------------------------------------------------------------ per-slot mask blend (mdx_slot_blend_f32)
// The blend at the top of a decode() iteration for the slots of a session: img = keep q + (1 - keep) img with
// q = a x0 + b noise, the noise drawn here -- quad_values<MODE_NORMAL> at (stream, draw0 + pos_b), scale 1 -- and never stored.
// r carries the generator's arguments (r.n = C * HW, r.draw = draw0, the slot tables, the tick).
struct SlotBlendParams {
    RngParams r;
    const float* x0;        // [B][C][HW]
    const float* keep;      // [B][C][HW]
    float* img;             // [B][C][HW]
    const float* blend_ab;  // [B][cap][2]
    const int* blend_on;    // [B]
    int cap;
};

// Items as rng_kernel's: V == 4 is quad i of sample b (HW % 4 == 0, so C * HW % 4 == 0, and the three tensors 16-byte aligned:
// the host decides), V == 1 element i, lane (i & 3) of its quad.  A slot that is not active, or does not blend, is skipped:
// nothing of its span is read or written.
template <int V>
__global__ __launch_bounds__(RNG_THREADS) void slot_blend_kernel(const SlotBlendParams p) {
    const unsigned long long per = p.r.n / V;
    for (unsigned long long j = (unsigned long long)blockIdx.x * RNG_THREADS + threadIdx.x; j < p.r.items;
         j += (unsigned long long)gridDim.x * RNG_THREADS) {
        const unsigned long long b = j / per, i = j - b * per;
        const int pos = mdx_slot_pos(p.r.slot_start, p.r.slot_len, (int)b, p.cap, p.r.tick);
        if (pos < 0 || p.blend_on[b] == 0) continue;
        const float* ab = p.blend_ab + ((size_t)b * p.cap + pos) * 2;
        const float ca = ab[0], cb = ab[1];
        const unsigned draw = p.r.draw + (unsigned)pos;
        const unsigned long long seed = p.r.seeds[b];
        const size_t at = (size_t)j * V;                        // == b * n + i * V
        unsigned bits[4];
        float nz[V], x[V], m[V], im[V];
        if constexpr (V == 4) {
            quad_values<MODE_NORMAL>(p.r, seed, draw, (unsigned)i, bits);
#pragma unroll
            for (int e = 0; e < 4; ++e) nz[e] = __uint_as_float(bits[e]);
        } else {
            quad_values<MODE_NORMAL>(p.r, seed, draw, (unsigned)(i >> 2), bits);
            const int lane = (int)(i & 3);
            nz[0] = __uint_as_float(lane == 0 ? bits[0] : lane == 1 ? bits[1] : lane == 2 ? bits[2] : bits[3]);
        }
        load_v<V>(p.x0 + at, x);
        load_v<V>(p.keep + at, m);
        load_v<V>(p.img + at, im);
#pragma unroll
        for (int e = 0; e < V; ++e) im[e] = blend_f(m[e], q_sample_f(x[e], nz[e], ca, cb), im[e]);
        store_v<V>(p.img + at, im);
    }
}

}  // namespace

extern "C" int mdx_philox_u32(const unsigned long long* seeds, unsigned stream, unsigned draw, unsigned* out, int B, long n,
                              mdx_stream_t s) {
    MDX_REQUIRE(seeds && out, "mdx_philox_u32: null pointer");
    MDX_REQUIRE(B > 0 && n > 0 && n <= RNG_MAX_N, "mdx_philox_u32: bad extents (B=%d n=%ld; 0 < n <= 2^34)", B, n);
    RngParams p;
    p.seeds = seeds; p.out = out;
    p.stream = stream; p.draw = draw;
    p.scale = 1.0f; p.dropout_p = 0.0f; p.inv_keep = 1.0f;
    p.n = (unsigned long long)n; p.items = 0;
    p.slot_start = p.slot_len = nullptr; p.tick = 0;
    rng_launch<MODE_U32>(p, B, (hipStream_t)s);
    MDX_LAUNCH_CHECK("mdx_philox_u32");
    return MDX_OK;
}

extern "C" int mdx_randn_f32(const unsigned long long* seeds, unsigned stream, unsigned draw, float scale, float dropout_p,
                             float* out, int B, long n, mdx_stream_t s) {
    MDX_REQUIRE(seeds && out, "mdx_randn_f32: null pointer");
    MDX_REQUIRE(B > 0 && n > 0 && n <= RNG_MAX_N, "mdx_randn_f32: bad extents (B=%d n=%ld; 0 < n <= 2^34)", B, n);
    MDX_REQUIRE(dropout_p >= 0.0f && dropout_p < 1.0f, "mdx_randn_f32: dropout_p must be in [0, 1), got %g", (double)dropout_p);
    MDX_REQUIRE(isfinite(scale), "mdx_randn_f32: scale must be finite");
    RngParams p;
    p.seeds = seeds; p.out = out;
    p.stream = stream; p.draw = draw;
    p.scale = scale; p.dropout_p = dropout_p; p.inv_keep = 1.0f / (1.0f - dropout_p);
    p.n = (unsigned long long)n; p.items = 0;
    p.slot_start = p.slot_len = nullptr; p.tick = 0;
    if (dropout_p > 0.0f)
        rng_launch<MODE_NORMAL_DROPOUT>(p, B, (hipStream_t)s);
    else
        rng_launch<MODE_NORMAL>(p, B, (hipStream_t)s);
    MDX_LAUNCH_CHECK("mdx_randn_f32");
    return MDX_OK;
}

extern "C" int mdx_randn_slots_f32(const unsigned long long* seeds, unsigned stream, unsigned draw0, float scale, float dropout_p,
                                   float* out, const int* slot_start, const int* slot_len, int tick, int B, long n,
                                   mdx_stream_t s) {
    MDX_REQUIRE(seeds && out && slot_start && slot_len, "mdx_randn_slots_f32: null pointer");
    MDX_REQUIRE(B > 0 && n > 0 && n <= RNG_MAX_N, "mdx_randn_slots_f32: bad extents (B=%d n=%ld; 0 < n <= 2^34)", B, n);
    MDX_REQUIRE(tick >= 0, "mdx_randn_slots_f32: tick must be >= 0, got %d", tick);
    MDX_REQUIRE(dropout_p >= 0.0f && dropout_p < 1.0f, "mdx_randn_slots_f32: dropout_p must be in [0, 1), got %g",
                (double)dropout_p);
    MDX_REQUIRE(isfinite(scale), "mdx_randn_slots_f32: scale must be finite");
    RngParams p;
    p.seeds = seeds; p.out = out;
    p.stream = stream; p.draw = draw0;
    p.scale = scale; p.dropout_p = dropout_p; p.inv_keep = 1.0f / (1.0f - dropout_p);
    p.n = (unsigned long long)n; p.items = 0;
    p.slot_start = slot_start; p.slot_len = slot_len; p.tick = tick;
    if (dropout_p > 0.0f)
        rng_launch<MODE_NORMAL_DROPOUT, true>(p, B, (hipStream_t)s);
    else
        rng_launch<MODE_NORMAL, true>(p, B, (hipStream_t)s);
    MDX_LAUNCH_CHECK("mdx_randn_slots_f32");
    return MDX_OK;
}

extern "C" int mdx_slot_blend_f32(const float* x0, const float* keep, float* img, const unsigned long long* seeds,
                                  unsigned stream, unsigned draw0, const float* blend_ab, const int* blend_on,
                                  const int* slot_start, const int* slot_len, int cap, int tick, int B, int C, int HW,
                                  mdx_stream_t s) {
    const char* fn = "mdx_slot_blend_f32";
    MDX_REQUIRE(x0 && keep && img && seeds && blend_ab && blend_on && slot_start && slot_len, "%s: null pointer", fn);
    MDX_REQUIRE(B > 0 && B <= 65535 && C > 0 && HW > 0 && (long long)C * HW <= RNG_MAX_N,
                "%s: bad extents (B=%d C=%d HW=%d; 0 < B <= 65535, 0 < C * HW <= 2^34)", fn, B, C, HW);
    MDX_REQUIRE(cap > 0 && tick >= 0, "%s: bad slot extents (cap=%d tick=%d; cap > 0, tick >= 0)", fn, cap, tick);
    SlotBlendParams p;
    p.r.seeds = seeds; p.r.out = nullptr;
    p.r.stream = stream; p.r.draw = draw0;
    p.r.scale = 1.0f; p.r.dropout_p = 0.0f; p.r.inv_keep = 1.0f;
    p.r.n = (unsigned long long)C * HW; p.r.items = 0;
    p.r.slot_start = slot_start; p.r.slot_len = slot_len; p.r.tick = tick;
    p.x0 = x0; p.keep = keep; p.img = img;
    p.blend_ab = blend_ab; p.blend_on = blend_on;
    p.cap = cap;
    if (HW % 4 == 0 && aligned16(x0) && aligned16(keep) && aligned16(img)) {
        p.r.items = (unsigned long long)B * (p.r.n / 4);
        hipLaunchKernelGGL(slot_blend_kernel<4>, dim3(rng_blocks(p.r.items)), dim3(RNG_THREADS), 0, (hipStream_t)s, p);
    } else {
        p.r.items = (unsigned long long)B * p.r.n;
        hipLaunchKernelGGL(slot_blend_kernel<1>, dim3(rng_blocks(p.r.items)), dim3(RNG_THREADS), 0, (hipStream_t)s, p);
    }
    MDX_LAUNCH_CHECK(fn);
    return MDX_OK;
}
