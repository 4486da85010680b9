// Hardware probes, none on the hot path: the MFMA register-layout probes and the DMA / L2 / VALU / mix-rate probes with
// their entries (tools/dma_probe.py, tools/l2_probe.py, tools/exp/).
#include "mdx_common.h"

namespace {

// ------------------------------------------------------------------ MFMA layout probe
__global__ void probe_mfma_kernel(const f16* a, const f16* b, float* c) {
    const int lane = threadIdx.x;
    const f16x8 av = *reinterpret_cast<const f16x8*>(a + lane * 8);
    const f16x8 bv = *reinterpret_cast<const f16x8*>(b + lane * 8);
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(av, bv, acc, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 16; ++r) c[lane * 16 + r] = acc[r];
}

__global__ void probe_mfma16_kernel(const f16* a, const f16* b, float* c) {
    const int lane = threadIdx.x;
    const f16x8 av = *reinterpret_cast<const f16x8*>(a + lane * 8);
    const f16x8 bv = *reinterpret_cast<const f16x8*>(b + lane * 8);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(av, bv, acc, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 4; ++r) c[lane * 4 + r] = acc[r];
}

}  // namespace

extern "C" int mdx_probe_mfma_32x32x16_f16(const void* a, const void* b, float* c, mdx_stream_t s) {
    MDX_REQUIRE(a && b && c, "mdx_probe_mfma_32x32x16_f16: null pointer");
    hipLaunchKernelGGL(probe_mfma_kernel, dim3(1), dim3(64), 0, (hipStream_t)s, (const f16*)a, (const f16*)b, c);
    MDX_LAUNCH_CHECK("mdx_probe_mfma_32x32x16_f16");
    return MDX_OK;
}

extern "C" int mdx_probe_mfma_16x16x32_f16(const void* a, const void* b, float* c, mdx_stream_t s) {
    MDX_REQUIRE(a && b && c, "mdx_probe_mfma_16x16x32_f16: null pointer");
    hipLaunchKernelGGL(probe_mfma16_kernel, dim3(1), dim3(64), 0, (hipStream_t)s, (const f16*)a, (const f16*)b, c);
    MDX_LAUNCH_CHECK("mdx_probe_mfma_16x16x32_f16");
    return MDX_OK;
}

// ------------------------------------------------------------------ DMA / load streaming probe (tools/dma_probe.py)
// Measures what ONE workgroup per CU can pull through `buffer_load ... lds` (mode 0) or through plain
// global_load_dwordx4 into registers (mode 1): tiles of 1 KiB per wave-instruction, `per` instructions per wave per
// tile, NS tiles in flight.  Not on the hot path.
namespace {
template <int NS>
__global__ __launch_bounds__(512) void dma_probe_kernel(const char* src, size_t bytes_per_block, int per, int mode,
                                                        int stride_tiles, float* sink) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nw = blockDim.x >> 6;
    const size_t tile_bytes = (size_t)nw * per * 1024;
    const int nt = (int)(bytes_per_block / tile_bytes);
    const bool shared = (mode & 4) != 0;        // every block streams the SAME region (L2-resident operands shared by the tiles of a launch)
    mode &= 3;
    const char* base = src + (shared ? 0 : (size_t)blockIdx.x * bytes_per_block);
    const __amdgpu_buffer_rsrc_t rs = make_rsrc(base, (unsigned)bytes_per_block);
    float acc = 0.f;
    if (mode == 2) {
        // BOTH paths at once (round 4): per tile every wave issues `per` LDS-DMA instructions AND `per` plain 16-byte loads into
        // registers (of the next region: 2 x tile_bytes per step), to see whether the two operand paths add up on a CU
        typedef unsigned pu4 __attribute__((ext_vector_type(4)));
        const int nt2 = nt / 2;
        auto issue = [&](int t, int stage) {
            for (int j = 0; j < per; ++j) {
                const unsigned off = (unsigned)((size_t)(2 * t) * tile_bytes + ((wave * per + j) * 64 + lane) * 16);
                dma16(rs, smem + (size_t)stage * tile_bytes + (wave * per + j) * 1024, off);
            }
        };
        pu4 v[8];
        unsigned x = 0;
        for (int i = 0; i < NS - 1 && i < nt2; ++i) issue(i, i);
        int wr = NS - 1;
        for (int t = 0; t < nt2; ++t) {
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (j < per) v[j] = __builtin_amdgcn_raw_buffer_load_b128(rs, (unsigned)(((wave * per + j) * 64 + lane) * 16), (unsigned)((size_t)(2 * t + 1) * tile_bytes), 0);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            if (t + NS - 1 < nt2) issue(t + NS - 1, wr);
            wr = (wr + 1 == NS) ? 0 : wr + 1;
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (j < per) x ^= v[j][0] ^ v[j][3];
        }
        acc = ((float*)smem)[threadIdx.x] + (float)(x & 1);
    } else if (mode == 0) {
        auto issue = [&](int t, int stage) {
            for (int j = 0; j < per; ++j) {
                const unsigned off = (unsigned)((size_t)(t * stride_tiles % nt) * tile_bytes + ((wave * per + j) * 64 + lane) * 16);
                dma16(rs, smem + (size_t)stage * tile_bytes + (wave * per + j) * 1024, off);
            }
        };
        for (int i = 0; i < NS - 1 && i < nt; ++i) issue(i, i);
        int wr = NS - 1;
        for (int t = 0; t < nt; ++t) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // conservative: drain own DMAs (depth comes from other waves/tiles)
            __builtin_amdgcn_s_barrier();
            if (t + NS - 1 < nt) issue(t + NS - 1, wr);
            wr = (wr + 1 == NS) ? 0 : wr + 1;
        }
        acc = ((float*)smem)[threadIdx.x];
    } else {
        const f32x4* g = reinterpret_cast<const f32x4*>(base);
        f32x4 v[8];
        for (int t = 0; t < nt; ++t) {
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (j < per) v[j] = g[((size_t)(t * stride_tiles % nt) * tile_bytes + ((wave * per + j) * 64 + lane) * 16) / 16];
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (j < per) acc += v[j][0] + v[j][3];
        }
    }
    if (acc == 123.456f) sink[0] = acc;
}
}  // namespace

extern "C" int mdx_probe_dma_stream(const void* src, size_t bytes_per_block, int nblocks, int waves, int per, int ns,
                                    int mode, int stride_tiles, float* sink, mdx_stream_t s) {
    MDX_REQUIRE(src && sink && nblocks > 0 && waves >= 1 && waves <= 8 && per >= 1 && per <= 8 && ns >= 2 && ns <= 4,
                "mdx_probe_dma_stream: bad arguments");
    const size_t lds = (size_t)ns * waves * per * 1024;
    MDX_REQUIRE(lds <= 160 * 1024, "mdx_probe_dma_stream: ring too large");
    hipStream_t st = (hipStream_t)s;
#define MDX_PROBE_LAUNCH(NSV)                                                                                        \
    {                                                                                                                \
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&dma_probe_kernel<NSV>),                             \
                                  hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);                           \
        hipLaunchKernelGGL(dma_probe_kernel<NSV>, dim3(nblocks), dim3(waves * 64), lds, st, (const char*)src,        \
                           bytes_per_block, per, mode, stride_tiles, sink);                                          \
    }
    if (ns == 2) MDX_PROBE_LAUNCH(2)
    else if (ns == 3) MDX_PROBE_LAUNCH(3)
    else MDX_PROBE_LAUNCH(4)
#undef MDX_PROBE_LAUNCH
    MDX_LAUNCH_CHECK("mdx_probe_dma_stream");
    return MDX_OK;
}

// ------------------------------------------------------------------ L2 -> VGPR streaming probe (tools/l2_probe.py)
// What the fused-chain kernels (stchain.hip) do with their weights: every wave streams its own contiguous region with one
// coalesced 1 KiB buffer_load_dwordx4 per piece, PF pieces in flight (schedule pinned), optionally the SAME region in every
// block (shared = 1: all CUs hit the same L2 lines, as all row blocks of a fused launch read the same weights).
namespace {
typedef unsigned pu32x4 __attribute__((ext_vector_type(4)));
template <int PFD>
__global__ __launch_bounds__(1024) void l2_probe_kernel(const char* src, unsigned bytes_per_wave, int shared, unsigned total_bytes,
                                                        float* sink) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nw = blockDim.x >> 6;
    const __amdgpu_buffer_rsrc_t rs = make_rsrc(src, total_bytes);
    const unsigned base = ((shared ? 0u : (unsigned)blockIdx.x * nw) + wave) * bytes_per_wave;
    const unsigned voff = lane * 16u;
    const int pieces = bytes_per_wave / 1024;
    pu32x4 ring[PFD];
#pragma unroll
    for (int j = 0; j < PFD; ++j) ring[j] = __builtin_amdgcn_raw_buffer_load_b128(rs, voff, base + j * 1024u, 0);
    unsigned acc = 0;
    for (int p0 = 0; p0 < pieces; p0 += PFD) {
#pragma unroll
        for (int j = 0; j < PFD; ++j) {
            acc ^= ring[j][0] ^ ring[j][3];
            ring[j] = __builtin_amdgcn_raw_buffer_load_b128(rs, voff, base + (unsigned)(p0 + j + PFD) * 1024u, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    if (acc == 0x12345678u) sink[0] = 1.f;
}
}  // namespace

extern "C" int mdx_probe_l2_stream(const void* src, size_t total_bytes, unsigned bytes_per_wave, int nblocks, int waves, int pf,
                                   int shared, float* sink, mdx_stream_t s) {
    MDX_REQUIRE(src && sink && nblocks > 0 && waves >= 1 && waves <= 16 && bytes_per_wave % (32 * 1024) == 0 &&
                    total_bytes <= 0xffffffffull, "mdx_probe_l2_stream: bad arguments");
    hipStream_t st = (hipStream_t)s;
    if (pf == 8) hipLaunchKernelGGL(l2_probe_kernel<8>, dim3(nblocks), dim3(waves * 64), 0, st, (const char*)src, bytes_per_wave, shared, (unsigned)total_bytes, sink);
    else if (pf == 16) hipLaunchKernelGGL(l2_probe_kernel<16>, dim3(nblocks), dim3(waves * 64), 0, st, (const char*)src, bytes_per_wave, shared, (unsigned)total_bytes, sink);
    else if (pf == 32) hipLaunchKernelGGL(l2_probe_kernel<32>, dim3(nblocks), dim3(waves * 64), 0, st, (const char*)src, bytes_per_wave, shared, (unsigned)total_bytes, sink);
    else MDX_REQUIRE(false, "mdx_probe_l2_stream: pf must be 8, 16 or 32");
    MDX_LAUNCH_CHECK("mdx_probe_l2_stream");
    return MDX_OK;
}

// ------------------------------------------------------------------ VALU issue-rate probe (tools/exp/r04n_valu_probe.py)
namespace {
// kind 0: v_fma_f32, 1: v_exp_f32, 2: v_pk_fma_f32 (two results), 3: v_cvt_pk_f16_f32, 4: v_max3_f32, 5: v_exp_f16, 6: v_pk_fma_f16 (two
// results), 7: v_pk_max_f16 (two results) -- eight independent chains per lane
template <int KIND>
__global__ __launch_bounds__(256) void valu_probe_kernel(int iters, float* sink) {
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    float x[8];
    f32x2 y[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        x[i] = 0.001f * (float)(threadIdx.x + i) - 0.5f;
        y[i] = f32x2{x[i], -x[i]};
    }
    const f32x2 c2 = {0.999f, 1.001f}, d2 = {1e-6f, -1e-6f};
    typedef _Float16 h2v __attribute__((ext_vector_type(2)));
    h2v hx[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) hx[i] = h2v{(_Float16)x[i], (_Float16)(-x[i])};
    const h2v hc = {(_Float16)0.999f, (_Float16)1.001f}, hd = {(_Float16)1e-3f, (_Float16)-1e-3f};
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if (KIND == 0) x[i] = __builtin_fmaf(x[i], 0.999f, 1e-6f);
            else if (KIND == 1) x[i] = __builtin_amdgcn_exp2f(x[i]);
            else if (KIND == 2) y[i] = __builtin_elementwise_fma(y[i], c2, d2);
            else if (KIND == 3) {
                typedef _Float16 h2 __attribute__((ext_vector_type(2)));
                const h2 h = {(_Float16)x[i], (_Float16)x[(i + 1) & 7]};
                x[i] = (float)h[0] + (float)h[1];
            } else if (KIND == 4) x[i] = __builtin_fmaxf(__builtin_fmaxf(x[i], x[(i + 1) & 7]), x[(i + 2) & 7]) * 0.5f;
            else if (KIND == 5) {      // v_exp_f16: is a half-precision exponential cheaper than v_exp_f32?  (round 5, attention softmax)
                _Float16 r;
                asm volatile("v_exp_f16 %0, %1" : "=v"(r) : "v"(hx[i][0]));
                hx[i][0] = r;
            } else if (KIND == 6) hx[i] = __builtin_elementwise_fma(hx[i], hc, hd);      // v_pk_fma_f16 (two results)
            else {                     // 7: v_pk_max_f16 (two results) -- the row-maximum fold on packed halves
                hx[i] = __builtin_elementwise_max(hx[i], hx[(i + 1) & 7]);
            }
        }
    }
    float a = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) a += x[i] + y[i].x + y[i].y + (float)hx[i][0] + (float)hx[i][1];
    if (a == 123.456f) sink[0] = a;
}
// Does VALU work run in the shadow of an MFMA?  (round 6, attention softmax.)  Four slots per iteration; a slot is
//   kind 0: one v_mfma_f32_32x32x16_f16 (two independent accumulator chains alternate)        kind 3: two v_exp_f32
//   kind 1: the MFMA + two v_exp_f32 (independent chains)                                       kind 4: eight v_fma_f32
//   kind 2: the MFMA + eight v_fma_f32                                                          kind 6: the softmax mix alone
//   kind 5: the MFMA + the softmax mix of one score pair (2 fma, 2 exp, 1 packed add, 1 cvt_pk)
template <int KIND>
__global__ __launch_bounds__(256) void mix_probe_kernel(int iters, float* sink) {
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    f32x16 acc[2];
    f16x8 a, b;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[0][r] = acc[1][r] = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        a[e] = (f16)(0.001f * (float)((threadIdx.x + e) & 15));
        b[e] = (f16)(0.002f * (float)((threadIdx.x + 3 * e) & 7));
    }
    float x[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] = 0.001f * (float)(threadIdx.x + i) - 0.5f;
    f32x2 ps = {0.f, 0.f};
    unsigned pw = 0;
    constexpr bool MF = KIND == 0 || KIND == 1 || KIND == 2 || KIND == 5;
    constexpr bool MFA = KIND >= 7;       // 7 / 8 / 9: the accumulators (9: A and B too) live in AccVGPRs (inline asm, "a" constraint)
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int sl = 0; sl < 4; ++sl) {
            if constexpr (MF) acc[sl & 1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, acc[sl & 1], 0, 0, 0);
            if constexpr (MFA) {
                if constexpr (KIND == 9)
                    asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, %0" : "+a"(acc[sl & 1]) : "a"(a), "a"(b));
                else
                    asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, %0" : "+a"(acc[sl & 1]) : "v"(a), "v"(b));
            }
            if constexpr (KIND == 1 || KIND == 3) {
                x[2 * sl] = __builtin_amdgcn_exp2f(x[2 * sl]);
                x[2 * sl + 1] = __builtin_amdgcn_exp2f(x[2 * sl + 1]);
            } else if constexpr (KIND == 2 || KIND == 4 || KIND == 7) {
#pragma unroll
                for (int i = 0; i < 8; ++i) x[i] = __builtin_fmaf(x[i], 0.999f, 1e-6f);
            } else if constexpr (KIND == 5 || KIND == 6 || KIND == 8 || KIND == 9) {
                const float u = __builtin_fmaf(x[2 * sl], 0.999f, -0.25f), v = __builtin_fmaf(x[2 * sl + 1], 0.999f, -0.25f);
                const f32x2 e2 = {__builtin_amdgcn_exp2f(u), __builtin_amdgcn_exp2f(v)};
                ps += e2;
                typedef _Float16 h2 __attribute__((ext_vector_type(2)));
                const h2 hv = {(_Float16)e2.x, (_Float16)e2.y};
                pw ^= __builtin_bit_cast(unsigned, hv);
                x[2 * sl] = e2.x - 1.0f;
                x[2 * sl + 1] = e2.y - 1.0f;
            }
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x002, 64, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    float t = ps.x + ps.y + (float)pw;
#pragma unroll
    for (int i = 0; i < 8; ++i) t += x[i];
#pragma unroll
    for (int r = 0; r < 16; ++r) t += acc[0][r] + acc[1][r];
    if (t == 123.456f) sink[0] = t;
}
}  // namespace

extern "C" int mdx_probe_mix_rate(int kind, int iters, int nblocks, float* sink, mdx_stream_t s) {
    MDX_REQUIRE(sink && iters > 0 && nblocks > 0 && kind >= 0 && kind <= 9, "mdx_probe_mix_rate: bad arguments");
    hipStream_t st = (hipStream_t)s;
    switch (kind) {
        case 0: hipLaunchKernelGGL(mix_probe_kernel<0>, dim3(nblocks), dim3(256), 0, st, iters, sink); break;
        case 1: hipLaunchKernelGGL(mix_probe_kernel<1>, dim3(nblocks), dim3(256), 0, st, iters, sink); break;
        case 2: hipLaunchKernelGGL(mix_probe_kernel<2>, dim3(nblocks), dim3(256), 0, st, iters, sink); break;
        case 3: hipLaunchKernelGGL(mix_probe_kernel<3>, dim3(nblocks), dim3(256), 0, st, iters, sink); break;
        case 4: hipLaunchKernelGGL(mix_probe_kernel<4>, dim3(nblocks), dim3(256), 0, st, iters, sink); break;
        case 5: hipLaunchKernelGGL(mix_probe_kernel<5>, dim3(nblocks), dim3(256), 0, st, iters, sink); break;
        case 7: hipLaunchKernelGGL(mix_probe_kernel<7>, dim3(nblocks), dim3(256), 0, st, iters, sink); break;
        case 8: hipLaunchKernelGGL(mix_probe_kernel<8>, dim3(nblocks), dim3(256), 0, st, iters, sink); break;
        case 9: hipLaunchKernelGGL(mix_probe_kernel<9>, dim3(nblocks), dim3(256), 0, st, iters, sink); break;
        default: hipLaunchKernelGGL(mix_probe_kernel<6>, dim3(nblocks), dim3(256), 0, st, iters, sink); break;
    }
    MDX_LAUNCH_CHECK("mdx_probe_mix_rate");
    return MDX_OK;
}

extern "C" int mdx_probe_valu_rate(int kind, int iters, int nblocks, float* sink, mdx_stream_t s) {
    MDX_REQUIRE(sink && iters > 0 && nblocks > 0 && kind >= 0 && kind <= 7, "mdx_probe_valu_rate: bad arguments");
    hipStream_t st = (hipStream_t)s;
    switch (kind) {
        case 0: hipLaunchKernelGGL(valu_probe_kernel<0>, dim3(nblocks), dim3(256), 0, st, iters, sink); break;
        case 1: hipLaunchKernelGGL(valu_probe_kernel<1>, dim3(nblocks), dim3(256), 0, st, iters, sink); break;
        case 2: hipLaunchKernelGGL(valu_probe_kernel<2>, dim3(nblocks), dim3(256), 0, st, iters, sink); break;
        case 3: hipLaunchKernelGGL(valu_probe_kernel<3>, dim3(nblocks), dim3(256), 0, st, iters, sink); break;
        case 5: hipLaunchKernelGGL(valu_probe_kernel<5>, dim3(nblocks), dim3(256), 0, st, iters, sink); break;
        case 6: hipLaunchKernelGGL(valu_probe_kernel<6>, dim3(nblocks), dim3(256), 0, st, iters, sink); break;
        case 7: hipLaunchKernelGGL(valu_probe_kernel<7>, dim3(nblocks), dim3(256), 0, st, iters, sink); break;
        default: hipLaunchKernelGGL(valu_probe_kernel<4>, dim3(nblocks), dim3(256), 0, st, iters, sink); break;
    }
    MDX_LAUNCH_CHECK("mdx_probe_valu_rate");
    return MDX_OK;
}
