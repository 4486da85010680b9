// Lean instantiation of the implicit-GEMM kernel for DENSE row-major launches (round 6).
//
//   out[m][n] = sum_k A[m][k] * W[n][k]      nn.Dense / 1x1 conv over tokens (attention.py:44, 66, 108-112, 212, 231; unet.py:267-310)
//
// Two thirds of the launches of a UNet evaluation are dense (ksize 1, stride 1, one source), and at UNet batch 2 every one of them
// runs one block per CU for 8-15 us -- of which, in the generic gemm_kernel (gemm.hip), 1.0-1.9 us went to a prologue written for
// convolutions (three integer divisions for the tile decode, tap masks, the (b, y, x) split of every loader row: ~700 scalar / vector
// instructions in front of the first DMA, issued by a wave that has its SIMD to itself at one instruction per ~4 clocks) and 1.1-2.6 us
// to an epilogue whose global loads (residual rows, the LayerNorm-fold row statistics and S[n]) each start a dependent round trip
// that nothing hides (profiles/r05_gemm_trace_kloop.txt, DESIGN.md section 8 items 1-2 of round 5).  This kernel is the same tile
// program -- same LDS image, same K order per output, same MFMA operand order, same epilogue arithmetic (gemm_epilogue of
// gemm_internal.h): results are BIT-IDENTICAL to the generic kernel's (tests/test_kernels_gpu.py) -- with
//   * a division-free prologue (2-D grid for the SPREAD order, multiply-high for the tile decode) that issues the first NS-1 K tiles'
//     DMAs ~80 instructions after the kernel-argument wait;
//   * everything the epilogue reads from global memory requested right behind those DMAs -- bias, the residual rows of the
//     thread's store passes, the LayerNorm-fold partials of the thread's row (up to 24 of them, held in registers: the adds run
//     after the K loop in the partials' order, so the statistics keep their bits) and S[n] -- so that the epilogue of a lone block is
//     staging + arithmetic + stores.
// Launch forms covered (mdx_dense_takes below): row-major output, unsplit or in-kernel split-K reduce (tickets), bias / residual / GEGLU / row statistics /
// column statistics / LayerNorm-fold consumer / the q|k row-major + V^T split store.  The 128 x 160 tile (four waves 4 x 1, epilogue_w41
// below; round 7) cuts M = 512 x N = 10240 and M = 2048 x N = 5120 into exactly 256 / 512 equal blocks: bias / residual / GEGLU /
// LayerNorm-fold consumer, unsplit.  A K-segmented A operand (two row-major sources, c1 % 64 == 0 and c2 % 64 == 0: template flag SEG)
// runs on the four 2 x 2-wave tiles with the plain epilogue.  Everything else (per-sample row bias, out_bs,
// GELU activations, transposed output, slab split-K, the GroupNorm-on-A form, eight waves) stays on the generic kernel.
#include "mdx_common.h"
#include "gemm_internal.h"

#include <algorithm>

namespace {

// 1 = the batched store loops of gemm_epilogue<..., LEAN> (round 6); 0 = the generic per-pass loops (A/B builds: make variant)
#ifndef MDX_LEAN_EPI
#define MDX_LEAN_EPI 1
#endif
constexpr bool LEAN_EPI = MDX_LEAN_EPI != 0;
constexpr int LNR_MAX = 24;      // LayerNorm-fold partials per row a thread holds across the K loop (K <= 1536); more: the epilogue folds
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

// Prefetch level PF -- how much of what the epilogue reads is requested before the K loop (measured in situ at UNet batch 2,
// profiles/r06_lean_dense_ab.txt; every level leaves the bits alone):
//   0  bias
//   1  + one dword of every line of the LayerNorm-fold consumer's row statistics and of S[n] (gemm_kernel's round-5 "touch")
//   2  + the residual rows of the thread's first store passes and S[n] itself, in registers
//   3  + the LayerNorm partials of the thread's row in registers (up to 24: ~50 more VGPRs, two blocks per CU) -- the full form;
//      a VMEM instruction costs a lone wave ~50 clocks to issue, and 29 of them in front of the first barrier cost the launch more
//      than the round trips they hide
// Cross-attention over a short cached context as the epilogue of the query projection (mdx_gemm_desc.xattn_k; BN = 64 = head dim): the
// tile's fp16 q rows are in LDS at `stg` ([BM][72]), the head's K / V^T tiles (64 keys each; attn_kernel's LDS images) at `xs`: two
// slots, tile t in slot t & 1.  Up to two tiles (xa_len <= 128) are all staged by the caller before this runs -- the only form until
// contexts longer than 128 keys came, and its LDS size, barriers and bits are what they were.  Longer contexts re-stage the two slots
// pair by pair (`restage`, every wave of the block issues its share) between two block barriers: readers of the old pair done | new
// pair landed.  The tile program and its order over the tiles do not depend on where a tile was staged, so the contract holds for
// any length (above two tiles mdx_attention_f16 runs attn_pipe_kernel, bit-identical to attn_kernel).
// Every wave takes 32 query rows through attn_kernel's tile program -- S^T = K Q^T, lazy-reference online softmax, O^T += V^T P^T, the
// masked form on a ragged last tile -- normalises, stages its 32 x 64 output rows over its own q rows and stores them: the same
// operations on the same values in the same order as mdx_attention_f16 on the stored q (bit-identical).
template <int BM, class Restage>
__device__ __forceinline__ void xattn_tile_epilogue(const GemmParams& p, char* smem, const char* xs, const int m0, const int n0,
                                                    const Restage& restage) {
    constexpr int SLD = 72;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ntile = (p.xa_len + 63) >> 6;
    if (wave * 32 >= BM) {      // no query rows: this wave only stages the later tile pairs of a long context
        for (int t0 = 2; t0 < ntile; t0 += 2) {
            __syncthreads();
            restage(t0);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
        }
        return;
    }
    const int hi = lane >> 5, l31 = lane & 31;
    f16* stg = reinterpret_cast<f16*>(smem);
    f16x8 qf[4];
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4) qf[s4] = *reinterpret_cast<const f16x8*>(&stg[(wave * 32 + l31) * SLD + 16 * s4 + 8 * hi]);
    f32x16 acc_o[2];
#pragma unroll
    for (int d = 0; d < 2; ++d)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc_o[d][r] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;
    const int vswz = (lane >> 1) & 7;
    const int krow_l = (l31 & 0x13) | ((l31 & 4) << 1) | ((l31 & 8) >> 1);      // attn_kernel's key permutation
    auto tile = [&](const int t, auto mask_c) {
        constexpr bool MASK = decltype(mask_c)::value;
        const char* sk = xs + (t & 1) * 16384;
        const char* sv = sk + 8192;
        f32x16 acc_s[2];
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) {
#pragma unroll
            for (int r = 0; r < 16; ++r) acc_s[kt][r] = 0.f;
            const int krow = kt * 32 + krow_l;
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) {
                const f16x8 kf = *reinterpret_cast<const f16x8*>(sk + krow * 128 + (((2 * s4 + hi) ^ ((krow >> 1) & 7)) << 4));
                acc_s[kt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf, qf[s4], acc_s[kt], 0, 0, 0);
            }
        }
        if constexpr (MASK) {
            const int key0 = t * 64, kmax = p.xa_len - 1;
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key = key0 + kt * 32 + (r & 3) + 4 * ((r >> 2) & 1) + 8 * hi + 16 * (r >> 3);
                    if (key > kmax) acc_s[kt][r] = -INFINITY;
                }
        }
        float mx = acc_s[0][0];
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int r = 0; r < 16; ++r) mx = fmaxf(mx, acc_s[kt][r]);
        {
            const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(mx), __float_as_uint(mx), false, false);
            mx = fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1]));
        }
        const float m_cand = fmaxf(m_run, mx);
        if (__builtin_amdgcn_ballot_w64((m_cand - m_run) * p.xa_scale_log2 > 8.0f)) {
            const float alpha = __builtin_amdgcn_exp2f((m_run - m_cand) * p.xa_scale_log2);
            l_run *= alpha;
#pragma unroll
            for (int d = 0; d < 2; ++d)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc_o[d][r] *= alpha;
            m_run = m_cand;
        }
        const float mb = m_run * p.xa_scale_log2;
        typedef float f32x2 __attribute__((ext_vector_type(2)));
        const f32x2 sc2 = {p.xa_scale_log2, p.xa_scale_log2}, nmb2 = {-mb, -mb};
        f32x2 psum2 = {0.f, 0.f};
        f16x8 pf[4];
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int r = 0; r < 16; r += 2) {
                const f32x2 x2 = {acc_s[kt][r], acc_s[kt][r + 1]};
                const f32x2 a2 = __builtin_elementwise_fma(x2, sc2, nmb2);
                const f32x2 pv2 = {__builtin_amdgcn_exp2f(a2.x), __builtin_amdgcn_exp2f(a2.y)};
                psum2 += pv2;
                pf[kt * 2 + (r >> 3)][r & 7] = (f16)pv2.x;
                pf[kt * 2 + (r >> 3)][(r & 7) + 1] = (f16)pv2.y;
            }
        l_run += psum2.x + psum2.y;
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int d = 0; d < 2; ++d) {
                const f16x8 vf = *reinterpret_cast<const f16x8*>(sv + (d * 32 + l31) * 128 + (((2 * c + hi) ^ vswz) << 4));
                acc_o[d] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, pf[c], acc_o[d], 0, 0, 0);
            }
    };
    for (int t = 0; t < ntile; ++t) {
        if (t >= 2 && !(t & 1)) {      // (block-uniform) both slots read by every wave -> the next pair
            __syncthreads();
            restage(t);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
        }
        if ((t + 1) * 64 > p.xa_len) tile(t, std::true_type{}); else tile(t, std::false_type{});
    }
    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    const float inv = 1.0f / l_tot;
    f16* og = stg + wave * 32 * SLD;      // this wave's own q rows: its fragments are in registers
#pragma unroll
    for (int d = 0; d < 2; ++d)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            f16x4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = (f16)(acc_o[d][4 * g + e] * inv);
            *reinterpret_cast<f16x4*>(&og[l31 * SLD + d * 32 + 8 * g + 4 * hi]) = v;
        }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // (wave-local hand-over through LDS)
    for (int idx = lane; idx < 32 * 8; idx += 64) {
        const int row = idx >> 3, chunk = idx & 7;
        const int m = m0 + wave * 32 + row;
        if (m < p.M) {
            const f16x8 v = *reinterpret_cast<const f16x8*>(&og[row * SLD + chunk * 8]);
            *reinterpret_cast<f16x8*>(p.out + (size_t)m * p.out_ld + n0 + chunk * 8) = v;
        }
    }
}

// Epilogue of the 128 x 160 tile (four waves 4 x 1: wave w owns rows 32 w .. 32 w + 31 of the tile and all BN columns, five 32 x 32
// accumulator tiles).  The arithmetic is gemm_epilogue's EMODE 1 -- LayerNorm-fold correction in fp32 in the accumulator registers, fp16
// staging, then per 8 columns  fp16(float(staged) + bias [+ residual])  or the GEGLU product -- on the same values in the same order:
// a launch on this tile gives the bits of the 64- / 128-column tiles (tests/test_dense_tile160_gpu.py).  What differs is the index
// work: BN / 8 = 20 (GEGLU: 10) chunks per row do not divide 256 threads, so the store loops run over the flat item index
// tid + 256 * pass (BM * BN / 8 / 256 = 10 passes, GEGLU 5: no idle lane, consecutive lanes on consecutive 16-byte chunks of a row)
// and the chunk of a thread changes from pass to pass -- the tile's bias columns therefore go through LDS (one dword per thread,
// fetched before the K loop together with the column's S[n] of the LayerNorm fold) instead of 16 registers.  GEGLU pairs column j with column j + BN / 2 of the tile (mdx_gemm_desc.geglu_unit
// = 80).  Not carried (the resolver keeps such launches on the other tiles): split-K tickets, row / column statistics, the q|k + V^T
// split store, the cross-attention epilogue.
template <int BM, int BN>
__device__ __forceinline__ void epilogue_w41(const GemmParams& p, f32x16 (&acc)[BN / 32], char* smem, const int m0, const int n0,
                                             const float bias_pre, const float lns_pre) {
    constexpr int NT = 256, TN = BN / 32, SLD = BN + 8;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int hi = lane >> 5, l31 = lane & 31;
    f16* stg = reinterpret_cast<f16*>(smem);
    float* lnrow = reinterpret_cast<float*>(smem + (size_t)BM * SLD * 2);      // [BM][2] mean, rstd
    float* lns = lnrow + 2 * BM;                                               // [BN] S[n]
    float* bs = lns + BN;                                                      // [BN] bias (zeros when the launch has none)
    if (tid < BN) bs[tid] = bias_pre;
    const int m_l = wave * 32 + l31;
    if (p.ln_stats) {
        for (int r = tid; r < BM; r += NT) {
            float mr[2];
            gemm_ln_row_fold(p, m0 + r, mr);
            lnrow[2 * r] = mr[0];
            lnrow[2 * r + 1] = mr[1];
        }
        if (tid < BN) lns[tid] = lns_pre;      // S[n0 + tid], fetched before the K loop (zero past N)
        __syncthreads();
        const float mean = lnrow[2 * m_l], rstd = lnrow[2 * m_l + 1];
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int n_l = j * 32 + 8 * (r >> 2) + 4 * hi + (r & 3);
                acc[j][r] = rstd * (acc[j][r] - mean * lns[n_l]);
            }
    }
    const bool geglu = p.epilogue == MDX_EPI_GEGLU;
    // plain store: the residual rows of ALL the thread's passes requested in front of the staging pass, through a descriptor that
    // answers zero when there is no residual (GEGLU with a residual is not a shape of the models: fetched in its loop)
    constexpr int CH = BN / 8, PASSES = BM * CH / NT;
    static_assert(BM * CH % NT == 0 && BM * (CH / 2) % NT == 0, "store loops: whole passes");
    const __amdgpu_buffer_rsrc_t rs_res = make_rsrc(p.residual, (p.residual && !geglu) ? p.res_bytes : 0u);
    f16x8 lres[PASSES];
#pragma unroll
    for (int pass = 0; pass < PASSES; ++pass) {
        const int idx = tid + pass * NT;
        const int row = idx / CH, c = idx - row * CH;
        const int m = m0 + row, n = n0 + c * 8;
        const unsigned off = (m < p.M && n < p.N) ? ((unsigned)m * (unsigned)p.residual_ld + (unsigned)n) * 2u : MDX_OOB;
        lres[pass] = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(rs_res, off, 0, 0));
    }
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int n_l = j * 32 + 8 * g + 4 * hi;
            *reinterpret_cast<f16x4*>(&stg[m_l * SLD + n_l]) =
                cvt4(acc[j][4 * g], acc[j][4 * g + 1], acc[j][4 * g + 2], acc[j][4 * g + 3]);
        }
    __syncthreads();
    trace_mark(p, 5);
    if (geglu) {
        // tile = BN / 2 'a' columns | BN / 2 gate columns -> BN / 2 outputs at column n0 / 2
        constexpr int U = BN / 2, GCH = U / 8, GP = BM * GCH / NT;
        const bool has_res = p.residual != nullptr;      // uniform
        f16x8 va[GP], vg[GP];
        f32x4 ba[GP][2], bg[GP][2];
#pragma unroll
        for (int pass = 0; pass < GP; ++pass) {
            const int idx = tid + pass * NT;
            const int row = idx / GCH, c = idx - row * GCH;
            va[pass] = *reinterpret_cast<const f16x8*>(&stg[row * SLD + c * 8]);
            vg[pass] = *reinterpret_cast<const f16x8*>(&stg[row * SLD + U + c * 8]);
            ba[pass][0] = *reinterpret_cast<const f32x4*>(&bs[c * 8]);
            ba[pass][1] = *reinterpret_cast<const f32x4*>(&bs[c * 8 + 4]);
            bg[pass][0] = *reinterpret_cast<const f32x4*>(&bs[U + c * 8]);
            bg[pass][1] = *reinterpret_cast<const f32x4*>(&bs[U + c * 8 + 4]);
        }
#pragma unroll
        for (int pass = 0; pass < GP; ++pass) {
            const int idx = tid + pass * NT;
            const int row = idx / GCH, c = idx - row * GCH;
            const int m = m0 + row;
            const int pn = n0 + c * 8;              // packed column of the 'a' part
            const int on = (n0 >> 1) + c * 8;       // output column
            if (m < p.M && pn < p.N) {
                float f[8];
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    f[e] = ((float)va[pass][e] + ba[pass][e >> 2][e & 3]) * gelu_tanh_f((float)vg[pass][e] + bg[pass][e >> 2][e & 3]);
                if (has_res) {
                    const f16x8 rr = *reinterpret_cast<const f16x8*>(p.residual + (size_t)m * p.residual_ld + on);
#pragma unroll
                    for (int e = 0; e < 8; ++e) f[e] += (float)rr[e];
                }
                f16x8 o;
#pragma unroll
                for (int e = 0; e < 8; ++e) o[e] = (f16)f[e];
                *reinterpret_cast<f16x8*>(p.out + (size_t)m * p.out_ld + on) = o;
            }
        }
        return;
    }
    const bool has_res = p.residual != nullptr;      // uniform
    f16x8 sv[PASSES];
    f32x4 bb[PASSES][2];
#pragma unroll
    for (int pass = 0; pass < PASSES; ++pass) {
        const int idx = tid + pass * NT;
        const int row = idx / CH, c = idx - row * CH;
        sv[pass] = *reinterpret_cast<const f16x8*>(&stg[row * SLD + c * 8]);
        bb[pass][0] = *reinterpret_cast<const f32x4*>(&bs[c * 8]);
        bb[pass][1] = *reinterpret_cast<const f32x4*>(&bs[c * 8 + 4]);
    }
#pragma unroll
    for (int pass = 0; pass < PASSES; ++pass) {
        const int idx = tid + pass * NT;
        const int row = idx / CH, c = idx - row * CH;
        const int m = m0 + row, n = n0 + c * 8;
        float f[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] = (float)sv[pass][e] + bb[pass][e >> 2][e & 3];
        if (has_res) {
#pragma unroll
            for (int e = 0; e < 8; ++e) f[e] += (float)lres[pass][e];
        }
        f16x8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (f16)f[e];
        if (m < p.M && n < p.N) *reinterpret_cast<f16x8*>(p.out + (size_t)m * p.out_ld + n) = o;
    }
}

// SEG: the A operand is K-segmented -- K tiles [0, c1 / 64) come from `a` (row stride c1), the rest from `a2` (row stride c2), both
// row-major; c1 % 64 == 0 and c2 % 64 == 0, so a K tile never straddles the sources (mdx_dense_takes_desc).  The source of a K tile
// is block-uniform: a scalar branch picks (descriptor, the lane offsets computed once per launch, scalar K offset) and the issue of
// a K tile stays AJ + BJ DMA instructions.  The weight side does not change: packed weights are K-tile-major over the concatenated K,
// which is also the order the generic kernel walks the two sources in (bit-identical to it).  SEG = false is the one-source kernel,
// instruction for instruction what it was (dense_kernel; the SEG form is dense_seg_kernel: dense_body.inc, included twice).
#define MDX_DENSE_SEG 0
#include "dense_body.inc"
#undef MDX_DENSE_SEG
#define MDX_DENSE_SEG 1
#include "dense_body.inc"
#undef MDX_DENSE_SEG

template <int BM, int BN, int NS, int PF, bool SEG = false>
void launch_dense_one(const GemmParams& p, dim3 grid, hipStream_t st) {
    constexpr size_t ring = (size_t)NS * (BM + BN) * 64 * 2;
    constexpr size_t epi = (size_t)(BM > BN ? BM : BN) * ((BM > BN ? BN : BM) + 8) * 2 + 4096;
    constexpr size_t lds = ring > epi ? ring : epi;
    static MdxPerDeviceOnce attr_once;
    if constexpr (SEG) {
        if (attr_once.first())
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&dense_seg_kernel<BM, BN, NS, PF>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL((dense_seg_kernel<BM, BN, NS, PF>), grid, dim3(256), lds, st, p);
    } else {
        if (attr_once.first())
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&dense_kernel<BM, BN, NS, PF>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL((dense_kernel<BM, BN, NS, PF>), grid, dim3(256), lds, st, p);
    }
}

// the cross-attention-epilogue instantiations (BN = 64, prefetch level 1): LDS = ring | staged q + LayerNorm extras + two K / V^T tile pairs
template <int BM, int NS>
void launch_dense_xa(const GemmParams& p, dim3 grid, hipStream_t st) {
    constexpr size_t ring = (size_t)NS * (BM + 64) * 64 * 2;
    constexpr size_t xa = (size_t)((BM * 72 * 2 + 2 * BM * 4 + 64 * 4 + 1023) / 1024) * 1024 + 2 * 16384;
    constexpr size_t lds = ring > xa ? ring : xa;
    static MdxPerDeviceOnce attr_once;
    if (attr_once.first())
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&dense_kernel<BM, 64, NS, 1, true>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL((dense_kernel<BM, 64, NS, 1, true>), grid, dim3(256), lds, st, p);
}

template <int BM, int BN, int NS, bool SEG = false>
void launch_dense_pf(const GemmParams& p, int pf, dim3 grid, hipStream_t st) {
    if constexpr (SEG) {      // the K-segmented form is built at prefetch levels 0 | 1 (the deeper levels are experiments of the one-source form)
        if (pf >= 1) return launch_dense_one<BM, BN, NS, 1, true>(p, grid, st);
        return launch_dense_one<BM, BN, NS, 0, true>(p, grid, st);
    }
    if constexpr (BM * BN < 128 * 128) {      // (128 x 128 tiles: the prefetch registers do not fit beside 64 accumulators)
        if (pf >= 3) return launch_dense_one<BM, BN, NS, 3>(p, grid, st);
        if (pf == 2) return launch_dense_one<BM, BN, NS, 2>(p, grid, st);
    }
    if (pf >= 1) return launch_dense_one<BM, BN, NS, 1>(p, grid, st);
    launch_dense_one<BM, BN, NS, 0>(p, grid, st);
}

template <int BM, int BN, bool SEG = false>
bool launch_dense_ns(const GemmParams& p, int ns, int pf, dim3 grid, hipStream_t st) {
    switch (ns) {
        case 2: launch_dense_pf<BM, BN, 2, SEG>(p, pf, grid, st); return true;
        case 3: launch_dense_pf<BM, BN, 3, SEG>(p, pf, grid, st); return true;
        case 4: if constexpr (BM == 64 || BN == 64) { launch_dense_pf<BM, BN, 4, SEG>(p, pf, grid, st); return true; } return false;
        case 5: if constexpr (BM == 64) { launch_dense_pf<BM, BN, 5, SEG>(p, pf, grid, st); return true; } return false;
        case 6: if constexpr (BM == 64) { launch_dense_pf<BM, BN, 6, SEG>(p, pf, grid, st); return true; } return false;
        default: return false;
    }
}

}  // namespace

// THE statement of which launches this kernel takes (gemm_internal.h), in two steps; plan_gemm and the tile-table lookup ask nobody
// else.  Step one, the descriptor alone -- what the tile-table lookup can know: dense (ksize 1, stride 1, one source or two whose K
// tiles are whole 64-channel chunks of ONE source), row-major, plain / GEGLU epilogue, no per-sample row bias, no out_bs, not the GroupNorm-on-A form.
bool mdx_dense_takes_desc(const GemmParams& p, int bn) {
    if (!mdx_opt(MDX_OPT_GEMM_LEAN_DENSE) || !p.dense_issue) return false;
    if (!(p.ksize == 1 && p.stride == 1 && !p.upsample && p.cin % 64 == 0 && p.out_mode == MDX_OUT_ROWMAJOR)) return false;
    if (p.c2 != 0) {
        // K-segmented A (dense_kernel SEG): whole 64-channel K tiles per source; plain epilogue with bias / residual / row statistics /
        // column statistics, unsplit or the in-kernel reduce; not on the 128 x 160 tile, no split store, no LayerNorm fold, no
        // cross-attention epilogue
        if (p.c1 % 64 != 0 || p.c2 % 64 != 0 || bn == 160) return false;
        if (p.epilogue != MDX_EPI_NONE || p.n_split || p.ln_stats || p.xa_k) return false;
    }
    if (p.gn_cs || p.rowbias || p.out_bs || p.skip_w || p.d2s_c) return false;
    if (p.epilogue != MDX_EPI_NONE && p.epilogue != MDX_EPI_GEGLU) return false;
    if (p.xa_k && bn != 64) return false;      // cross-attention epilogue: one head per 64-column tile
    if (bn == 160) {
        // four waves 4 x 1 (epilogue_w41): bias / residual / GEGLU packed at 80 / LayerNorm-fold consumer; no statistics, no split
        // store, no cross-attention
        if (p.stats_out || p.colstats_out || p.n_split || p.xa_k) return false;
        if (p.epilogue == MDX_EPI_GEGLU && p.geglu_unit != 80) return false;
    }
    return true;
}

// Step two, the planned launch: through the staged epilogue (unsplit or in-kernel reduce; the 160 tile unsplit only), four waves, a
// (tile, ring depth) that is built (launch_dense_ns / launch_dense_xa), offsets and tile ids that fit.
bool mdx_dense_takes(const GemmParams& p, int bm, int bn, int ring, int nsplit, bool fixup, bool nw8) {
    if (!mdx_dense_takes_desc(p, bn)) return false;
    if (!(nsplit == 1 || (fixup && bn != 160)) || nw8) return false;
    int built = (bm == 64 && (bn == 64 || bn == 128)) ? 6 : (bm == 128 && bn == 64) ? 4 : (bm == 128 && (bn == 128 || bn == 160)) ? 3 : 0;
    if (p.xa_k) built = std::min(built, 4);
    if (ring < 2 || ring > built) return false;
    // buffer descriptors of the epilogue prefetches: 32-bit offsets
    if ((size_t)p.M * (size_t)(p.residual ? p.residual_ld : 0) * 2 >= 0x80000000ull) return false;
    if (p.ln_stats && (size_t)p.M * (size_t)p.ln_nt * 8 >= 0x80000000ull) return false;
    // tile ids must fit the multiply-high decode
    return (long)((p.M + bm - 1) / bm) * ((p.N + bn - 1) / bn) < 65536;
}

// pl.grid is the generic kernel's; the SPREAD order becomes a 2-D grid (tiles, splits) here.
// Option gemm_lean_dense: 1 = prefetch level 1 (the product), 2 = level 0, 3 / 4 = levels 2 / 3 on launches of at most two blocks
// per CU (beyond that the register-hungry levels would take a block per CU away: level 1).
int mdx_dense_launch(const GemmParams& p, const GemmPlan& pl, hipStream_t st) {
    const int bm = pl.bm, bn = pl.bn, ns = pl.ring;
    const dim3 g = p.spread ? dim3((unsigned)(p.tiles_m * p.tiles_n), (unsigned)p.nsplit) : pl.grid;
    const int opt = mdx_opt(MDX_OPT_GEMM_LEAN_DENSE);
    const bool small = (long)g.x * g.y <= 512;
    const int pf = opt == 2 ? 0 : (opt == 3 && small ? 2 : (opt == 4 && small ? 3 : 1));
    bool ok = false;
    if (pl.form == GEMM_LEAN_XA) {
        ok = bn == 64 && ns >= 2 && ns <= 4 && (bm == 64 || bm == 128);
        if (ok && bm == 64) { if (ns == 2) launch_dense_xa<64, 2>(p, g, st); else if (ns == 3) launch_dense_xa<64, 3>(p, g, st); else launch_dense_xa<64, 4>(p, g, st); }
        if (ok && bm == 128) { if (ns == 2) launch_dense_xa<128, 2>(p, g, st); else if (ns == 3) launch_dense_xa<128, 3>(p, g, st); else launch_dense_xa<128, 4>(p, g, st); }
    }
    else if (p.c2 != 0) {
        if (bm == 64 && bn == 64) ok = launch_dense_ns<64, 64, true>(p, ns, pf, g, st);
        else if (bm == 64 && bn == 128) ok = launch_dense_ns<64, 128, true>(p, ns, pf, g, st);
        else if (bm == 128 && bn == 64) ok = launch_dense_ns<128, 64, true>(p, ns, pf, g, st);
        else if (bm == 128 && bn == 128) ok = launch_dense_ns<128, 128, true>(p, ns, pf, g, st);
    }
    else if (bm == 64 && bn == 64) ok = launch_dense_ns<64, 64>(p, ns, pf, g, st);
    else if (bm == 64 && bn == 128) ok = launch_dense_ns<64, 128>(p, ns, pf, g, st);
    else if (bm == 128 && bn == 64) ok = launch_dense_ns<128, 64>(p, ns, pf, g, st);
    else if (bm == 128 && bn == 128) ok = launch_dense_ns<128, 128>(p, ns, pf, g, st);
    else if (bm == 128 && bn == 160) ok = launch_dense_ns<128, 160>(p, ns, pf, g, st);
    MDX_REQUIRE(ok, "mdx_gemm_f16: internal error: the plan names a lean dense tile %d x %d at ring depth %d that is not built", bm, bn, ns);
    return MDX_OK;
}
