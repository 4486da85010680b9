// Implicit-GEMM conv3x3 / conv1x1 / Dense for gfx950 (MI355X).
//
//   out[m][n] = sum_k A[m][k] * W[n][k]      m = (b,yo,xo), k = (tap,cin), NHWC fp16, fp32 accumulate
//
// Replaces the reference's nn.Conv2d / nn.Dense call sites (include/mdx.h cites them).
//
// Design (MI355X-first):
//  * gemm_kernel: 256 threads = 4 wave64 (2x2), block tile {128,64} x {128,64}, BK = 64, MFMA 32x32x16 f16.
//    conv3x3_halo_kernel: stride-1 3x3 convs on 8x16-pixel patches whose 10x18 halo is DMA'd once per 64-channel
//    chunk and serves all nine taps (6x fewer activation bytes through the DMA path).
//  * Both operand tiles go HBM -> LDS with `buffer_load_dwordx4 ... lds` (16 B per lane, no VGPR
//    round trip).  The im2col gather, zero padding, stride-2, nearest-2x upsample and the
//    two-source channel concat are all folded into the per-lane SOURCE offset; out-of-range
//    offsets rely on the buffer descriptor's bounds check returning zeros.
//  * LDS image is lane-linear per DMA (8 rows x 128 B); the bank-conflict XOR swizzle
//    (chunk ^= (row>>1)&7; halo: keyed on the halo column) is applied on the source side and again on the
//    ds_read_b128 side.  Weights are stored tile-major and pre-swizzled so each DMA reads 1 KiB contiguous.
//  * 2-6 stage LDS ring, counted `s_waitcnt vmcnt(N)` + raw `s_barrier` (DMAs stay in flight across the
//    barrier); per K tile: ring-refill DMA issue, then the tile's fragment reads pinned with sched_barriers, then the MFMAs
//    (round 5); dense launches issue through the DMA's scalar offset; XCD-aware tile order; kernel arguments warmed at entry.
//  * Epilogue is staged through LDS so that global stores are full 16-B / 128-B-row coalesced;
//    bias (fetched before the K loop), per-sample time-embedding bias, residual add, GEGLU / GELU / QuickGELU, the
//    transposed (V^T) store and the split q|k row-major + V^T output are fused there.
//  * split-K = fp32 slabs + a fused reduce/epilogue kernel (fixed slab order: deterministic), or the in-kernel reduce.
//
// This file holds the kernels, the launch_* templates that instantiate them and mdx_gemm_launch_plan, which launches a filled
// GemmPlan.  What a descriptor launches -- tile, split, kernel form, ring depth, grid -- is decided in gemm_plan.hip (plan_gemm),
// which also holds descriptor validation, the tile tables and the public entry points.
#include "mdx_common.h"
#include "gemm_internal.h"

#include <algorithm>
#include <type_traits>

namespace {


// GNA (dense launches, ksize 1): nn.GroupNorm(32) of the INPUT -- no activation: SpatialTransformer.norm -> proj_in (attention.py:
// 243-247), GLIDE's AttentionBlock.norm -> qkv -- applied to the A fragments on their way from LDS to the matrix pipe.  GroupNorm
// without an activation is affine per (sample, channel): x' = a[b][k] x + s[b][k], a = gamma rstd, s = beta - mean a.  The block
// folds its sample's column partials (the producer's colstats_out, exactly as the HALO conv does below) into two fp16 tables in LDS
// and every A fragment becomes ONE packed fma per two halves (v_pk_fma_f16, single rounding) right after its ds_read: the
// normalised tensor is never written or read, and the GroupNorm launch disappears.  An M tile lies inside one sample
// (tokens per sample %% BM == 0, checked on the host).
// EXT: the instantiations that carry the SRGAN epilogues (MDX_EPI_PRELU, MDX_OUT_D2S2; launch_ext) -- kept apart so that the
// register allocation of the instantiations every other launch uses does not pay for them.
template <int BM, int BN, int BK, int NS, bool SWAP, bool FASTK, int NW, bool GNA = false, bool EXT = false>
__global__ __launch_bounds__(NW * 64, NW == 4 ? 2 : 1) void gemm_kernel(const GemmParams p) {
    // NW = 4 (2 x 2 waves) or 8 (4 x 2 waves, BM = 128 only).  The 8-wave form is for grids of at most one block per
    // CU: a wave's K-step is a serial chain (wait -> barrier -> DMA issue -> ds_read -> MFMA), so a lone 4-wave block
    // leaves each SIMD idle for most of it; eight waves halve every wave's share of the DMA issue and MFMAs and give
    // each SIMD a second wave to overlap with.
    mdx_kernarg_touch<sizeof(GemmParams)>();
    constexpr int WROWS = BM / (NW / 2);    // rows per wave row
    constexpr int TM = WROWS / 32;          // 32-row MFMA tiles per wave along m
    constexpr int TN = BN / 64;             // 32-wide MFMA tiles per wave along n
    static_assert(TM >= 1, "tile too short for this many waves");
    constexpr int ROWB = BK * 2;            // bytes per LDS row (128 | 64)
    constexpr int CPRW = BK / 8;            // 16-B chunks per row (8 | 4)
    constexpr int RPI = 64 / CPRW;          // rows covered by one wave-wide DMA instruction (8 | 16)
    constexpr int RP256 = 256 / ROWB;       // rows per 256-B LDS bank row (2 | 4): swizzle key = (row / RP256) % CPRW
    constexpr int KS = BK / 16;             // MFMA k-steps per K tile
    constexpr int A_BYTES = BM * ROWB;
    constexpr int B_BYTES = BN * ROWB;
    constexpr int STAGE = A_BYTES + B_BYTES;
    constexpr int AJ = BM / RPI / NW;       // A-tile DMA instructions per wave
    constexpr int BJ = BN / RPI / NW;       // B-tile DMA instructions per wave
    static_assert(AJ >= 1 && BJ >= 1, "tile too small for this many loader waves");
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int hi = lane >> 5;
    const int l31 = lane & 31;

    // XCD-aware tile order: the dispatcher places block b on XCD b % 8 (per-XCD L2s are private), so give every
    // XCD a CONTIGUOUS run of tile ids; ids run fastest along the dimension that shares the bigger operand.
    // SPREAD order (one row of M tiles, i.e. no two blocks share a weight tile): consecutive block ids -- consecutive
    // XCDs -- take consecutive (tile, split) items, so the weight stream is pulled through all 8 XCDs' fabric links
    // even when there are only 10 N tiles (the contiguous order would park them on 5 XCDs and leave 3 idle).
    const int ntiles = p.tiles_m * p.tiles_n;
    const int tile_id = p.spread ? (int)(blockIdx.x % (unsigned)ntiles) : (blockIdx.x & 7) * p.tiles_per_xcd + (blockIdx.x >> 3);
    if (tile_id >= ntiles) return;
    trace_mark(p, 0);
    int tile_m, tile_n;
    if (p.n_fastest) {
        tile_m = tile_id / p.tiles_n;
        tile_n = tile_id - tile_m * p.tiles_n;
    } else {
        tile_n = tile_id / p.tiles_m;
        tile_m = tile_id - tile_n * p.tiles_m;
    }
    const int m0 = tile_m * BM, n0 = tile_n * BN;
    const int split = p.spread ? (int)(blockIdx.x / (unsigned)ntiles) : (int)blockIdx.y;
    const int kt_begin = split * p.ktiles_per_split;
    const int kt_end = min(p.ktiles, kt_begin + p.ktiles_per_split);

    const __amdgpu_buffer_rsrc_t rs_a = make_rsrc(p.a, p.a_bytes);
    const __amdgpu_buffer_rsrc_t rs_a2 = make_rsrc(p.a2 ? p.a2 : p.a, p.a2 ? p.a2_bytes : p.a_bytes);
    const __amdgpu_buffer_rsrc_t rs_w = make_rsrc(p.w, p.w_bytes);

    // ---- loader coordinates (fixed per thread across K tiles)
    // DMA instruction j of a wave covers rows (wave*AJ + j)*RPI .. +RPI-1; lane -> row + lane/CPRW, physical chunk lane%CPRW
    const int lrow = lane / CPRW, lchk = lane % CPRW;
    int a_pix[AJ];            // pixel index of tap (0,0): (b*H + y0)*W + x0 (may lie outside the image)
    int a_y[AJ], a_x[AJ];     // y0, x0 (source coordinates of tap (0,0); upsampled coordinates when p.upsample)
    int a_b[AJ];              // b*H*W
    unsigned a_cb[AJ];        // byte offset of this lane's logical chunk inside a row
    unsigned a_mask[AJ];      // bit t set <=> tap t is inside the image for this row (and the row exists)
    const int Hs = p.upsample ? 2 * p.H : p.H;  // extent the taps are clipped against
    const int Ws = p.upsample ? 2 * p.W : p.W;
#pragma unroll
    for (int j = 0; j < AJ; ++j) {
        const int row = (wave * AJ + j) * RPI + lrow;
        const int m = m0 + row;
        const bool okm = m < p.M;
        a_cb[j] = (unsigned)((lchk ^ ((row / RP256) % CPRW)) * 16);
        if (p.ksize == 1 && p.stride == 1 && !p.upsample) {
            // Dense / 1x1 conv (most launches): the source pixel IS the output row -- skip the (b, y, x) divisions
            a_y[j] = a_x[j] = 0;
            a_pix[j] = a_b[j] = okm ? m : 0;
            a_mask[j] = okm ? 1u : 0u;
            continue;
        }
        const int mm = okm ? m : 0;
        const int b = mm / p.HoWo;
        const int rem = mm - b * p.HoWo;
        const int yo = rem / p.Wo;
        const int xo = rem - yo * p.Wo;
        a_b[j] = b * p.H * p.W;
        a_y[j] = yo * p.stride - p.pad;
        a_x[j] = xo * p.stride - p.pad;
        a_pix[j] = a_b[j] + a_y[j] * p.W + a_x[j];
        unsigned mk = 0;
        for (int t = 0; t < p.ksize * p.ksize; ++t) {
            const int ky = (p.ksize == 3) ? t / 3 : 0, kx = (p.ksize == 3) ? t - ky * 3 : 0;
            const int yi = a_y[j] + ky, xi = a_x[j] + kx;
            if (okm && yi >= 0 && yi < Hs && xi >= 0 && xi < Ws) mk |= 1u << t;
        }
        a_mask[j] = mk;
    }
    // B (weights): stored tile-major and PRE-SWIZZLED on the host -- [N/64 panels][K/64 tiles][64 rows][8 chunks][8]
    // with chunk position q holding logical chunk q ^ ((row>>1)&7) -- so every DMA instruction reads 1 KiB of
    // CONTIGUOUS memory (no L2 channel camping on the K*2-byte row stride, sequential HBM streaming along K).
    static_assert(BK == 64, "weight storage is tiled for BK = 64");
    unsigned b_off[BJ];  // byte offset of this lane's 16 B inside K tile 0
#pragma unroll
    for (int j = 0; j < BJ; ++j) {
        const int row = (wave * BJ + j) * RPI + lrow;   // 0 .. BN-1
        const int panel = (n0 >> 6) + (row >> 6);
        b_off[j] = (unsigned)(((size_t)panel * p.kt64) * 8192 + ((row & 63) * 8 + lchk) * 16);
    }

    // Dense launches (ksize 1, stride 1, no upsample, one source: every token GEMM and 1x1 conv -- two thirds of the launches of a
    // UNet evaluation): the source offset of a K tile is the lane's row offset + kt * 128 bytes.  The lane part is fixed for the
    // whole launch and the K part is UNIFORM, so it rides in the DMA instruction's scalar offset: issuing a K tile is AJ + BJ
    // instructions and their m0 moves, instead of the tap / source decode (~45 scalar instructions: a division by the tap count)
    // plus ~10 instructions per DMA.  A block that has a SIMD to itself issues one instruction per ~4 clocks, and its K step
    // (~190 instructions at 64 x 64) was issue-bound as much as DMA-bound (round 5).
    const bool dense = FASTK && p.ksize == 1 && p.stride == 1 && !p.upsample && p.c2 == 0 && p.dense_issue;
    unsigned a_voff[AJ];
#pragma unroll
    for (int j = 0; j < AJ; ++j)
        a_voff[j] = (a_mask[j] & 1u) ? (unsigned)(a_pix[j] * (p.c1 * 2)) + a_cb[j] : MDX_OOB;

    auto stage_tile = [&](int kt, int buf) {
        char* sbase = smem + buf * STAGE;
        const int k0 = kt * BK;
        if (dense) {
#pragma unroll
            for (int j = 0; j < AJ; ++j) dma16s(rs_a, sbase + (wave * AJ + j) * 1024, a_voff[j], (unsigned)k0 * 2u);
#pragma unroll
            for (int j = 0; j < BJ; ++j) dma16s(rs_w, sbase + A_BYTES + (wave * BJ + j) * 1024, b_off[j], (unsigned)kt * 8192u);
            return;
        }
        if constexpr (FASTK) {
            // K is ordered [cin chunk of 64][tap][64] (weights packed to match; Cin % 64 == 0, c1 % 64 == 0), so a K
            // tile lies in one tap and one source, and consecutive K tiles re-read the SAME pixels' cache lines
            // shifted by one tap: the 9x im2col re-read of the activations is served by L2, not by the fabric.
            const int taps = p.ksize * p.ksize;
            const int g = k0 >> 6;
            const int chunk = g / taps;
            const int tap = g - chunk * taps;
            int ci0 = chunk * 64 + (k0 & 63);
            const int ky = (p.ksize == 3) ? tap / 3 : 0;
            const int kx = (p.ksize == 3) ? tap - ky * 3 : 0;
            const bool second = ci0 >= p.c1;
            const int cs2 = (second ? p.c2 : p.c1) * 2;
            if (second) ci0 -= p.c1;
            if (!p.upsample) {
                const int dpix = ky * p.W + kx;
#pragma unroll
                for (int j = 0; j < AJ; ++j) {
                    const unsigned off = ((a_mask[j] >> tap) & 1u)
                                             ? (unsigned)((a_pix[j] + dpix) * cs2) + (unsigned)(ci0 * 2) + a_cb[j]
                                             : MDX_OOB;
                    void* dst = sbase + (wave * AJ + j) * 1024;
                    if (second)
                        dma16(rs_a2, dst, off);
                    else
                        dma16(rs_a, dst, off);
                }
            } else {
#pragma unroll
                for (int j = 0; j < AJ; ++j) {
                    const int yi = (a_y[j] + ky) >> 1, xi = (a_x[j] + kx) >> 1;
                    const unsigned off = ((a_mask[j] >> tap) & 1u)
                                             ? (unsigned)((a_b[j] + yi * p.W + xi) * cs2) + (unsigned)(ci0 * 2) + a_cb[j]
                                             : MDX_OOB;
                    void* dst = sbase + (wave * AJ + j) * 1024;
                    if (second)
                        dma16(rs_a2, dst, off);
                    else
                        dma16(rs_a, dst, off);
                }
            }
        } else {
            // generic: tap-major K, per-lane tap decode (single source only; conv_in with Cin = 8)
#pragma unroll
            for (int j = 0; j < AJ; ++j) {
                const int kk = k0 + (int)(a_cb[j] >> 1);
                const int tap = kk / p.cin;
                const int ci = kk - tap * p.cin;
                const int ky = (p.ksize == 3) ? tap / 3 : 0;
                const int kx = (p.ksize == 3) ? tap - ky * 3 : 0;
                int yi = a_y[j] + ky, xi = a_x[j] + kx;
                const bool ok = kk < p.K && ((a_mask[j] >> tap) & 1u);
                if (p.upsample) {
                    yi >>= 1;
                    xi >>= 1;
                }
                const unsigned off = ok ? (unsigned)(((size_t)(a_b[j] + yi * p.W + xi) * p.cin + ci) * 2) : MDX_OOB;
                dma16(rs_a, sbase + (wave * AJ + j) * 1024, off);
            }
        }
#pragma unroll
        for (int j = 0; j < BJ; ++j) dma16s(rs_w, sbase + A_BYTES + (wave * BJ + j) * 1024, b_off[j], (unsigned)kt * 8192u);
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // fragment read offsets: row*ROWB + ((2s+hi) ^ key(row))*16; key(row) depends only on the lane for all our row bases
    const int swz = (l31 / RP256) % CPRW;
    const int a_row_off = (wm * WROWS + l31) * ROWB;
    const int b_row_off = A_BYTES + (wn * (BN / 2) + l31) * ROWB;

    // ---- main loop: NS-stage LDS ring.  DMAs of the next NS-1 K tiles stay in flight ACROSS the per-tile barrier
    // (counted s_waitcnt vmcnt + raw s_barrier: __syncthreads() would drain them), fragments for k-step s+1 are
    // fetched from LDS while the MFMAs of k-step s run.
    //   iteration t:  wait(tile t landed for this wave) -> s_barrier (=> landed for all waves, and every wave is
    //                 done reading stage (t-1)%NS) -> issue tile t+NS-1 into stage (t-1)%NS -> compute tile t.
    constexpr int LPT = AJ + BJ;  // DMA instructions per wave per K tile
    const int nt = kt_end - kt_begin;
    float bpre[16];
    gemm_bias_prefetch<BN, SWAP, NW>(p, n0, bpre);
    // LayerNorm-fold consumer (round 5): the epilogue opens with the tile's row statistics (BM x K / 64 {sum, sumsq} pairs, written by
    // the previous launch on other XCDs) and S[n] (a weight-like vector, cold in HBM): 2-3 us of misses at the head of the epilogue of
    // every q|k|v, cross-attention q and GEGLU ff1 launch, which one block per CU cannot hide.  Each thread TOUCHES one 128-byte line
    // of them here, ahead of the prologue DMAs (older in the vmcnt order: the counted waits of the main loop cover them), so that
    // the epilogue's own loads hit this XCD's L2.  Two VGPRs, kept live to the epilogue so that the loads are not sunk; the values
    // are not used -- the arithmetic is the epilogue's, unchanged.
    [[maybe_unused]] float touch_ln = 0.f, touch_s = 0.f;
    if constexpr (SWAP) {
        if (p.ln_stats != nullptr && p.ln_prefetch) {
            const int rows = min(BM, p.M - m0);
            const unsigned bytes = (unsigned)rows * (unsigned)p.ln_nt * 8u;
            const char* base = reinterpret_cast<const char*>(p.ln_stats) + (size_t)m0 * p.ln_nt * 8;
            // (one line per thread covers BM x K / 64 pairs up to K = 2048; beyond that the rest stays cold.  No loop, no add: a
            // dependent instruction here would make the compiler wait for the miss in front of the prologue)
            if ((unsigned)tid * 128u < bytes) touch_ln = *reinterpret_cast<const float*>(base + (unsigned)tid * 128u);
            if (tid < BN / 32 && n0 + tid * 32 < p.N) touch_s = p.ln_s[n0 + tid * 32];
        }
    }
#pragma unroll
    for (int i = 0; i < NS - 1; ++i)
        if (i < nt) stage_tile(kt_begin + i, i);
    // GNA tables live behind everything the ring and the epilogue staging use: [cin] a, [cin] s (fp16), [cin] {sum, sumsq} scratch
    constexpr size_t GNA_RING = (size_t)NS * (BM + BN) * BK * 2;
    constexpr size_t GNA_EPI = (size_t)(BM > BN ? BM : BN) * ((BM > BN ? BN : BM) + 8) * 2 + 4096;
    constexpr size_t GNA_BASE = GNA_RING > GNA_EPI ? GNA_RING : GNA_EPI;
    [[maybe_unused]] const f16* gta = reinterpret_cast<const f16*>(smem + GNA_BASE);
    [[maybe_unused]] const f16* gts = gta + p.cin;
    if constexpr (GNA) {
        // (the prologue DMAs above are already in flight: the fold's global round trip overlaps them)
        f16* wa = reinterpret_cast<f16*>(smem + GNA_BASE);
        f16* wsft = wa + p.cin;
        float2* csum = reinterpret_cast<float2*>(wsft + p.cin);
        const int pb = m0 / p.HoWo;
        const int cpg = p.cin >> 5;
        const float2* src = reinterpret_cast<const float2*>(p.gn_cs) + (size_t)pb * p.gn_nrb * p.cin;
        // gamma / beta of this thread's channels first: they are cold in HBM (weights stream through the caches between two uses),
        // and fetched here their miss overlaps the partials' round trip instead of following it
        constexpr int GNA_CPT = 2560 / (NW * 64);      // channels per thread at the largest Cin
        float gg[GNA_CPT], gb[GNA_CPT];
#pragma unroll
        for (int i = 0; i < GNA_CPT; ++i) {
            const int c = tid + i * NW * 64;
            gg[i] = c < p.cin ? p.gn_gamma[c] : 0.f;
            gb[i] = c < p.cin ? p.gn_beta[c] : 0.f;
        }
        for (int c = tid; c < p.cin; c += NW * 64) {
            float su = 0.f, sq = 0.f;
            int k = 0;
            for (; k + 8 <= p.gn_nrb; k += 8) {
                float2 v[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = src[(size_t)(k + e) * p.cin + c];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    su += v[e].x;
                    sq += v[e].y;
                }
            }
            for (; k < p.gn_nrb; ++k) {
                const float2 v = src[(size_t)k * p.cin + c];
                su += v.x;
                sq += v.y;
            }
            csum[c] = make_float2(su, sq);
        }
        __syncthreads();
        const float inv = 1.0f / ((float)cpg * (float)p.HoWo);
#pragma unroll
        for (int i = 0; i < GNA_CPT; ++i) {
            const int c = tid + i * NW * 64;
            if (c < p.cin) {
                const int g = c / cpg;
                float su = 0.f, sq = 0.f;
                for (int e = 0; e < cpg; ++e) {
                    const float2 v = csum[g * cpg + e];
                    su += v.x;
                    sq += v.y;
                }
                const float mean = su * inv;
                float var = sq * inv - mean * mean;
                var = var < 0.f ? 0.f : var;
                const float a = gg[i] * rsqrtf(var + p.gn_eps);
                wa[c] = (f16)a;
                wsft[c] = (f16)(gb[i] - mean * a);
            }
        }
        __syncthreads();
    }
    int rd = 0;            // stage holding tile t
    int wr = NS - 1;       // stage that tile t+NS-1 goes to
    trace_mark(p, 1);
    for (int t = 0; t < nt; ++t) {
        // tiles t .. min(t+NS-2, nt-1) are outstanding; allow all but the oldest to stay in flight
        const int ahead = min(NS - 2, nt - 1 - t);
        if (NS >= 6 && ahead >= 4)
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(4 * LPT) : "memory");
        else if (NS >= 5 && ahead == 3)
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(3 * LPT) : "memory");
        else if (NS >= 4 && ahead == 2)
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * LPT) : "memory");
        else if (NS >= 3 && ahead == 1)
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(LPT) : "memory");
        else
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if (t == 0) trace_mark(p, 2);
        // Order inside a K tile (round 5).  A block that has its SIMDs to itself -- nearly every launch at UNet batch 2 -- runs the
        // chain wait -> barrier -> DMA issue -> ds_read -> MFMA serially, one instruction per ~3 ns, and the ISA of round 4 showed
        // the machine scheduler sinking every fragment read to its use: each MFMA waited for a ds_read issued right before it, KS
        // LDS round trips per K tile with nothing to hide them.  Now: (i) the ring-refill DMAs are issued FIRST (the operand
        // stream is latency x ring-depth bound: with the reads in front of the issue the convs lost 10-35 %), (ii) then the
        // fragment reads of the tile -- of ALL KS k-steps on tiles with at most two MFMAs per k-step, which have nothing to hide a
        // read behind; a double buffer on 128 x 128 -- pinned where they are written by sched_barriers, (iii) then the MFMAs.
        const char* sb = smem + rd * STAGE;
        constexpr bool ALLK = (TM * TN <= 2) && !GNA;
        constexpr int FD = ALLK ? KS : 2;
        static_assert(KS == 4, "64-deep K tiles");
        f16x8 af[FD][TM], bf[FD][TN];
        [[maybe_unused]] f16x8 gna[2], gns[2];      // GNA: this lane's 8 channels' {a, s} of k-step s (channel = K index: dense launch)
        [[maybe_unused]] const int gk = (kt_begin + t) * BK + hi * 8;
        auto rdfrag = [&](auto slot_c, const int ks) {
            constexpr int slot = decltype(slot_c)::value;
            const int coff = (((2 * ks + hi) ^ swz) << 4);
#pragma unroll
            for (int i = 0; i < TM; ++i) af[slot][i] = *reinterpret_cast<const f16x8*>(sb + a_row_off + i * 32 * ROWB + coff);
#pragma unroll
            for (int j = 0; j < TN; ++j) bf[slot][j] = *reinterpret_cast<const f16x8*>(sb + b_row_off + j * 32 * ROWB + coff);
            if constexpr (GNA) {
                gna[slot & 1] = *reinterpret_cast<const f16x8*>(gta + gk + 16 * ks);
                gns[slot & 1] = *reinterpret_cast<const f16x8*>(gts + gk + 16 * ks);
            }
        };
        auto mfmas = [&](auto slot_c) {
            constexpr int slot = decltype(slot_c)::value;
            if constexpr (GNA) {
#pragma unroll
                for (int i = 0; i < TM; ++i) af[slot][i] = af[slot][i] * gna[slot & 1] + gns[slot & 1];      // v_pk_fma_f16 x 4
            }
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    if constexpr (SWAP)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bf[slot][j], af[slot][i], acc[i][j], 0, 0, 0);
                    else
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[slot][i], bf[slot][j], acc[i][j], 0, 0, 0);
                }
        };
        using I0 = std::integral_constant<int, 0>;
        using I1 = std::integral_constant<int, 1>;
        const bool refill = t + NS - 1 < nt;
        if (refill) stage_tile(kt_begin + t + NS - 1, wr);
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (ALLK) {
            using I2 = std::integral_constant<int, 2>;
            using I3 = std::integral_constant<int, 3>;
            rdfrag(I0{}, 0); rdfrag(I1{}, 1); rdfrag(I2{}, 2); rdfrag(I3{}, 3);
            __builtin_amdgcn_sched_barrier(0);
            mfmas(I0{}); mfmas(I1{}); mfmas(I2{}); mfmas(I3{});
        } else {
            rdfrag(I0{}, 0);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int ks = 0; ks < KS; ks += 2) {
                rdfrag(I1{}, ks + 1);
                __builtin_amdgcn_sched_barrier(0);
                mfmas(I0{});
                __builtin_amdgcn_sched_barrier(0);
                if (ks + 2 < KS) {
                    rdfrag(I0{}, ks + 2);
                    __builtin_amdgcn_sched_barrier(0);
                }
                mfmas(I1{});
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        rd = (rd + 1 == NS) ? 0 : rd + 1;
        wr = (wr + 1 == NS) ? 0 : wr + 1;
    }

    __syncthreads();  // all waves done with the ring before the epilogue reuses it
    trace_mark(p, 3);
    if constexpr (SWAP) asm volatile("" ::"v"(touch_ln), "v"(touch_s));      // (the touches above stay loads issued up there)
    gemm_epilogue<BM, BN, SWAP, NW, LinearRows, 0, 0, EXT>(p, acc, smem, LinearRows{m0}, n0, split, bpre, tile_m, tile_id);
    trace_mark(p, 4);
}

// ---------------------------------------------------------------------------------------------------------------
// HALO conv kernel: 3x3, stride 1, pad 1, single source, Cin % 64 == 0, H % 8 == 0, W % 16 == 0.
//
// The generic kernel DMAs a fresh 128 x 64 activation tile for each of the 9 taps (L2 serves the re-read, but the
// per-CU DMA rate -- the measured limiter, profiles/r01_dma_probe.txt -- still pays 9x).  Here the M tile is an
// 8 x 16 PIXEL PATCH: for each 64-channel chunk the 10 x 18 halo (180 rows x 128 B, zero padding supplied by the
// buffer bounds check) is brought into LDS ONCE and the A fragments of all 9 taps are read from it at
// halo row (py+ky)*18 + (px+kx).  Activation DMA bytes drop 9 x 16 KiB -> 24 KiB per chunk (6x); with the weight
// tiles (unchanged, one per tap) total DMA bytes per chunk drop 288 -> 168 KiB (BN = 128), 216 -> 96 KiB (BN = 64).
//
// LDS: halo[2][192 rows][128 B] (double buffered across chunks; same XOR swizzle keyed by the halo row) followed by an
// NSB-stage ring of weight tiles.  The next chunk's halo is fetched one DMA instruction per wave per tap during
// taps 0..5 of the current chunk, so the DMA stream stays even.
//
// BM = 128: 8 x 16 patch, 4 waves (2 blocks per CU).  BM = 256: 16 x 16 patch, 8 waves (one block per CU): the halo grows
// 180 -> 324 rows for twice the pixels and every weight tile is shared by twice as many rows, so the DMA bytes per MAC --
// what bounds this kernel (about 60 GB/s per CU, 6 TB/s chip-wide through buffer_load..lds) -- drop by another 45 %.
//
// PW = 8 (BM = 128 only): the 8 x 8-pixel images of the deepest UNet level (64 x 64 latents: 16 of the 49 stride-1 convs,
// K = 11520 / 23040, M = 64 per sample).  An M tile is TWO WHOLE SAMPLES (2 x 64 pixels); each sample's 10 x 10 halo
// (zero padding from the buffer bounds check) sits in LDS once per 64-channel chunk: 200 halo rows instead of nine
// 128-row im2col tiles -- the activation share of the per-CU DMA stream (what bounds a lone block per CU,
// profiles/r01_dma_probe.txt) drops from 144 to 25 KiB per chunk, 288 -> 169 KiB in all at BN = 128.
//
// BDIR (weight-streaming form, for M <= 512 where every launch is bound by how fast it pulls cold weights): the weights are
// packed in MFMA-fragment order ([N / 32][K / 16][64 lanes][8], ops.pack_frag_weight) and go HBM/L2 -> VGPR directly, PFB
// pieces of 1 KiB in flight per wave and column tile -- no weight tiles in LDS, no weight DMA, and ONE barrier per 64-channel
// chunk (the halo swap) instead of one per tap.  With the LDS ring a block keeps two 8 KiB weight tiles in flight (32 KiB
// per CU: ~2 TB/s chip-wide at the HBM round trip); here 4 waves x 12 KiB x 2 blocks = 96 KiB per CU.  Same k order per
// output, same epilogue: bit-identical results.
// W4 (BDIR, 128 x 128 tiles, slab output only): the four waves sit side by side along N -- each owns 32 columns and ALL 128 rows --
// instead of 2 x 2.  In the 2 x 2 arrangement the two waves of a column pair fetch the same weight pieces, so half of the bytes
// a CU has in flight are duplicates; side by side every piece is fetched once (the A fragments, which come from LDS, are read
// by all four waves instead).
template <int BM, int BN, int NSB, bool SWAP, int PW, bool BDIR = false, bool W4 = false>
__global__ __launch_bounds__(BM * 2, BM == 128 ? 2 : 1) void conv3x3_halo_kernel(const GemmParams p) {
    static_assert(PW == 16 || (PW == 8 && BM == 128), "patch width 16, or 8 with two-sample tiles");
    static_assert(!W4 || (BDIR && BM == 128 && BN == 128 && !SWAP), "W4: weight-streaming 128 x 128 tiles with slab output");
    constexpr int NW = BM / 32;              // waves: (NW/2) x 2, each 64 patch pixels x BN/2 channels
    constexpr int PH = BM / 16;              // PW = 16: patch rows (8 | 16)
    constexpr int HWD = PW + 2;              // halo width in pixels (18 | 10)
    constexpr int WROWS = W4 ? BM : BM / (NW / 2);     // patch pixels per wave row (64; W4: all 128)
    constexpr int TM = WROWS / 32;
    constexpr int TN = W4 ? 1 : BN / 64;
    constexpr int HROWS = PW == 16 ? (PH + 2) * 18 : (BM / 64) * 100;   // halo pixels (180 | 324 | 200)
    constexpr int HINST = (HROWS + 7) / 8;   // halo DMA instructions per chunk (23 | 41)
    constexpr int HALO_BYTES = HINST * 1024;
    constexpr int HJ = (HINST + NW - 1) / NW;   // ... per wave (6 | 6)
    constexpr int B_BYTES = BN * 128;
    constexpr int BJ = BN / 8 / NW;
    static_assert(BJ >= 1, "weight tile too small for this many loader waves");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    mdx_kernarg_touch<sizeof(GemmParams)>();

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = W4 ? 0 : wave >> 1, wn = W4 ? wave : wave & 1;
    const int hi = lane >> 5;
    const int l31 = lane & 31;

    // SPREAD order (see gemm_kernel): a single row of M tiles deals its (tile, split) items round-robin to the XCDs
    const int ntiles = p.tiles_m * p.tiles_n;
    const int tile_id = p.spread ? (int)(blockIdx.x % (unsigned)ntiles) : (blockIdx.x & 7) * p.tiles_per_xcd + (blockIdx.x >> 3);
    if (tile_id >= ntiles) return;
    int tile_m, tile_n;
    if (p.n_fastest) {
        tile_m = tile_id / p.tiles_n;
        tile_n = tile_id - tile_m * p.tiles_n;
    } else {
        tile_n = tile_id / p.tiles_m;
        tile_m = tile_id - tile_n * p.tiles_m;
    }
    trace_mark(p, 0);
    const int n0 = tile_n * BN;
    // PW = 16: tile = one PH x 16 patch of sample pb.  PW = 8: tile = samples 2 * tile_m and 2 * tile_m + 1 (8 x 8 pixels each).
    const int pw = PW == 16 ? p.W >> 4 : 1, ph = PW == 16 ? p.H / PH : 1;
    const int pb = PW == 16 ? tile_m / (ph * pw) : tile_m * (BM / 64);
    const int prem = PW == 16 ? tile_m - pb * (ph * pw) : 0;
    const int py0 = (prem / pw) * PH, px0 = (prem % pw) * 16;
    const int split = p.spread ? (int)(blockIdx.x / (unsigned)ntiles) : (int)blockIdx.y;
    const int kt_begin = split * p.ktiles_per_split;            // multiples of 9 (host guarantees chunk-aligned splits)
    const int kt_end = min(p.ktiles, kt_begin + p.ktiles_per_split);
    const int nt = kt_end - kt_begin;
    const int c_begin = kt_begin / 9, c_end = kt_end / 9;

    const __amdgpu_buffer_rsrc_t rs_a = make_rsrc(p.a, p.a_bytes);
    const __amdgpu_buffer_rsrc_t rs_w = make_rsrc(p.w, p.w_bytes);

    // halo loader: DMA instruction q of this wave covers halo rows (wave*HJ + q)*8 .. +7, lane -> row + lane/8.
    // Swizzle: physical chunk = logical chunk ^ ((halo column >> 1) & 7).  A ds_read_b128 lane group reads 16 pixels
    // that span two patch rows (halo rows 18 apart) but 16 CONSECUTIVE columns, so keying on the column (not on the
    // linear halo row) puts them on 16 distinct 16-B slots of the 256-B bank row: conflict-free.
    const int lrow = lane >> 3, lchk = lane & 7;
    unsigned hal_off[HJ];
    const unsigned row_bytes = (unsigned)p.cin * 2;
#pragma unroll
    for (int q = 0; q < HJ; ++q) {
        const int hp = (wave * HJ + q) * 8 + lrow;
        if constexpr (PW == 16) {
            const int hr = hp / 18, hc = hp - hr * 18;
            const int y = py0 - 1 + hr, x = px0 - 1 + hc;
            const bool ok = hp < HROWS && y >= 0 && y < p.H && x >= 0 && x < p.W;
            hal_off[q] = ok ? (unsigned)((pb * p.H + y) * p.W + x) * row_bytes + (unsigned)((lchk ^ ((hc >> 1) & 7)) * 16)
                            : MDX_OOB;
        } else {
            // two 10 x 10 halos back to back.  Swizzle key = (halo column / 2) % 4 | (halo row % 2) << 2: a ds_read_b128
            // lane group covers four 4-pixel runs on four consecutive patch rows (8-wide rows), and this key sends its
            // eight even and eight odd halo pixels to eight distinct 16-B slots each (conflict-free, as for PW = 16)
            const int sm = hp / 100, r = hp - sm * 100;
            const int hr = r / 10, hc = r - hr * 10;
            const int y = hr - 1, x = hc - 1;
            const bool ok = hp < HROWS && pb + sm < p.B && y >= 0 && y < 8 && x >= 0 && x < 8;
            const int key = ((hc >> 1) & 3) | ((hr & 1) << 2);
            hal_off[q] = ok ? (unsigned)(((pb + sm) * 8 + y) * 8 + x) * row_bytes + (unsigned)((lchk ^ key) * 16) : MDX_OOB;
        }
    }
    unsigned b_off[BJ];
#pragma unroll
    for (int j = 0; j < BJ; ++j) {
        const int row = (wave * BJ + j) * 8 + lrow;
        const int panel = (n0 >> 6) + (row >> 6);
        b_off[j] = (unsigned)(((size_t)panel * p.kt64) * 8192 + ((row & 63) * 8 + lchk) * 16);
    }
    auto dma_halo = [&](int q, int chunk, int hb) {
        if (wave * HJ + q >= HINST) return;   // (wave-uniform) the last wave's spare slots lie beyond the halo image
        const unsigned off = hal_off[q] == MDX_OOB ? MDX_OOB : hal_off[q] + (unsigned)chunk * 128u;
        dma16(rs_a, smem + hb * HALO_BYTES + (wave * HJ + q) * 1024, off);
    };
    auto dma_b = [&](int kt, int stage) {
        char* sb = smem + 2 * HALO_BYTES + stage * B_BYTES;
#pragma unroll
        for (int j = 0; j < BJ; ++j) dma16s(rs_w, sb + (wave * BJ + j) * 1024, b_off[j], (unsigned)kt * 8192u);
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // fragment addressing: A rows are patch pixels q = wm*64 + i*32 + l31 -> halo row of tap (0,0) = (q>>4)*18 + (q&15)
    int hp0[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int q = wm * WROWS + i * 32 + l31;
        hp0[i] = PW == 16 ? (q >> 4) * 18 + (q & 15) : (q >> 6) * 100 + ((q >> 3) & 7) * 10 + (q & 7);
    }
    const int swz_b = (l31 >> 1) & 7;
    const int b_row_off = 2 * HALO_BYTES + (wn * (BN / 2) + l31) * 128;

    float bpre[16];
    gemm_bias_prefetch<BN, SWAP, NW>(p, n0, bpre);

    if constexpr (BDIR) {
        constexpr int PFB = 12;                                  // divides the 36 k-steps of a chunk: static ring positions
        const unsigned kpieces = (unsigned)p.kt64 * 4u;          // 1 KiB pieces (16-wide k-steps) per 32-column tile
        unsigned pbase[TN];
#pragma unroll
        for (int j = 0; j < TN; ++j)
            pbase[j] = (unsigned)((n0 + (W4 ? wn * 32 : wn * (BN / 2) + j * 32)) >> 5) * kpieces + (unsigned)kt_begin * 4u;
        const unsigned voffw = (unsigned)lane * 16u;
        // halo first, then the ring: the halo DMAs are then older than the PFB * TN youngest loads at every chunk boundary
#pragma unroll
        for (int q = 0; q < HJ; ++q) dma_halo(q, c_begin, 0);
        u32x4 ring[TN][PFB];
#pragma unroll
        for (int q = 0; q < PFB; ++q)
#pragma unroll
            for (int j = 0; j < TN; ++j) ring[j][q] = __builtin_amdgcn_raw_buffer_load_b128(rs_w, voffw, (pbase[j] + q) * 1024u, 0);
        trace_mark(p, 1);
        unsigned step = 0;
        for (int c = c_begin; c < c_end; ++c) {
            const int hb = (c - c_begin) & 1;
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PFB * TN) : "memory");     // this chunk's halo has landed (own DMAs)
            __builtin_amdgcn_s_barrier();                                      // ... everyone's; buffer hb ^ 1 is free
            if (c + 1 < c_end) {
#pragma unroll
                for (int q = 0; q < HJ; ++q) dma_halo(q, c + 1, hb ^ 1);
            }
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const int ky = tap / 3, kx = tap - ky * 3;
                const int dq = ky * HWD + kx;
                int a_row[TM], a_key[TM];
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    a_row[i] = hb * HALO_BYTES + (hp0[i] + dq) * 128;
                    if constexpr (PW == 16)
                        a_key[i] = ((((l31 & 15) + kx) >> 1) & 7) << 4;
                    else
                        a_key[i] = (((((l31 & 7) + kx) >> 1) & 3) | ((((l31 >> 3) + ky) & 1) << 2)) << 4;
                }
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    f16x8 af[TM];
#pragma unroll
                    for (int i = 0; i < TM; ++i)
                        af[i] = *reinterpret_cast<const f16x8*>(smem + a_row[i] + (((2 * s + hi) << 4) ^ a_key[i]));
                    constexpr int dummy = 0;
                    (void)dummy;
                    const int rp = (tap * 4 + s) % PFB;
#pragma unroll
                    for (int j = 0; j < TN; ++j) {
                        const f16x8 b = __builtin_bit_cast(f16x8, ring[j][rp]);
                        ring[j][rp] = __builtin_amdgcn_raw_buffer_load_b128(rs_w, voffw, (pbase[j] + step + (unsigned)(tap * 4 + s) + PFB) * 1024u, 0);
#pragma unroll
                        for (int i = 0; i < TM; ++i) {
                            if constexpr (SWAP)
                                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(b, af[i], acc[i][j], 0, 0, 0);
                            else
                                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[i], b, acc[i][j], 0, 0, 0);
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);      // keep every refill where it is written (else they sink to their use)
                }
            }
            step += 36;
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // ring refills past the end of the range are still in flight
        __syncthreads();
        trace_mark(p, 3);
        if constexpr (W4) {
            // split-K partial slab [split][M][N], C layout (lane -> column, registers -> rows): 128-byte row segments per store
            float* wsz = p.ws + (size_t)split * p.M * p.N;
            const int n = n0 + wn * 32 + l31;
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = i * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                    int m;
                    if constexpr (PW == 16)
                        m = (pb * p.H + py0) * p.W + px0 + (row >> 4) * p.W + (row & 15);
                    else
                        m = tile_m * BM + row;
                    if (m < p.M && n < p.N) wsz[(size_t)m * p.N + n] = acc[i][0][r];
                }
            trace_mark(p, 4);
            return;
        } else {
            if constexpr (PW == 16)
                gemm_epilogue<BM, BN, SWAP, NW, PatchRows, 0, 2>(p, acc, smem, PatchRows{(pb * p.H + py0) * p.W + px0, p.W, pb}, n0,
                                                                          split, bpre, tile_m, tile_id);
            else
                gemm_epilogue<BM, BN, SWAP, NW>(p, acc, smem, LinearRows{tile_m * BM}, n0, split, bpre, tile_m, tile_id);
            trace_mark(p, 4);
            return;
        }
    }
    if constexpr (!BDIR) {
    // ---- GroupNorm(32) [+ SiLU] of the INPUT inside the conv (nn.GroupNorm -> SiLU -> Conv2d of a ResBlock, openaimodel.py:
    // 136-138, 159-163): the producer of the input emitted per-row-block column partials (colstats); this block folds its
    // sample's partials into a per-channel {scale, shift} table in LDS and normalises every halo slice IN PLACE after it has
    // landed (each thread the 16-byte pieces its own DMAs brought, so no extra barrier): the normalised tensor is never
    // written or read, and the GroupNorm launch disappears.  Zero padding stays zero (pieces outside the image are skipped).
    float2* gn_tab = reinterpret_cast<float2*>(smem + 2 * HALO_BYTES + NSB * B_BYTES);     // [Cin] {a, shift}
    if constexpr (PW == 16) {
        if (p.gn_cs) {
            float2* csum = reinterpret_cast<float2*>(smem);      // [Cin] channel {sum, sumsq}: the halo area is still unused
            const int cpg = p.cin >> 5;
            const float2* src = reinterpret_cast<const float2*>(p.gn_cs) + (size_t)pb * p.gn_nrb * p.cin;
            for (int c = tid; c < p.cin; c += NW * 64) {
                float su = 0.f, sq = 0.f;
                int k = 0;
                for (; k + 8 <= p.gn_nrb; k += 8) {
                    float2 v[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[e] = src[(size_t)(k + e) * p.cin + c];
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        su += v[e].x;
                        sq += v[e].y;
                    }
                }
                for (; k < p.gn_nrb; ++k) {
                    const float2 v = src[(size_t)k * p.cin + c];
                    su += v.x;
                    sq += v.y;
                }
                csum[c] = make_float2(su, sq);
            }
            __syncthreads();
            for (int c = tid; c < p.cin; c += NW * 64) {
                const int g = c / cpg;
                float su = 0.f, sq = 0.f;
                for (int e = 0; e < cpg; ++e) {
                    const float2 v = csum[g * cpg + e];
                    su += v.x;
                    sq += v.y;
                }
                const float inv = 1.0f / ((float)cpg * (float)(p.H * p.W));
                const float mean = su * inv;
                float var = sq * inv - mean * mean;
                var = var < 0.f ? 0.f : var;
                const float a = p.gn_gamma[c] * rsqrtf(var + p.gn_eps);
                gn_tab[c] = make_float2(a, p.gn_beta[c] - mean * a);
            }
            __syncthreads();      // table complete; the halo area may be overwritten by the prologue DMAs
        }
    }
    auto gn_transform = [&](int chunk, int hb) {      // normalise this thread's own pieces of halo buffer hb (chunk `chunk`)
#pragma unroll
        for (int q = 0; q < HJ; ++q) {
            if (wave * HJ + q >= HINST || hal_off[q] == MDX_OOB) continue;
            char* pc = smem + hb * HALO_BYTES + (wave * HJ + q) * 1024 + lane * 16;
            const int ch0 = chunk * 64 + (int)((hal_off[q] >> 4) & 7u) * 8;       // logical chunk of this lane's piece
            const f16x8 x = *reinterpret_cast<const f16x8*>(pc);
            f16x8 y;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float2 t = gn_tab[ch0 + e];
                const float v = (float)x[e] * t.x + t.y;
                y[e] = (f16)(p.gn_silu ? silu_f(v) : v);
            }
            *reinterpret_cast<f16x8*>(pc) = y;
        }
    };
    // prologue: whole halo of the first chunk + the first NSB-1 weight tiles
#pragma unroll
    for (int q = 0; q < HJ; ++q) dma_halo(q, c_begin, 0);
#pragma unroll
    for (int i = 0; i < NSB - 1; ++i)
        if (i < nt) dma_b(kt_begin + i, i);

    int t = 0;
    int rd = 0, wr = NSB - 1;
    trace_mark(p, 1);
    for (int c = c_begin; c < c_end; ++c) {
        const int hb = (c - c_begin) & 1;
        const bool more = c + 1 < c_end;
#pragma unroll      // (the pinned form is not unrolled on the compiler's own judgement; the tap decode is nine constants only when it is:
                    // rolled, the convs of UNet batch 2 were 10-35 % slower -- profiles/r05_kloop_ab.txt)
        for (int tap = 0; tap < 9; ++tap, ++t) {
            // weight tiles t .. t+NSB-2 (and at most one halo slice per tap, each older than the weight tile issued with it) are
            // outstanding: all but the youngest (tiles ahead) x BJ instructions must have landed -- that covers tile t and, with a
            // four-stage ring, one instruction of tile t+1 when a halo slice sits between the two (conservative, never short)
            if (NSB >= 4 && t + 2 < nt)
                asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * BJ) : "memory");
            else if (NSB >= 3 && t + 1 < nt)
                asm volatile("s_waitcnt vmcnt(%0)" ::"n"(BJ) : "memory");
            else
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if constexpr (PW == 16) {
                if (tap == 0 && p.gn_cs) {     // own slices have landed (they are older than the newest weight tile)
                    gn_transform(c, hb);
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // ... and are rewritten before anyone passes the barrier
                }
            }
            __builtin_amdgcn_s_barrier();
            if (t == 0) trace_mark(p, 2);
            // (round 5: DMA issue first -- the weight stream is latency x ring-depth bound, every instruction in front of the issue is
            // added to the chain: measured +10...35 % with the fragment reads in front -- then the fragment reads, pinned by
            // sched_barriers: see gemm_kernel's main loop)
            if (more && tap < HJ) dma_halo(tap, c + 1, hb ^ 1);
            if (t + NSB - 1 < nt) dma_b(kt_begin + t + NSB - 1, wr);
            __builtin_amdgcn_sched_barrier(0);
            const int ky = tap / 3, kx = tap - ky * 3;
            const int dq = ky * HWD + kx;
            int a_row[TM], a_key[TM];
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int hp = hp0[i] + dq;
                a_row[i] = hb * HALO_BYTES + hp * 128;
                if constexpr (PW == 16)
                    a_key[i] = ((((l31 & 15) + kx) >> 1) & 7) << 4;   // swizzle key = halo COLUMN / 2 (see the loader)
                else   // halo column (l31 & 7) + kx, halo row parity ((l31 >> 3) + ky) & 1 (i * 4 rows keep the parity)
                    a_key[i] = (((((l31 & 7) + kx) >> 1) & 3) | ((((l31 >> 3) + ky) & 1) << 2)) << 4;
            }
            const char* sb = smem + rd * B_BYTES;
            constexpr bool ALLK = TM * TN <= 2;      // at most two MFMAs per k-step: nothing to hide a fragment read behind
            constexpr int FD = ALLK ? 4 : 2;
            f16x8 af[FD][TM], bf[FD][TN];
            auto rdfrag = [&](auto slot_c, const int ks) {
                constexpr int slot = decltype(slot_c)::value;
#pragma unroll
                for (int i = 0; i < TM; ++i)
                    af[slot][i] = *reinterpret_cast<const f16x8*>(smem + a_row[i] + (((2 * ks + hi) << 4) ^ a_key[i]));
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    bf[slot][j] = *reinterpret_cast<const f16x8*>(sb + b_row_off + j * 32 * 128 + (((2 * ks + hi) ^ swz_b) << 4));
            };
            auto mfmas = [&](auto slot_c) {
                constexpr int slot = decltype(slot_c)::value;
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j) {
                        if constexpr (SWAP)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bf[slot][j], af[slot][i], acc[i][j], 0, 0, 0);
                        else
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[slot][i], bf[slot][j], acc[i][j], 0, 0, 0);
                    }
            };
            using I0 = std::integral_constant<int, 0>;
            using I1 = std::integral_constant<int, 1>;
            if constexpr (ALLK) {
                using I2 = std::integral_constant<int, 2>;
                using I3 = std::integral_constant<int, 3>;
                rdfrag(I0{}, 0); rdfrag(I1{}, 1); rdfrag(I2{}, 2); rdfrag(I3{}, 3);
                __builtin_amdgcn_sched_barrier(0);
                mfmas(I0{}); mfmas(I1{}); mfmas(I2{}); mfmas(I3{});
            } else {
                rdfrag(I0{}, 0);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int ks = 0; ks < 4; ks += 2) {
                    rdfrag(I1{}, ks + 1);
                    __builtin_amdgcn_sched_barrier(0);
                    mfmas(I0{});
                    __builtin_amdgcn_sched_barrier(0);
                    if (ks + 2 < 4) {
                        rdfrag(I0{}, ks + 2);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                    mfmas(I1{});
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            rd = (rd + 1 == NSB) ? 0 : rd + 1;
            wr = (wr + 1 == NSB) ? 0 : wr + 1;
        }
    }

    if (p.skip_w) {
        // ---- ResBlock skip_connection (openaimodel.py:174, 201-205: conv1x1 over the block's RAW input, the virtual concat of
        // x and the UNet skip tensor on the up path) as extra K tiles of this launch: out = conv3x3(h) + conv1x1(x), one
        // accumulator, one epilogue, no second launch and no fp16 round trip of the skip tensor.  Generic 128-byte-row A tiles
        // of this block's patch pixels (rows = patch pixels, 64 channels per tile) in the halo area, weight tiles in the ring
        // area, two stages, one barrier per tile; this split's share of the skip K tiles.
        constexpr int SA_BYTES = BM * 128;
        static_assert(2 * SA_BYTES <= 2 * HALO_BYTES && NSB >= 2, "skip tiles reuse the halo / ring areas");
        const __amdgpu_buffer_rsrc_t rs_s1 = make_rsrc(p.skip_a, p.skip_a_bytes);
        const __amdgpu_buffer_rsrc_t rs_s2 = make_rsrc(p.skip_a2 ? p.skip_a2 : p.skip_a, p.skip_a2 ? p.skip_a2_bytes : p.skip_a_bytes);
        const __amdgpu_buffer_rsrc_t rs_sw = make_rsrc(p.skip_w, p.skip_w_bytes);
        const int sk_begin = split * p.skip_kt_per_split, sk_end = min(p.skip_kt, sk_begin + p.skip_kt_per_split);
        constexpr int SAJ = BM / 8 / NW;              // A DMA instructions per wave per tile (8 rows each)
        int s_pix[SAJ];                               // source pixel of this lane's row, or -1
        unsigned s_cb[SAJ];
#pragma unroll
        for (int j = 0; j < SAJ; ++j) {
            const int row = (wave * SAJ + j) * 8 + lrow;
            int pix;
            if constexpr (PW == 16) {
                pix = (pb * p.H + py0 + (row >> 4)) * p.W + px0 + (row & 15);
            } else {
                pix = tile_m * BM + row;
                if (pix >= p.M) pix = -1;
            }
            s_pix[j] = pix;
            s_cb[j] = (unsigned)((lchk ^ ((row >> 1) & 7)) * 16);
        }
        unsigned sb_off[BJ];
        const int skt64 = p.skip_kt;
#pragma unroll
        for (int j = 0; j < BJ; ++j) {
            const int row = (wave * BJ + j) * 8 + lrow;
            const int panel = (n0 >> 6) + (row >> 6);
            sb_off[j] = (unsigned)(((size_t)panel * skt64) * 8192 + ((row & 63) * 8 + lchk) * 16);
        }
        auto stage_skip = [&](int kt, int st) {
            int ci0 = kt * 64;
            const bool second = ci0 >= p.skip_c1;
            const int cs2 = (second ? p.skip_c2 : p.skip_c1) * 2;
            if (second) ci0 -= p.skip_c1;
#pragma unroll
            for (int j = 0; j < SAJ; ++j) {
                const unsigned off = s_pix[j] >= 0 ? (unsigned)(s_pix[j] * cs2) + (unsigned)(ci0 * 2) + s_cb[j] : MDX_OOB;
                void* dst = smem + st * SA_BYTES + (wave * SAJ + j) * 1024;
                if (second)
                    dma16(rs_s2, dst, off);
                else
                    dma16(rs_s1, dst, off);
            }
#pragma unroll
            for (int j = 0; j < BJ; ++j)
                dma16(rs_sw, smem + 2 * HALO_BYTES + st * B_BYTES + (wave * BJ + j) * 1024, sb_off[j] + (unsigned)kt * 8192);
        };
        __syncthreads();            // every wave is done with the halos and the weight ring
        const int sa_row_off = (wm * WROWS + l31) * 128;
        const int s_swz = (l31 >> 1) & 7;
        if (sk_begin < sk_end) stage_skip(sk_begin, 0);
        for (int kt = sk_begin; kt < sk_end; ++kt) {
            const int st = (kt - sk_begin) & 1;
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();      // tile kt landed for everyone; stage st ^ 1 (tile kt - 1) is free
            if (kt + 1 < sk_end) stage_skip(kt + 1, st ^ 1);
            const char* sa = smem + st * SA_BYTES;
            const char* sbk = smem + 2 * HALO_BYTES + st * B_BYTES;
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) {
                f16x8 af[TM], bf[TN];
#pragma unroll
                for (int i = 0; i < TM; ++i)
                    af[i] = *reinterpret_cast<const f16x8*>(sa + sa_row_off + i * 32 * 128 + (((2 * s4 + hi) ^ s_swz) << 4));
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    bf[j] = *reinterpret_cast<const f16x8*>(sbk + (b_row_off - 2 * HALO_BYTES) + j * 32 * 128 + (((2 * s4 + hi) ^ swz_b) << 4));
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j) {
                        if constexpr (SWAP)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bf[j], af[i], acc[i][j], 0, 0, 0);
                        else
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[i], bf[j], acc[i][j], 0, 0, 0);
                    }
            }
        }
    }

    __syncthreads();
    trace_mark(p, 3);
    if constexpr (PW == 16)
        gemm_epilogue<BM, BN, SWAP, NW, PatchRows, 0, 2>(p, acc, smem, PatchRows{(pb * p.H + py0) * p.W + px0, p.W, pb}, n0, split, bpre,
                                                                  tile_m, tile_id);
    else   // two whole 64-pixel samples: tile rows are consecutive output rows
        gemm_epilogue<BM, BN, SWAP, NW>(p, acc, smem, LinearRows{tile_m * BM}, n0, split, bpre, tile_m, tile_id);
    trace_mark(p, 4);
    }
}

// 8 consecutive fp32 of row m from every split-K slab, summed in slab order (deterministic).  The loads of up to four
// slabs are issued before the first add so that the HBM/L2 latency is paid once per batch, not once per slab.
__device__ __forceinline__ void splitk_sum8(const GemmParams& p, const float* base, const size_t slab, float (&f)[8]) {
    int z = 0;
    for (; z + 4 <= p.nsplit; z += 4) {
        float4 v[4][2];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float4* s = reinterpret_cast<const float4*>(base + (size_t)(z + u) * slab);
            v[u][0] = s[0];
            v[u][1] = s[1];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            f[0] += v[u][0].x; f[1] += v[u][0].y; f[2] += v[u][0].z; f[3] += v[u][0].w;
            f[4] += v[u][1].x; f[5] += v[u][1].y; f[6] += v[u][1].z; f[7] += v[u][1].w;
        }
    }
    for (; z < p.nsplit; ++z) {
        const float4* s = reinterpret_cast<const float4*>(base + (size_t)z * slab);
        const float4 s0 = s[0], s1 = s[1];
        f[0] += s0.x; f[1] += s0.y; f[2] += s0.z; f[3] += s0.w; f[4] += s1.x; f[5] += s1.y; f[6] += s1.z; f[7] += s1.w;
    }
}

// split-K reduce + fused epilogue: one thread per (m, 8 output columns).  EXT: the instantiation for PReLU / depth-to-space launches.
template <bool EXT = false>
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const GemmParams p) {
    mdx_kernarg_touch<sizeof(GemmParams)>();
    const bool geglu = p.epilogue == MDX_EPI_GEGLU;
    const int ncols = geglu ? p.N / 2 : p.N;
    const int cpr = ncols / 8;
    const size_t total = (size_t)p.M * cpr;
    const size_t slab = (size_t)p.M * p.N;
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
        const int m = (int)(idx / cpr);
        const int oc = (int)(idx - (size_t)m * cpr) * 8;
        // time-embedding row / residual first: their latency overlaps the slab loads instead of following them
        Row8Extras xtra;
        if (p.out_mode != MDX_OUT_TRANSPOSED) xtra = epilogue_prefetch_row8(p, m, oc);
        // LayerNorm fold (consumer side): the 8 lanes of a 64-column slice share the row, so each adds every 8th of the
        // producer's partials and an xor tree finishes {sum, sumsq}; N % 64 == 0 keeps the groups whole.
        const bool ln = p.ln_stats != nullptr;
        float mean = 0.f, rstd = 1.f;
        if (ln) {
            const float2* stp = reinterpret_cast<const float2*>(p.ln_stats) + (size_t)m * p.ln_nt;
            float su = 0.f, sq = 0.f;
            for (int j = threadIdx.x & 7; j < p.ln_nt; j += 8) {
                const float2 v = stp[j];
                su += v.x;
                sq += v.y;
            }
#pragma unroll
            for (int off = 4; off >= 1; off >>= 1) {
                su += __shfl_xor(su, off, 64);
                sq += __shfl_xor(sq, off, 64);
            }
            const float inv = 1.0f / (float)p.K;
            mean = su * inv;
            float var = sq * inv - mean * mean;
            var = var < 0.f ? 0.f : var;
            rstd = rsqrtf(var + p.ln_eps);
        }
        float f[8];
        if (geglu) {
            const int pa = (oc >> 6) * 128 + (oc & 63);
            float a[8], g[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                a[e] = (p.bias && !ln) ? p.bias[pa + e] : 0.f;
                g[e] = (p.bias && !ln) ? p.bias[pa + 64 + e] : 0.f;
            }
            splitk_sum8(p, p.ws + (size_t)m * p.N + pa, slab, a);
            splitk_sum8(p, p.ws + (size_t)m * p.N + pa + 64, slab, g);
            if (ln) {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    a[e] = rstd * (a[e] - mean * p.ln_s[pa + e]) + (p.bias ? p.bias[pa + e] : 0.f);
                    g[e] = rstd * (g[e] - mean * p.ln_s[pa + 64 + e]) + (p.bias ? p.bias[pa + 64 + e] : 0.f);
                }
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) f[e] = a[e] * gelu_tanh_f(g[e]);
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) f[e] = (p.bias && !ln) ? p.bias[oc + e] : 0.f;
            splitk_sum8(p, p.ws + (size_t)m * p.N + oc, slab, f);
            if (ln) {
#pragma unroll
                for (int e = 0; e < 8; ++e) f[e] = rstd * (f[e] - mean * p.ln_s[oc + e]) + (p.bias ? p.bias[oc + e] : 0.f);
            }
            if (p.epilogue == MDX_EPI_GELU) {
#pragma unroll
                for (int e = 0; e < 8; ++e) f[e] = gelu_tanh_f(f[e]);
            } else if (p.epilogue == MDX_EPI_QUICKGELU) {
#pragma unroll
                for (int e = 0; e < 8; ++e) f[e] = quick_gelu_f(f[e]);
            } else if constexpr (EXT) {
                if (p.epilogue == MDX_EPI_PRELU) {
                    const float* sp = p.act_slope + oc % p.act_slope_n;
#pragma unroll
                    for (int e = 0; e < 8; ++e) f[e] = f[e] > 0.f ? f[e] : sp[e] * f[e];
                }
            }
        }
        if (p.out_mode == MDX_OUT_TRANSPOSED) {
            const int b = m / p.HoWo;
            const int tok = m - b * p.HoWo;
#pragma unroll
            for (int e = 0; e < 8; ++e) p.out[((size_t)b * p.N + oc + e) * p.out_ld + tok] = (f16)f[e];
        } else if (p.n_split && oc >= p.n_split) {
            const int b = m / p.HoWo;
            const int tok = m - b * p.HoWo;
            const int nv = p.N - p.n_split;
#pragma unroll
            for (int e = 0; e < 8; ++e) p.out2[((size_t)b * nv + (oc - p.n_split + e)) * p.out2_ld + tok] = (f16)f[e];
        } else {
            const f16x8 o = epilogue_apply_row8<EXT>(p, f, m, oc, xtra);
            if (p.stats_out) {   // producer side of the LayerNorm fold, as in gemm_epilogue
                float su = 0.f, sq = 0.f;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float t = (float)o[e];
                    su += t;
                    sq += t * t;
                }
#pragma unroll
                for (int off = 4; off >= 1; off >>= 1) {
                    su += __shfl_xor(su, off, 64);
                    sq += __shfl_xor(sq, off, 64);
                }
                if ((threadIdx.x & 7) == 0)
                    reinterpret_cast<float2*>(p.stats_out)[(size_t)m * (p.N >> 6) + (oc >> 6)] = make_float2(su, sq);
            }
        }
    }
}

// split-K reduce for GroupNorm producers (mdx_gemm_desc.colstats_out): 64-row x 64-column tiles, thread = (row lane,
// 8 columns) with two rows each, so that the per-column {sum, sumsq} of a 64-row block fold inside the block (fixed order).
// Plain row-major epilogue only: bias, per-sample time-embedding row, residual.
__global__ __launch_bounds__(256) void splitk_reduce_colstats_kernel(const GemmParams p) {
    mdx_kernarg_touch<sizeof(GemmParams)>();
    __shared__ float part[32][64][2];
    const int tid = threadIdx.x;
    const int chunk = tid & 7, rl = tid >> 3;
    const int rb = blockIdx.y, n = blockIdx.x * 64 + chunk * 8;
    const size_t slab = (size_t)p.M * p.N;
    float cs[8], cq[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) cs[e] = cq[e] = 0.f;
    if (n < p.N) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int m = rb * CS_ROWS + rl + 32 * h;
            if (m >= p.M) continue;
            const Row8Extras xtra = epilogue_prefetch_row8(p, m, n);
            float f[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) f[e] = p.bias ? p.bias[n + e] : 0.f;
            splitk_sum8(p, p.ws + (size_t)m * p.N + n, slab, f);
            const f16x8 o = epilogue_apply_row8(p, f, m, n, xtra);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float t = (float)o[e];
                cs[e] += t;
                cq[e] += t * t;
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        part[rl][chunk * 8 + e][0] = cs[e];
        part[rl][chunk * 8 + e][1] = cq[e];
    }
    __syncthreads();
    if (tid < 128) {
        const int c = tid >> 1;
        float a = 0.f;
        for (int r = 0; r < 32; ++r) a += part[r][c][tid & 1];
        const int nn = blockIdx.x * 64 + c;
        if (nn < p.N) p.colstats_out[((size_t)rb * p.N + nn) * 2 + (tid & 1)] = a;
    }
}

template <int BM, int BN, int BK, int NS, bool SWAP, bool FASTK, int NW, bool EXT = false>
void launch_one(const GemmParams& p, dim3 grid, hipStream_t st) {
    constexpr size_t ring = (size_t)NS * (BM + BN) * BK * 2;
    constexpr size_t epi = (size_t)(BM > BN ? BM : BN) * ((BM > BN ? BN : BM) + 8) * 2 + 4096;  // staged C tile
    constexpr size_t lds = ring > epi ? ring : epi;
    static MdxPerDeviceOnce attr_once;
    if (attr_once.first()) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_kernel<BM, BN, BK, NS, SWAP, FASTK, NW, false, EXT>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    }
    hipLaunchKernelGGL((gemm_kernel<BM, BN, BK, NS, SWAP, FASTK, NW, false, EXT>), grid, dim3(NW * 64), lds, st, p);
}

// SRGAN launches (PReLU / depth-to-space; fill_params: single source, Cin % 64 == 0): the EXT instantiations, four waves, ring depth
// 2 | 3 (a deeper ring or the eight-wave form of the tile table / overrides runs at depth 3 on four waves: same tile program, same bits)
template <int BM, int BN>
void launch_ext(const GemmParams& p, int ns, bool swap, dim3 grid, hipStream_t st) {
    if (ns >= 3) {
        if (swap) launch_one<BM, BN, 64, 3, true, true, 4, true>(p, grid, st); else launch_one<BM, BN, 64, 3, false, true, 4, true>(p, grid, st);
    } else {
        if (swap) launch_one<BM, BN, 64, 2, true, true, 4, true>(p, grid, st); else launch_one<BM, BN, 64, 2, false, true, 4, true>(p, grid, st);
    }
}

// GNA form (GroupNorm of the input on the A fragments): four waves, ring depth 2 | 3, K-contiguous (dense) launches only
template <int BM, int BN, int NS, bool SWAP>
void launch_gna_one(const GemmParams& p, dim3 grid, hipStream_t st) {
    constexpr size_t ring = (size_t)NS * (BM + BN) * 64 * 2;
    constexpr size_t epi = (size_t)(BM > BN ? BM : BN) * ((BM > BN ? BN : BM) + 8) * 2 + 4096;
    constexpr size_t lds0 = ring > epi ? ring : epi;
    const size_t lds = lds0 + (size_t)p.cin * 12;       // a, s (fp16) + {sum, sumsq} scratch (fp32 pairs)
    static MdxPerDeviceOnce attr_once;
    if (attr_once.first()) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_kernel<BM, BN, 64, NS, SWAP, true, 4, true>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)(lds0 + 2560 * 12));
    }
    hipLaunchKernelGGL((gemm_kernel<BM, BN, 64, NS, SWAP, true, 4, true>), grid, dim3(256), lds, st, p);
}

template <int BM, int BN>
void launch_gna(const GemmParams& p, int ns, bool swap, dim3 grid, hipStream_t st) {
    if (ns >= 3) {
        if (swap) launch_gna_one<BM, BN, 3, true>(p, grid, st); else launch_gna_one<BM, BN, 3, false>(p, grid, st);
    } else {
        if (swap) launch_gna_one<BM, BN, 2, true>(p, grid, st); else launch_gna_one<BM, BN, 2, false>(p, grid, st);
    }
}

template <int BM, int BN, int BK, int NS, int NW>
void launch_cfg(const GemmParams& p, bool swap, bool fastk, dim3 grid, hipStream_t st) {
    if (swap) {
        if (fastk)
            launch_one<BM, BN, BK, NS, true, true, NW>(p, grid, st);
        else
            launch_one<BM, BN, BK, NS, true, false, NW>(p, grid, st);
    } else {
        if (fastk)
            launch_one<BM, BN, BK, NS, false, true, NW>(p, grid, st);
        else
            launch_one<BM, BN, BK, NS, false, false, NW>(p, grid, st);
    }
}

template <int BM, int BN>
bool launch_bn(const GemmParams& p, int ns, bool swap, bool fastk, dim3 grid, hipStream_t st, bool nw8 = false) {
    if constexpr (BM == 128) {
        // eight waves (4 x 2) on the same 128-row tile: each wave owns half the rows of the 4-wave form, so a block that has a
        // CU to itself keeps two waves per SIMD busy (tile-table choice, mdx_gemm_desc.stages 10 | 11)
        if (nw8 && (ns == 2 || ns == 3)) {
            if (ns == 2) launch_cfg<128, BN, 64, 2, 8>(p, swap, fastk, grid, st); else launch_cfg<128, BN, 64, 3, 8>(p, swap, fastk, grid, st);
            return true;
        }
    }
    if (ns == 2) launch_cfg<BM, BN, 64, 2, 4>(p, swap, fastk, grid, st);
    else if (ns == 3) launch_cfg<BM, BN, 64, 3, 4>(p, swap, fastk, grid, st);
    else if (BM == 128 && ns == 4) launch_cfg<128, BN, 64, 4, 4>(p, swap, fastk, grid, st);
    else if (BM == 128 && ns == 5) launch_cfg<128, BN, 64, 5, 4>(p, swap, fastk, grid, st);
    // 64-row tiles stage only 16 / 24 KB per K tile: deeper rings are cheap, and a launch with one or two blocks per CU is
    // bound by how many tiles it keeps in flight (tile-table choice)
    else if (BM == 64 && ns == 4) launch_cfg<64, BN, 64, 4, 4>(p, swap, fastk, grid, st);
    else if (BM == 64 && ns == 5) launch_cfg<64, BN, 64, 5, 4>(p, swap, fastk, grid, st);
    else if (BM == 64 && ns == 6) launch_cfg<64, BN, 64, 6, 4>(p, swap, fastk, grid, st);
    else return false;
    return true;
}

template <int BM, int BN, int NSB, bool SWAP, int PW = 16, bool BDIR = false, bool W4 = false>
void launch_halo(const GemmParams& p, dim3 grid, hipStream_t st) {
    constexpr size_t hinst = ((PW == 16 ? (BM / 16 + 2) * 18 : (BM / 64) * 100) + 7) / 8;
    constexpr size_t ring = 2 * hinst * 1024 + (BDIR ? 0 : (size_t)NSB * BN * 128);
    constexpr size_t epi = (size_t)BM * (BN + 8) * 2 + 4096;
    constexpr size_t lds0 = ring > epi ? ring : epi;
    constexpr size_t gn_tab_max = (BDIR || PW != 16) ? 0 : 640 * 8;      // {scale, shift} table of the fused input GroupNorm
    const size_t lds = lds0 + (p.gn_cs ? (size_t)p.cin * 8 : 0);
    static MdxPerDeviceOnce attr_once;
    if (attr_once.first()) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&conv3x3_halo_kernel<BM, BN, NSB, SWAP, PW, BDIR, W4>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)(lds0 + gn_tab_max));
    }
    hipLaunchKernelGGL((conv3x3_halo_kernel<BM, BN, NSB, SWAP, PW, BDIR, W4>), grid, dim3(BM * 2), lds, st, p);
}

// weight-streaming form (fragment-major weights): 128-row tiles only, no weight ring in LDS
template <int BN, int PW>
void launch_halo_bdir(const GemmParams& p, bool swap, dim3 grid, hipStream_t st) {
    if (swap) launch_halo<128, BN, 2, true, PW, true>(p, grid, st); else launch_halo<128, BN, 2, false, PW, true>(p, grid, st);
}
template <int PW>
void launch_halo_bdir_w4(const GemmParams& p, dim3 grid, hipStream_t st) {
    launch_halo<128, 128, 2, false, PW, true, true>(p, grid, st);
}

template <int BM, int BN, int PW = 16>
void launch_halo_cfg(const GemmParams& p, int nsb, bool swap, dim3 grid, hipStream_t st) {
    if (nsb == 4) {      // (round 5) the weight stream of a lone block is latency x tiles-in-flight bound: a fourth stage
        if (swap) launch_halo<BM, BN, 4, true, PW>(p, grid, st); else launch_halo<BM, BN, 4, false, PW>(p, grid, st);
    } else if (nsb == 3) {
        if (swap) launch_halo<BM, BN, 3, true, PW>(p, grid, st); else launch_halo<BM, BN, 3, false, PW>(p, grid, st);
    } else {
        if (swap) launch_halo<BM, BN, 2, true, PW>(p, grid, st); else launch_halo<BM, BN, 2, false, PW>(p, grid, st);
    }
}

}  // namespace

// Launches a plan (plan_gemm, gemm_plan.hip): ONE switch on the kernel form -- every form a descriptor can resolve to has its
// case here and nowhere else -- then the reduce kernel of a slab split-K.
int mdx_gemm_launch_plan(const GemmParams& p, const GemmPlan& pl, hipStream_t st) {
    const dim3 grid = pl.grid;
    const bool swap = pl.swap, wide = pl.bn == 128;      // (the tile programs below come in 64 and 128 columns)
    int rc;
    switch (pl.form) {
        case GEMM_CONV8P:
            rc = mdx_conv8p_launch(p, pl.bn, st);
            if (rc != MDX_OK) return rc;
            MDX_LAUNCH_CHECK("mdx_gemm_f16(conv8p)");
            return MDX_OK;
        case GEMM_LEAN:
        case GEMM_LEAN_XA:      // dense.hip: the same tile program with a division-free prologue and the epilogue's reads prefetched
            rc = mdx_dense_launch(p, pl, st);
            if (rc != MDX_OK) return rc;
            break;
        case GEMM_HALO:
            if (pl.bm == 256) {
                if (wide) launch_halo_cfg<256, 128>(p, pl.ring, swap, grid, st); else launch_halo_cfg<256, 64>(p, pl.ring, swap, grid, st);
            } else if (pl.pw == 8) {
                if (wide) launch_halo_cfg<128, 128, 8>(p, pl.ring, swap, grid, st); else launch_halo_cfg<128, 64, 8>(p, pl.ring, swap, grid, st);
            } else {
                if (wide) launch_halo_cfg<128, 128>(p, pl.ring, swap, grid, st); else launch_halo_cfg<128, 64>(p, pl.ring, swap, grid, st);
            }
            break;
        case GEMM_HALO_FRAG:
            if (pl.pw == 8) {
                if (wide) launch_halo_bdir<128, 8>(p, swap, grid, st); else launch_halo_bdir<64, 8>(p, swap, grid, st);
            } else {
                if (wide) launch_halo_bdir<128, 16>(p, swap, grid, st); else launch_halo_bdir<64, 16>(p, swap, grid, st);
            }
            break;
        case GEMM_HALO_FRAG_W4:
            if (pl.pw == 8) launch_halo_bdir_w4<8>(p, grid, st); else launch_halo_bdir_w4<16>(p, grid, st);
            break;
        case GEMM_GNA:
            if (pl.bm == 64) {
                if (wide) launch_gna<64, 128>(p, pl.ring, swap, grid, st); else launch_gna<64, 64>(p, pl.ring, swap, grid, st);
            } else {
                if (wide) launch_gna<128, 128>(p, pl.ring, swap, grid, st); else launch_gna<128, 64>(p, pl.ring, swap, grid, st);
            }
            break;
        case GEMM_EXT:
            if (pl.bm == 64) {
                if (wide) launch_ext<64, 128>(p, pl.ring, swap, grid, st); else launch_ext<64, 64>(p, pl.ring, swap, grid, st);
            } else {
                if (wide) launch_ext<128, 128>(p, pl.ring, swap, grid, st); else launch_ext<128, 64>(p, pl.ring, swap, grid, st);
            }
            break;
        case GEMM_GENERIC:
        case GEMM_GENERIC_NW8: {
            const bool nw8 = pl.form == GEMM_GENERIC_NW8;
            bool ok;
            if (pl.bm == 64)
                ok = wide ? launch_bn<64, 128>(p, pl.ring, swap, pl.fastk, grid, st) : launch_bn<64, 64>(p, pl.ring, swap, pl.fastk, grid, st);
            else
                ok = wide ? launch_bn<128, 128>(p, pl.ring, swap, pl.fastk, grid, st, nw8) : launch_bn<128, 64>(p, pl.ring, swap, pl.fastk, grid, st, nw8);
            MDX_REQUIRE(ok, "mdx_gemm_f16: internal error: the plan names a generic tile %d x %d at ring depth %d that is not built", pl.bm,
                        pl.bn, pl.ring);
            break;
        }
    }
    MDX_LAUNCH_CHECK("mdx_gemm_f16");
    if (pl.reduce == GEMM_REDUCE_NONE || pl.reduce == GEMM_REDUCE_DEFERRED) return MDX_OK;
    if (pl.reduce == GEMM_REDUCE_COLSTATS) {
        hipLaunchKernelGGL(splitk_reduce_colstats_kernel, dim3((p.N + 63) / 64, (p.M + CS_ROWS - 1) / CS_ROWS), dim3(256), 0, st, p);
    } else {
        const int ncols = p.epilogue == MDX_EPI_GEGLU ? p.N / 2 : p.N;
        const size_t total = (size_t)p.M * (ncols / 8);
        const int blocks = (int)std::min<size_t>((total + 255) / 256, 2048);
        if (pl.reduce == GEMM_REDUCE_EXT)
            hipLaunchKernelGGL(splitk_reduce_kernel<true>, dim3(blocks), dim3(256), 0, st, p);
        else
            hipLaunchKernelGGL(splitk_reduce_kernel<false>, dim3(blocks), dim3(256), 0, st, p);
    }
    MDX_LAUNCH_CHECK("mdx_gemm_f16(splitk reduce)");
    return MDX_OK;
}
