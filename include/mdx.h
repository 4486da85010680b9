/* mdx.h -- C-ABI of libmdx.so: the MI355X (gfx950) kernels under the minddiffusion
 * UNet-denoising hot path.
 *
 * The reference (mindspore-lab/minddiffusion) has no FFI / operator-plugin interface:
 * its hot path is Python calling stock MindSpore primitives.  Each
 * entry point below therefore replaces one *primitive call site group* of the reference;
 * the file:line it replaces is cited per function (paths under
 * vision/stablediffusionv2/ unless noted).  INTEGRATION.md shows the ctypes binding.
 *
 * Conventions
 *  - All pointers are DEVICE pointers (HBM) unless noted; the caller owns every buffer
 *    including workspaces; the library never allocates device memory and never
 *    synchronises -- with ONE exception: the arrival counters of the in-kernel split-K reduce
 *    (16 KiB per distinct workspace address, carved from 1 MiB chunks that are zeroed when they
 *    are allocated; see mdx_gemm_desc.workspace and mdx_gemm_release_counters) for a workspace the
 *    caller has NOT bound counters of its own to (mdx_gemm_bind_counters: with it, no exception).  All work is
 *    enqueued on the caller's stream (hipStream_t passed as void*), so calls are capturable
 *    into a hipGraph.
 *  - Activations are NHWC ("token-major") fp16: [B][H*W][C]; the reference's NCHW fp32
 *    tensors exist only at the apply_model boundary (mdx_nchw_to_nhwc_f16 /
 *    mdx_nhwc_to_nchw_f32).
 *  - Weights are fp16 in a kernel-native packed format (minddiffusion_amd/ops.py: pack_gemm_weight /
 *    pack_conv_weight produce it; it is the only format mdx_gemm_f16 accepts):
 *      1. K order: nn.Dense weight [out][in] as is; nn.Conv2d weight [out][in][kh][kw] becomes
 *         [out][in/64][kh*kw][64] when in % 64 == 0 (channel-chunk major, tap minor: consecutive K tiles touch
 *         the same pixels), else [out][kh*kw][in] (only conv_in, in = 4 padded to 8);
 *      2. N and K zero-padded to multiples of 64 and stored tile-major, [N/64][K/64][64 rows][8 chunks][8 halves],
 *         with the 16-byte chunk at position q of row r holding logical chunk q ^ ((r >> 1) & 7) (the LDS
 *         bank-conflict swizzle, applied once offline), so each DMA instruction reads 1 KiB of contiguous HBM.
 *  - Return value: 0 = ok, negative = error (MDX_E_*); mdx_last_error() returns a
 *    thread-local message.  Nothing throws or exits across the ABI.
 */
#ifndef MDX_H_
#define MDX_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MDX_OK 0
#define MDX_E_INVALID (-1)     /* bad argument / unsupported shape */
#define MDX_E_WORKSPACE (-2)   /* workspace too small */
#define MDX_E_HIP (-3)         /* HIP runtime error at launch */

typedef void* mdx_stream_t; /* hipStream_t */

int mdx_version(void);
const char* mdx_last_error(void);
/* Tuning / experiment switches of the library.  PROCESS-GLOBAL MUTABLE STATE -- the one place the library departs from "re-entrant
 * per call, no global state" (SURVEY 8(b)): plain ints shared by every thread, stream and device of the process, read when a
 * launch is resolved (so a captured graph holds the values of its capture).  Defaults = what the product runs; they exist for A/B
 * measurements and the tuner.  Set them before the first launch they affect, from one thread; a host that needs two settings at
 * once needs two processes.  The library itself reads NO environment variables.  Names:
 *   gemm_tuned (1)  gemm_bm (0 = auto)  gemm_bn (0)  gemm_ring (0 = auto, 2..5)  gemm_halo (1)  gemm_halo8 (1)
 *   gemm_splitk_fixup_max (4)  gemm_spread (1)  halo_nsb (0 = auto)  gn_min_blocks (512)  gn_fused (1)
 *   attn_fast_stage (1): the attention kernel issues full KV tiles with fixed per-lane offsets + a scalar tile offset
 *   gemm_dense_issue (1): dense launches of the generic GEMM kernel issue their K tiles with a fixed per-lane offset + a scalar K offset
 *   gn_prefetch (1)  gemm_ln_prefetch (1): round-5 "latency diet" -- parameters that are cold in HBM (GroupNorm gamma / beta /
 *   FiLM rows, LayerNorm-fold S[n] and row statistics) are fetched at the top of the kernel instead of behind the dependency
 *   they used to follow; 0 restores the round-4 order for A/B runs (same results bit for bit either way)
 *   gemm_lean_dense (1): round 6 -- dense row-major launches run the lean kernel of csrc/dense.hip (same tile program and bits as the
 *   generic kernel; division-free prologue, the epilogue's global reads prefetched before the K loop); 0 = generic kernel, for A/B runs
 *   (the full list with defaults: csrc/mdx_common.h enum MdxOpt)
 * Unknown names return MDX_E_INVALID. */
int mdx_set_option(const char* name, int value);
int mdx_get_option(const char* name, int* value);

/* ---- layout boundary: LatentDiffusion.apply_model casts/wraps (ldm/models/diffusion/ddpm.py:290-306) */
/* x [B][C][H][W] fp32 -> y [B][H*W][Cpad] fp16, channels C..Cpad-1 zero-filled. */
int mdx_nchw_to_nhwc_f16(const float* x, void* y, int B, int C, int H, int W, int Cpad, mdx_stream_t s);
/* x [B][H*W][Cstride] fp16 -> y [B][C][H][W] fp32 (first C channels). */
int mdx_nhwc_to_nchw_f32(const void* x, float* y, int B, int C, int H, int W, int Cstride, mdx_stream_t s);

/* ---- SRGAN post-upscaler of Taichu-GLIDE (Taichu-GLIDE/model/glide_text2im/model/srgan.py:75-117): the two 9 x 9 convs at the
 *      ends of the Generator (the 3 x 3 trunk and the sub-pixel layers run on mdx_gemm_f16 with MDX_EPI_PRELU / MDX_OUT_D2S2).
 * conv_in  (srgan.py:83-85):   x fp32 NCHW [B][3][H][W] -> out = PReLU(conv9x9(x) + bias), NHWC fp16 [B][H][W][64];
 *                              w fp16 [64][3][9][9] (reference layout), bias / slope fp32 [64].
 * conv_out (srgan.py:115-116): x NHWC fp16 [B][H][W][64] -> out = tanh(conv9x9(x) + bias), fp32 NCHW [B][3][H][W];
 *                              w fp16 [3][64][9][9], bias fp32 [3].
 * Zero "same" padding (4), stride 1; the input is rounded to fp16 inside conv_in, accumulation is fp32. */
int mdx_srgan_conv_in_f16(const float* x, const void* w, const float* bias, const float* slope, void* out, int B, int H, int W,
                          mdx_stream_t s);
int mdx_srgan_conv_out_f32(const void* x, const void* w, const float* bias, float* out, int B, int H, int W, mdx_stream_t s);

/* ---- nn.GroupNorm(32,C,eps) [+ SiLU]  (ldm/modules/diffusionmodules/util.py:87-108,
 *      openaimodel.py:136-137,159-160,521-523; attention.py:83-84 eps 1e-6)
 * Input is the channel-concatenation of x1 [B][HW][C1] and optional x2 [B][HW][C2]
 * (openaimodel.py:568 Concat is never materialised).  Statistics in fp32.
 * y [B][HW][C1+C2] fp16.  gamma/beta fp32 [C1+C2].
 * ws: fp32 workspace of at least mdx_groupnorm_ws_floats(B, HW, C1+C2, groups) floats. */
size_t mdx_groupnorm_ws_floats(int B, int HW, int C, int groups);
int mdx_groupnorm_f16(const void* x1, int C1, const void* x2, int C2, const float* gamma, const float* beta,
                      void* y, int B, int HW, int groups, float eps, int silu, float* ws, mdx_stream_t s);

/* Which launch form mdx_groupnorm_f16 / mdx_groupnorm_scaleshift_f16 (colstats_nrb == 0) or mdx_groupnorm_colstats_f16
 * (colstats_nrb > 0: row blocks per sample of the column partials) resolves to for this shape under the current library options
 * (host only, no launch; the launch and this query share one decision function).
 * out6 = { form, cw (16-byte chunk columns per block), ncb (column blocks), nblk (pixel slabs per sample), pix (pixels per slab),
 *          threads per block };  form: 0 two launches (statistics + apply), 1 one launch that reads the tensor twice,
 * 2 one launch that keeps its pixels in registers, 3 one launch with 256-thread blocks, 4 apply with column statistics.
 * (mdx_groupnorm_from_splitk_f16 has its own predicate, mdx_groupnorm_from_splitk_ok.) */
int mdx_groupnorm_query(int C1, int C2, int B, int HW, int groups, int colstats_nrb, int* out6);

/* GroupNorm whose statistics come from its producers' column partials (mdx_gemm_desc.colstats_out) instead of a reduction
 * pass over the tensor: ONE launch (normalise + affine [+ SiLU]) and one read of x instead of two launches and two reads.
 * cs1 / cs2: the producers' colstats buffers of x1 / x2 ([B * nrb][C][2] fp32), nrb1 / nrb2 = row blocks per sample
 * (HW / rows per block).  scale / shift: optional FiLM rows as in mdx_groupnorm_scaleshift_f16 (NULL for the plain norm).
 * Deterministic (fixed-order folds, no atomics). */
int mdx_groupnorm_colstats_f16(const void* x1, int C1, const float* cs1, int nrb1, const void* x2, int C2, const float* cs2,
                               int nrb2, const float* gamma, const float* beta, const float* scale, const float* shift,
                               int mod_ld, void* y, int B, int HW, int groups, float eps, int silu, mdx_stream_t s);

/* Two-level fold of a producer's column partials: dst[b][j][c] = sum of the f = ceil(nrb / nrb2) consecutive row blocks
 * j f .. j f + f - 1 of src[b][.][c] (src [B * nrb][C][2], dst [B * nrb2][C][2], nrb2 == ceil(nrb / f)).  Tensors with hundreds of
 * row blocks per sample (Taichu-GLIDE's 128 x 128 / 256 x 256 levels) are folded once to <= 64 blocks and then normalised by
 * mdx_groupnorm_colstats_f16 -- one small launch instead of the statistics pass over the tensor. */
int mdx_colstats_fold_f32(const float* src, int nrb, float* dst, int nrb2, int B, int C, mdx_stream_t s);

/* Same with the FiLM modulation of GLIDE's ResBlock (Taichu-GLIDE/.../unet.py:203-208):
 *   y = silu?( GN(x) * (1 + scale[b][c]) + shift[b][c] ),  scale/shift fp32 rows of stride mod_ld. */
int mdx_groupnorm_scaleshift_f16(const void* x1, int C1, const void* x2, int C2, const float* gamma,
                                 const float* beta, const float* scale, const float* shift, int mod_ld, void* y,
                                 int B, int HW, int groups, float eps, int silu, float* ws, mdx_stream_t s);

/* ---- nn.LayerNorm([C], eps) (attention.py:176-178): rows x C fp16 -> fp16, fp32 statistics. */
int mdx_layernorm_f16(const void* x, const float* gamma, const float* beta, void* y, int rows, int C, float eps,
                      mdx_stream_t s);

/* ---- nn.Conv2d 3x3/1x1 and nn.Dense as one MFMA implicit-GEMM
 *      (openaimodel.py:50,81,138,163,174,352,524; attention.py:44,66,108-112,212,231)
 * out[m][n] = sum_k A[m][k] * W[n][k]  (+bias[n]) (+rowbias[b(m)][n]) (+residual[m][n])
 *   m = (b, yo, xo) output pixel / token;  k = (tap, cin);  A gathered on the fly from the
 *   NHWC source(s) with zero padding, optional stride 2 (Downsample) and optional nearest-2x
 *   upsample of the source (Upsample, openaimodel.py:57) folded into the gather.             */
typedef struct mdx_gemm_desc {
    const void* a;        /* source 1, NHWC fp16 [B][H][W][c1] */
    const void* a2;       /* optional source 2 (channel concat), [B][H][W][c2], or NULL */
    int c1, c2;           /* Cin = c1 + c2 (each a multiple of 8) */
    const void* w;        /* packed weights (format above), logical shape [N][ksize*ksize*Cin] */
    const float* bias;    /* [N] fp32 or NULL */
    const float* rowbias; /* [B][rowbias_ld] fp32 per-sample bias (ResBlock emb add, openaimodel.py:188-200) or NULL */
    int rowbias_ld;
    const void* residual; /* fp16 [M][residual_ld] or NULL (skip / transformer residual adds) */
    int residual_ld;
    void* out;            /* fp16 */
    int out_ld;           /* row stride (elements) of out for out_mode 0; token stride for out_mode 1 */
    int B, H, W;          /* source spatial extent per sample (Dense: H = tokens, W = 1) */
    int N;                /* output channels (multiple of 8; GEGLU: 2x the produced width, interleaved packing) */
    int ksize;            /* 1 or 3 (3 => pad 1) */
    int stride;           /* 1 or 2 */
    int upsample;         /* 1: nearest-2x upsample the source before the conv */
    int epilogue;         /* MDX_EPI_* */
    int out_mode;         /* MDX_OUT_* */
    int splitk;           /* 0 = auto, >=1 = number of K splits */
    void* workspace;      /* split-K workspace, 16-byte aligned (may be NULL when splitk <= 1).  Row-major launches reduce IN the
                             kernel: every (tile, split) block parks its fp32 partial in the workspace and takes a ticket on
                             the tile's arrival counter; the block that completes a tile sums the partials in split order and
                             runs the epilogue (no reduce launch).  The counters are LIBRARY-owned, one set per (device,
                             workspace address), always zero between launches: the workspace needs no initialisation (rounds 2
                             and 3 kept them in the first MDX_GEMM_WS_HEAD bytes of the workspace, which made "zeroed by the
                             caller" -- later "zeroed on first sight of an address" -- part of the contract; both broke on
                             buffers an allocator hands out twice).  The first MDX_GEMM_WS_HEAD bytes stay reserved.  Launches
                             that can run concurrently (two streams) need distinct workspaces, as their partials always did.
                             Transposed-output split launches use [split][M][N] slabs + a reduce
                             launch as before (no counters). */
    size_t workspace_bytes;
    long out_bs;          /* row-major only: element stride between samples (0 = dense); lets a projection write
                             into a token sub-range of a larger [B][tokens][C] buffer (GLIDE text|image keys) */
    void* out2;           /* split output (n_split > 0): columns [0, n_split) go row-major to `out` as usual, columns      */
    int out2_ld;          /* [n_split, N) go TRANSPOSED to out2[(b * (N - n_split) + n - n_split) * out2_ld + tok]:      */
    int n_split;          /* q|k and V^T of a self-attention in ONE launch (attention.py:108-112; Taichu-GLIDE unet.py:289-297 with
                             out_bs: q | k of the image tokens behind the text keys).  Multiple of 128; bias only (no rowbias /
                             residual / epilogue). */
    int asym_pad;         /* 3x3 stride-2 only: zero-pad bottom / right instead of all around (VAE Encoder Downsample,
                             ldm/modules/diffusionmodules/model.py:55-78) */
    /* nn.LayerNorm folded into the two GEMMs around it (BasicTransformerBlock, attention.py:176-185):
     *   LN(x) W^T + b  =  rstd_m * ( x (gamma (.) W)^T  -  mean_m * S )  +  (W beta + b),   S[n] = sum_k (gamma (.) W)[n][k]
     * PRODUCER (the GEMM that writes the token rows x; row-major, N % 64 == 0): stats_out[m][N / 64][2] fp32 receives
     * {sum, sum of squares} of every 64-column slice of the fp16 row it stores.
     * CONSUMER (dense 1x1 GEMM over those rows, K = the producer's N): `w` holds fp16(gamma (.) W), `bias` holds
     * W beta + b, ln_stats = the producer's stats_out, ln_nt = K / 64, ln_s = S computed from the fp16 weights.
     * The correction is applied to the fp32 accumulators (or to the split-K sum) before bias / activation. */
    float* stats_out;
    const float* ln_stats;
    const float* ln_s;
    int ln_nt;
    float ln_eps;
    /* GroupNorm statistics from the producer (openaimodel.py:136,159: every GroupNorm input is a conv / Dense output): when
     * set, the launch also writes, for every ROW BLOCK of its output and every output column n,
     *   colstats_out[(row_block * N + n) * 2 + {0,1}] = {sum, sum of squares} of the fp16 values stored in that column,
     * rows per block = the M tile (a HALO conv tile = one 8x16 pixel patch), 64 for a split-K launch that still uses the
     * separate reduce kernel; mdx_gemm_query reports the number.  Per COLUMN, so that any consumer grouping -- channel
     * concats, groups that are not aligned to the store granule -- can fold them (mdx_groupnorm_colstats_f16).  Plain row-major
     * launches only (no GEGLU / transposed / n_split / LayerNorm fold / out_bs); tokens per sample % rows per block == 0. */
    float* colstats_out;
    int colstats_cap;     /* row blocks colstats_out has room for: a launch that would write more fails (MDX_E_INVALID) */
    int defer_reduce;     /* split-K launches only: write the fp32 slabs and do NOT launch the reduce -- the consumer,
                             mdx_groupnorm_from_splitk_f16, sums them while it normalises (it must run before any other launch
                             reuses the workspace).  mdx_gemm_f16 fails if the launch does not split. */
    int tile_m;           /* 0 = auto (tuned table, then the cost model); 64 | 128 forces the M tile.  For tools/tune_gemm.py,
                             which measures the (tile_m, splitk) candidates of every UNet shape on the device. */
    int tile_n;           /* 0 = auto; 64 | 128 forces the N tile (same purpose; GEGLU uses 128 with geglu_unit 0 / 64).  160 with
                             tile_m = 128: the 128 x 160 tile of the lean dense kernel (four waves 4 x 1) -- dense row-major launches
                             with bias / residual / GEGLU (geglu_unit = 80) / LayerNorm-fold consumer, unsplit; anything else is
                             refused with tile_n = 160 */
    /* nn.GroupNorm(32) [+ SiLU] of the conv's INPUT applied inside the conv (openaimodel.py:136-138, 159-163: GroupNorm -> SiLU ->
     * Conv2d): gn_colstats = the column partials the input's producer emitted (mdx_gemm_desc.colstats_out /
     * mdx_st_tail_desc.colstats_out: [B * gn_nrb][Cin][2]), gn_gamma / gn_beta fp32 [Cin].  Every block folds its sample's
     * partials into a per-channel {scale, shift} table and normalises the halo slices in LDS after they land; `a` is then the RAW
     * tensor and no GroupNorm launch runs.  Single-source 3x3 stride-1 convs with Cin %% 64 == 0, Cin <= 640, images larger than
     * 8 x 8, that resolve to the HALO kernel with 64-column tiles (mdx_gemm_query: out7[3] == 1, out7[1] == 64).
     * DENSE launches (ksize = 1; round 5): nn.GroupNorm(32) WITHOUT an activation in front of a Dense / 1x1 conv
     * (SpatialTransformer.norm -> proj_in, attention.py:243-247; GLIDE AttentionBlock.norm -> qkv): set gn_silu = 0.  The block folds
     * the partials into fp16 {scale, shift} tables and applies them to the A fragments between LDS and the matrix pipe (one packed fma
     * per two values).  Single source, Cin %% 64 == 0, Cin <= 2560, tokens per sample %% tile_m == 0 (mdx_gemm_query out7[0]). */
    const float* gn_colstats;
    const float* gn_gamma;
    const float* gn_beta;
    int gn_nrb;
    int gn_silu;
    float gn_eps;
    /* ResBlock skip_connection fused into the block's second conv (openaimodel.py:174, 201-205): when skip_w is set,
     *   out = conv3x3(a) + conv1x1(cat(skip_a, skip_a2)) (+ bias + rowbias + residual ...),
     * the 1x1 conv over the block's RAW input riding on this launch as extra K tiles (one accumulator, one epilogue; `bias` must
     * hold the SUM of the two convs' biases).  skip_a / skip_a2: NHWC fp16 [B][H][W][skip_c1 / skip_c2] (same H, W), channels
     * multiples of 64; skip_w: packed tile-major weights of logical shape [N][skip_c1 + skip_c2].  Single-source 3x3 stride-1
     * convs that resolve to the HALO kernel only (mdx_gemm_query out7[3] == 1); not with w_frag. */
    const void* skip_a;
    const void* skip_a2;
    int skip_c1, skip_c2;
    const void* skip_w;
    int w_frag;           /* 1: `w` is packed in MFMA-FRAGMENT order instead of the tile-major format above -- [N / 32 column tiles]
                             [K / 16 k-steps][64 lanes][8 halves], piece (ct, s)[lane] = W[32 ct + lane % 32][16 s + 8 (lane / 32)
                             + 0..7], K in the conv order of item 1 (ops.pack_conv_weight_frag) -- and the launch streams it
                             HBM -> registers (weight-streaming form of the HALO 3x3 conv for M <= 512: no weight tiles in LDS,
                             one barrier per 64-channel chunk).  3x3 / stride 1 / single source / Cin % 64 == 0 convs that
                             resolve to the HALO kernel only; set tile_m = 128.  Results are bit-identical to the tile-major form. */
    int stages;           /* 0 = auto; 2 .. 6 forces the depth of the LDS ring the K tiles are DMA'd through (same purpose; 64-row
                             tiles up to 6, 128-row tiles up to 5, HALO weight ring 2 | 3); 10 | 11 = depth 2 | 3 with EIGHT
                             waves per block (generic kernel, tile_m = 128 only); 8 | 9 with tile_m = 256 = the eight-wave 3x3 conv
                             core (conv8p.hip; 9: one phase per 32-deep k-step) */
    const void* w_sub;    /* upsample = 1 only, optional: the SUB-PIXEL weights of the nearest-2x + 3x3 conv (openaimodel.py:57-60).
                             For output parity (dy, dx) the conv is a 2 x 2 conv of the low-resolution source with pre-summed taps --
                             rows {y-1+dy, y+dy}: dy = 0 -> {w[0], w[1]+w[2]}, dy = 1 -> {w[0]+w[1], w[2]}; columns likewise -- packed like
                             a conv weight of logical shape [4 N][Cin][2][2], parity-major rows (ops.pack_subpixel_conv_weight).  When set
                             and the shape suits the eight-wave conv core (Cin % 64 == 0, N % 64 == 0, H % 16 == 0, W % 16 == 0, single
                             source) the launch computes 4 Cin instead of 9 Cin products per output on the un-upsampled tensor; otherwise
                             `w` and the upsampling gather are used.  The summed taps are rounded to fp16 once: results differ from the
                             nine-product form by fp16 rounding of the weights (parity-tested against the oracle at the usual 1e-3). */
    /* Cross-attention over a short cached context as the EPILOGUE of its query projection (round 6; BasicTransformerBlock.attn2,
     * attention.py:108, 138-152 with the context keys / values of :119-121 cached per context tensor): when xattn_k is set the launch
     * computes q = a W^T (with the LayerNorm fold if ln_stats is set), keeps each 64-column tile of it -- ONE HEAD: the head dim must be
     * 64 -- on chip, and writes  out[m][64 h ..] = softmax(q_h K_h^T * xattn_scale) V_h  instead of q: the separate attention launch and
     * the fp16 round trip of q disappear, the arithmetic is that of mdx_attention_f16 on the fp16-rounded q (bit-identical).
     *   xattn_k  [B][xattn_cap][N] fp16 (keys, row-major: head h in columns 64 h ..), xattn_vt [B][N][xattn_cap] fp16 (values, transposed),
     *   xattn_len <= 1024 keys of xattn_cap rows are attended to (64-key tiles; past two tiles they are re-staged in LDS pair by pair:
     *   a launch with xattn_len <= 128 keeps its LDS size, its occupancy and its bits).
     * Dense row-major launches only (ksize 1, one source, no epilogue / residual / statistics / n_split / out_bs), N % 64 == 0, tokens per
     * sample % 128 == 0 (or % 64 == 0 with tile_m = 64); set tile_n = 64 and splitk = 1. */
    const void* xattn_k;
    const void* xattn_vt;
    int xattn_len;
    int xattn_cap;
    float xattn_scale;
    /* MDX_EPI_PRELU (SRGAN, Taichu-GLIDE model/glide_text2im/model/srgan.py:41-72,83-96): per-channel slope of column n =
     * act_slope[n % act_slope_n] (fp32; act_slope_n % 8 == 0, N % act_slope_n == 0).  out = prelu(acc + bias) (+ residual): the
     * residual is added AFTER the activation (Generator.conv2 + conv1, srgan.py:113).  No rowbias. */
    const float* act_slope;
    int act_slope_n;
    /* MDX_EPI_GEGLU only: the packing unit of `w` / `bias` / `ln_s` -- every 2 * unit consecutive packed columns are `unit` 'a' columns
     * followed by their `unit` gate columns.  0 (= 64): the 128-column tiles; 80: the 128 x 160 tile of the lean dense kernel
     * (N %% 160 == 0).  The unit must be the one of the tile that runs: a descriptor whose unit does not match the resolved tile_n is
     * refused (MDX_E_INVALID) by mdx_gemm_check / mdx_gemm_query / mdx_gemm_f16 -- a mismatch would pair the wrong columns silently. */
    int geglu_unit;
} mdx_gemm_desc;

#define MDX_GEMM_WS_HEAD 16384 /* reserved bytes at the head of mdx_gemm_desc.workspace (the arrival counters' former home; their size) */
#define MDX_EPI_NONE 0
#define MDX_EPI_GEGLU 1 /* out[m][j] = a * gelu_tanh(g); packed so that each 128-wide N tile = 64 'a' | 64 'gate' cols
                           (attention.py:41-51); mdx_gemm_desc.geglu_unit = 80: 80 'a' | 80 'gate' per 160-wide tile */
#define MDX_EPI_GELU 2  /* out = gelu_tanh(acc + bias)  (GLIDE text-transformer MLP, xf.py:52-59; SDv2 text encoder MLP) */
#define MDX_EPI_QUICKGELU 3 /* out = x * sigmoid(1.702 x), x = acc + bias  (Wukong text encoder, WK text_encoder.py:67-74) */
#define MDX_EPI_PRELU 4 /* out = x > 0 ? x : act_slope[n % act_slope_n] * x, x = acc + bias  (SRGAN nn.PReLU, srgan.py:41-117) */
#define MDX_OUT_ROWMAJOR 0   /* out[m * out_ld + n] */
#define MDX_OUT_TRANSPOSED 1 /* out[(b * N + n) * out_ld + tok]: V^T for mdx_attention_f16 */
#define MDX_OUT_D2S2 2       /* depth-to-space by 2 in DCR order (MindSpore ops.DepthToSpace(2), srgan.py:60-72): N = 4 C, and column n of
                                output pixel (b, y, x) goes to out[((b * 2 Ho + 2 y + q / 2) * 2 Wo + 2 x + q % 2) * out_ld + n % C],
                                q = n / C; out_ld >= C is the pixel stride of the [B][2 Ho][2 Wo][out_ld] output.  C % 8 == 0; plain or
                                PReLU epilogue, no residual / out_bs / n_split / statistics.  Runs on the generic kernel. */

int mdx_gemm_f16(const mdx_gemm_desc* d, mdx_stream_t s);
/* Frees the library-owned split-K arrival counters (nothing may be in flight); later launches allocate them again.  Every hipGraph
 * captured with a split launch holds the address of its workspace's counters: destroy such graphs first. */
int mdx_gemm_release_counters(void);
/* Hands the counters of ONE workspace (16 KiB per distinct workspace address) back for reuse by the next workspace that needs a set:
 * call it when a workspace is freed, so that a long-lived process that plans at many resolutions does not accumulate them.  Same
 * precondition (nothing in flight, no live graph captured with this workspace).  Returns the number of sets released (0 = the
 * workspace never carried a split launch).  The counters' device is taken from the workspace POINTER, not the calling thread. */
int mdx_gemm_release_workspace(const void* workspace);
/* Caller-owned arrival counters: binds `counters` -- MDX_GEMM_WS_HEAD bytes of ZEROED device memory on the workspace's device,
 * 16-byte aligned, alive and untouched by the caller until mdx_gemm_release_workspace(workspace) -- to the workspace ADDRESS.
 * Launches on a bound workspace take their tickets there, and the library then allocates NOTHING for them: the ownership rule
 * above holds without its exception (what a host that captures graphs on its own allocator wants; minddiffusion_amd/ops.py
 * new_gemm_workspace binds a set to every workspace it creates).  Every launch leaves the counters zero.  Rebinding the same
 * pair is a no-op; binding another set replaces the previous one (nothing may be in flight, no live graph captured with it). */
int mdx_gemm_bind_counters(const void* workspace, void* counters);
/* Bytes of split-K workspace mdx_gemm_f16 wants for this problem under its auto heuristic (0 if none). */
size_t mdx_gemm_workspace_bytes(const mdx_gemm_desc* d);
/* Host-only validation of a descriptor (no launch): MDX_OK or MDX_E_INVALID with mdx_last_error() set. */
int mdx_gemm_check(const mdx_gemm_desc* d);
/* What mdx_gemm_f16 WOULD launch for this descriptor (host only, nothing is launched):
 * out7 = {tile_m, tile_n, splitk, kernel (0 = generic implicit GEMM, 1 = HALO 3x3 conv, 2 = the lean dense kernel), 1 if the choice came from the
 * measured tile table csrc/gemm_tuned.inc (0 for a row of csrc/gemm_tuned160.inc, the table of the 128 x 160 tile: tile_n = 160
 * says so), rows per colstats_out row block (0 = this launch cannot produce column
 * statistics), 1 if a split launch reduces in the kernel (no reduce launch follows)}.  The parity tests assert with it that
 * the table rows are hit at the benchmarked shapes. */
int mdx_gemm_query(const mdx_gemm_desc* d, int* out7);
/* First-use tuner for shapes the measured tile table does not list (no reference counterpart; the reference's graph compiler
 * picks its kernels).  Times every distinct launch form the library has for this descriptor (tile_m x tile_n x split-K) on
 * stream `s` -- median of `reps` (1 .. 31, 0 = 5) launches each, after a hipMemsetAsync of `flush` (may be NULL; >= 512 MiB
 * evicts L2 and the Infinity Cache, i.e. weights arrive cold as they do inside a UNet evaluation) -- and returns the fastest in
 * best4 = {tile_m, tile_n, splitk, stages} for the descriptor's override fields; all zero = keep the library's choice (it won, or
 * lost by < 2 %).  us2 (may be NULL) = {library's choice, best} in microseconds.  The CALLER keeps the answer (ops.tune_cache);
 * the library stores nothing.  This is the one entry that SYNCHRONISES (event waits on `s`): not capturable; every trial
 * overwrites d->out.  Descriptors with colstats_out, defer_reduce or w_frag are refused (their consumer / weight packing is
 * tied to the launch form). */
int mdx_gemm_tune(const mdx_gemm_desc* d, mdx_stream_t s, void* flush, size_t flush_bytes, int reps, int* best4, float* us2);

/* GroupNorm fused with the split-K reduce of its producer (the small tensors of the deep UNet levels, where one block
 * normalises a whole (sample, column block) and the conv in front of it is always split): `prod` is the descriptor of a conv /
 * Dense that ran with defer_reduce = 1.  One launch sums the slabs in slab order, applies the producer's bias / time-embedding
 * row / residual, stores the producer's fp16 output, computes the statistics of those fp16 values and writes
 * y = GroupNorm(out) [+ SiLU] -- bit-identical to the reduce kernel followed by mdx_groupnorm_f16.  Returns MDX_E_INVALID when
 * the tensor does not fit the one-block-per-column-block scheme (the caller then must not defer). */
int mdx_groupnorm_from_splitk_f16(const mdx_gemm_desc* prod, const float* gamma, const float* beta, void* y, int groups,
                                  float eps, int silu, mdx_stream_t s);
/* 1 if mdx_groupnorm_from_splitk_f16 can consume this producer (host only). */
int mdx_groupnorm_from_splitk_ok(const mdx_gemm_desc* prod, int groups);

/* ---- CrossAttention core: softmax(q k^T * scale) v, flash-style (attention.py:138-152);
 *      the [b*h, N, N] score tensor of the reference is never materialised.
 * q  : fp16, element (b, i, h*D + d) at q[b*q_bs + i*q_ld + h*D + d]
 * k  : fp16, element (b, j, h*D + d) at k[b*k_bs + j*k_ld + h*D + d]
 * vt : fp16 TRANSPOSED values, element (b, h*D + d, j) at vt[b*vt_bs + (h*D+d)*vt_ld + j];
 *      columns Nk..vt_ld-1 must be finite (zero-filled by the caller)
 * o  : fp16, same addressing as q with o_bs/o_ld.   D in {40, 64, 80, 160}
 *      (SDv2 / GLIDE: 64; Wukong-Huahua num_heads=8: 40 / 80 / 160, WK/configs/v1-inference-chinese.yaml:31). */
int mdx_attention_f16(const void* q, long q_bs, int q_ld, const void* k, long k_bs, int k_ld, const void* vt,
                      long vt_bs, int vt_ld, void* o, long o_bs, int o_ld, int B, int heads, int D, int Nq, int Nk,
                      float scale, mdx_stream_t s);

/* ---- The same attention with the KEY tiles of every (batch, head, 128-query block) item dealt to `kv_splits` blocks
 *      (attention.py:138-152; flash-decoding style).  For launches whose items do not fill the chip once -- the 64 x 64 and
 *      32 x 32 self-attentions of a UNet evaluation at batch 2: 320 / 160 items on 256 CUs -- every split block keeps its own
 *      running (reference, row sum, O), parks the normalised fp16 partial in `ws`, and the last arriver of an item stores
 *      sum_s w_s O_s / sum_s w_s with w_s = l_s 2^(m_s - max m), summed in split order (schedule-independent bits).
 * kv_splits : 0 = the library chooses (mdx_attention_ws_bytes tells how much workspace that needs; option attn_kv_split),
 *             1 = no split (same launch as mdx_attention_f16), 2..8 = that many (each split needs >= 2 key tiles of 64).
 * ws        : device memory, ZERO on the first use, at least mdx_attention_ws_bytes() bytes for kv_splits = 0 or
 *             65536 + items * kv_splits * (128 * D * 2 + 1024) bytes otherwise (items = B * heads * ceil(Nq / 128) <= 16384);
 *             its first 64 KiB hold one arrival counter per item, which every launch leaves at zero -- so one workspace serves all attention launches of a
 *             stream in turn, but never two streams at once.  NULL: no split. */
size_t mdx_attention_ws_bytes(int B, int heads, int D, int Nq, int Nk);
int mdx_attention_splitkv_f16(const void* q, long q_bs, int q_ld, const void* k, long k_bs, int k_ld, const void* vt,
                              long vt_bs, int vt_ld, void* o, long o_bs, int o_ld, int B, int heads, int D, int Nq, int Nk,
                              float scale, int kv_splits, void* ws, size_t ws_bytes, mdx_stream_t s);

/* ---- Row-local fused tail of a SpatialTransformer block: everything BasicTransformerBlock.construct does after the
 *      self-attention core, plus SpatialTransformer's proj_out, as ONE launch (attention.py:151-152 to_out, :177 norm2,
 *      :108 to_q, :138-150 cross-attention over the cached context keys, :183, :178 norm3, :41-70 GEGLU feed-forward, :184,
 *      :231 proj_out, :256 residual):
 *        t1 = attn_out Wo1^T + bo1 + tok;   q2 = LN2(t1) Wq2^T;   o2 = softmax(q2 K_ctx^T scale) V_ctx;
 *        t2 = o2 Wo2^T + bo2 + t1;   h = GEGLU(LN3(t2) W1^T + b1);   t3 = h W2^T + b2 + t2;   out = t3 Wpo^T + bpo + x_in
 *      A block owns `tile_rows` token rows for the whole chain (A operands resident in LDS, weights streamed HBM/L2 -> registers
 *      in MFMA fragment order); none of q2, o2, t1, t2, the [M][4C] GEGLU intermediate or t3 goes through HBM.
 * attn_out / tok / x_in / out: fp16 [B * tokens][C] dense.  ctx_k: fp16 [B][ctx_cap][C] = to_k(context), rows >= ctx_len
 * finite; ctx_vt: fp16 [B][C][ctx_cap] = to_v(context) transposed (what the cached-context GEMMs of the unfused path write).
 * wstream: the six weight matrices packed by minddiffusion_amd/ops.py: pack_st_tail (per wave w of the C / 32 waves, ONE
 *   contiguous stream of 1 KiB pieces in consumption order; piece (matrix, column tile ct, k-step s)[lane][8] =
 *   W[32 ct + lane % 32][16 s + 8 (lane / 32) + 0..7]); mdx_st_tail_stream_bytes(C) bytes.
 * vec: fp32 [16 C] = [bo1 | gamma2 | beta2 | bo2 | gamma3 | beta3 | b1 (8C: a | gate, reference order) | b2 | bpo].
 * colstats_out: optional [B * tokens / tile_rows][C][2] fp32 = per row block and column {sum, sum of squares} of the fp16
 *   values stored to `out` (the layout of mdx_gemm_desc.colstats_out, rows per block = tile_rows), for the next GroupNorm.
 * debug_out (tests only): when non-NULL the launch stops after stage `debug_stage` and writes that stage's [M][C] fp16 rows
 *   there instead of finishing (1 t1, 2 LN2(t1), 3 q2, 4 o2, 5 t2, 6 LN3(t2), 7 t3). */
typedef struct mdx_st_tail_desc {
    const void* attn_out;
    const void* tok;
    const void* x_in;
    void* out;
    const void* ctx_k;
    const void* ctx_vt;
    const void* wstream;
    const float* vec;
    float* colstats_out;
    void* debug_out;
    int debug_stage;
    int B, tokens;        /* M = B * tokens rows; tokens % tile_rows == 0 */
    int C, heads, dim_head;
    int ctx_len, ctx_cap; /* keys used / row capacity of ctx_k (ctx_vt row length); ctx_cap % 8 == 0, <= 1024.
                           * ctx_len <= 96: one pass over the keys (whatever ctx_cap is); longer: 96-key chunks with online softmax */
    float scale;          /* dim_head ** -0.5 */
    float ln_eps;
    int tile_rows;        /* 32 | 64 */
    int warm;             /* 0 = no L2 warmer wave (A/B switch), anything else = default */
} mdx_st_tail_desc;
#define MDX_ST_DEBUG_COUNT_BARRIERS 100 /* debug_stage: run the whole chain WITHOUT the L2 warmer wave and write the number of block
                                           barriers the compute waves executed (int32) to debug_out[0] */
/* Barriers in the schedule the warmer wave walks beside the compute waves (hand-mirrored in csrc/stchain.hip): the two must agree
 * or the product launch deadlocks; tests compare them. */
int mdx_st_tail_sched_barriers(int C, int tile_rows);
int mdx_st_head_sched_barriers(int C, int tile_rows);
int mdx_st_tail_f16(const mdx_st_tail_desc* d, mdx_stream_t s);
/* 1 if mdx_st_tail_f16 has a kernel for this shape (host only): C = 320 with 5 x 64 or 8 x 40 heads today. */
int mdx_st_tail_supported(int C, int heads, int dim_head, int tokens_per_sample, int tile_rows);
size_t mdx_st_tail_stream_bytes(int C);

/* ---- Row-local fused head of a SpatialTransformer block, one launch: SpatialTransformer.norm (GroupNorm(32, eps 1e-6), its
 *      statistics folded from the producer's column partials) -> proj_in -> BasicTransformerBlock.norm1 -> attn1.to_q | to_k |
 *      to_v (attention.py:83-84, 212, 241-247, 176, 108-112).
 * x: fp16 [B * tokens][C] (the block's NHWC input); colstats: [B * nrb][C][2] fp32 = per row block and column {sum, sum of
 * squares} of x as its producer emitted them (mdx_gemm_desc.colstats_out / mdx_st_tail_desc.colstats_out), nrb row blocks per
 * sample.  Outputs: tok [M][C] (the token stream = residual of attn1), qk [M][2C] row-major (q | k), vt [B][C][vt_ld] = V
 * transposed -- the operands of mdx_attention_f16.
 * wstream: ops.pack_st_head (per wave: proj_in, to_q, to_k, to_v column tiles in MFMA fragment order);
 * vec fp32 [5C] = [gn gamma | gn beta | b_proj_in | ln1 gamma | ln1 beta].
 * debug_out / debug_stage (tests): 1 GroupNorm(x), 2 tok, 3 LN1(tok). */
typedef struct mdx_st_head_desc {
    const void* x;
    const float* colstats;
    int nrb;
    const void* wstream;
    const float* vec;
    void* tok;
    void* qk;
    void* vt;
    int vt_ld;
    void* debug_out;
    int debug_stage;
    int B, tokens, C;
    float gn_eps, ln_eps;
    int tile_rows;        /* 32 | 64 */
    int warm;             /* 0 = no L2 warmer wave (A/B switch) */
} mdx_st_head_desc;
int mdx_st_head_f16(const mdx_st_head_desc* d, mdx_stream_t s);
int mdx_st_head_supported(int C, int tokens_per_sample, int tile_rows);
size_t mdx_st_head_stream_bytes(int C);

/* ---- timestep_embedding (util.py:111-131): t [M] fp32 -> out [M][dim] fp32 = [cos | sin]. */
int mdx_timestep_embedding_f32(const float* t, float* out, int M, int dim, float max_period, mdx_stream_t s);

/* ---- small-M nn.Dense for the time-embedding MLP and the 22 emb_layers
 *      (openaimodel.py:341-345,150-157): out[M][N] = act_out(act_in(x)[M][K] @ W[N][K]^T + b)
 * x, out fp32; W fp16; b fp32.  act: 0 none, 1 SiLU. */
int mdx_dense_small_f32(const float* x, int x_ld, const void* w, const float* b, float* out, int out_ld, int M,
                        int N, int K, int act_in, int act_out, mdx_stream_t s);

/* ---- fused sampler update (ldm/models/diffusion/plms.py:188-197, 210-244)
 * eps_u / eps_c: UNet outputs, NHWC fp16 [B][HW][eps_ld] (first C channels used).
 *   e_t = eps_c                                  if eps_u == NULL
 *       = eps_u + cfg_scale * (eps_c - eps_u)    otherwise            (plms.py:197)
 *   e'  = coef[0]*e_t + coef[1]*old1 + coef[2]*old2 + coef[3]*old3     (plms.py:231-244; DDIM: coef = {1,0,0,0};
 *         the 'pseudo improved Euler' second call passes coef = {.5,.5,0,0} with old1 = first e_t)
 *   pred_x0 = (x - sqrt_one_minus_at * e') / sqrt_at                   (plms.py:218)
 *   x_prev  = sqrt_a_prev * pred_x0 + dir_coef * e' + sigma * noise    (plms.py:222-226)
 * x, old*, noise, e_t_out, x_prev, pred_x0: NCHW fp32 [B][C][H][W] (noise may be NULL when sigma == 0;
 * old* may be NULL when their coef is 0; e_t_out / pred_x0 may be NULL).  x_prev may alias x.
 * coef4 is a HOST pointer to 4 floats (read at call time). */
int mdx_sampler_step_f32(const float* x, const void* eps_u, const void* eps_c, int eps_ld, float cfg_scale,
                         const float* old1, const float* old2, const float* old3, const float* coef4,
                         float sqrt_at, float sqrt_one_minus_at, float sqrt_a_prev, float dir_coef, float sigma,
                         const float* noise, float* e_t_out, float* x_prev, float* pred_x0, int B, int C, int H,
                         int W, mdx_stream_t s);

/* ---- the same fused update for a model whose output is eps or v (SD 2.x 768-v checkpoints, `parameterization: "v"`)
 * The reference's LatentDiffusion stops at eps / x0 (ddpm.py:65); its dpm_solver.py:281-284 carries the conversion for
 * model_type "v", and upstream LDM's predict_eps_from_z_and_v is the same two lines.
 * out_u / out_c: UNet outputs, NHWC fp16 [B][HW][out_ld] (first C channels used).
 *   m   = out_c                                  if out_u == NULL
 *       = out_u + cfg_scale * (out_c - out_u)    otherwise            (plms.py:197, applied to the model outputs)
 *   e_t = m                                                            pred_type == MDX_PRED_EPS
 *       = sqrt_at_model * m + sqrt_one_minus_at_model * x_model        pred_type == MDX_PRED_V   (dpm_solver.py:281-284)
 * then e', pred_x0, x_prev exactly as mdx_sampler_step_f32 (e_t_out receives the converted eps, so a multistep history
 * holds eps).  x_model, sqrt_at_model, sqrt_one_minus_at_model: the latent and the schedule point the model was EVALUATED
 * at -- not x / sqrt_at / sqrt_one_minus_at in the second call of the PLMS first step (plms.py:231-235: model at
 * (x_next, t_next), update applied to x at index).  x_model: NCHW fp32 like x; NULL = x; not read for MDX_PRED_EPS.
 * x_prev may alias x and / or x_model (x_model[i] is read before the first store for element i, x[i] before x_prev[i] is
 * stored); the outputs may alias no other input.
 * With MDX_PRED_EPS the launch IS mdx_sampler_step_f32's (x_model is not read), bit for bit.
 * coef4 is a HOST pointer to 4 floats (read at call time). */
#define MDX_PRED_EPS 0
#define MDX_PRED_V 1
int mdx_sampler_step_pred_f32(const float* x, const float* x_model, const void* out_u, const void* out_c, int out_ld,
                              float cfg_scale, int pred_type, float sqrt_at_model, float sqrt_one_minus_at_model,
                              const float* old1, const float* old2, const float* old3, const float* coef4,
                              float sqrt_at, float sqrt_one_minus_at, float sqrt_a_prev, float dir_coef, float sigma,
                              const float* noise, float* e_t_out, float* x_prev, float* pred_x0, int B, int C, int H,
                              int W, mdx_stream_t s);

/* ---- the same fused update with guidance rescale (Lin et al., "Common Diffusion Noise Schedules and Sample Steps are
 * Flawed", section 3.4; `guidance_rescale` of the SD 2.x samplers).  Neither reference tree has it.  Per sample b, on the
 * model outputs as the UNet wrote them (v or eps: before the conversion), N = C * H * W:
 *   m    = out_u + cfg_scale * (out_c - out_u)
 *   f[b] = guidance_rescale * std(out_c[b]) / std(m[b]) + (1 - guidance_rescale)      std unbiased (/ (N - 1)), fp32, from
 *          the fp16 values as stored (first C of out_ld channels); f[b] = 1 when std(m[b]) is 0 or not finite
 *   m'   = f[b] * m
 * then e_t from m', e', pred_x0, x_prev exactly as mdx_sampler_step_pred_f32.  ONE launch: a workgroup per sample reduces the
 * statistics (sums of v - K, K = the mean of the sample's first 64 values: not a one-pass E[x^2] - E[x]^2) and then applies
 * the update.  factor_out: device [B] fp32, receives f; may be NULL.
 * Aliasing as mdx_sampler_step_pred_f32: x_prev may alias x and / or x_model, the outputs (factor_out included) alias no
 * other input; the statistics read only out_u / out_c.
 * guidance_rescale == 0 or out_u == NULL (no guidance: f == 1) is the launch of mdx_sampler_step_pred_f32 with the same
 * arguments, bit for bit, and factor_out is filled with 1.0 on the same stream.
 * Refused before any launch: guidance_rescale outside [0, 1] or not finite, C * H * W < 2, and everything
 * mdx_sampler_step_pred_f32 refuses.  coef4 is a HOST pointer to 4 floats (read at call time). */
int mdx_sampler_step_rescale_f32(const float* x, const float* x_model, const void* out_u, const void* out_c, int out_ld,
                                 float cfg_scale, int pred_type, float sqrt_at_model, float sqrt_one_minus_at_model,
                                 const float* old1, const float* old2, const float* old3, const float* coef4,
                                 float sqrt_at, float sqrt_one_minus_at, float sqrt_a_prev, float dir_coef, float sigma,
                                 const float* noise, float* e_t_out, float* x_prev, float* pred_x0,
                                 float guidance_rescale, float* factor_out, int B, int C, int H, int W, mdx_stream_t s);

/* ---- the same fused update with every per-sample scalar read from a device table: requests with different guidance
 * scales, rescale strengths and step counts (so different schedule points) share ONE launch.  Neither reference tree has it.
 * table: device [B][MDX_STEP_ROW] fp32, row b = the scalars of sample b:
 *   [MDX_STEP_ACTIVE]                   1 = update this sample, 0 = its schedule has ended (below)
 *   [MDX_STEP_CFG_SCALE]                cfg_scale
 *   [MDX_STEP_RESCALE]                  guidance_rescale (phi), in [0, 1]
 *   [MDX_STEP_SQRT_AT_MODEL], [MDX_STEP_SQRT_ONE_MINUS_AT_MODEL]     read for MDX_PRED_V only
 *   [MDX_STEP_C0 + k], k = 0..3         coef4[k]
 *   [MDX_STEP_SQRT_AT], [MDX_STEP_SQRT_ONE_MINUS_AT], [MDX_STEP_SQRT_A_PREV], [MDX_STEP_DIR_COEF], [MDX_STEP_SIGMA]
 *   [14]                                reserved, 0 (for the middle scale of three-branch guidance, mdx_sampler_step_dual_f32:
 *                                       the table and slot entries take no middle branch yet)
 *   [15]                                reserved, 0
 * An ACTIVE row b computes what the scalar entry for its scalars computes on sample b alone, bit for bit:
 * mdx_sampler_step_rescale_f32 if phi != 0 and out_u is given, else mdx_sampler_step_pred_f32 (with MDX_PRED_EPS:
 * mdx_sampler_step_f32).  A term is skipped -- its tensor not read -- when its pointer is NULL OR the row's coefficient is
 * exactly 0 (coef4[1..3] for old1..3, sigma for noise): one sample of a batch may be on a lower-order step while the pointer
 * is live for the others.  A row with phi == 0 has f = 1 exactly, reads no statistics, and factor_out[b] = 1.
 * An INACTIVE row b: x_prev[b] = x[b], copied (nothing to do where x_prev aliases x); pred_x0[b], e_t_out[b] and
 * factor_out[b] are NOT written.
 * any_rescale: non-zero iff some active row has phi != 0.  Then a workgroup owns a sample (as in
 * mdx_sampler_step_rescale_f32) and out_u must be given; with 0 every row runs with f = 1 whatever its phi says, and a
 * sample is spread over several workgroups.
 * Aliasing as mdx_sampler_step_pred_f32: x_prev may alias x and / or x_model element for element; the outputs alias no
 * other input, and nothing aliases the table.  Only x_prev, pred_x0, e_t_out and factor_out are written.
 * Refused before any launch: everything mdx_sampler_step_pred_f32 refuses, table == NULL, any_rescale with out_u == NULL or
 * with C * H * W < 2, C * H * W above 31 bits, B above 65535 without any_rescale.  The table's VALUES are on the device and are
 * not checked here: whoever builds the table checks them (finite, phi in [0, 1], sqrt_at != 0 on active rows). */
#define MDX_STEP_ROW 16
#define MDX_STEP_ACTIVE 0
#define MDX_STEP_CFG_SCALE 1
#define MDX_STEP_RESCALE 2
#define MDX_STEP_SQRT_AT_MODEL 3
#define MDX_STEP_SQRT_ONE_MINUS_AT_MODEL 4
#define MDX_STEP_C0 5
#define MDX_STEP_SQRT_AT 9
#define MDX_STEP_SQRT_ONE_MINUS_AT 10
#define MDX_STEP_SQRT_A_PREV 11
#define MDX_STEP_DIR_COEF 12
#define MDX_STEP_SIGMA 13
int mdx_sampler_step_table_f32(const float* x, const float* x_model, const void* out_u, const void* out_c, int out_ld,
                               int pred_type, const float* old1, const float* old2, const float* old3,
                               const float* noise, float* e_t_out, float* x_prev, float* pred_x0, const float* table,
                               int any_rescale, float* factor_out, int B, int C, int H, int W, mdx_stream_t s);

/* ---- Sampling sessions: the B samples of a batch are SLOTS that requests enter and leave while the batch keeps running
 * (continuous batching; neither reference tree has it).  Slot b owns, all on the device and written only when a request is
 * admitted into it:
 *   sched[b][cap][MDX_STEP_ROW] fp32   the rows of its request, one per model evaluation, as mdx_sampler_step_table_f32 reads them
 *   slot_start[b], slot_len[b]  int32  the session tick of the request's first model evaluation, and its step count
 * At session tick `tick` (a host argument of every entry below) the slot stands at pos = tick - slot_start[b] and is ACTIVE iff
 * 0 <= pos < min(slot_len[b], cap).  Nothing on the device changes between admissions: no cursor, no advance launch.
 *
 * mdx_sampler_step_slots_f32: mdx_sampler_step_table_f32 with row b = sched[b][pos_b].  An active slot computes, bit for bit,
 * what the table entry computes on that row (the kernels run the same device bodies); a slot that is not active, or whose row has
 * [MDX_STEP_ACTIVE] == 0, is an INACTIVE row of the table entry: x_prev[b] = x[b] (nothing to do where they alias), pred_x0[b],
 * e_t_out[b] and factor_out[b] not written.  any_rescale, the two launch forms and the aliasing contract are the table entry's;
 * nothing aliases sched / slot_start / slot_len.  Refused before any launch: what the table entry refuses, a NULL sched /
 * slot_start / slot_len, cap <= 0, tick < 0. */
int mdx_sampler_step_slots_f32(const float* x, const float* x_model, const void* out_u, const void* out_c, int out_ld,
                               int pred_type, const float* old1, const float* old2, const float* old3,
                               const float* noise, float* e_t_out, float* x_prev, float* pred_x0, const float* sched,
                               const int* slot_start, const int* slot_len, int cap, int tick, int any_rescale,
                               float* factor_out, int B, int C, int H, int W, mdx_stream_t s);
/* dst[r * B + b][0 .. n) = src[b][pos_b][0 .. n) for r < reps and every ACTIVE slot b (src [B][cap][n], dst [reps * B][n], fp32,
 * contiguous, not overlapping); the dst rows of a slot that is not active are not written.  One launch; 16-byte loads and
 * stores where n % 4 == 0 and both bases are 16-byte aligned, single floats otherwise.  With reps = 2 this puts the
 * time-embedding rows of a tick into the [uncond; cond] layout of the guidance batch.  MDX_E_INVALID (nothing launched): a NULL
 * pointer, B <= 0 or > 65535, n <= 0, reps <= 0, cap <= 0, tick < 0. */
int mdx_slot_gather_f32(const float* src, const int* slot_start, const int* slot_len, int cap, int tick, float* dst, int B, long n,
                        int reps, mdx_stream_t s);

/* ---- the step launch of the whole DPM-Solver (dpm_solver.py:332-1123: orders 1-3, multistep and singlestep, data and noise
 * prediction form, dynamic thresholding): the model value of one evaluation and the linear form every update of the solver is
 * (dpm_solver.solver_plan folds the reference's difference terms into the coefficients), ONE launch.
 * x_base, x_model: NCHW fp32 [B][C][H][W]; out_u (NULL = no guidance) / out_c: UNet outputs, NHWC fp16 [B][HW][out_ld], first C
 * channels used.  Per element, in this order (N = C * H * W per sample):
 *   1. m = out_c, or out_u + cfg_scale * (out_c - out_u) with out_u
 *   2. m = f[b] * m       guidance rescale, f[b] as mdx_sampler_step_rescale_f32 defines it (on the outputs as stored, before
 *                         any conversion); only with guidance_rescale != 0 and out_u
 *   3. e = m                                  pred_type == MDX_PRED_EPS
 *        = alpha_m * m + sigma_m * x_model    pred_type == MDX_PRED_V       (dpm_solver.py:281-284)
 *   4. val = e                                value_type == MDX_VALUE_EPS   (noise_prediction_fn)
 *          = (x_model - sigma_m * e) / alpha_m   value_type == MDX_VALUE_X0 (data_prediction_fn :370-373), an IEEE divide
 *   5. thresholding != 0 (:374-383, MDX_VALUE_X0 only): with k = (int)((N - 1) * 0.995) and a <= b the k-th and (k+1)-th
 *      smallest |val| of sample b (0-based, ties counted),
 *        s = a + (b - a) * 0.995f      each operation rounded to fp32, nothing fused
 *        s = max(s, max_val)
 *        val = min(max(val, -s), s) / s
 *      a and b are found EXACTLY: a radix select (8-bit digits, most significant first) on the bit patterns of |val|, which
 *      order as unsigned integers; b = a if at least k + 2 values are <= a, else the smallest value above a.  This is the
 *      reference's interpolation between two order statistics, not torch.quantile's.  A NaN orders above every number.
 *   6. model_out = val
 *   7. x_out = A * x_base + c0 * val + c1 * h1 + c2 * h2
 * A term of 7 whose coefficient is exactly 0 is SKIPPED, not multiplied: its tensor (x_base for A, h1, h2) is not read and
 * may hold anything (h1 / h2 may then be NULL).  (alpha_m, sigma_m): the schedule point the model was evaluated at, where
 * x_model is the latent it was evaluated on; x_base is the latent the update starts from (in a singlestep update the latent at
 * the start of the step while x_model is the intermediate point).
 * Outputs: model_out, x_out (NCHW fp32, required); model_pre_out (NCHW fp32, may be NULL): val before step 5 -- equal to
 * model_out without thresholding; thr_out (device [B] fp32, may be NULL): s, written only with thresholding; factor_out
 * (device [B] fp32, may be NULL): f, 1.0 where step 2 does not apply.
 * Two launch forms.  SPREAD (no rescale, no thresholding): the elements are dealt to many workgroups.  OWNED (either of them):
 * one 1024-thread workgroup per sample, which reduces the statistics and / or selects the order statistics and then applies the
 * update; with thresholding the values of step 4 wait in model_out between the passes.
 * Aliasing: x_out may be x_base and / or x_model, element for element (the same pointer).  Nothing else may overlap: no
 * output with another output, no output with an input that is read.
 * Refused before any launch (MDX_E_INVALID): a NULL x_base, x_model, out_c, model_out or x_out; a non-zero c1 / c2 with a NULL
 * h1 / h2; B, C, H, W <= 0 or out_ld < C; C * H * W above 2^31 - 1; an unknown pred_type or value_type;
 * alpha_m == 0 with MDX_VALUE_X0; thresholding with MDX_VALUE_EPS or with C * H * W < 2; thresholding with max_val not finite
 * or <= 0; guidance_rescale outside [0, 1] or not finite, or != 0 with out_u and C * H * W < 2; an overlap other than the
 * allowed aliases. */
#define MDX_VALUE_X0 0
#define MDX_VALUE_EPS 1
int mdx_sampler_step_lin_f32(const float* x_base, const float* x_model, const void* out_u, const void* out_c, int out_ld,
                             float cfg_scale, int pred_type, float guidance_rescale, int value_type, float alpha_m,
                             float sigma_m, int thresholding, float max_val, const float* h1, const float* h2, float A,
                             float c0, float c1, float c2, float* model_out, float* x_out, float* model_pre_out,
                             float* thr_out, float* factor_out, int B, int C, int H, int W, mdx_stream_t s);

/* ---- the step launch of a STOCHASTIC update (dpm_solver.solver_plan with sde_eta > 0, "DPM++ 2M SDE"): every argument of
 * mdx_sampler_step_lin_f32 with its meaning, steps 1-7 as above, and
 *   8. x_out = (the value of step 7) + cn * z       one fma
 * in the same ONE launch.  z ~ N(0, 1) per element comes from exactly one of two sources:
 *   noise: NCHW fp32 [B][C][H][W], z = noise[i]; or
 *   seeds: device [B] 64-bit seeds, z = the value mdx_randn_f32(seeds, stream, draw, scale 1, dropout 0) stores for element i
 *          of sample b (counted from the sample's start) -- drawn inside the launch, bit for bit (Philox4x32-10 at counter
 *          (i >> 2, draw, stream, 0) under key seeds[b], Box-Muller as described there), never stored.
 * Sample b's noise depends on seeds[b] alone: a row of a batch is bit-equal to the B == 1 launch with that seed.
 * cn == 0 IS mdx_sampler_step_lin_f32, bit for bit: neither source is read (both may be NULL, or point anywhere).
 * Both launch forms carry step 8 (with thresholding it belongs to the finishing pass).  In them a thread works on the four
 * consecutive elements of one Philox call, with either source, so the two sources give the same bits for the same z.
 * Aliasing: as above -- x_out may be x_base and / or x_model; noise and seeds may overlap no output.
 * Refused before any launch (MDX_E_INVALID): cn not finite; cn != 0 with both sources or with neither; stream >= 2^31 (the top
 * bit belongs to the dropout decisions of a stream); everything mdx_sampler_step_lin_f32 refuses. */
int mdx_sampler_step_lin_noise_f32(const float* x_base, const float* x_model, const void* out_u, const void* out_c, int out_ld,
                                   float cfg_scale, int pred_type, float guidance_rescale, int value_type, float alpha_m,
                                   float sigma_m, int thresholding, float max_val, const float* h1, const float* h2, float A,
                                   float c0, float c1, float c2, float* model_out, float* x_out, float* model_pre_out,
                                   float* thr_out, float* factor_out, float cn, const float* noise,
                                   const unsigned long long* seeds, unsigned stream, unsigned draw, int B, int C, int H, int W,
                                   mdx_stream_t s);

/* ---- three-branch guidance (InstructPix2Pix, Brooks et al. 2023: an instruction and an input image guide separately).  Every
 * model evaluation has three outputs, out_u (empty text, zero image latent), out_m (empty text, image latent) and out_c
 * (instruction, image latent), and step 1 of both step families becomes, per element,
 *   m = out_u + mid_scale * (out_m - out_u) + cfg_scale * (out_c - out_m)
 *     = fma(cfg_scale, out_c - out_m, fma(mid_scale, out_m - out_u, out_u))      both differences rounded, both products fused
 * (mid_scale is the image guidance scale s_I, cfg_scale the text guidance scale s_T).  Everything after step 1 acts on m as
 * before: the guidance rescale (f[b] pulls std(m[b]) to std(out_c[b]), the statistics read all three outputs), the v -> eps
 * conversion, the multistep / history terms, the data or noise prediction, dynamic thresholding and the step noise.
 * out_m: NHWC fp16 with the layout and out_ld of out_u / out_c, first C channels used.
 *   mdx_sampler_step_dual_f32      every argument of mdx_sampler_step_rescale_f32 with its meaning, plus out_m, mid_scale.
 *                                  guidance_rescale == 0: the SPREAD form (factor_out filled with 1.0), else the OWNED form.
 *   mdx_sampler_step_lin_dual_f32  every argument of mdx_sampler_step_lin_noise_f32 with its meaning, plus out_m, mid_scale.
 *                                  SPREAD or OWNED by that entry's rule (rescale or thresholding: OWNED); cn == 0 reads no noise
 *                                  source and launches the kernels without step 8.
 * ONE launch each.  In the OWNED forms the third stream of loads is issued with the others of a thread's batch of four elements.
 * out_m == out_u (the same pointer) gives the two-branch entry's bits for cfg_scale, out_m == out_c its bits for
 * cfg_scale = mid_scale: a difference of exactly 0 adds exactly 0.
 * out_m == NULL is the two-branch entry (mdx_sampler_step_rescale_f32 / mdx_sampler_step_lin_noise_f32) with the remaining
 * arguments: the same checks, the same launch, mid_scale not read.
 * Aliasing: as the two-branch entries; out_m may overlap no output.
 * Refused before any launch (MDX_E_INVALID), with out_m given: out_u == NULL ("out_m without out_u"); mid_scale not finite; out_m
 * overlapping e_t_out, x_prev, pred_x0 or factor_out (eps entry) / any output (lin entry); everything the two-branch entry
 * refuses. */
int mdx_sampler_step_dual_f32(const float* x, const float* x_model, const void* out_u, const void* out_c, int out_ld,
                              float cfg_scale, int pred_type, float sqrt_at_model, float sqrt_one_minus_at_model,
                              const float* old1, const float* old2, const float* old3, const float* coef4, float sqrt_at,
                              float sqrt_one_minus_at, float sqrt_a_prev, float dir_coef, float sigma, const float* noise,
                              float* e_t_out, float* x_prev, float* pred_x0, float guidance_rescale, float* factor_out,
                              const void* out_m, float mid_scale, int B, int C, int H, int W, mdx_stream_t s);
int mdx_sampler_step_lin_dual_f32(const float* x_base, const float* x_model, const void* out_u, const void* out_c, int out_ld,
                                  float cfg_scale, int pred_type, float guidance_rescale, int value_type, float alpha_m,
                                  float sigma_m, int thresholding, float max_val, const float* h1, const float* h2, float A,
                                  float c0, float c1, float c2, float* model_out, float* x_out, float* model_pre_out,
                                  float* thr_out, float* factor_out, float cn, const float* noise,
                                  const unsigned long long* seeds, unsigned stream, unsigned draw, const void* out_m,
                                  float mid_scale, int B, int C, int H, int W, mdx_stream_t s);

/* ---- the step launch of UniPC (Zhao et al. 2023, the multistep predictor-corrector; uni_pc.unipc_plan folds the paper's
 * difference terms D_j into the coefficients): after one model evaluation, the CORRECTED latent at the evaluation's time and the
 * PREDICTED latent at the next time -- the next model input, built from the corrected one -- in ONE launch.
 * Every argument up to max_val is mdx_sampler_step_lin_f32's, and steps 1-6 (CFG combine, guidance rescale, v -> eps, data or
 * noise prediction, dynamic thresholding, model_out = val) are that entry's, statement for statement.  Then, per element:
 *   7. xc = Ac * x_base + d0 * val + d1 * h1 + d2 * h2 + d3 * h3      has_corrector != 0: step 7 of the lin entry on
 *                                                                     (Ac, x_base, d0, d1 h1, d2 h2), then one fma with d3 h3
 *      xc = x_model                                                   has_corrector == 0: the bits copied (Ac, d0 .. d3 not read)
 *      x_corr_out = xc
 *   8. xp = Ap * xc + e0 * val + e1 * h1 + e2 * h2                    step 7 of the lin entry on (Ap, xc as stored, e0, e1 h1, e2 h2)
 *      x_pred_out = xp
 * h1, h2, h3: the model values of the three evaluations before this one, newest first (NCHW fp32).  A term whose coefficient
 * is exactly 0 is SKIPPED, not multiplied; a history neither form has a coefficient for is not read and may be NULL or hold
 * anything, and so may x_base with has_corrector == 0 or Ac == 0.
 * So has_corrector == 0 gives, in model_out, x_pred_out, thr_out and factor_out, the bits of mdx_sampler_step_lin_f32 on
 * (x_base = x_model, A = Ap, c = e), and d3 == 0 gives, in model_out, x_corr_out, thr_out and factor_out, its bits on
 * (x_base, A = Ac, c = d0 .. d2).
 * Outputs: model_out, x_corr_out, x_pred_out (NCHW fp32, required); model_pre_out, thr_out, factor_out as the lin entry has
 * them.  Launch forms by the lin entry's rule: SPREAD without rescale and thresholding, else OWNED (one 1024-thread workgroup
 * per sample, the lin entry's statistics pass and radix select; a thresholded value waits in model_out between the passes).
 * Every form reads each input once and makes one pass over the latents.
 * Aliasing: x_corr_out may be x_base and x_pred_out may be x_model, element for element (the same pointer).  Nothing else may
 * overlap: no output with another output (x_corr_out and x_pred_out included), no output with an input that is read.
 * Refused before any launch (MDX_E_INVALID): everything mdx_sampler_step_lin_f32 refuses (x_base may be NULL here without a
 * corrector; x_corr_out and x_pred_out take x_out's place); a non-zero d1 / e1, d2 / e2 or d3 with a NULL h1, h2 or h3;
 * has_corrector with a NULL x_base; an overlap other than the two allowed aliases. */
int mdx_sampler_step_pc_f32(const float* x_base, const float* x_model, const void* out_u, const void* out_c, int out_ld,
                            float cfg_scale, int pred_type, float guidance_rescale, int value_type, float alpha_m,
                            float sigma_m, int thresholding, float max_val, const float* h1, const float* h2, const float* h3,
                            int has_corrector, float Ac, float d0, float d1, float d2, float d3, float Ap, float e0, float e1,
                            float e2, float* model_out, float* x_corr_out, float* x_pred_out, float* model_pre_out,
                            float* thr_out, float* factor_out, int B, int C, int H, int W, mdx_stream_t s);

/* ---- GLIDE (Taichu-GLIDE/model/glide_text2im) specifics --------------------------------------------------
 * AvgPool2d(2,2) / ResizeNearestNeighbor x2 of a ResBlock's skip path (unet.py:46-49,74,180-185); NHWC fp16. */
int mdx_avgpool2x2_f16(const void* x, void* y, int B, int H, int W, int C, mdx_stream_t s);
int mdx_upsample_nearest2x_f16(const void* x, void* y, int B, int H, int W, int C, mdx_stream_t s);
/* token + positional embedding with padding replacement (text2im_model.py:88-92):
 * out[b][t][:] = mask[b][t] ? tok_emb[tokens[b][t]] + pos[t] : pad[t];  fp16 tables, int32 tokens/mask. */
int mdx_glide_text_embed_f16(const int* tokens, const int* mask, const void* tok_emb, const void* pos,
                             const void* pad, void* out, int B, int T, int width, int n_vocab, mdx_stream_t s);
/* super-res UNet input (text2im_model.py:214-216 + gaussian_diffusion.py:307-313):
 * out NHWC fp16 [B][S*S][8] = [x (3ch) | legacy-bilinear(round((low+1)*127.5)/127.5-1, s->S) (3ch) | 0 0];
 * x [B][3][S][S] fp32, low [B][3][s][s] fp32. */
int mdx_glide_superres_input_f16(const float* x, const float* low, void* out, int B, int S, int s_low,
                                 mdx_stream_t s);
/* one fused sampler update (guider.py:73-86, gaussian_diffusion.py:79-142, 229-254):
 *   eps = out_u ? out_u[:3] + scale*(out_c[:3] - out_u[:3]) : out_c[:3];  v = out_c[3:6]
 *   logvar = (v+1)/2*log_beta + (1-(v+1)/2)*post_logvar;  x0 = clip(sqrt_recip*x - sqrt_recipm1*eps, -1, 1)
 *   mode 0 (ancestral): x_next = coef1*x0 + coef2*x + noise_scale*exp(logvar/2)*noise   (noise_scale = 0 at t = 0)
 *   mode 1 (DDIM eta=0): eps' = (sqrt_recip*x - x0)/sqrt_recipm1; x_next = sqrt_ab_prev*x0 + sqrt(1-ab_prev)*eps'
 * out_c/out_u: UNet outputs NHWC fp16 [B][HW][ld] (6 channels used); x, noise, x_next, pred_x0: NCHW fp32 [B][3][H][W].
 * coef: HOST pointer to 8 floats {log_beta, post_logvar, sqrt_recip, sqrt_recipm1, coef1, coef2, sqrt_ab_prev,
 * sqrt_one_minus_ab_prev}. */
int mdx_glide_step_f32(const float* x, const void* out_c, const void* out_u, int ld, float guidance_scale,
                       const float* coef8, int mode, float noise_scale, const float* noise, float* x_next,
                       float* pred_x0, int B, int H, int W, mdx_stream_t s);

/* Taichu-GLIDE sampling loops know every prompt before the first step (main_funcs.py:21-44 draws the unconditional prompt of
 * step k inside the loop, but from a stream that does not depend on the model): the text transformer (xf.py:126-154) and every
 * AttentionBlock's encoder_kv projection (unet.py:289-297) of ALL steps' prompts run once per loop into tables, and each step
 * copies its prompt's rows into the text slots of the blocks' key / value buffers -- ONE launch for all blocks:
 *   for slot in [0, nslots), b in [b0, b0 + nb):  entry e = entry0 + (b - b0) * entry_per_b (entry_per_b in {0, 1})
 *     dst[b * dst_batch_bytes + r * dst_pitch + 0..row_bytes) = src[e * src_entry_bytes + r * src_pitch + 0..row_bytes),  r < rows
 * (keys: rows = text tokens, row_bytes = 2 C, both pitches 2 C; transposed values: rows = C, row_bytes = 2 text tokens,
 * dst_pitch = 2 (text + image tokens)).  `slots_dev` is a DEVICE array (caller-owned); every pointer and byte count a multiple
 * of 16.  blocks_per_copy = grid blocks that share one (slot, b) copy. */
typedef struct mdx_glide_kv_slot {
    const void* src;
    void* dst;
    long src_entry_bytes;
    long dst_batch_bytes;
    long src_pitch, dst_pitch;
    int rows, row_bytes;
} mdx_glide_kv_slot;
int mdx_glide_kv_select_f16(const mdx_glide_kv_slot* slots_dev, int nslots, long entry0, int entry_per_b, int b0, int nb,
                            int blocks_per_copy, mdx_stream_t s);

/* Causal self-attention (key j visible to query i iff j <= i): the text encoder's triu(-inf) mask
 * (ldm/modules/encoders/text_encoder.py:136-139, MultiheadAttention :43-66).  Same arguments; Nq must equal Nk. */
int mdx_attention_causal_f16(const void* q, long q_bs, int q_ld, const void* k, long k_bs, int k_ld, const void* vt,
                             long vt_bs, int vt_ld, void* o, long o_bs, int o_ld, int B, int heads, int D, int Nq,
                             int Nk, float scale, mdx_stream_t s);

/* ---- VAE decoder attention (AutoencoderKL.decode -> Decoder.mid.attn_1, ldm/modules/diffusionmodules/model.py:151-206):
 * one head of d = C = 512, scores materialised as in the reference: S = Q K^T and O = P V run through mdx_gemm_f16. */
/* Re-lay a row-major fp16 ACTIVATION matrix src[rows][K] (row stride src_ld elements) as the packed B operand of
 * mdx_gemm_f16 (the format ops.pack_gemm_weight builds for weights): dst holds ceil(rows/64)*ceil(K/64)*4096 halves. */
int mdx_pack_b_operand_f16(const void* src, long src_ld, int rows, int K, void* dst, mdx_stream_t s);
/* In place: x[r][0..cols) = softmax(scale * x[r][0..cols)) for fp16 scores (P.Softmax(axis=2), model.py:192-194);
 * fp32 max / sum.  cols % 8 == 0, cols <= 16384. */
int mdx_softmax_rows_f16(void* x, long ld, int rows, int cols, float scale, mdx_stream_t s);

/* AutoencoderKL.encode's DiagonalGaussianDistribution sample (autoencoder.py:70-78): moments NHWC fp16 [B][HW][ld] =
 * [mean (zc) | logvar (zc) | ..]; out NCHW fp32 [B][zc][HW] = mean + exp(0.5 * clip(logvar, -30, 20)) * noise
 * (noise NCHW fp32, or NULL for the mode). */
int mdx_vae_gaussian_sample_f32(const void* moments, int ld, const float* noise, float* out, int B, int zc, int HW,
                                mdx_stream_t s);

/* ---- img2img: the forward-process sample and its fusion onto the encoder's posterior sample (csrc/qsample.hip).
 * q = a * x0 + b * noise (ddpm.py:197-200: a = sqrt(alphas_cumprod[t]), b = sqrt(1 - alphas_cumprod[t])), computed as
 * fma(a, x0, b * noise).  mask == NULL: out = q.  Otherwise the running latent keeps its unmasked part (plms.py:153-157):
 *   out = m * q + (1 - m) * img,   m = mask[b][mask_c == 1 ? 0 : c][p]      (mask_c is 1 or C)
 * x0, noise, img, out: NCHW fp32 [B][C][HW]; mask NCHW fp32 [B][mask_c][HW].  Where m == 0 out is img and where m == 1 out is
 * q, bit for bit; a = 1, b = 0 without a mask returns x0.  out may alias img element for element (out == img) and nothing
 * else.  16-byte accesses when HW % 4 == 0 and every pointer is 16-byte aligned, scalar ones otherwise.
 * Refused before any launch: null x0 / noise / out, mask without img, mask_c not in {1, C}, non-positive extents, an out
 * that overlaps an input other than img == out. */
int mdx_q_sample_f32(const float* x0, const float* noise, float a, float b, const float* mask, int mask_c,
                     const float* img, float* out, int B, int C, int HW, mdx_stream_t s);

/* Encoder moments -> start latent of an img2img run, one launch: with moments as mdx_vae_gaussian_sample_f32 takes them,
 *   z  = mean + exp(0.5 * clip(logvar, -30, 20)) * post_noise      (post_noise NULL: the mode, z = mean)
 *   z0 = scale_factor * z                                           (get_first_stage_encoding)
 *   xt = a * z0 + b * noise                                         (the q-sample statement of mdx_q_sample_f32)
 * post_noise, noise, z0_out, xt_out: NCHW fp32 [B][zc][HW].  Either output may be NULL, not both; xt_out needs noise.
 * scale_factor = 1 makes z0_out mdx_vae_gaussian_sample_f32's output and xt_out is mdx_q_sample_f32(z0_out, noise, a, b),
 * both bit for bit. */
int mdx_vae_encode_noised_f32(const void* moments, int ld, const float* post_noise, float scale_factor, float a, float b,
                              const float* noise, float* z0_out, float* xt_out, int B, int zc, int HW, mdx_stream_t s);

/* ---- Inpainting: the work around the sampler (wukong-huahua/inpaint.py:39-63, 76-85, 110-115; csrc/inpaint.hip).
 * Everything NCHW fp32 and contiguous unless said otherwise.  Mask convention (inpaint.py:51-55): a value >= 0.5 is the hole
 * (repaint), m = (mask >= 0.5); a mask of batch mask_b == 1 is shared by all B samples (make_batch_sd repeats it).
 * 16-byte accesses where the plane size is a multiple of 4 and the pointers are 16-byte aligned, scalar ones otherwise.
 * Every entry refuses, before any launch: null pointers (other than the ones documented as optional), non-positive extents, a
 * mask / alpha batch that is neither 1 nor B.  None of them writes outside its output.
 *
 * masked image (inpaint.py:55): out[b][c][p] = image[b][c][p] * (mask[mask_b == 1 ? 0 : b][0][p] < 0.5 ? 1 : 0), bit for bit the
 * torch expression image * (mask < 0.5).  image, out [B][C][HW]; mask [mask_b][1][HW]. */
int mdx_inpaint_mask_image_f32(const float* image, const float* mask, int mask_b, float* out, int B, int C, int HW,
                               mdx_stream_t s);

/* c_concat of the hybrid UNet, one launch after the encoder (inpaint.py:76-85): out [B][1 + zc][h][w] with
 *   channel 0      = m[(i * H) / h][(j * W) / w]  (integer arithmetic: ResizeNearestNeighbor, align_corners = False, of the
 *                    binarised [mask_b][1][H][W] mask; F.interpolate(mode="nearest") for integer ratios)
 *   channels 1..zc = scale_factor * (mean + exp(0.5 * clip(logvar, -30, 20)) * post_noise)   (post_noise NULL: the mode)
 * moments as mdx_vae_gaussian_sample_f32 takes them (NHWC fp16 [B][h * w][ld], ld >= 2 zc), post_noise [B][zc][h][w].
 * Channels 1..zc are mdx_vae_encode_noised_f32's z0_out bit for bit (the same statements in the same order).  zc == 0 (moments
 * may then be NULL) writes the resized mask alone, [B][1][h][w]. */
int mdx_inpaint_concat_f32(const void* moments, int ld, const float* post_noise, float scale_factor, const float* mask,
                           int mask_b, int H, int W, float* out, int B, int zc, int h, int w, mdx_stream_t s);

/* Soft compositing weight: alpha = min(max(m, G * m), 1), m the binarised mask [Bm][1][H][W], G the separable Gaussian whose
 * 2 * radius + 1 normalised taps `weights` (device fp32; the caller computes them in float64) are applied along rows, then along
 * columns, with replicate edges.  Inside the hole alpha is exactly 1; the ramp extends outward only.  out [Bm][1][H][W] must not
 * overlap mask.  0 <= radius <= 48.  One launch: a 32 x 32 output tile with its halo lives in LDS. */
int mdx_mask_feather_f32(const float* mask, const float* weights, int radius, float* out, int Bm, int H, int W,
                         mdx_stream_t s);

/* Output stage after the decoder (inpaint.py:110-115), one launch:
 *   t = alpha * decoded + (1 - alpha) * image   (computed as fma(alpha, decoded, (1 - alpha) * image); alpha NULL: t = decoded
 *                                                and image is not read)
 *   v = clamp((t + 1) / 2, 0, 1)
 * out_f32 NCHW [B][C][H][W] = v;  out_u8 NHWC [B][H][W][C] = (uint8)(v * 255.0f) (truncation, inpaint.py:112-115).  Either
 * output may be NULL, not both.  decoded, image [B][C][H][W]; alpha [alpha_b][1][H][W], alpha_b 1 or B.  Where alpha is 0 the
 * result is clamp((image + 1) / 2, 0, 1) and where it is 1 (or NULL) clamp((decoded + 1) / 2, 0, 1), bit for bit.  out_f32
 * must not overlap an input (refused). */
int mdx_inpaint_composite_f32(const float* decoded, const float* image, const float* alpha, int alpha_b, float* out_f32,
                              unsigned char* out_u8, int B, int C, int H, int W, mdx_stream_t s);

/* ---- Per-sample seeded noise (not in the reference, whose draws are whole-batch ms.ops.StandardNormal calls).
 * A counter-based generator: element e (0 <= e < n) of sample b is a pure function of (seeds[b], stream, draw, e) and of nothing
 * else -- not B, not b, not the alignment of out, not the launch geometry.  seeds: B 64-bit values on the device; out: [B][n]
 * contiguous, n = the elements of ONE sample (a latent: C * H * W, e = the NCHW flat index inside the sample).
 *   words   Philox4x32-10 with the Random123 constants (multipliers 0xD2511F53, 0xCD9E8D57; Weyl increments 0x9E3779B9,
 *           0xBB67AE85; ten rounds), key = (seed & 0xffffffff, seed >> 32), counter = (e >> 2, draw, stream, 0); element e takes
 *           word (e & 3) of the four output words.  mdx_philox_u32 stores that word as it is.
 *   uniform U(w) = fmaf((float)(w >> 9), 2^-23, 2^-24) = (2 (w >> 9) + 1) * 2^-24: the 23-bit integer converts exactly and the
 *           fma is exact, so 2^-24 <= U <= 1 - 2^-24 (the open interval) in fp32 and in fp64 alike.
 *   normal  Box-Muller on the word pairs (0, 1) and (2, 3) of a counter: r = sqrtf(-2 logf(U(w_a))), (s, c) = sincospif(2 U(w_b))
 *           with w_a the pair's first word; the EVEN element gets r * c (cosine), the ODD element r * s (sine).  |z| < 5.8.
 *           mdx_randn_f32 stores scale * z.  Precise logf / sqrtf / sincospif: a float64 restatement agrees to 1e-5.
 *   dropout (dropout_p > 0; plms.py:224-225 `ops.dropout(noise, p)`) element e is kept when U(word (e & 3) of the SAME counter
 *           under stream | 0x80000000) >= dropout_p and then stores (scale * z) * (1 / (1 - dropout_p)); otherwise 0.
 *           dropout_p == 0 runs a kernel without the second Philox call, so callers keep stream < 2^31.
 * n % 4 == 0 with a 16-byte aligned out writes one 16-byte vector per lane, anything else one element per lane: the same bits for
 * the same element.  MDX_E_INVALID (nothing launched) for a NULL pointer, B <= 0, n <= 0 or n > 2^34 (e >> 2 is a 32-bit counter
 * word), dropout_p outside [0, 1), a scale that is not finite. */
int mdx_philox_u32(const unsigned long long* seeds, unsigned stream, unsigned draw, unsigned* out, int B, long n, mdx_stream_t s);
int mdx_randn_f32(const unsigned long long* seeds, unsigned stream, unsigned draw, float scale, float dropout_p, float* out, int B,
                  long n, mdx_stream_t s);
/* mdx_randn_f32 with the draw counter per session slot (above): sample b of an ACTIVE slot gets draw = draw0 + pos_b (mod 2^32)
 * -- the same stream, scale and dropout semantics and the same bits per element as mdx_randn_f32 called with that draw on that
 * sample alone; the [n] span of a slot that is not active (0 <= tick - slot_start[b] < slot_len[b] fails) is not written.  Both
 * store widths as mdx_randn_f32.  MDX_E_INVALID (nothing launched): what mdx_randn_f32 refuses, a NULL slot pointer, tick < 0. */
int mdx_randn_slots_f32(const unsigned long long* seeds, unsigned stream, unsigned draw0, float scale, float dropout_p, float* out,
                        const int* slot_start, const int* slot_len, int tick, int B, long n, mdx_stream_t s);
/* The mask blend of an img2img request in a session (plms.py:153-157 per slot), one launch: for every slot b that is ACTIVE at
 * `tick` (above, with `cap`) and has blend_on[b] != 0, and every element e of its [C][HW] sample,
 *   n   = the value mdx_randn_f32 gives sample b at (stream, draw0 + pos_b mod 2^32) with scale 1 and no dropout
 *   q   = fma(a, x0[b][e], b * n),   (a, b) = blend_ab[b][pos_b][0 .. 2)           (the q-sample statement of mdx_q_sample_f32)
 *   img[b][e] = fma(keep[b][e], q, (1 - keep[b][e]) * img[b][e])                    (its blend statement)
 * x0, keep, img: NCHW fp32 [B][C][HW], contiguous; blend_ab fp32 [B][cap][2]; blend_on int32 [B].  Only the img spans of those
 * slots are written (in place); the span of a slot that is not active or has blend_on[b] == 0 is neither read nor written, and
 * the noise is never stored.  Bit for bit, per slot: mdx_randn_f32 on sample b alone at that draw followed by
 * mdx_q_sample_f32(x0[b], noise, a, b, mask = keep[b] (mask_c = C), img = out = img[b]) -- the kernels run the same device
 * bodies; where keep == 0 the element keeps its bits and where keep == 1 it is q.  16-byte accesses where HW % 4 == 0 and x0,
 * keep and img are 16-byte aligned, single floats otherwise: the same bits per element.  img aliases nothing, and nothing
 * aliases blend_ab / blend_on / seeds / slot_start / slot_len.  MDX_E_INVALID (nothing launched): a NULL pointer, B <= 0 or
 * > 65535, C <= 0, HW <= 0, C * HW > 2^34 (the generator's extent limit), cap <= 0, tick < 0. */
int mdx_slot_blend_f32(const float* x0, const float* keep, float* img, const unsigned long long* seeds, unsigned stream,
                       unsigned draw0, const float* blend_ab, const int* blend_on, const int* slot_start, const int* slot_len,
                       int cap, int tick, int B, int C, int HW, mdx_stream_t s);

/* ---- Separable resampling (not in the reference; csrc/resample.hip): the enlargement between the two passes of
 * DiffusionPipeline.hires.  One table-driven kernel: the interpolation mode never reaches the device, only tap tables do
 * (minddiffusion_amd/resample.py computes them in float64 and rounds once to fp32, as mdx_mask_feather_f32's taps travel).
 * in [B][C][H_in][W_in], out [B][C][H_out][W_out]: NCHW fp32, contiguous.  Tables, all on the device: y_start[H_out] int32 and
 * y_w[H_out][Ty] fp32 for the rows, x_start[W_out] and x_w[W_out][Tx] for the columns; a row of a table that needs fewer taps is
 * padded with zero weights.  Tap k of output column j reads input column e(x_start[j] + k): e clamps to [0, W_in - 1] (replicate
 * edge), or with wrap_x != 0 is the index mod W_in, non-negative.  Rows always clamp.  The arithmetic, fixed:
 *   1. horizontal first:  t = 0; for k ascending:  t = fmaf(x_w[j][k], in[..][e(x_start[j] + k)], t)
 *   2. t is kept in fp32
 *   3. vertical over the t values of the rows e(y_start[i] + k), the same way with y_w
 *   4. no atomics: an output element depends on its own sample and plane only.
 * Inputs must be finite where a tap reads them, zero-weight padding included (0 * inf is NaN).  16-byte stores where
 * W_out % 4 == 0 and out is 16-byte aligned, scalar ones otherwise: an element gets the same bits either way.
 * One launch; a block owns a 16 x 32 tile of outputs of one plane and stages the horizontally resampled strip it needs in LDS.
 * The strip is sized from the geometry, ceil(15 * H_in / H_out) + Ty + 2 input rows: tables whose 16 consecutive output rows
 * reach further (none of resample.tap_table's do) give wrong values there, never an access outside `in`.
 * Refused before any launch (MDX_E_INVALID): null pointers, non-positive extents, a plane of more than 2^30 pixels, B * C > 65535,
 * Tx or Ty outside [1, MDX_RESAMPLE_MAX_TAPS] (32 covers antialiased bicubic down to x1/8 and Lanczos-3 down to x1/5), an out
 * that overlaps in, a tile whose strip and tables would exceed the kernel's 40 KiB of LDS (a very large downscale: beyond
 * about x1/20 with one tap, x1/15 with 32; the message says so). */
#define MDX_RESAMPLE_MAX_TAPS 32
int mdx_resample_f32(const float* in, float* out, int B, int C, int H_in, int W_in, int H_out, int W_out, const int* y_start,
                     const float* y_w, int Ty, const int* x_start, const float* x_w, int Tx, int wrap_x, mdx_stream_t s);
/* The resample fused onto the start of an img2img run (hires with per-sample seeds), one launch: with r the value
 * mdx_resample_f32 computes,
 *   z0 = scale * r                       (one fp32 multiply)
 *   xt = fmaf(a, z0, b * n)              (the q-sample statement of mdx_q_sample_f32)
 * n = noise[b][c][i][j], or with noise == NULL the value mdx_randn_f32 gives sample b at (seeds[b], stream, draw), scale 1 and no
 * dropout, for the NCHW flat index of the element inside its OUTPUT sample [C][H_out][W_out].  A passed noise wins over seeds.
 * z0_out, xt_out, noise: [B][C][H_out][W_out].  Either output may be NULL, not both; xt_out needs a noise source.  Bit for bit:
 * scale = 1 makes z0_out mdx_resample_f32's output, and xt_out is mdx_randn_f32 followed by mdx_q_sample_f32 on z0_out -- the
 * kernels run the same device bodies (csrc/rng_device.h, csrc/qsample_device.h).  16-byte accesses where W_out % 4 == 0 and the
 * outputs and noise are 16-byte aligned, scalar ones otherwise: the same bits.  Refused: what mdx_resample_f32 refuses, no
 * output, xt_out without noise and seeds, C * H_out * W_out > 2^34, outputs that overlap in, noise or each other. */
int mdx_resample_noised_f32(const float* in, int B, int C, int H_in, int W_in, int H_out, int W_out, const int* y_start,
                            const float* y_w, int Ty, const int* x_start, const float* x_w, int Tx, int wrap_x, float scale,
                            float a, float b, const float* noise, const unsigned long long* seeds, unsigned stream, unsigned draw,
                            float* z0_out, float* xt_out, mdx_stream_t s);

/* ---- Windowed UNet evaluation (not in the reference; MultiDiffusion, Bar-Tal et al. 2023; csrc/window.hip): a latent canvas
 * larger than the resolution the UNet was trained at is evaluated as a batch of overlapping windows of that resolution, and the
 * outputs are averaged where windows overlap.
 * The window grid: per axis of canvas length L, window w and stride s the offsets are 0, s, 2s, ... while o + w < L, then a last
 * offset L - w (clamped, not padded); L == w has the single offset 0.  Window k = iy * nx + ix sits at (oy[iy], ox[ix]).  The
 * offsets are one int32 table [ny + nx], rows then columns, passed twice: `offsets` on the device (the kernels read it) and
 * `offsets_host`, the same values in host memory (checked before any launch; the kernels clamp what they read into the canvas).
 * Both entries refuse, before any launch (MDX_E_INVALID): null pointers, non-positive extents, h > Hc or w > Wc, an offset that
 * leaves the canvas (o < 0 or o + w > L), an axis whose offsets do not ascend from 0 to L - w or leave pixels uncovered (a step
 * larger than the window), an output that overlaps the input.
 *
 * gather: windows k0 .. k0 + n - 1 of canvas NCHW fp32 [NB][C][Hc][Wc] (C counts every input channel, c_concat included) into out
 * NCHW fp32 [NB * n][C][h][w]; window kk of canvas row j is output row j * n + kk, so a [uncond ; cond] canvas batch gives a
 * [uncond ; cond] window batch.  A copy: 16 bytes per lane when w, Wc and every x-offset of the range are multiples of 4 and both
 * bases are 16-byte aligned, single floats otherwise -- the same bits.  Also refused: a range outside [0, ny * nx).  Only the
 * NB * n output rows are written. */
int mdx_window_gather_f32(const float* canvas, float* out, const int* offsets, const int* offsets_host, int ny, int nx, int k0,
                          int n, int NB, int C, int Hc, int Wc, int h, int w, mdx_stream_t s);
/* average: windows NHWC fp16 [NB * N][h * w][ld], N = ny * nx, row j * N + k (the gather's order with n = N) onto out NHWC fp16
 * [NB][Hc * Wc][ld].  One lane owns 8 halves (one 16-byte access; ld == 8: one canvas pixel) and visits the windows that cover
 * its pixel in ascending k; every output element has one writer, no atomics.  Per channel c < C, with e_k the window's fp16 value:
 *   weights == NULL:  acc = (float)e_k0;  acc += (float)e_k for each further window (plain fp32 adds);
 *                     out = fp16_rne(acc / (float)count)                                   (IEEE fp32 division)
 *   weights [h * w] fp32, all > 0 (n_weights == h * w), indexed by the pixel's place inside the window:
 *                     acc = w_k0 * e_k0;  acc = fmaf(w_k, e_k, acc);  wsum = w_k0 + w_k + ... (plain adds);
 *                     out = fp16_rne(acc / wsum)
 * A pixel covered by ONE window takes that window's halves unchanged, in both forms.  Channels [C, ld) of out are written 0.
 * Also refused: ld < C or ld % 8 != 0, windows / out not 16-byte aligned, weights with n_weights <= 0 or != h * w. */
int mdx_window_average_f16(const void* windows, void* out, const float* weights, int n_weights, const int* offsets,
                           const int* offsets_host, int ny, int nx, int NB, int C, int ld, int Hc, int Wc, int h, int w,
                           mdx_stream_t s);

/* ---- Regions and wrap-around windows on the same canvas (csrc/window.hip; MultiDiffusion section 4.2 without bootstrapping).  The
 * two entries above keep their behaviour; these two add a table of window numbers, masks per region, and `wrap_x`.
 * wrap_x (0 | 1): with 1 a window at x-offset o covers canvas columns (o + i) mod Wc, i < w (w <= Wc), so the right and the left
 * edge of the canvas lie inside one window.  The wrapped x offsets are 0, s, 2s, ... while o < Wc (nx = ceil(Wc / s)); rows never
 * wrap.  Refused for a wrapped x axis: offsets that do not start at 0, do not ascend, step by more than w, a last offset >= Wc
 * or with Wc - last > w.  Everything the two entries above refuse is refused here too, the x axis by the wrapped rule when
 * wrap_x is 1; wrap_x other than 0 | 1 is refused.
 *
 * gather_rows: mdx_window_gather_f32 with the windows named by a table: rows[n] on the device, rows_host the same values on the
 * host (checked: every entry in [0, ny * nx)).  Window numbers may repeat and come in any order; output row j * n + i is window
 * rows[i] of canvas row j.  A copy: 16 bytes per lane when w, Wc and every x offset the rows use are multiples of 4 and both bases
 * are 16-byte aligned (a float4 then never straddles the seam), single floats otherwise -- the same bits.  Only the NB * n output
 * rows are written. */
int mdx_window_gather_rows_f32(const float* canvas, float* out, const int* offsets, const int* offsets_host, int ny, int nx,
                               const int* rows, const int* rows_host, int n, int wrap_x, int NB, int C, int Hc, int Wc, int h,
                               int w, mdx_stream_t s);
/* average_regions: the outputs of P (window, region) pairs, NHWC fp16 [NB * P][h * w][ld], row j * P + p, onto out NHWC fp16
 * [NB][Hc * Wc][ld].  The pairs are sorted by window k, then region r: pair_window_host[P] (host only), pair_region[P] and the
 * CSR index pair_first[N + 1] (the pairs of window k are [pair_first[k], pair_first[k + 1])), the last two on the device and
 * on the host.  masks: device fp32 [R][Hc][Wc], finite, >= 0, their sum > 0 at every pixel, and region r active (paired) in every
 * window that covers a pixel where M_r > 0 -- the caller's to guarantee (ops.RegionPlan does).  R == 0: no regions; masks and
 * the pair tables are NULL, P == ny * nx, pair p is window p and M == 1.
 *   out(p) = sum_r sum_{k covers p} q * e_{r,k}(p) / sum q,   q = M_r(p) * wt(p - origin_k),   wt == 1 without `weights`.
 * One lane owns 8 halves of one canvas pixel; one writer per element, no atomics; the covering windows are visited in ascending
 * k and the pairs of a window in ascending r.  The arithmetic, per channel c < C, is part of the contract:
 *   a term with M_r(p) == 0 is skipped BEFORE its window row is read: whatever that row holds, NaN included, cannot reach p;
 *   q = m without weights; with weights q = m * wt, one fp32 multiply;
 *   first term: acc = q * e (fp32 multiply), qsum = q;  later terms: acc = fmaf(q, e, acc), qsum = qsum + q (plain fp32 add);
 *   out = fp16_rne(acc / qsum), an IEEE fp32 division;  a pixel with exactly ONE term takes that term's halves unchanged.
 * Channels [C, ld) are written 0.  With R == 0 and wrap_x == 0, or R == 1 and an all-ones mask, this is the arithmetic of
 * mdx_window_average_f16 (1 * e and fmaf(1, e, acc) are its adds, qsum its count or weight sum) and the results are bit-equal.
 * Also refused: ld < C or ld % 8 != 0, windows / out not 16-byte aligned or overlapping, weights with n_weights != h * w,
 * P <= 0, R < 0; R == 0 with masks or P != ny * nx; R > 0 with a NULL mask or pair table, pair_first not running from 0 to P
 * without descending, a pair whose window differs from its CSR slot, a region outside [0, R), regions of one window that do not
 * ascend. */
int mdx_window_average_regions_f16(const void* windows, void* out, const float* weights, int n_weights, const int* offsets,
                                   const int* offsets_host, int ny, int nx, int wrap_x, const int* pair_window_host,
                                   const int* pair_region, const int* pair_region_host, const int* pair_first,
                                   const int* pair_first_host, int P, const float* masks, int R, int NB, int C, int ld, int Hc,
                                   int Wc, int h, int w, mdx_stream_t s);

/* ---- Tiled VAE decode (csrc/window.hip): the decoder's outputs on the tiles of a large canvas, fp32 NCHW [NB * N][C][TH][TW],
 * tile k = iy * nx + ix of canvas row j in row j * N + k (the gather's row order), blended onto the image canvas out fp32 NCHW
 * [NB][C][Hc][Wc] with feathered weights.  The grid is a window grid on the IMAGE canvas, in output pixels: offsets / offsets_host
 * as above, wrap_x (0 | 1) as in the two entries above.  One lane owns four consecutive columns of one (b, c, y) row (16-byte
 * accesses) when TW, Wc and every x offset are multiples of 4 and both bases are 16-byte aligned, one column otherwise -- the same
 * bits; every output element has one writer, no atomics, no weight tensor.  The arithmetic is part of the contract:
 *   the weight of tile-local pixel (yy, xx) is q = (float)(min(yy + 1, TH - yy, ramp_y) * min(xx + 1, TW - xx, ramp_x)), an
 *   integer (ramps in [1, 4096]: the product is exact in fp32);
 *   the covering tiles are visited in ascending k (rows, then columns);
 *   first term: acc = q * e, qsum = q;  later terms: acc = acc + q * e with the fp32 multiply and the fp32 add ROUNDED
 *   SEPARATELY (not an fma), qsum = qsum + q;
 *   raw = acc / qsum, one IEEE fp32 division;  a pixel covered by exactly ONE tile takes that tile's bits unchanged;
 *   MDX_TILE_RAW writes raw;  MDX_TILE_UNIT writes min(max((raw + 1.0f) / 2.0f, 0.0f), 1.0f), the bits of
 *   torch.clamp((raw + 1.0) / 2.0, 0.0, 1.0).
 * Refused, before any launch (MDX_E_INVALID): null pointers, wrap_x other than 0 | 1, everything the window entries refuse of the
 * extents and the offset table (the x axis by the wrapped rule when wrap_x is 1), a ramp < 1 or > 4096, an unknown mode, out
 * overlapping tiles.  Only out is written. */
enum { MDX_TILE_RAW = 0, MDX_TILE_UNIT = 1 };
int mdx_tile_blend_f32(const float* tiles, float* out, const int* offsets, const int* offsets_host, int ny, int nx, int wrap_x,
                       int NB, int C, int Hc, int Wc, int TH, int TW, int ramp_y, int ramp_x, int mode, mdx_stream_t s);

/* ---- LoRA merge (wukong-huahua ldm/modules/attention.py:118-126 applies y = x W^T + (alpha / rank) (x A^T) B^T + b as a side
 * branch of every LoRADense; here the adapter is merged into the weight, in place, in the layout the kernels read):
 *     acc = 0;  for r in 0..R-1 (ascending): acc = fmaf(B[n][r], A[r][k], acc)          (fp32)
 *     W'[n][k] = fp16_rne(fmaf(scale, acc, base[n][k]))
 * base fp32 [N][K] row-major, A fp32 [R][K], B fp32 [N][R] (A or B NULL, or R == 0: a pure re-pack, W' = fp16(base)), R <= 64,
 * K % 8 == 0.  With gamma != NULL the LayerNorm fold of mdx_gemm_desc.ln_stats is applied to the MERGED matrix exactly as
 * ops.fold_layernorm does from its fp16 input: the stored value is wg = fp16(fp32(double(W') double(gamma[k]))) (the exact product, through fp32 as that conversion goes),
 * S[n] = fp32(sum_k double(wg)), cb[n] = fp32(sum_k double(W') double(beta[k]) + bias[n]) (bias may be NULL); S / cb point at
 * this matrix's first entry.  Reductions are deterministic (no atomics).
 * The matrix occupies rows [dst_n0, dst_n0 + N) of a destination of dst_N rows:
 *   MDX_LORA_ROWMAJOR  fp16 [dst_N][ld];
 *   MDX_LORA_TILED     the packed weight storage of mdx_gemm_f16: [ceil(dst_N/64)][ceil(K/64)][64][8][8], position q of row r
 *                      holds logical chunk q ^ ((r >> 1) & 7); padding columns are written as zeros, and the matrix that ends
 *                      the destination (dst_n0 + N == dst_N) also writes the zero padding rows;
 *   MDX_LORA_FRAG      MFMA-fragment pieces [dst_N/32][piece_stride][512] (ops.pack_frag_weight); the matrix's K/16 k-steps are
 *                      pieces [piece_offset, piece_offset + K/16) of every column tile (the per-wave streams of
 *                      mdx_st_tail_f16 / mdx_st_head_f16).
 * Bytes of dst outside that region are not touched. */
enum { MDX_LORA_ROWMAJOR = 0, MDX_LORA_TILED = 1, MDX_LORA_FRAG = 2 };
typedef struct mdx_lora_merge_desc {
    const float* base;
    const float* A;
    const float* B;
    int N, K, R;
    float scale;
    const float* gamma;
    const float* beta;
    const float* bias;
    float* S;
    float* cb;
    void* dst;
    int layout;
    int ld;               /* ROWMAJOR: row stride in halves */
    int dst_n0, dst_N;
    int piece_stride, piece_offset;     /* FRAG */
} mdx_lora_merge_desc;
int mdx_lora_merge_f16(const mdx_lora_merge_desc* d, mdx_stream_t s);

/* ---- ControlNet residual add (Zhang et al. 2023, cldm.py ControlledUnetModel.forward: `h += control.pop()` on the middle
 * block's output and on every skip connection): up to MDX_CONTROL_MAX_SEGS residual tensors added into the UNet's activations,
 * in place, by ONE launch.  Segment s is {dst[s], src[s], elems_per_row[s]}: dst[s] fp16 [nb][elems_per_row[s]] (rows dense),
 * src[s] fp16 [>= 1 + max src_row][elems_per_row[s]].  For destination row r of segment s and element e, with q = src_row[r]:
 *     q < 0:   dst[s][r][e] is neither read nor written;
 *     else:    dst[s][r][e] = fp16_rne(fmaf(scale[s * nb + r], float(src[s][q][e]), float(dst[s][r][e])))      (fp32)
 * -- one fused multiply-add in fp32 and one explicit round-to-nearest-even to fp16.  src (n_seg device pointers), src_row
 * (int32 [nb]) and scale (fp32 [n_seg][nb]) are DEVICE tables read when the kernel runs: a captured graph serves any scales,
 * any row mapping and any source buffers without being captured again.  The caller guarantees src_row[r] < the rows of every
 * source.  No atomics; the same inputs give the same bits.
 * Refused, before any launch (MDX_E_INVALID): a null descriptor, n_seg outside [1, 16], nb < 1, a null or misaligned table
 * (src 8-byte, src_row / scale 4-byte), a null dst, a dst that is not 16-byte aligned, an elems_per_row that is not a positive
 * multiple of 8.  The source pointers live on the device: their 16-byte alignment is the table writer's to check
 * (ops.ControlAdd.set_sources).  Only the dst rows with src_row >= 0 are written. */
#define MDX_CONTROL_MAX_SEGS 16
typedef struct mdx_control_add_desc {
    int n_seg;
    int nb;                                     /* destination batch rows */
    void* dst[MDX_CONTROL_MAX_SEGS];
    int elems_per_row[MDX_CONTROL_MAX_SEGS];    /* halves per batch row (H * W * C of the tensor) */
    const void* const* src;                     /* DEVICE: n_seg pointers */
    const int* src_row;                         /* DEVICE: [nb] */
    const float* scale;                         /* DEVICE: [n_seg][nb] */
} mdx_control_add_desc;
int mdx_control_add_f16(const mdx_control_add_desc* d, mdx_stream_t s);

/* x <- silu(x) in place on n fp16 values (n a positive multiple of 8, x 16-byte aligned), fp32 arithmetic inside: the
 * activation between the convs of the ControlNet hint block (seven launches per hint, once per hint image). */
int mdx_silu_f16(void* x, size_t n, mdx_stream_t s);

/* ---- probes used by tests to pin hardware layout assumptions (not on the hot path) */
int mdx_probe_mfma_32x32x16_f16(const void* a, const void* b, float* c, mdx_stream_t s);
/* Same for v_mfma_f32_16x16x32_f16 (the conv8p core): a, b = 64 lanes x 8 halves, c = 64 lanes x 4 floats. */
int mdx_probe_mfma_16x16x32_f16(const void* a, const void* b, float* c, mdx_stream_t s);
/* streaming-bandwidth probe of the HBM/L2 -> LDS DMA path (mode 0) vs plain vector loads (mode 1) */
int mdx_probe_dma_stream(const void* src, size_t bytes_per_block, int nblocks, int waves, int per, int ns, int mode,
                         int stride_tiles, float* sink, mdx_stream_t s);

/* streaming probe of the L2 -> VGPR path the fused-chain kernels use for their weights: each wave reads its own contiguous
 * bytes_per_wave region in 1 KiB pieces, pf in flight; shared = 1: every block reads the same regions (tools/l2_probe.py) */
int mdx_probe_l2_stream(const void* src, size_t total_bytes, unsigned bytes_per_wave, int nblocks, int waves, int pf,
                        int shared, float* sink, mdx_stream_t s);

/* diagnostics: register a device buffer (bytes >= 64 x blocks) that the blocks of subsequent mdx_gemm_f16 launches
 * fill with phase timestamps (8 x u64 per block, 100 MHz realtime counter); NULL unregisters.  tools/gemm_trace.py */
int mdx_probe_gemm_trace(void* buf, size_t bytes);
/* VALU issue-rate probe (no reference counterpart; diagnostics): `iters` rounds of eight independent chains per lane of one
 * instruction kind -- 0 v_fma_f32, 1 v_exp_f32, 2 v_pk_fma_f32, 3 v_cvt_pk_f16_f32 (+ two converts back), 4 v_max3_f32, 5 v_exp_f16,
 * 6 v_pk_fma_f16, 7 v_pk_max_f16 -- on
 * `nblocks` blocks of 256 threads; time it from the host (tools/exp/r04n_valu_probe.py). */
int mdx_probe_valu_rate(int kind, int iters, int nblocks, float* sink, mdx_stream_t s);
/* Diagnostics (round 6): four slots per iteration of { one 32x32x16 MFMA } and / or VALU work -- kind 0 MFMA alone, 1 MFMA + 2 v_exp_f32,
 * 2 MFMA + 8 v_fma_f32, 3 the 2 exps alone, 4 the 8 fmas alone, 5 MFMA + the softmax mix of one score pair, 6 that mix alone: does VALU
 * work run in the shadow of an MFMA?  (tools/exp/r06_mix_probe.py) */
int mdx_probe_mix_rate(int kind, int iters, int nblocks, float* sink, mdx_stream_t s);

#ifdef __cplusplus
}
#endif
#endif /* MDX_H_ */
