// Host side of the implicit-GEMM / conv launches (kernels: gemm.hip, dense.hip, conv8p.hip): descriptor validation (fill_params),
// the measured tile tables, plan_gemm -- the ONE place that decides what a descriptor launches -- the arrival counters of the
// in-kernel split-K reduce, and the public entry points.  No kernel is instantiated here: a change to a host rule or a new row of
// gemm_tuned.inc rebuilds this file only.
#include "mdx_common.h"
#include "gemm_internal.h"

#include <stdlib.h>

#include <algorithm>
#include <map>
#include <mutex>
#include <utility>
#include <vector>

static int fill_params(const mdx_gemm_desc* d, GemmParams& p) {
    MDX_REQUIRE(d && d->a && d->w && d->out, "mdx_gemm_f16: null pointer");
    MDX_REQUIRE(d->ksize == 1 || d->ksize == 3, "mdx_gemm_f16: ksize must be 1 or 3 (got %d)", d->ksize);
    MDX_REQUIRE(d->stride == 1 || d->stride == 2, "mdx_gemm_f16: stride must be 1 or 2");
    MDX_REQUIRE(!(d->upsample && d->stride != 1), "mdx_gemm_f16: upsample requires stride 1");
    MDX_REQUIRE(d->B > 0 && d->H > 0 && d->W > 0 && d->N > 0, "mdx_gemm_f16: bad extents");
    MDX_REQUIRE(d->c1 > 0 && d->c1 % 8 == 0 && d->c2 >= 0 && d->c2 % 8 == 0, "mdx_gemm_f16: c1/c2 must be multiples of 8");
    MDX_REQUIRE((d->c2 == 0) == (d->a2 == nullptr), "mdx_gemm_f16: a2/c2 mismatch");
    MDX_REQUIRE(d->N % 8 == 0, "mdx_gemm_f16: N must be a multiple of 8 (got %d)", d->N);
    p.a = (const f16*)d->a;
    p.a2 = (const f16*)d->a2;
    p.w = (const f16*)d->w;
    p.bias = d->bias;
    p.rowbias = d->rowbias;
    p.residual = (const f16*)d->residual;
    p.out = (f16*)d->out;
    p.out2 = (f16*)d->out2;
    p.stats_out = d->stats_out;
    p.colstats_out = d->colstats_out;
    p.ln_stats = d->ln_stats;
    p.ln_s = d->ln_s;
    p.ln_prefetch = mdx_opt(MDX_OPT_GEMM_LN_PREFETCH) ? 1 : 0;
    p.dense_issue = mdx_opt(MDX_OPT_GEMM_DENSE_ISSUE) ? 1 : 0;
    p.ln_nt = d->ln_nt;
    p.ln_eps = d->ln_eps;
    p.bn_hint = d->tile_n;
    p.st_hint = d->stages;
    p.out2_ld = d->out2_ld;
    p.n_split = d->n_split;
    p.ws = (float*)d->workspace;
    p.c1 = d->c1;
    p.c2 = d->c2;
    p.cin = d->c1 + d->c2;
    p.rowbias_ld = d->rowbias_ld;
    p.residual_ld = d->residual_ld;
    p.out_ld = d->out_ld;
    p.out_bs = d->out_bs;
    p.B = d->B;
    p.H = d->H;
    p.W = d->W;
    p.ksize = d->ksize;
    p.stride = d->stride;
    p.upsample = d->upsample ? 1 : 0;
    // asym_pad: zero padding on the bottom / right only (VAE Encoder Downsample: nn.Pad((0,1),(0,1)) + valid 3x3 stride 2,
    // ldm/modules/diffusionmodules/model.py:55-78) -- the taps start AT the output pixel instead of one before it
    MDX_REQUIRE(!d->asym_pad || (d->ksize == 3 && d->stride == 2 && !d->upsample),
                "mdx_gemm_f16: asym_pad applies to the 3x3 stride-2 conv only");
    p.pad = d->ksize == 3 ? (d->asym_pad ? 0 : 1) : 0;
    const int pad_hi = d->ksize == 3 ? 1 : 0;
    const int Hs = p.upsample ? 2 * d->H : d->H, Ws = p.upsample ? 2 * d->W : d->W;
    p.Ho = (Hs + p.pad + pad_hi - d->ksize) / d->stride + 1;
    p.Wo = (Ws + p.pad + pad_hi - d->ksize) / d->stride + 1;
    p.HoWo = p.Ho * p.Wo;
    p.M = d->B * p.HoWo;
    p.N = d->N;
    p.K = d->ksize * d->ksize * p.cin;
    p.epilogue = d->epilogue;
    p.out_mode = d->out_mode;
    MDX_REQUIRE(p.epilogue == MDX_EPI_NONE || p.epilogue == MDX_EPI_GEGLU || p.epilogue == MDX_EPI_GELU ||
                    p.epilogue == MDX_EPI_QUICKGELU || p.epilogue == MDX_EPI_PRELU, "mdx_gemm_f16: bad epilogue");
    MDX_REQUIRE(p.out_mode == MDX_OUT_ROWMAJOR || p.out_mode == MDX_OUT_TRANSPOSED || p.out_mode == MDX_OUT_D2S2,
                "mdx_gemm_f16: bad out_mode");
    p.act_slope = d->act_slope;
    p.act_slope_n = d->act_slope_n;
    p.d2s_c = 0;
    if (p.epilogue == MDX_EPI_PRELU) {
        MDX_REQUIRE(p.act_slope && p.act_slope_n > 0 && p.act_slope_n % 8 == 0 && p.N % p.act_slope_n == 0,
                    "mdx_gemm_f16: PReLU needs act_slope and act_slope_n > 0 with act_slope_n %% 8 == 0 and N %% act_slope_n == 0");
        MDX_REQUIRE(p.out_mode != MDX_OUT_TRANSPOSED && !d->rowbias && !d->n_split && !d->xattn_k,
                    "mdx_gemm_f16: PReLU takes a row-major or depth-to-space store with bias (and residual) only");
    }
    if (p.epilogue == MDX_EPI_PRELU || p.out_mode == MDX_OUT_D2S2) {      // the generic kernel's EXT instantiations (launch_ext)
        MDX_REQUIRE(d->c2 == 0 && d->c1 % 64 == 0 && !d->gn_colstats && !d->skip_w && !d->w_frag && !d->upsample,
                    "mdx_gemm_f16: PReLU / depth-to-space launches take one source with Cin %% 64 == 0 (no fused GroupNorm / skip, "
                    "tile-major weights, no upsample)");
    }
    if (p.out_mode == MDX_OUT_D2S2) {
        // (a row-major launch to the tile programs: only the store index of epilogue_apply_row8 differs)
        MDX_REQUIRE(p.N % 32 == 0 && p.out_ld >= p.N / 4 && (p.epilogue == MDX_EPI_NONE || p.epilogue == MDX_EPI_PRELU),
                    "mdx_gemm_f16: depth-to-space store needs N = 4 C with C %% 8 == 0, out_ld >= C and a plain or PReLU epilogue");
        MDX_REQUIRE(!d->residual && !d->out_bs && !d->n_split && !d->stats_out && !d->colstats_out && !d->ln_stats && !d->xattn_k &&
                        !d->skip_w && !d->defer_reduce,
                    "mdx_gemm_f16: depth-to-space store takes bias / time-embedding row / PReLU only");
        p.d2s_c = p.N / 4;
        p.out_mode = MDX_OUT_ROWMAJOR;
    }
    p.geglu_unit = 0;
    MDX_REQUIRE(d->geglu_unit == 0 || p.epilogue == MDX_EPI_GEGLU, "mdx_gemm_f16: geglu_unit belongs to the GEGLU epilogue");
    if (p.epilogue == MDX_EPI_GEGLU) {
        MDX_REQUIRE(d->geglu_unit == 0 || d->geglu_unit == 64 || d->geglu_unit == 80, "mdx_gemm_f16: geglu_unit must be 0 (= 64), 64 or 80");
        p.geglu_unit = d->geglu_unit == 80 ? 80 : 64;
        MDX_REQUIRE(p.N % (2 * p.geglu_unit) == 0, "mdx_gemm_f16: GEGLU needs N %% %d == 0 (geglu_unit %d)", 2 * p.geglu_unit, p.geglu_unit);
        MDX_REQUIRE(p.out_mode == MDX_OUT_ROWMAJOR, "mdx_gemm_f16: GEGLU is row-major only");
    }
    if (p.out_mode == MDX_OUT_TRANSPOSED) {
        // (tokens per sample need not be a multiple of 8: the epilogue then stores element-wise; out_ld is the padded row length)
        MDX_REQUIRE(p.out_ld % 8 == 0 && p.out_ld >= p.HoWo, "mdx_gemm_f16: transposed store needs out_ld %% 8 == 0 and out_ld >= tokens");
        MDX_REQUIRE(!p.rowbias && !p.residual, "mdx_gemm_f16: transposed store takes bias only");
    }
    if (p.n_split) {
        MDX_REQUIRE(p.out2 && p.n_split > 0 && p.n_split < p.N && p.n_split % 128 == 0,
                    "mdx_gemm_f16: n_split must be a multiple of 128 inside (0, N) with out2 set");
        // (out_bs is allowed since round 6: the row-major part may land in a token sub-range of a larger [B][tokens][C] buffer --
        // Taichu-GLIDE's q | k of the image tokens behind the text keys, unet.py:289-297; both store paths go through
        // epilogue_apply_row8, which knows it)
        MDX_REQUIRE(p.out_mode == MDX_OUT_ROWMAJOR && p.epilogue == MDX_EPI_NONE && !p.rowbias && !p.residual,
                    "mdx_gemm_f16: the split row-major | transposed output takes bias only");
        MDX_REQUIRE(p.out2_ld % 8 == 0 && p.out2_ld >= p.HoWo,
                    "mdx_gemm_f16: transposed part needs out2_ld %% 8 == 0 and out2_ld >= tokens");
    }
    if (p.ln_stats) {
        MDX_REQUIRE(p.ln_s && p.ln_nt * 64 == p.K && p.ksize == 1 && p.c2 == 0 && p.stride == 1 && !p.upsample &&
                        p.out_mode == MDX_OUT_ROWMAJOR && p.N % (p.epilogue == MDX_EPI_GEGLU ? 2 * p.geglu_unit : 64) == 0,
                    "mdx_gemm_f16: LayerNorm fold needs ln_s, ln_nt == K / 64, N %% 64 == 0 and a dense row-major GEMM");
    }
    if (p.stats_out)
        MDX_REQUIRE(p.out_mode == MDX_OUT_ROWMAJOR && p.epilogue != MDX_EPI_GEGLU && !p.n_split && p.N % 64 == 0,
                    "mdx_gemm_f16: row statistics are produced by plain row-major stores with N %% 64 == 0 only");
    if (p.colstats_out)
        MDX_REQUIRE(p.out_mode == MDX_OUT_ROWMAJOR && p.epilogue == MDX_EPI_NONE && !p.n_split && !p.ln_stats && !p.stats_out &&
                        !p.out_bs && p.N % 8 == 0,
                    "mdx_gemm_f16: column statistics come from plain row-major launches only");
    p.gn_cs = d->gn_colstats;
    p.gn_gamma = d->gn_gamma;
    p.gn_beta = d->gn_beta;
    p.gn_nrb = d->gn_nrb;
    p.gn_silu = d->gn_silu ? 1 : 0;
    p.gn_eps = d->gn_eps;
    if (p.gn_cs) {
        MDX_REQUIRE(p.gn_gamma && p.gn_beta && p.gn_nrb > 0, "mdx_gemm_f16: gn_colstats needs gn_gamma, gn_beta and gn_nrb > 0");
        if (p.ksize == 1) {     // GroupNorm (no activation) -> Dense / 1x1 conv: applied to the A fragments (gemm_kernel GNA)
            MDX_REQUIRE(p.stride == 1 && !p.upsample && p.c2 == 0 && p.cin % 64 == 0 && p.cin <= 2560 && !p.gn_silu &&
                            p.HoWo % 64 == 0,
                        "mdx_gemm_f16: the fused input GroupNorm of a dense launch needs a single source, Cin %% 64 == 0, "
                        "Cin <= 2560, gn_silu = 0 and tokens per sample %% 64 == 0");
        } else {
            MDX_REQUIRE(p.ksize == 3 && p.stride == 1 && !p.upsample && p.c2 == 0 && p.cin % 64 == 0 && p.cin % 32 == 0 &&
                            p.cin <= 640 && !d->w_frag && !(d->H == 8 && d->W == 8),
                        "mdx_gemm_f16: the fused input GroupNorm rides on a single-source 3x3 stride-1 conv with Cin %% 64 == 0, "
                        "Cin <= 640, images larger than 8 x 8 and tile-major weights");
        }
    }
    p.xa_k = (const f16*)d->xattn_k;
    p.xa_vt = (const f16*)d->xattn_vt;
    p.xa_len = d->xattn_len;
    p.xa_cap = d->xattn_cap;
    p.xa_scale_log2 = d->xattn_scale * 1.4426950408889634f;
    if (p.xa_k) {
        const int howo = d->H * d->W;
        MDX_REQUIRE(p.xa_vt && d->xattn_len > 0 && d->xattn_len <= 1024 && d->xattn_cap >= d->xattn_len && d->xattn_cap % 8 == 0,
                    "mdx_gemm_f16: cross-attention epilogue needs xattn_vt, 0 < xattn_len <= 1024 and xattn_len <= xattn_cap (a multiple of 8)");
        MDX_REQUIRE(d->ksize == 1 && d->stride == 1 && !d->upsample && d->c2 == 0 && d->N % 64 == 0 && d->c1 % 64 == 0 &&
                        d->epilogue == MDX_EPI_NONE && d->out_mode == MDX_OUT_ROWMAJOR && !d->residual && !d->rowbias && !d->stats_out &&
                        !d->colstats_out && !d->n_split && !d->out_bs && !d->gn_colstats && !d->defer_reduce,
                    "mdx_gemm_f16: the cross-attention epilogue rides on a plain dense row-major projection (N %% 64 == 0, Cin %% 64 == 0)");
        MDX_REQUIRE(d->tile_n == 64 && d->splitk == 1 && (howo % 128 == 0 || (howo % 64 == 0 && d->tile_m == 64)) &&
                        (d->tile_m == 0 || d->tile_m == 64 || d->tile_m == 128),
                    "mdx_gemm_f16: the cross-attention epilogue needs tile_n = 64 (one head per tile), splitk = 1 and an M tile inside one sample "
                    "(tokens per sample %% 128 == 0, or %% 64 == 0 with tile_m = 64)");
        MDX_REQUIRE((size_t)d->xattn_cap * d->N * 2 <= 0x80000000ull, "mdx_gemm_f16: cross-attention context larger than 2 GiB per sample");
    }
    p.w_sub = (const f16*)d->w_sub;
    p.w_sub_bytes = 0;
    p.c8_sub = 0;
    if (p.w_sub) {
        MDX_REQUIRE(d->upsample && d->ksize == 3 && d->stride == 1, "mdx_gemm_f16: w_sub belongs to the nearest-2x + 3x3 conv (upsample = 1)");
        const size_t sb = (size_t)((4 * (size_t)d->N + 63) / 64) * ((4 * (size_t)(d->c1 + d->c2) + 63) / 64) * 8192;
        MDX_REQUIRE(sb <= 0x80000000ull, "mdx_gemm_f16: sub-pixel weights larger than 2 GiB");
        p.w_sub_bytes = (unsigned)sb;
    }
    p.skip_a = (const f16*)d->skip_a;
    p.skip_a2 = (const f16*)d->skip_a2;
    p.skip_w = (const f16*)d->skip_w;
    p.skip_c1 = d->skip_c1;
    p.skip_c2 = d->skip_c2;
    if (p.skip_w) {
        MDX_REQUIRE(p.skip_a && d->skip_c1 > 0 && d->skip_c1 % 64 == 0 && d->skip_c2 >= 0 && d->skip_c2 % 64 == 0 &&
                        (d->skip_c2 == 0) == (d->skip_a2 == nullptr),
                    "mdx_gemm_f16: fused skip needs skip_a, skip_c1 %% 64 == 0, skip_c2 %% 64 == 0 and skip_a2 iff skip_c2");
        MDX_REQUIRE(p.ksize == 3 && p.stride == 1 && !p.upsample && p.c2 == 0 && p.out_mode == MDX_OUT_ROWMAJOR && !d->w_frag,
                    "mdx_gemm_f16: the fused skip rides on a single-source 3x3 stride-1 row-major conv (tile-major weights)");
        p.skip_kt = (d->skip_c1 + d->skip_c2) / 64;
        const size_t s1 = (size_t)d->B * d->H * d->W * d->skip_c1 * 2, s2 = (size_t)d->B * d->H * d->W * d->skip_c2 * 2;
        const size_t sw = (size_t)((p.N + 63) / 64) * p.skip_kt * 8192;
        MDX_REQUIRE(s1 <= 0x80000000ull && s2 <= 0x80000000ull && sw <= 0x80000000ull, "mdx_gemm_f16: skip operand larger than 2 GiB");
        p.skip_a_bytes = (unsigned)s1;
        p.skip_a2_bytes = (unsigned)s2;
        p.skip_w_bytes = (unsigned)sw;
    }
    if (p.rowbias) MDX_REQUIRE(p.rowbias_ld % 4 == 0, "mdx_gemm_f16: rowbias_ld must be a multiple of 4");
    if (p.residual) MDX_REQUIRE(p.residual_ld % 8 == 0, "mdx_gemm_f16: residual_ld must be a multiple of 8");
    MDX_REQUIRE(p.out_ld % 8 == 0 && p.out_bs % 8 == 0 && p.out_bs >= 0, "mdx_gemm_f16: out_ld / out_bs must be multiples of 8");
    MDX_REQUIRE(!(p.out_bs && p.out_mode == MDX_OUT_TRANSPOSED), "mdx_gemm_f16: out_bs applies to row-major output only");
    const size_t ab = (size_t)d->B * d->H * d->W * d->c1 * 2, a2b = (size_t)d->B * d->H * d->W * d->c2 * 2;
    p.kt64 = (p.K + 63) / 64;
    const size_t wb = (size_t)((p.N + 63) / 64) * p.kt64 * 8192;   // padded, tile-major storage
    MDX_REQUIRE(ab <= 0x80000000ull && a2b <= 0x80000000ull && wb <= 0x80000000ull,
                "mdx_gemm_f16: operand larger than 2 GiB is not addressable by one buffer descriptor");
    p.a_bytes = (unsigned)ab;
    p.a2_bytes = (unsigned)a2b;
    p.w_bytes = (unsigned)wb;
    return MDX_OK;
}

// Measured (tile_m, tile_n, splitk) per UNet shape: tools/tune_gemm.py times every candidate on the device with cold
// weights and writes gemm_tuned.inc.  Shapes that are not in the table fall through to plan_gemm's defaults / the cost model.
// A row is keyed by shape AND launch variant: the same (M, N, K) occurs with different epilogues / operand forms in one UNet
// (proj_in, attention out + residual + row statistics, LayerNorm-fold consumers ...), and a split or tile that was measured
// for one of them says nothing about the others.  var1 = variant + 1; 0 (rows written before the key existed) = any variant,
// consulted only when no exact row matches.
struct TunedEntry {
    int M, N, K, ksize, bm, bn, ns;   // bn 0 = plan_gemm's default
    int var1;
    int st;                           // LDS ring depth (0 = the occupancy rule of plan_gemm)
};
static const TunedEntry g_tuned[] = {
#include "gemm_tuned.inc"
    {0, 0, 0, 0, 0, 0, 0, 0, 0}};
// Rows of the 128 x 160 tile of the lean dense kernel (same fields, same tool): a table of their own, consulted FIRST.  A row the launch
// cannot take -- in particular a GEGLU descriptor whose weights are packed at 64 -- is passed over and the main table decides as before.
static const TunedEntry g_tuned160[] = {
#include "gemm_tuned160.inc"
    {0, 0, 0, 0, 0, 0, 0, 0, 0}};

// Launch variant of a descriptor (tools/tune_gemm.py computes the same number from the mdx_gemm_desc fields).
static int tuned_variant(const GemmParams& p) {
    // (epilogue in bits 1-2 for NONE .. QUICKGELU; PReLU = 4 would reach the n_split bit and has a bit of its own)
    return (p.c2 > 0 ? 1 : 0) | (p.epilogue == MDX_EPI_PRELU ? 2048 : p.epilogue << 1) | (p.n_split ? 8 : 0) | (p.ln_stats ? 16 : 0) |
           (p.stats_out ? 32 : 0) |
           (p.out_mode == MDX_OUT_TRANSPOSED ? 64 : 0) | (p.colstats_out ? 128 : 0) | (p.residual ? 256 : 0) |
           (p.rowbias ? 512 : 0) | (p.d2s_c ? 1024 : 0);
}

// 8 x 8-pixel images (the deepest UNet level at a 64 x 64 latent): two whole samples per 128-row tile (PW = 8).
static bool halo8_eligible(const GemmParams& p) {
    if (!mdx_opt(MDX_OPT_GEMM_HALO8)) return false;
    return p.H == 8 && p.W == 8;
}

// Epilogues the HALO kernel's store loop implements.  Its batched patch loops (gemm_epilogue EMODE 2) carry the plain and GEGLU
// stores only: a GELU / QuickGELU / PReLU launch or a depth-to-space store must resolve to the generic kernel, which implements them,
// instead of storing un-activated values.
static bool halo_epilogue_ok(const GemmParams& p) {
    return !p.d2s_c && (p.epilogue == MDX_EPI_NONE || p.epilogue == MDX_EPI_GEGLU);
}

// The HALO kernel applies to 3x3 / stride 1 / single-source convs whose image tiles into 8 x 16 (16 x 16) patches, or
// whose images are 8 x 8 (bm = 128 only).
static bool halo_eligible(const GemmParams& p, int bm) {
    if (!mdx_opt(MDX_OPT_GEMM_HALO)) return false;
    if (!halo_epilogue_ok(p)) return false;
    if (!(p.ksize == 3 && p.stride == 1 && !p.upsample && p.c2 == 0 && p.cin % 64 == 0 && p.out_mode == MDX_OUT_ROWMAJOR))
        return false;
    if (p.out_bs) return false;      // (no conv writes a strided-sample output; the patch epilogue does not carry the form)
    if (p.residual && (size_t)p.M * (size_t)p.residual_ld * 2 >= 0x80000000ull) return false;      // (its residual rows go through a 32-bit-offset descriptor)
    if (bm == 128 && halo8_eligible(p)) return true;
    return p.H % (bm / 16) == 0 && p.W % 16 == 0;
}

// The row of the tile tables that describes this launch, or null.  plan_gemm asks once per launch.
static const TunedEntry* lookup_tuned(const GemmParams& p) {
    const bool use_table = mdx_opt(MDX_OPT_GEMM_TUNED) && !mdx_opt(MDX_OPT_GEMM_BM) && !mdx_opt(MDX_OPT_GEMM_BN);
    if (!use_table || p.bn_hint || p.st_hint || p.stride != 1 || p.upsample) return nullptr;
    if (p.epilogue == MDX_EPI_PRELU || p.d2s_c) return nullptr;      // (SRGAN launches: no measured rows; a var1 = 0 row says nothing)
    const int var1 = tuned_variant(p) + 1;
    if (mdx_dense_takes_desc(p, 160))
        for (const TunedEntry* e = g_tuned160; e->M; ++e)
            if (e->M == p.M && e->N == p.N && e->K == p.K && e->ksize == p.ksize && e->var1 == var1 && e->bn == 160) return e;
    const TunedEntry* any = nullptr;
    for (const TunedEntry* e = g_tuned; e->M; ++e)
        if (e->M == p.M && e->N == p.N && e->K == p.K && e->ksize == p.ksize) {
            if (e->var1 == var1) {
                any = e;
                break;
            }
            if (e->var1 == 0 && !any) any = e;
        }
    if (!any) return nullptr;
    // The key is (M, N, K, ksize), not the image geometry: a row measured at one (B, H, W) also matches other factorizations of M.
    // A 256-row entry means the 16 x 16-patch HALO kernel; where that kernel does not apply (8 x 8 images at UNet batch 8 share
    // M = 512 with the 16 x 16 level at batch 2) the row does not describe this launch -- round 5: it used to be taken, the generic
    // kernel then ran its 128-row tiles on a grid sized for 256-row ones and left the second half of every tile pair unwritten
    if (any->bm == 256 && !halo_eligible(p, 256)) return nullptr;
    return (any->bm >= 128 || !halo_eligible(p, 128)) ? any : nullptr;
}

// Tile height and split-K factor from a cost model fitted to the B=2 micro-benchmarks
// (profiles/r01_gemm_auto_tiling.txt, tools/gemm_trace.py), in microseconds:
//   main loop   = K tiles per split x tau(kernel, tile) x occupancy    tau = 0.65 us for the generic 128x128 tile:
//                 a K-tile step of ONE block is bound by its own DMA-issue + MFMA + barrier chain, so small grids
//                 finish sooner with more, smaller blocks -- until every CU holds one (occupancy = 1 up to 256
//                 blocks, 1.15 x rounds of 512 beyond); never less than streaming the cold operands once from HBM;
//   split-K     = 3.5 (the extra reduce launch) + 0.3 x splits x slab MB (slab write + re-read);
// fixed per-launch costs are the same for every candidate and drop out.  Splits keep >= 4 K tiles (HALO convs: whole
// 64-channel chunks).  The 64-row tile is only a candidate for the generic kernel, the 256-row tile only for HALO.
static void cost_model_tiling(const GemmParams& p, int bn, int forced_ns, int forced_bm, int& best_bm, int& best_ns) {
    const int envbm = mdx_opt(MDX_OPT_GEMM_BM);
    const int kt = (p.K + 63) / 64;
    const int chunks = p.cin / 64;
    const double slab_mb = (double)p.M * p.N * 4.0 / 1048576.0;
    const double unique_mb = ((double)p.N * p.K + (double)p.M * p.cin) * 2.0 / 1048576.0;
    best_bm = 128, best_ns = 1;
    double best_cost = 1e30;
    static const int order[3] = {128, 256, 64};   // increasing launch complexity (see the hysteresis below)
    for (int oi = 0; oi < 3; ++oi) {
        const int bm = order[oi];
        if (envbm && envbm != bm) continue;
        if (forced_bm > 0 && forced_bm != bm) continue;
        const bool halo = bm >= 128 && halo_eligible(p, bm);
        // 256-row tiles exist for the HALO kernel only and are opt-in (MDX_GEMM_BM=256): measured on MI355X they move
        // 45 % fewer DMA bytes per MAC yet run no faster than two co-resident 128-row blocks (profiles/
        // r01_halo256_ab.txt) -- the K-step's barrier/issue structure, not the DMA rate, is what bounds this kernel
        if (bm == 256 && (!halo || !(envbm || forced_bm == 256))) continue;
        if (bm == 64 && halo_eligible(p, 128) && !envbm && forced_bm <= 0) continue;  // HALO beats the generic kernel on every conv
        const int tiles = ((p.M + bm - 1) / bm) * ((p.N + bn - 1) / bn);
        // us per K-tile step of one block running alone on its CU (tools/gemm_trace.py): fewer DMA instructions and
        // MFMAs per step for the smaller tiles and for the HALO kernel (one activation DMA per 9 taps)
        const double tau = (halo ? (bm == 256 ? 0.65 : 0.60) : 0.65) * (bm == 64 ? 0.7 : 1.0) * (bn == 64 ? 0.7 : 1.0);
        const int max_ns = forced_ns > 0 ? forced_ns : 16;
        for (int ns = forced_ns > 0 ? forced_ns : 1; ns <= max_ns; ++ns) {
            int kps, eff;
            if (halo) {
                if (ns > chunks && forced_ns <= 0) break;
                const int cps = (chunks + std::min(ns, chunks) - 1) / std::min(ns, chunks);
                kps = cps * 9;
                eff = (chunks + cps - 1) / cps;
            } else {
                if (forced_ns <= 0 && ns > 1 && kt / ns < 4) break;
                kps = (kt + std::min(ns, kt) - 1) / std::min(ns, kt);
                eff = (kt + kps - 1) / kps;
            }
            if (forced_ns <= 0 && eff != ns) continue;   // same launch as a smaller ns
            // up to 256 blocks run one per CU.  128/64-row tiles: beyond that two share a CU (their stalls overlap:
            // only ~1.15x slower each) and the grid runs in rounds of 512; 256-row tiles own a CU: rounds of 256.
            // The last, partly filled round costs as much as a full one.
            const int blocks = tiles * eff;
            const double occ = blocks <= 256 ? 1.0 : (bm == 256 ? (blocks + 255) / 256 : 1.15 * ((blocks + 511) / 512));
            const double main_us = std::max(kps * tau * occ, unique_mb / 3.5);   // cold operands stream at ~3.5 TB/s
            const double cost = main_us + (eff > 1 ? 3.5 + 0.3 * eff * slab_mb : 0.0);
            // the model is only good to ~10-20 %, so a more complex candidate must promise a clear win
            if (cost < 0.9 * best_cost) {
                best_cost = cost;
                best_bm = bm, best_ns = ns;
            }
        }
    }
}

// Split-K launches of at most `gemm_splitk_fixup_max` (mdx_set_option; default 4) splits reduce in the kernel (splitk_last_block_reduce)
// when the output is row-major and the tiles fit the ticket area.  The last arriver reads nsplit partials serially at the
// ~65 GB/s one block can pull, so the in-kernel form only beats the reduce launch it replaces for few splits (measured at UNet
// batch 2, profiles/r02_l_splitk_fixup.txt: 4 splits -1.7 us, 3 splits -1.4 us, 5 splits 0 ... +1.7 us, 10 splits +7 us,
// 20 splits +8 us per launch); deeper splits, transposed outputs and deferred reduces keep the [split][M][N] slabs + reduce kernel.
static bool fixup_eligible(const mdx_gemm_desc* d, const GemmParams& p, int bm, int bn, int ns) {
    const int max_ns = mdx_opt(MDX_OPT_GEMM_SPLITK_FIXUP_MAX);
    if (ns > max_ns) return false;
    if (p.out_mode != MDX_OUT_ROWMAJOR || d->defer_reduce) return false;
    const long tiles = (long)((p.M + bm - 1) / bm) * ((p.N + bn - 1) / bn);
    return tiles <= MDX_TICKET_SLOTS;
}

// bytes of workspace one split of this launch occupies (+ `head` bytes once)
static size_t split_bytes(const mdx_gemm_desc* d, const GemmParams& p, int bm, int bn, int ns, size_t* head) {
    if (fixup_eligible(d, p, bm, bn, ns)) {
        *head = (size_t)MDX_TICKET_SLOTS * sizeof(unsigned);
        return (size_t)((p.M + bm - 1) / bm) * ((p.N + bn - 1) / bn) * bm * bn * sizeof(float);
    }
    *head = (size_t)MDX_TICKET_SLOTS * sizeof(unsigned);     // never used for slabs: other launches keep their tickets there
    return (size_t)p.M * p.N * sizeof(float);
}

// The eight-wave 256-pixel conv core takes a launch when the descriptor forces it (tile_m = 256 with stages = 8) or, by default,
// when the shape is eligible, has at least gemm_conv8p_min_m output pixels and at least 128 tiles (UNet batch >= 8 down to the
// 16 x 16 level): below that even a 4-way tail split cannot fill 256 CUs and the 128-row HALO tiles with their own split-K win
// (tools/conv8p_bench.py at UNet batch 2: 462 vs 603 TF/s).
static bool conv8p_wanted(const mdx_gemm_desc* d, const GemmParams& p) {
    if (d->w_frag || d->defer_reduce || d->splitk > 1 || d->asym_pad) return false;
    if (mdx_opt(MDX_OPT_GEMM_BM) || !mdx_opt(MDX_OPT_GEMM_HALO)) return false;
    if (!mdx_conv8p_eligible(p)) return false;
    if (d->tile_m == 256 && (d->stages == 8 || d->stages == 9)) return true;      // forced (9: one phase per 32-deep k-step)
    if (!mdx_opt(MDX_OPT_GEMM_CONV8P)) return false;
    if (d->tile_m != 0 || d->stages != 0) return false;
    if (d->tile_n != 0 && d->tile_n != 64 && d->tile_n != 96 && d->tile_n != 128 && d->tile_n != 160 && d->tile_n != 192) return false;
    if (p.upsample) return mdx_conv8p_tiles(p) >= mdx_opt(MDX_OPT_GEMM_SUBPIXEL_MIN_TILES);      // 2.25x fewer FLOPs: pays from far fewer tiles
    return p.M >= mdx_opt(MDX_OPT_GEMM_CONV8P_MIN_M) && mdx_conv8p_tiles(p) >= 128;
}

// Everything decided before a launch, decided once: tile, split-K factor (clamped to the caller's workspace), kernel form, ring depth,
// grid, the reduce that follows -- and every requirement a descriptor must meet for that form to exist, so that mdx_gemm_check and
// mdx_gemm_query refuse exactly what mdx_gemm_f16 would.  Fills the resolved fields of `p` (call it once per fill_params).
// sizing (mdx_gemm_workspace_bytes): stop behind the tile and split choice, with the workspace the unclamped split asks for.
static int plan_gemm(const mdx_gemm_desc* d, GemmParams& p, GemmPlan& pl, bool sizing = false) {
    pl = GemmPlan{};
    pl.pw = 16;
    p.bk = 64;
    p.ktiles = (p.K + 63) / 64;
    p.tickets = nullptr;
    // Rows per colstats_out row block the planned launch produces (0 = it cannot): the M tile for a single-pass launch (a HALO
    // patch is one row block), CS_ROWS for a slab split-K launch; a row block never straddles two samples.
    auto colstats_rows = [&](bool halo) {
        if (p.out_mode != MDX_OUT_ROWMAJOR || p.epilogue != MDX_EPI_NONE || p.n_split || p.ln_stats || p.stats_out || p.out_bs ||
            p.d2s_c)
            return 0;
        if (pl.nsplit > 1 && !pl.fixup) return p.HoWo % CS_ROWS == 0 ? CS_ROWS : 0;
        if (halo) return pl.pw == 8 ? 0 : pl.bm;
        return p.HoWo % pl.bm == 0 ? pl.bm : 0;
    };
    if (conv8p_wanted(d, p)) {
        pl.form = GEMM_CONV8P;
        pl.bm = 256;
        pl.bn = mdx_conv8p_pick_bn(p, d->tile_n);
        pl.nsplit = 1;
        p.ktiles_per_split = p.ktiles;
        p.skip_kt_per_split = p.skip_w ? p.skip_kt : 0;
        pl.ws_head = mdx_conv8p_plan(p, pl.bn, sizing ? 0 : d->workspace_bytes, !sizing && d->workspace != nullptr, sizing);
        pl.colstats_rows = colstats_rows(true);
        return MDX_OK;
    }

    // ---- tile and split: the descriptor's overrides, the measured row, library options, then the cost model
    const TunedEntry* row = lookup_tuned(p);
    const int optbn = mdx_opt(MDX_OPT_GEMM_BN);
    int bn;
    if (p.epilogue == MDX_EPI_GEGLU) bn = (p.bn_hint == 160 || (row && row->bn == 160)) ? 160 : 128;      // (the packing unit is checked below)
    else if (p.bn_hint == 64 || p.bn_hint == 128 || p.bn_hint == 160) bn = p.bn_hint;
    else if (row && row->bn) bn = row->bn;
    else if (optbn == 64 || optbn == 128) bn = optbn;
    else if (p.N % 128 == 0) bn = 128;
    else if (p.N % 64 == 0 || p.N < 128) bn = 64;
    else bn = (p.N % 128 > 64) ? 128 : 64;
    pl.tuned = (d->splitk <= 0 && d->tile_m <= 0) ? row : nullptr;
    const int stages = pl.tuned ? pl.tuned->st : p.st_hint;      // ring depth / eight waves asked for (0 = the occupancy rule)
    int bm, ns;
    if (pl.tuned) bm = row->bm, ns = row->ns;
    else cost_model_tiling(p, bn, d->splitk, d->tile_m, bm, ns);
    pl.bm = bm;
    pl.bn = bn;
    if (ns > 1) {
        // counted in the larger of the two layouts (tile-padded partials of the in-kernel form >= [M][N] slabs): a launch that a
        // small workspace clamps to fewer splits may switch form, and the split count that fits must fit the form it ends up in
        pl.ws_per_split = std::max(split_bytes(d, p, bm, bn, 2, &pl.ws_head), split_bytes(d, p, bm, bn, 1 << 30, &pl.ws_head));
    }
    if (sizing) {      // only bm, bn, nsplit (unclamped) and ws_* are valid: no form, ring, grid, and no requirement was checked
        pl.nsplit = ns;
        return MDX_OK;
    }
    if (ns > p.ktiles) ns = p.ktiles;
    if (ns > 1) {
        // shrink to what the caller's workspace can hold
        const size_t cap = (d->workspace && d->workspace_bytes > pl.ws_head) ? (d->workspace_bytes - pl.ws_head) / pl.ws_per_split : 0;
        if ((size_t)ns > cap) ns = (int)cap;
        if (ns < 1) ns = 1;
        if (d->splitk > 1 && ns != d->splitk) {
            mdx_set_error("mdx_gemm_f16: workspace too small for splitk=%d (need %zu bytes)", d->splitk,
                          pl.ws_head + (size_t)d->splitk * pl.ws_per_split);
            return MDX_E_WORKSPACE;
        }
    }
    const bool halo = bm >= 128 && halo_eligible(p, bm);
    if (halo && bm == 128 && halo8_eligible(p)) pl.pw = 8;
    // (what the descriptor and the split rule out is reported here; what the ring depth or the tile count rules out, below)
    MDX_REQUIRE(bn != 160 || (bm == 128 && ns == 1 && mdx_dense_takes_desc(p, 160)),
                "mdx_gemm_f16: tile_n = 160 runs with tile_m = 128, unsplit, on dense row-major launches with bias / residual / "
                "GEGLU (geglu_unit = 80) / LayerNorm-fold consumer only (got tile_m %d, %d splits, geglu_unit %d)",
                bm, ns, p.geglu_unit);
    // the epilogue pairs column j with column j + tile_n / 2 of a tile: weights packed for another tile would give wrong numbers silently
    MDX_REQUIRE(p.epilogue != MDX_EPI_GEGLU || 2 * p.geglu_unit == bn,
                "mdx_gemm_f16: GEGLU weights packed with unit %d need tile_n = %d, this launch resolves to tile_n = %d", p.geglu_unit,
                2 * p.geglu_unit, bn);
    // 256-row tiles exist for the HALO conv only (forced tile_m = 256 on another launch)
    MDX_REQUIRE(bm != 256 || halo,
                "mdx_gemm_f16: tile_m = 256 needs a launch the 16 x 16-patch HALO conv applies to (3x3, stride 1, H %% 16 == 0, "
                "W %% 16 == 0, Cin %% 64 == 0)");
    if (p.gn_cs && p.ksize == 1)
        MDX_REQUIRE(p.HoWo % bm == 0, "mdx_gemm_f16: the fused input GroupNorm of a dense launch needs tokens per sample (%d) %% tile_m (%d) == 0",
                    p.HoWo, bm);
    else if (p.gn_cs)
        MDX_REQUIRE(halo && bn == 64 && !halo8_eligible(p),
                    "mdx_gemm_f16: the fused input GroupNorm needs a launch that resolves to the HALO 3x3 kernel with 64-column "
                    "tiles (ask mdx_gemm_query first)");
    MDX_REQUIRE(!p.skip_w || halo, "mdx_gemm_f16: the fused skip needs a launch that resolves to the HALO 3x3 kernel (ask mdx_gemm_query first)");
    if (halo) {
        // chunk-aligned splits: a split owns whole 64-channel chunks (9 K tiles each)
        const int chunks = p.cin / 64;
        if (ns > chunks) ns = chunks;
        p.ktiles_per_split = ((chunks + ns - 1) / ns) * 9;
    } else {
        p.ktiles_per_split = (p.ktiles + ns - 1) / ns;
    }
    ns = p.nsplit = pl.nsplit = (p.ktiles + p.ktiles_per_split - 1) / p.ktiles_per_split;  // no empty splits
    p.skip_kt_per_split = p.skip_w ? (p.skip_kt + ns - 1) / ns : 0;      // every split takes its share of the skip tiles
    pl.fixup = ns > 1 && fixup_eligible(d, p, bm, bn, ns);
    if (ns <= 1) pl.ws_head = pl.ws_per_split = 0;
    if (pl.fixup) p.tickets = reinterpret_cast<unsigned*>(p.ws);      // (a placeholder: mdx_gemm_f16 puts the workspace's counters here)
    else if (ns > 1) p.ws += MDX_TICKET_SLOTS;      // [split][M][N] slabs of the reduce-kernel path start behind the head
    if (ns > 1 && !pl.fixup)
        pl.reduce = d->defer_reduce ? GEMM_REDUCE_DEFERRED : p.colstats_out ? GEMM_REDUCE_COLSTATS
                    : (p.epilogue == MDX_EPI_PRELU || p.d2s_c) ? GEMM_REDUCE_EXT : GEMM_REDUCE_PLAIN;
    pl.colstats_rows = colstats_rows(halo);

    // ---- tile grid and ring depth
    p.tiles_m = (p.M + bm - 1) / bm;
    p.tiles_n = (p.N + bn - 1) / bn;
    pl.fastk = (p.cin % 64 == 0) && (p.c2 == 0 || p.c1 % 64 == 0);
    MDX_REQUIRE(pl.fastk || p.c2 == 0, "mdx_gemm_f16: two-source input needs c1 %% 64 == 0 and Cin %% 64 == 0");
    const int ntiles = p.tiles_m * p.tiles_n;
    p.tiles_per_xcd = (ntiles + 7) / 8;
    p.inv_tiles_n = p.tiles_n > 1 ? (unsigned)((0x100000000ull + (unsigned)p.tiles_n - 1) / (unsigned)p.tiles_n) : 0u;
    p.inv_tiles_m = p.tiles_m > 1 ? (unsigned)((0x100000000ull + (unsigned)p.tiles_m - 1) / (unsigned)p.tiles_m) : 0u;
    p.res_bytes = p.residual ? (unsigned)std::min<size_t>((size_t)p.M * (size_t)p.residual_ld * 2, 0x7fffffffull) : 0u;
    // share the bigger operand inside an XCD: unique activation bytes vs weight bytes
    p.n_fastest = ((size_t)p.M * p.cin >= (size_t)p.N * p.K) ? 1 : 0;
    p.spread = (p.tiles_m == 1 && mdx_opt(MDX_OPT_GEMM_SPREAD)) ? 1 : 0;
    pl.grid = p.spread ? dim3(ntiles * ns, 1) : dim3(8 * p.tiles_per_xcd, ns);
    const bool nw8 = stages >= 10;                         // eight waves per block (generic kernel, 128-row tiles)
    const int st_req = nw8 ? stages - 8 : stages;          // requested ring depth (0 = the rule below)
    const int optring = mdx_opt(MDX_OPT_GEMM_RING);        // experiments: 2..5 forces the LDS ring depth
    int ring = optring;
    if (!(optring >= 2 && optring <= 5)) {
        // ring depth: three stages wherever they still leave two blocks per CU (every tile but 128 x 128: 3 x 24 KB), and for
        // 128 x 128 tiles when the grid has at most one block per CU anyway; otherwise two.  tools/tune_gemm.py measures both
        // depths per shape (round 2: 143 of 153 retuned rows chose three) and the table overrides this rule.
        ring = (ntiles * ns <= 256 || bm + bn <= 192) ? 3 : 2;
        if (st_req >= 2 && st_req <= 6) ring = st_req;
    }
    pl.swap = (ns == 1 || pl.fixup) && (p.out_mode == MDX_OUT_ROWMAJOR);
    const bool lean = !halo && mdx_dense_takes(p, bm, bn, ring, ns, pl.fixup, nw8);
    MDX_REQUIRE(bn != 160 || lean, "mdx_gemm_f16: the 128 x 160 tile exists in the lean dense kernel only (ring depth 2 | 3, four waves; got stages %d)",
                stages);

    // ---- what the form the launch resolves to asks of the descriptor
    MDX_REQUIRE(!d->defer_reduce || ns > 1, "mdx_gemm_f16: defer_reduce set but the launch does not split K");
    MDX_REQUIRE(!p.xa_k || (lean && bn == 64 && ns == 1 && (p.HoWo % bm) == 0),
                "mdx_gemm_f16: the cross-attention epilogue needs the lean dense kernel on %d x 64 tiles inside one sample (got tile %d x %d, %d splits)",
                bm, bm, bn, ns);
    MDX_REQUIRE(!d->w_frag || halo, "mdx_gemm_f16: fragment-major weights (w_frag) are read by the HALO 3x3 conv only");

    // ---- kernel form
    if (halo) {
        if (d->w_frag) {
            MDX_REQUIRE(bm == 128, "mdx_gemm_f16: fragment-major weights run on 128-row HALO tiles only (got tile_m %d)", bm);
            // 128-column tiles whose split-K partials go to slabs (no in-kernel reduce): waves side by side along N
            pl.form = (bn == 128 && ns > 1 && !pl.fixup) ? GEMM_HALO_FRAG_W4 : GEMM_HALO_FRAG;
        } else {
            // weight ring depth: three stages where two blocks per CU still fit (64-column tiles: 46 KB halos + 3 x 8 KB; measured
            // -5...-25 % against two stages at the UNet shapes, batch 2 and 16) and for 256-pixel patches, which own the CU; 128 x 128
            // tiles keep two (a third stage would evict the second block); a fourth stage for the weight stream of a lone block
            pl.form = GEMM_HALO;
            pl.ring = (bm == 256 || bn == 64) ? 3 : 2;
            if (st_req >= 2 && st_req <= 4) pl.ring = st_req;
            if (mdx_opt(MDX_OPT_HALO_NSB) >= 2 && mdx_opt(MDX_OPT_HALO_NSB) <= 4) pl.ring = mdx_opt(MDX_OPT_HALO_NSB);
        }
    } else if (p.gn_cs || p.epilogue == MDX_EPI_PRELU || p.d2s_c) {
        // (ring depth as the occupancy rule / tile table chose it, capped at the three stages these forms are built with, four waves)
        pl.form = p.gn_cs ? GEMM_GNA : GEMM_EXT;
        pl.ring = ring >= 3 ? 3 : 2;
    } else if (lean) {
        pl.form = p.xa_k ? GEMM_LEAN_XA : GEMM_LEAN;
        pl.ring = ring;
    } else {
        // eight waves exist on 128-row tiles at ring depth 2 | 3; any other request runs the four-wave form
        pl.form = (nw8 && bm == 128 && (ring == 2 || ring == 3)) ? GEMM_GENERIC_NW8 : GEMM_GENERIC;
        pl.ring = ring;
        // (the text keeps the numbers it has always printed, the K tile and the ring depth BEFORE the occupancy rule / `stages`, so that
        // callers matching on it see no change; the depth that is not built is `ring`)
        MDX_REQUIRE(ring <= (bm == 128 ? 5 : 6), "mdx_gemm_f16: unsupported tile configuration bk=%d ns=%d", 64,
                    (optring >= 2 && optring <= 5) ? optring : 2);
    }
    return MDX_OK;
}

static unsigned long long* g_gemm_trace = nullptr;
static size_t g_gemm_trace_slots = 0;

// Diagnostics: while a buffer is registered, every block of the next mdx_gemm_f16 launches writes 8 x u64 phase
// timestamps (s_memrealtime, 100 MHz): 0 start, 1 prologue issued, 2 first tile landed, 3 main loop done, 4 epilogue
// done.  NULL unregisters.  Not thread safe; not for production use.
extern "C" int mdx_probe_gemm_trace(void* buf, size_t bytes) {
    g_gemm_trace = (unsigned long long*)buf;
    g_gemm_trace_slots = buf ? bytes / 64 : 0;
    return MDX_OK;
}

// Arrival counters of the in-kernel split-K reduce.  They used to sit in the first MDX_GEMM_WS_HEAD bytes of the caller's
// workspace, which made "hand the workspace over zeroed" part of the contract: a fresh hipMalloc'd buffer trapped, and zeroing on
// the first sight of an ADDRESS broke as soon as an allocator handed the same address out twice (round 3: the stress test after
// another test's workspace).  Now the library owns them: MDX_TICKET_SLOTS counters per (device, workspace address), carved from
// 1 MiB chunks that are zeroed once when they are allocated -- the ONE exception to "the library never allocates device memory"
// (include/mdx.h).  Every launch leaves its counters zero, so a slot is valid for whatever buffer an address names later; launches
// that may run concurrently have distinct workspaces (their partials) and therefore distinct counters.  The chunk is allocated with
// the thread's stream-capture mode relaxed and zeroed on a private stream, so a first use inside a capture works too.
struct TicketPools {
    std::mutex mu;
    std::map<std::pair<int, const void*>, unsigned*> slot;
    std::map<std::pair<int, const void*>, bool> caller_owned;      // slots bound by mdx_gemm_bind_counters: never recycled / freed here
    struct Dev { char* next = nullptr; int left = 0; hipStream_t zero_stream = nullptr; std::vector<unsigned*> free_slots; };
    std::map<int, Dev> dev;
    std::vector<std::pair<int, void*>> chunks;
};
static TicketPools g_tickets;
constexpr int TICKET_CHUNK_SLOTS = 64;

// The device a workspace lives on comes from the POINTER (hipPointerGetAttributes), not from the calling thread's current device: a
// C caller that drives several GPUs from one thread gets the right pool either way.
static int ticket_device_of(const void* ws) {
    hipPointerAttribute_t at;
    if (ws && hipPointerGetAttributes(&at, ws) == hipSuccess) return at.device;
    (void)hipGetLastError();
    int dv = 0;
    (void)hipGetDevice(&dv);
    return dv;
}

static int ticket_slot(const void* ws, unsigned** out) {
    const int dv = ticket_device_of(ws);
    std::lock_guard<std::mutex> lk(g_tickets.mu);
    const auto key = std::make_pair(dv, ws);
    const auto it = g_tickets.slot.find(key);
    if (it != g_tickets.slot.end()) {
        *out = it->second;
        return MDX_OK;
    }
    TicketPools::Dev& d = g_tickets.dev[dv];
    if (!d.free_slots.empty()) {        // a slot handed back by mdx_gemm_release_workspace: every launch left its counters zero
        unsigned* s = d.free_slots.back();
        d.free_slots.pop_back();
        g_tickets.slot.emplace(key, s);
        *out = s;
        return MDX_OK;
    }
    if (d.left == 0) {
        const size_t bytes = (size_t)TICKET_CHUNK_SLOTS * MDX_GEMM_WS_HEAD;
        int cur = 0;
        (void)hipGetDevice(&cur);
        if (cur != dv) (void)hipSetDevice(dv);
        hipStreamCaptureMode mode = hipStreamCaptureModeRelaxed;
        (void)hipThreadExchangeStreamCaptureMode(&mode);
        void* mem = nullptr;
        hipError_t e = hipMalloc(&mem, bytes);
        if (e == hipSuccess && !d.zero_stream) e = hipStreamCreateWithFlags(&d.zero_stream, hipStreamNonBlocking);
        if (e == hipSuccess) e = hipMemsetAsync(mem, 0, bytes, d.zero_stream);
        if (e == hipSuccess) e = hipStreamSynchronize(d.zero_stream);
        (void)hipThreadExchangeStreamCaptureMode(&mode);
        if (cur != dv) (void)hipSetDevice(cur);
        if (e != hipSuccess) {
            if (mem) (void)hipFree(mem);
            mdx_set_error("mdx_gemm_f16: allocating the split-K arrival counters failed: %s", hipGetErrorString(e));
            return MDX_E_HIP;
        }
        g_tickets.chunks.emplace_back(dv, mem);
        d.next = static_cast<char*>(mem);
        d.left = TICKET_CHUNK_SLOTS;
    }
    unsigned* s = reinterpret_cast<unsigned*>(d.next);
    d.next += MDX_GEMM_WS_HEAD;
    d.left -= 1;
    g_tickets.slot.emplace(key, s);
    *out = s;
    return MDX_OK;
}

// Caller-owned arrival counters (include/mdx.h): `counters` = MDX_GEMM_WS_HEAD bytes of ZEROED device memory on the workspace's
// device, bound to the workspace ADDRESS until mdx_gemm_release_workspace(workspace).  Launches on a bound workspace take their
// tickets there and the library makes no device allocation for them: a host that owns every byte (a graph-capturing caller on its
// own allocator) binds one set per workspace and the "one exception" of the ownership rule never fires.
extern "C" int mdx_gemm_bind_counters(const void* workspace, void* counters) {
    MDX_REQUIRE(workspace && counters && ((uintptr_t)counters % 16) == 0,
                "mdx_gemm_bind_counters: workspace and a 16-byte aligned counters buffer of MDX_GEMM_WS_HEAD zeroed bytes are required");
    const int dv = ticket_device_of(workspace);
    MDX_REQUIRE(ticket_device_of(counters) == dv, "mdx_gemm_bind_counters: the counters must live on the workspace's device");
    std::lock_guard<std::mutex> lk(g_tickets.mu);
    const auto key = std::make_pair(dv, workspace);
    const auto it = g_tickets.slot.find(key);
    if (it != g_tickets.slot.end()) {
        if (it->second == counters) return MDX_OK;
        // a library-owned set was handed to this address by an earlier launch: give it back, the caller's replaces it
        if (!g_tickets.caller_owned.count(key)) g_tickets.dev[dv].free_slots.push_back(it->second);
        g_tickets.slot.erase(it);
    }
    g_tickets.slot.emplace(key, static_cast<unsigned*>(counters));
    g_tickets.caller_owned[key] = true;
    return MDX_OK;
}

// Hands the arrival counters of ONE workspace back for reuse (include/mdx.h): call it when the workspace is freed.  Nothing may be
// in flight on it and every hipGraph captured with it must have been destroyed (a captured launch holds the counters' address).
// A caller-owned set (mdx_gemm_bind_counters) is only unbound: its memory is the caller's.
extern "C" int mdx_gemm_release_workspace(const void* workspace) {
    std::lock_guard<std::mutex> lk(g_tickets.mu);
    int n = 0;
    for (auto it = g_tickets.slot.begin(); it != g_tickets.slot.end();) {
        if (it->first.second == workspace) {
            const auto own = g_tickets.caller_owned.find(it->first);
            if (own != g_tickets.caller_owned.end())
                g_tickets.caller_owned.erase(own);
            else
                g_tickets.dev[it->first.first].free_slots.push_back(it->second);
            it = g_tickets.slot.erase(it);
            ++n;
        } else {
            ++it;
        }
    }
    return n;
}

// Frees the arrival counters (nothing may be in flight).  Later launches allocate again.
extern "C" int mdx_gemm_release_counters(void) {
    std::lock_guard<std::mutex> lk(g_tickets.mu);
    int dv = 0;
    (void)hipGetDevice(&dv);
    for (auto& c : g_tickets.chunks) {
        (void)hipSetDevice(c.first);
        (void)hipFree(c.second);
    }
    for (auto& d : g_tickets.dev)
        if (d.second.zero_stream) {
            (void)hipSetDevice(d.first);
            (void)hipStreamDestroy(d.second.zero_stream);
        }
    (void)hipSetDevice(dv);
    g_tickets.chunks.clear();
    g_tickets.slot.clear();
    g_tickets.caller_owned.clear();
    g_tickets.dev.clear();
    return MDX_OK;
}

extern "C" size_t mdx_gemm_workspace_bytes(const mdx_gemm_desc* d) {
    GemmParams p{};
    GemmPlan pl;
    if (fill_params(d, p) != MDX_OK || plan_gemm(d, p, pl, /*sizing=*/true) != MDX_OK) return 0;
    return pl.ws_head + (pl.nsplit > 1 ? (size_t)pl.nsplit * pl.ws_per_split : 0);
}

// Validation + launch resolution, no launch: a forced tile / a tile-table row whose kernel does not apply to this geometry is an
// error HERE, at plan time, not a launch that silently takes another form.
extern "C" int mdx_gemm_check(const mdx_gemm_desc* d) {
    GemmParams p{};
    GemmPlan pl;
    const int rc = fill_params(d, p);
    if (rc != MDX_OK) return rc;
    // (this entry has always reported an unaligned two-source input ahead of whatever the resolver objects to)
    MDX_REQUIRE(p.c2 == 0 || (p.cin % 64 == 0 && p.c1 % 64 == 0), "mdx_gemm_f16: two-source input needs c1 %% 64 == 0 and Cin %% 64 == 0");
    return plan_gemm(d, p, pl);
}

// What mdx_gemm_f16 would launch for this descriptor (no launch): out7 = {tile_m, tile_n, splitk, kernel (0 generic implicit
// GEMM, 1 HALO conv, 2 lean dense kernel of dense.hip), from_tuned_table, colstats rows per block, in-kernel split-K reduce}.  Parity tests use it to assert that the measured tile table
// (gemm_tuned.inc) is actually hit at the benchmarked shapes; the UNet plan asks it where GroupNorm statistics can come from.
extern "C" int mdx_gemm_query(const mdx_gemm_desc* d, int* out7) {
    GemmParams p{};
    GemmPlan pl;
    int rc = fill_params(d, p);
    if (rc != MDX_OK) return rc;
    MDX_REQUIRE(out7, "mdx_gemm_query: null output");
    rc = plan_gemm(d, p, pl);
    if (rc != MDX_OK) return rc;
    out7[0] = pl.bm;
    out7[1] = pl.bn;
    out7[2] = pl.nsplit;
    const bool conv = pl.form == GEMM_HALO || pl.form == GEMM_HALO_FRAG || pl.form == GEMM_HALO_FRAG_W4 || pl.form == GEMM_CONV8P;
    out7[3] = conv ? 1 : (pl.form == GEMM_LEAN || pl.form == GEMM_LEAN_XA) ? 2 : 0;
    out7[4] = (pl.tuned && pl.bn != 160) ? 1 : 0;      // (a row of gemm_tuned.inc; the 128 x 160 tile's rows are a table of their own)
    out7[5] = pl.colstats_rows;
    out7[6] = pl.fixup ? 1 : 0;
    return MDX_OK;
}

// Producer side of mdx_groupnorm_from_splitk_f16: the launch geometry of `d` as mdx_gemm_f16 resolves it.
int mdx_internal_split_info(const mdx_gemm_desc* d, MdxSplitInfo* info) {
    GemmParams p{};
    GemmPlan pl;
    int rc = fill_params(d, p);
    if (rc != MDX_OK) return rc;
    rc = plan_gemm(d, p, pl);
    if (rc != MDX_OK) return rc;
    MDX_REQUIRE(p.out_mode == MDX_OUT_ROWMAJOR && p.epilogue == MDX_EPI_NONE && !p.n_split && !p.ln_stats && !p.stats_out &&
                    !p.out_bs && !p.colstats_out && p.out_ld == p.N && p.N % 8 == 0,
                "deferred split-K reduce: plain dense row-major producers only");
    info->ws = p.ws;
    info->nsplit = pl.nsplit;
    info->M = p.M;
    info->N = p.N;
    info->HoWo = p.HoWo;
    info->B = p.B;
    info->bias = p.bias;
    info->rowbias = p.rowbias;
    info->rowbias_ld = p.rowbias_ld;
    info->residual = p.residual;
    info->residual_ld = p.residual_ld;
    info->out = p.out;
    return MDX_OK;
}

extern "C" int mdx_gemm_f16(const mdx_gemm_desc* d, mdx_stream_t s) {
    GemmParams p{};
    GemmPlan pl;
    int rc = fill_params(d, p);
    if (rc != MDX_OK) return rc;
    rc = plan_gemm(d, p, pl);
    if (rc != MDX_OK) return rc;
    if (p.colstats_out) {      // (not plan_gemm's: mdx_gemm_query must answer "0 rows" for such a descriptor, not fail)
        const int rows = pl.colstats_rows;
        MDX_REQUIRE(rows > 0, "mdx_gemm_f16: this launch cannot produce column statistics (ask mdx_gemm_query first)");
        MDX_REQUIRE((p.M + rows - 1) / rows <= d->colstats_cap,
                    "mdx_gemm_f16: colstats_out holds %d row blocks, this launch writes %d (%d rows each)", d->colstats_cap,
                    (p.M + rows - 1) / rows, rows);
    }
    // arrival counters: the in-kernel split-K reduce, and conv8p's tail tiles split along K (partials in the workspace)
    if (pl.fixup || (pl.form == GEMM_CONV8P && p.c8_split > 1)) {
        MDX_REQUIRE((uintptr_t)p.ws % 16 == 0, "mdx_gemm_f16: workspace must be 16-byte aligned");
        rc = ticket_slot(d->workspace, &p.tickets);
        if (rc != MDX_OK) return rc;
    }
    if (pl.form != GEMM_CONV8P)
        p.trace = (g_gemm_trace && (size_t)pl.grid.x * pl.grid.y <= g_gemm_trace_slots) ? g_gemm_trace : nullptr;
    return mdx_gemm_launch_plan(p, pl, (hipStream_t)s);
}

// First-use tuner (include/mdx.h).  The tile table (gemm_tuned.inc) covers the shapes of the benchmarked configurations; any
// other resolution / batch resolves through the cost model, which is 10-20 % off on some shapes.  This entry measures the
// launch forms the library has for ONE descriptor on the caller's stream -- tile_m x tile_n x split-K, every distinct form
// mdx_gemm_query resolves them to -- and returns the fastest as values for the descriptor's tile_m / tile_n / splitk / stages
// override fields (all zero = the library's own choice was the fastest, or within 2 % of it).  The caller keeps the answer (the
// cache is on the caller's side: minddiffusion_amd/ops.py tune_cache); the library keeps nothing.  It is the one entry that
// SYNCHRONISES (event waits on `s`) and so cannot be captured; the descriptor's output buffer is overwritten by every trial.
extern "C" int mdx_gemm_tune(const mdx_gemm_desc* d, mdx_stream_t s, void* flush, size_t flush_bytes, int reps, int* best4,
                             float* us2) {
    MDX_REQUIRE(d != nullptr && best4 != nullptr, "mdx_gemm_tune: null argument");
    MDX_REQUIRE(!d->defer_reduce && !d->colstats_out && !d->w_frag,
                "mdx_gemm_tune: descriptors whose consumer depends on the launch form (colstats_out, defer_reduce) or whose weights "
                "are packed for one form (w_frag) keep the library's choice");
    hipStream_t st = reinterpret_cast<hipStream_t>(s);
    if (reps < 1) reps = 5;
    if (reps > 31) reps = 31;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) {
        if (e0) (void)hipEventDestroy(e0);
        mdx_set_error("mdx_gemm_tune: hipEventCreate failed");
        return MDX_E_HIP;
    }
    auto measure = [&](const mdx_gemm_desc& c, float* us) -> int {
        int rc = mdx_gemm_f16(&c, st);       // warm-up; also the validity check of this form
        if (rc != MDX_OK) return rc;
        float t[32];
        for (int r = 0; r < reps; ++r) {
            if (flush && flush_bytes) (void)hipMemsetAsync(flush, r & 1, flush_bytes, st);      // evict L2 / MALL: cold weights
            (void)hipEventRecord(e0, st);
            rc = mdx_gemm_f16(&c, st);
            (void)hipEventRecord(e1, st);
            if (rc != MDX_OK) return rc;
            if (hipEventSynchronize(e1) != hipSuccess) {
                mdx_set_error("mdx_gemm_tune: a trial launch failed on the device");
                return MDX_E_HIP;
            }
            float ms = 0.f;
            (void)hipEventElapsedTime(&ms, e0, e1);
            t[r] = ms * 1e3f;
        }
        std::sort(t, t + reps);
        *us = t[reps / 2];
        return MDX_OK;
    };
    mdx_gemm_desc base = *d;
    base.tile_m = base.tile_n = base.splitk = base.stages = 0;
    int q0[7];
    int rc = mdx_gemm_query(&base, q0);
    float t_auto = 0.f;
    if (rc == MDX_OK) rc = measure(base, &t_auto);
    if (rc != MDX_OK) {
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
        return rc;
    }
    float t_best = t_auto;
    int best[4] = {0, 0, 0, 0};
    std::vector<long> seen;
    auto form = [](const int* q) { return (long)q[0] | ((long)q[1] << 10) | ((long)q[2] << 20) | ((long)q[3] << 30) | ((long)q[6] << 31); };
    seen.push_back(form(q0));
    static const int BMS[] = {64, 128, 256}, BNS[] = {64, 128}, NSS[] = {1, 2, 3, 4, 6, 8, 12, 16, 20};
    for (int bm : BMS)
        for (int bn : BNS)
            for (int ns : NSS) {
                mdx_gemm_desc c = base;
                c.tile_m = bm;
                c.tile_n = bn;
                c.splitk = ns;
                int q[7];
                if (mdx_gemm_query(&c, q) != MDX_OK) continue;
                if (q[0] != bm || q[1] != bn || q[2] != ns) continue;      // clamped to something another trial covers
                const long f = form(q);
                if (std::find(seen.begin(), seen.end(), f) != seen.end()) continue;
                seen.push_back(f);
                float t = 0.f;
                if (measure(c, &t) != MDX_OK) continue;
                if (t < t_best) {
                    t_best = t;
                    best[0] = bm, best[1] = bn, best[2] = ns, best[3] = 0;
                }
            }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (!(t_best < t_auto * 0.98f)) {
        best[0] = best[1] = best[2] = best[3] = 0;
        t_best = t_auto;
    }
    for (int i = 0; i < 4; ++i) best4[i] = best[i];
    if (us2) us2[0] = t_auto, us2[1] = t_best;
    return MDX_OK;
}
