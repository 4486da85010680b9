// LoRA merge (mdx_lora_merge_f16): W' = fp16(base + scale * B A) for one logical nn.Dense weight [N, K], written straight
// into the storage a kernel reads -- plain row-major, the tile-major pre-swizzled GEMM storage (ops.pack_gemm_weight) or the
// MFMA-fragment pieces of the fused SpatialTransformer streams (ops.pack_frag_weight) -- optionally with the LayerNorm fold
// (ops.fold_layernorm: gamma (.) W', S[n], W' beta + b) computed from the merged matrix.  The reference applies LoRA as a side
// branch of every LoRADense (wukong-huahua ldm/modules/attention.py:118-126); here the adapter is merged into the weights, in
// place, so that plans and captured graphs keep their pointers.
//
// Memory-bound: 4 N K bytes of base in, 2 N K bytes out.  One lane owns one 8-half chunk column (a 16-byte vector store in all
// three layouts) and walks RPT rows of it with the R rows of A for that column held in registers (R <= 8; larger ranks re-read
// A through L2); B[n, :] is a block-uniform read per row.  The fold's row sums are reduced in double with a fixed xor butterfly
// + a fixed-order LDS pass: no atomics, the same inputs give the same bits.
#include "mdx_common.h"

namespace {

constexpr int RPT = 4;      // rows per thread

struct LoraParams {
    const float* base;
    const float* A;
    const float* B;
    const float* gamma;
    const float* beta;
    const float* bias;
    float* S;
    float* cb;
    f16* dst;
    int N, K, R;
    float scale;
    int layout, ld, n0;
    int rows;           // N, or N + the zero padding rows this launch owns (TILED, last matrix of the destination)
    int kc;             // chunks per row written: K / 8, or ceil(K / 64) * 8 for TILED
    int cw;             // lanes along a row: power of two in [8, 256]
    int piece_stride, piece_offset;
};

__device__ __forceinline__ size_t chunk_offset(const LoraParams& p, int g, int c) {     // in halves; g = destination row
    if (p.layout == MDX_LORA_TILED) {
        const int r = g & 63;
        const int pos = (c & 7) ^ ((r >> 1) & 7);
        return ((((size_t)(g >> 6) * (p.kc >> 3) + (c >> 3)) * 64 + r) * 8 + pos) * 8;
    }
    if (p.layout == MDX_LORA_FRAG)
        return ((size_t)(g >> 5) * p.piece_stride + p.piece_offset + (c >> 1)) * 512 + (size_t)(((c & 1) * 32 + (g & 31)) * 8);
    return (size_t)g * p.ld + (size_t)c * 8;
}

// (the folded weights are rounded with f16_rne_from_f32_bits of mdx_common.h instead of a cast: ops.fold_layernorm's value is
// rounded twice, below)

// RREG: rows of A a lane keeps in registers (R <= RREG), or -1 = any R <= 64 with A read inside the row loop
template <int RREG>
__global__ __launch_bounds__(256) void lora_merge_kernel(const LoraParams p) {
    __shared__ double red[2][RPT][256];
    const int tid = threadIdx.x;
    const int cc = tid & (p.cw - 1);
    const int rl = tid / p.cw;
    const int nrl = 256 / p.cw;
    const int row0 = blockIdx.x * (nrl * RPT);
    const bool fold = p.gamma != nullptr;
    double s_acc[RPT], c_acc[RPT];
#pragma unroll
    for (int j = 0; j < RPT; ++j) s_acc[j] = c_acc[j] = 0.0;

    for (int c = cc; c < p.kc; c += p.cw) {
        const int k = c * 8;
        const bool kin = k < p.K;
        constexpr int RA = RREG > 0 ? RREG : 1;
        float a[RA][8];
        if (RREG > 0) {
#pragma unroll
            for (int r = 0; r < RA; ++r) {
                f32x4 lo = {0.f, 0.f, 0.f, 0.f}, hi = lo;
                if (kin && r < p.R) {
                    lo = *reinterpret_cast<const f32x4*>(p.A + (size_t)r * p.K + k);
                    hi = *reinterpret_cast<const f32x4*>(p.A + (size_t)r * p.K + k + 4);
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    a[r][e] = lo[e];
                    a[r][4 + e] = hi[e];
                }
            }
        }
        float ga[8], be[8];
        if (fold && kin) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                ga[e] = p.gamma[k + e];
                be[e] = p.beta[k + e];
            }
        }
#pragma unroll
        for (int j = 0; j < RPT; ++j) {
            const int n = row0 + j * nrl + rl;
            if (n >= p.rows) continue;
            f16x8 o;
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = (f16)0.f;
            if (n < p.N && kin) {
                const f32x4 lo = *reinterpret_cast<const f32x4*>(p.base + (size_t)n * p.K + k);
                const f32x4 hi = *reinterpret_cast<const f32x4*>(p.base + (size_t)n * p.K + k + 4);
                float v[8], acc[8];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    v[e] = lo[e];
                    v[4 + e] = hi[e];
                }
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[e] = 0.f;
                if (RREG > 0) {
#pragma unroll
                    for (int r = 0; r < RA; ++r) {
                        if (r < p.R) {
                            const float b = p.B[(size_t)n * p.R + r];
#pragma unroll
                            for (int e = 0; e < 8; ++e) acc[e] = __builtin_fmaf(b, a[r][e], acc[e]);
                        }
                    }
                } else if (RREG < 0) {
                    for (int r = 0; r < p.R; ++r) {
                        const float b = p.B[(size_t)n * p.R + r];
                        const f32x4 al = *reinterpret_cast<const f32x4*>(p.A + (size_t)r * p.K + k);
                        const f32x4 ah = *reinterpret_cast<const f32x4*>(p.A + (size_t)r * p.K + k + 4);
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            acc[e] = __builtin_fmaf(b, al[e], acc[e]);
                            acc[4 + e] = __builtin_fmaf(b, ah[e], acc[4 + e]);
                        }
                    }
                }
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    // R == 0: the pure re-pack keeps base's bits (a fused multiply-add with a zero product would turn -0 into +0)
                    const f16 wm = (f16)(RREG == 0 ? v[e] : __builtin_fmaf(p.scale, acc[e], v[e]));
                    if (fold) {
                        // ops.fold_layernorm: (double(W') double(gamma)).to(fp16).  The product is exact in double and the tensor
                        // library converts double -> half THROUGH fp32: fp16(fp32(product)) = one correctly rounded fp32 multiply,
                        // then the fp16 rounding as a separate step (a single-rounding conversion is
                        // 1 ulp away where the fp32 value is an fp16 tie, about 6e-5 of the elements)
                        const f16 wg = f16_rne_from_f32_bits((float)wm * ga[e]);
                        s_acc[j] += (double)wg;
                        c_acc[j] += (double)wm * (double)be[e];
                        o[e] = wg;
                    } else {
                        o[e] = wm;
                    }
                }
            }
            *reinterpret_cast<f16x8*>(p.dst + chunk_offset(p, p.n0 + n, c)) = o;
        }
    }
    if (!fold) return;      // (block-uniform)
    // row sums: xor butterfly over the lanes of a row inside the wave, then the row's waves in a fixed order through LDS
    const int span = p.cw < 64 ? p.cw : 64;
#pragma unroll
    for (int j = 0; j < RPT; ++j) {
        for (int o = span >> 1; o > 0; o >>= 1) {
            s_acc[j] += __shfl_xor(s_acc[j], o, 64);
            c_acc[j] += __shfl_xor(c_acc[j], o, 64);
        }
        red[0][j][tid] = s_acc[j];
        red[1][j][tid] = c_acc[j];
    }
    __syncthreads();
    if (cc == 0) {
#pragma unroll
        for (int j = 0; j < RPT; ++j) {
            const int n = row0 + j * nrl + rl;
            if (n >= p.N) continue;
            double s = 0.0, c = 0.0;
            for (int wv = 0; wv < p.cw; wv += 64) {     // one partial per wave of the row (a single pass when cw <= 64)
                s += red[0][j][tid + wv];
                c += red[1][j][tid + wv];
            }
            if (p.bias) c += (double)p.bias[n];
            p.S[n] = (float)s;
            p.cb[n] = (float)c;
        }
    }
}

}  // namespace

extern "C" int mdx_lora_merge_f16(const mdx_lora_merge_desc* d, mdx_stream_t s) {
    MDX_REQUIRE(d && d->base && d->dst, "mdx_lora_merge_f16: null descriptor / base / dst");
    MDX_REQUIRE(d->N > 0 && d->K > 0 && d->K % 8 == 0, "mdx_lora_merge_f16: K must be a multiple of 8 (N=%d K=%d)", d->N, d->K);
    MDX_REQUIRE(d->R >= 0 && d->R <= 64, "mdx_lora_merge_f16: rank %d outside [0, 64]", d->R);
    MDX_REQUIRE(d->scale == d->scale && d->scale - d->scale == 0.f, "mdx_lora_merge_f16: scale must be finite");
    MDX_REQUIRE(d->dst_n0 >= 0 && d->dst_n0 + d->N <= d->dst_N, "mdx_lora_merge_f16: rows [%d, %d) outside a destination of %d rows",
                d->dst_n0, d->dst_n0 + d->N, d->dst_N);
    MDX_REQUIRE(((size_t)d->base | (size_t)d->dst | (size_t)d->A) % 16 == 0, "mdx_lora_merge_f16: base / A / dst must be 16-byte aligned");
    const bool fold = d->gamma != nullptr;
    MDX_REQUIRE(!fold || (d->beta && d->S && d->cb), "mdx_lora_merge_f16: the fold needs gamma, beta, S and cb");
    MDX_REQUIRE(fold || !(d->beta || d->bias || d->S || d->cb), "mdx_lora_merge_f16: beta / bias / S / cb given without gamma");
    LoraParams p;
    p.base = d->base;
    p.R = (d->A && d->B) ? d->R : 0;
    p.A = p.R ? d->A : nullptr;
    p.B = p.R ? d->B : nullptr;
    p.gamma = d->gamma, p.beta = d->beta, p.bias = d->bias, p.S = d->S, p.cb = d->cb;
    p.dst = (f16*)d->dst;
    p.N = d->N, p.K = d->K, p.scale = d->scale, p.layout = d->layout, p.ld = d->ld, p.n0 = d->dst_n0;
    p.rows = d->N, p.kc = d->K / 8;
    p.piece_stride = d->piece_stride, p.piece_offset = d->piece_offset;
    if (d->layout == MDX_LORA_ROWMAJOR) {
        MDX_REQUIRE(d->ld >= d->K && d->ld % 8 == 0, "mdx_lora_merge_f16: ROWMAJOR ld must be a multiple of 8 and >= K (ld=%d)", d->ld);
    } else if (d->layout == MDX_LORA_TILED) {
        p.kc = (d->K + 63) / 64 * 8;
        if (d->dst_n0 + d->N == d->dst_N) p.rows = (d->dst_N + 63) / 64 * 64 - d->dst_n0;     // the last matrix zeroes the padding rows
    } else if (d->layout == MDX_LORA_FRAG) {
        MDX_REQUIRE(d->N % 32 == 0 && d->dst_n0 % 32 == 0 && d->K % 16 == 0,
                    "mdx_lora_merge_f16: FRAG needs N, dst_n0 multiples of 32 and K a multiple of 16 (N=%d n0=%d K=%d)", d->N, d->dst_n0, d->K);
        MDX_REQUIRE(d->piece_offset >= 0 && d->piece_offset + d->K / 16 <= d->piece_stride,
                    "mdx_lora_merge_f16: k-steps [%d, %d) outside a stream of %d pieces per column tile", d->piece_offset,
                    d->piece_offset + d->K / 16, d->piece_stride);
    } else {
        MDX_REQUIRE(false, "mdx_lora_merge_f16: unknown layout %d", d->layout);
    }
    int cw = 8;
    while (cw < p.kc && cw < 256) cw *= 2;
    p.cw = cw;
    const int rows_per_block = 256 / cw * RPT;
    const int blocks = (p.rows + rows_per_block - 1) / rows_per_block;
    hipStream_t st = (hipStream_t)s;
    if (p.R == 0)
        hipLaunchKernelGGL(lora_merge_kernel<0>, dim3(blocks), dim3(256), 0, st, p);
    else if (p.R <= 4)
        hipLaunchKernelGGL(lora_merge_kernel<4>, dim3(blocks), dim3(256), 0, st, p);
    else if (p.R <= 8)
        hipLaunchKernelGGL(lora_merge_kernel<8>, dim3(blocks), dim3(256), 0, st, p);
    else
        hipLaunchKernelGGL(lora_merge_kernel<-1>, dim3(blocks), dim3(256), 0, st, p);
    MDX_LAUNCH_CHECK("mdx_lora_merge_f16");
    return MDX_OK;
}
