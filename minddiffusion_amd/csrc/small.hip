// Small / elementwise kernels of the path: layout boundary, timestep embedding, small-M Dense, and the library's error
// plumbing and options.  (The fused sampler step family is sampler_step.hip, the hardware probes probes.hip.)
#include "mdx_common.h"

#include <string.h>

// ------------------------------------------------------------------ error plumbing
static thread_local char g_err[512] = "";

void mdx_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" const char* mdx_last_error(void) { return g_err; }

// ------------------------------------------------------------------ library options
static const char* const g_opt_names[MDX_OPT_COUNT] = {"gemm_tuned", "gemm_bm", "gemm_bn", "gemm_ring", "gemm_halo", "gemm_halo8",
                                                        "gemm_splitk_fixup_max", "gemm_spread", "halo_nsb", "gn_min_blocks",
                                                        "gn_fused", "gn_col_chunks", "gemm_conv8p", "gemm_conv8p_min_m", "gemm_subpixel_min_tiles", "gemm_conv8p_var", "attn8", "attn8_min_blocks",
                                                        "gn_wide_rows", "gn_fused_small", "gn_boost_mb", "attn_occ3", "attn_kv_split", "attn_fast_stage",
                                                        "gn_prefetch", "gemm_dense_issue", "gemm_ln_prefetch", "gemm_lean_dense", "attn_pipe"};
static int g_opt[MDX_OPT_COUNT] = {1, 0, 0, 0, 1, 1, 4, 1, 0, 512, 1, 4, 1, 4096, 32, 0, 0, 192, 0, 0, 40, 1, 1, 1, 1, 1, 1, 1, 1};

int mdx_opt(int id) { return g_opt[id]; }

extern "C" int mdx_set_option(const char* name, int value) {
    MDX_REQUIRE(name, "mdx_set_option: null name");
    for (int i = 0; i < MDX_OPT_COUNT; ++i)
        if (!strcmp(name, g_opt_names[i])) {
            g_opt[i] = value;
            return MDX_OK;
        }
    mdx_set_error("mdx_set_option: unknown option '%s'", name);
    return MDX_E_INVALID;
}

extern "C" int mdx_get_option(const char* name, int* value) {
    MDX_REQUIRE(name && value, "mdx_get_option: null argument");
    for (int i = 0; i < MDX_OPT_COUNT; ++i)
        if (!strcmp(name, g_opt_names[i])) {
            *value = g_opt[i];
            return MDX_OK;
        }
    mdx_set_error("mdx_get_option: unknown option '%s'", name);
    return MDX_E_INVALID;
}
extern "C" int mdx_version(void) { return 1; }

namespace {

// ------------------------------------------------------------------ layout boundary
__global__ __launch_bounds__(256) void nchw_to_nhwc_kernel(const float* __restrict__ x, f16* __restrict__ y, int B,
                                                           int C, int HW, int Cpad) {
    const size_t total = (size_t)B * HW * Cpad;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int c = (int)(i % Cpad);
        const size_t bp = i / Cpad;
        const int pix = (int)(bp % HW);
        const int b = (int)(bp / HW);
        y[i] = c < C ? (f16)x[((size_t)b * C + c) * HW + pix] : (f16)0.f;
    }
}

__global__ __launch_bounds__(256) void nhwc_to_nchw_kernel(const f16* __restrict__ x, float* __restrict__ y, int B,
                                                           int C, int HW, int Cs) {
    const size_t total = (size_t)B * C * HW;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int pix = (int)(i % HW);
        const size_t bc = i / HW;
        const int c = (int)(bc % C);
        const int b = (int)(bc / C);
        y[i] = (float)x[((size_t)b * HW + pix) * Cs + c];
    }
}

// ------------------------------------------------------------------ timestep embedding (util.py:111-131)
__global__ __launch_bounds__(256) void timestep_embedding_kernel(const float* __restrict__ t, float* __restrict__ out,
                                                                 int M, int dim, float neg_log_period) {
    const int half = dim / 2;
    const int total = M * half;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
        const int m = i / half, k = i - m * half;
        const float freq = expf(neg_log_period * (float)k / (float)half);
        const float arg = t[m] * freq;
        out[(size_t)m * dim + k] = cosf(arg);
        out[(size_t)m * dim + half + k] = sinf(arg);
        if ((dim & 1) && k == 0) out[(size_t)m * dim + dim - 1] = 0.f;
    }
}

// ------------------------------------------------------------------ small-M Dense
// One wave per output column n, MB rows of x per pass.  W row is streamed once per pass
// (16 B per lane); x is tiny and L2-resident.
template <int MB>
__global__ __launch_bounds__(256) void dense_small_kernel(const float* __restrict__ x, int x_ld,
                                                          const f16* __restrict__ w, const float* __restrict__ bias,
                                                          float* __restrict__ out, int out_ld, int M, int N, int K,
                                                          int act_in, int act_out) {
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;
    const f16* wr = w + (size_t)n * K;
    for (int m0 = 0; m0 < M; m0 += MB) {
        float acc[MB];
#pragma unroll
        for (int i = 0; i < MB; ++i) acc[i] = 0.f;
        for (int k = lane * 8; k < K; k += 64 * 8) {
            const f16x8 wv = *reinterpret_cast<const f16x8*>(wr + k);
            float wf[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) wf[e] = (float)wv[e];
#pragma unroll
            for (int i = 0; i < MB; ++i) {
                if (m0 + i < M) {
                    const float4* xp = reinterpret_cast<const float4*>(x + (size_t)(m0 + i) * x_ld + k);
                    const float4 a = xp[0], b = xp[1];
                    float xv[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const float v = act_in ? silu_f(xv[e]) : xv[e];
                        acc[i] += v * wf[e];
                    }
                }
            }
        }
#pragma unroll
        for (int i = 0; i < MB; ++i) {
            const float s = wave_sum(acc[i]);
            if (lane == 0 && m0 + i < M) {
                float v = s + (bias ? bias[n] : 0.f);
                if (act_out) v = silu_f(v);
                out[(size_t)(m0 + i) * out_ld + n] = v;
            }
        }
    }
}

}  // namespace

extern "C" int mdx_nchw_to_nhwc_f16(const float* x, void* y, int B, int C, int H, int W, int Cpad, mdx_stream_t s) {
    MDX_REQUIRE(x && y && B > 0 && C > 0 && H > 0 && W > 0 && Cpad >= C, "mdx_nchw_to_nhwc_f16: bad arguments");
    const size_t total = (size_t)B * H * W * Cpad;
    hipLaunchKernelGGL(nchw_to_nhwc_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)s, x, (f16*)y, B, C,
                       H * W, Cpad);
    MDX_LAUNCH_CHECK("mdx_nchw_to_nhwc_f16");
    return MDX_OK;
}

extern "C" int mdx_nhwc_to_nchw_f32(const void* x, float* y, int B, int C, int H, int W, int Cstride,
                                    mdx_stream_t s) {
    MDX_REQUIRE(x && y && B > 0 && C > 0 && H > 0 && W > 0 && Cstride >= C, "mdx_nhwc_to_nchw_f32: bad arguments");
    const size_t total = (size_t)B * C * H * W;
    hipLaunchKernelGGL(nhwc_to_nchw_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)s, (const f16*)x, y, B,
                       C, H * W, Cstride);
    MDX_LAUNCH_CHECK("mdx_nhwc_to_nchw_f32");
    return MDX_OK;
}

extern "C" int mdx_timestep_embedding_f32(const float* t, float* out, int M, int dim, float max_period,
                                          mdx_stream_t s) {
    MDX_REQUIRE(t && out && M > 0 && dim >= 2 && max_period > 0.f, "mdx_timestep_embedding_f32: bad arguments");
    hipLaunchKernelGGL(timestep_embedding_kernel, dim3(grid_for((size_t)M * (dim / 2))), dim3(256), 0, (hipStream_t)s,
                       t, out, M, dim, -logf(max_period));
    MDX_LAUNCH_CHECK("mdx_timestep_embedding_f32");
    return MDX_OK;
}

extern "C" int mdx_dense_small_f32(const float* x, int x_ld, const void* w, const float* b, float* out, int out_ld,
                                   int M, int N, int K, int act_in, int act_out, mdx_stream_t s) {
    MDX_REQUIRE(x && w && out, "mdx_dense_small_f32: null pointer");
    MDX_REQUIRE(M > 0 && N > 0 && K > 0 && K % 8 == 0 && x_ld % 4 == 0 && x_ld >= K && out_ld >= N,
                "mdx_dense_small_f32: bad extents (M=%d N=%d K=%d)", M, N, K);
    dim3 grid((N + 3) / 4);
    hipStream_t st = (hipStream_t)s;
    if (M <= 2)
        hipLaunchKernelGGL(dense_small_kernel<2>, grid, dim3(256), 0, st, x, x_ld, (const f16*)w, b, out, out_ld, M, N, K, act_in, act_out);
    else
        hipLaunchKernelGGL(dense_small_kernel<8>, grid, dim3(256), 0, st, x, x_ld, (const f16*)w, b, out, out_ld, M, N, K, act_in, act_out);
    MDX_LAUNCH_CHECK("mdx_dense_small_f32");
    return MDX_OK;
}
