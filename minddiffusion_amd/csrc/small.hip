// Small / elementwise kernels of the path: layout boundary, timestep embedding, small-M Dense,
// fused sampler update, hardware-layout probes, and the library's error plumbing.
#include "mdx_common.h"
#include "rng_device.h"

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

// ------------------------------------------------------------------ fused sampler update (plms.py:188-244)
struct StepParams {
    const float* x;
    const f16* eps_u;
    const f16* eps_c;
    const float* old1;
    const float* old2;
    const float* old3;
    const float* noise;
    float* e_t_out;
    float* x_prev;
    float* pred_x0;
    int eps_ld, B, C, HW;
    float cfg_scale, c0, c1, c2, c3;
    float sqrt_at, sqrt_one_minus_at, sqrt_a_prev, dir_coef, sigma;
    // MDX_PRED_V only: the latent the model was evaluated on, sqrt(alphas_cumprod) and sqrt(1 - alphas_cumprod) there
    const float* x_model;
    float am, bm;
};

// PRED: MDX_PRED_EPS | MDX_PRED_V.  No __restrict__: x_prev may alias x, and for MDX_PRED_V also x_model (the second call of
// the PLMS first step writes the latent its model output was computed on).  The outputs may alias no other input, so what
// matters is that x_model[i] is read before the first store for i and x[i] before x_prev[i] is stored -- both hold below.
// MDX_PRED_EPS compiles to exactly the statements mdx_sampler_step_f32 has always launched.
// sampler_step_element is the update of ONE element, the body of sampler_step_kernel and of sampler_step_table_kernel.
template <int PRED>
__device__ __forceinline__ void sampler_step_element(const StepParams& p, size_t i, size_t ei) {
    float e_t = (float)p.eps_c[ei];
    if (p.eps_u) {
        const float eu = (float)p.eps_u[ei];
        e_t = eu + p.cfg_scale * (e_t - eu);
    }
    if constexpr (PRED == MDX_PRED_V) e_t = p.am * e_t + p.bm * p.x_model[i];   // eps = a v + b x_m (dpm_solver.py:281-284)
    if (p.e_t_out) p.e_t_out[i] = e_t;
    float ep = p.c0 * e_t;
    if (p.old1) ep += p.c1 * p.old1[i];
    if (p.old2) ep += p.c2 * p.old2[i];
    if (p.old3) ep += p.c3 * p.old3[i];
    const float xv = p.x[i];
    const float px0 = (xv - p.sqrt_one_minus_at * ep) / p.sqrt_at;
    float xp = p.sqrt_a_prev * px0 + p.dir_coef * ep;
    if (p.noise) xp += p.sigma * p.noise[i];
    if (p.pred_x0) p.pred_x0[i] = px0;
    p.x_prev[i] = xp;
}

template <int PRED>
__global__ __launch_bounds__(256) void sampler_step_kernel(const StepParams p) {
    mdx_kernarg_touch<sizeof(StepParams)>();
    const size_t total = (size_t)p.B * p.C * p.HW;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int pix = (int)(i % p.HW);
        const size_t bc = i / p.HW;
        const int c = (int)(bc % p.C);
        const int b = (int)(bc / p.C);
        sampler_step_element<PRED>(p, i, ((size_t)b * p.HW + pix) * p.eps_ld + c);
    }
}

// ------------------------------------------------------------------ fused sampler update with guidance rescale
// Lin et al., "Common Diffusion Noise Schedules and Sample Steps are Flawed", section 3.4: the CFG-combined model output m is
// scaled by f[b] = phi * std(out_c[b]) / std(m[b]) + (1 - phi) before the step.  The statistics are per sample over C * HW,
// so ONE workgroup owns a sample: pass 1 reads only the two model outputs (which no output may alias) in their own NHWC order,
// pass 2 is sampler_step_kernel's statement sequence with m *= f after the combine.
struct RescaleParams {
    StepParams s;
    float phi;
    float* factor_out;
};

constexpr int RESCALE_THREADS = 1024;

// Sums are taken of d = v - K with K = the mean of the sample's first 64 values (the same bits in every wave), so that
// sum(d^2) - sum(d)^2 / N cancels nothing to speak of when the outputs sit on an offset far above their spread.
// The two passes are device functions of (parameters, sample): sampler_step_rescale_kernel runs them on its kernel arguments,
// sampler_step_table_kernel on the parameters of the sample's table row.
__device__ __forceinline__ float rescale_factor(const StepParams& p, float phi, int b, float (*part)[4]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned N = (unsigned)p.C * (unsigned)p.HW;      // per sample: the host refuses what does not fit 31 bits
    const unsigned C = p.C, HW = p.HW;
    const f16* ou = p.eps_u + (size_t)b * HW * p.eps_ld;
    const f16* oc = p.eps_c + (size_t)b * HW * p.eps_ld;

    // ---- pass 1: unbiased per-sample std of out_c and of m, in the outputs' own (pixel, channel) order
    float kc, km;
    {
        const unsigned j = (unsigned)lane < N ? (unsigned)lane : N - 1;
        const size_t ei = (size_t)(j / C) * p.eps_ld + j % C;
        const float c = (float)oc[ei], u = (float)ou[ei];
        kc = wave_sum(c) * (1.f / 64.f);
        km = wave_sum(u + p.cfg_scale * (c - u)) * (1.f / 64.f);
    }
    float sc = 0.f, scc = 0.f, sm = 0.f, smm = 0.f;
#pragma unroll 4
    for (unsigned j = threadIdx.x; j < N; j += RESCALE_THREADS) {
        const size_t ei = (size_t)(j / C) * p.eps_ld + j % C;
        const float c = (float)oc[ei], u = (float)ou[ei];
        const float dc = c - kc, dm = u + p.cfg_scale * (c - u) - km;
        sc += dc;
        scc += dc * dc;
        sm += dm;
        smm += dm * dm;
    }
    sc = wave_sum(sc);
    scc = wave_sum(scc);
    sm = wave_sum(sm);
    smm = wave_sum(smm);
    if (lane == 0) {
        part[wave][0] = sc;
        part[wave][1] = scc;
        part[wave][2] = sm;
        part[wave][3] = smm;
    }
    __syncthreads();
    sc = scc = sm = smm = 0.f;
#pragma unroll
    for (int w = 0; w < RESCALE_THREADS / 64; ++w) {     // the same order in every thread: one f per sample, bit for bit
        sc += part[w][0];
        scc += part[w][1];
        sm += part[w][2];
        smm += part[w][3];
    }
    const float n = (float)N;
    const float std_c = sqrtf(fmaxf(scc - sc * sc / n, 0.f) / (n - 1.f));
    const float std_m = sqrtf(fmaxf(smm - sm * sm / n, 0.f) / (n - 1.f));
    float f = 1.f;
    if (std_m > 0.f && std_m <= 3.402823466e38f) f = phi * std_c / std_m + (1.f - phi);   // NaN fails both tests
    return f;
}

template <int PRED>
__device__ __forceinline__ void rescale_apply(const StepParams& p, float f, int b) {
    const unsigned N = (unsigned)p.C * (unsigned)p.HW;
    const unsigned HW = p.HW;
    const f16* ou = p.eps_u + (size_t)b * HW * p.eps_ld;
    const f16* oc = p.eps_c + (size_t)b * HW * p.eps_ld;
    // ---- pass 2: the step (sampler_step_kernel's statements on m' = f m), U elements of a thread at a time: all their
    // loads first, then the arithmetic and the stores.  The outputs may alias x / x_model only element for element, so a
    // thread that has read its own U elements may store them; without the batching every trip of the loop waits out one
    // memory latency behind the previous trip's stores (a workgroup has a sample to itself, so there is no one else to hide it).
    constexpr int U = 4;
    const size_t base = (size_t)b * N;
    for (unsigned j0 = threadIdx.x; j0 < N; j0 += RESCALE_THREADS * U) {
        float m[U], xm[U], xv[U], o1[U], o2[U], o3[U], nz[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const unsigned j = j0 + u * RESCALE_THREADS;
            if (j < N) {
                const size_t i = base + j;
                const unsigned c = j / HW;
                const size_t ei = (size_t)(j - c * HW) * p.eps_ld + c;
                const float eu = (float)ou[ei];
                m[u] = eu + p.cfg_scale * ((float)oc[ei] - eu);
                if constexpr (PRED == MDX_PRED_V) xm[u] = p.x_model[i];
                xv[u] = p.x[i];
                if (p.old1) o1[u] = p.old1[i];
                if (p.old2) o2[u] = p.old2[i];
                if (p.old3) o3[u] = p.old3[i];
                if (p.noise) nz[u] = p.noise[i];
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const unsigned j = j0 + u * RESCALE_THREADS;
            if (j < N) {
                const size_t i = base + j;
                float e_t = m[u] * f;
                // eps = a v + b x_m (dpm_solver.py:281-284).  This statement and x_prev below are spelled in the form
                // sampler_step_kernel's expressions compile to (here: the product with x_m rounded, the one with m' fused;
                // below: both products rounded, then added), so that with f == 1 the two kernels agree to the bit
                // (test_constant_outputs_give_factor_one holds them to it).
                if constexpr (PRED == MDX_PRED_V) e_t = __builtin_fmaf(p.am, e_t, p.bm * xm[u]);
                if (p.e_t_out) p.e_t_out[i] = e_t;
                float ep = p.c0 * e_t;
                if (p.old1) ep += p.c1 * o1[u];
                if (p.old2) ep += p.c2 * o2[u];
                if (p.old3) ep += p.c3 * o3[u];
                const float px0 = (xv[u] - p.sqrt_one_minus_at * ep) / p.sqrt_at;
                float xp;
                {
#pragma clang fp contract(off)
                    xp = p.sqrt_a_prev * px0 + p.dir_coef * ep;
                }
                if (p.noise) xp += p.sigma * nz[u];
                if (p.pred_x0) p.pred_x0[i] = px0;
                p.x_prev[i] = xp;
            }
        }
    }
}

template <int PRED>
__global__ __launch_bounds__(RESCALE_THREADS) void sampler_step_rescale_kernel(const RescaleParams rp) {
    mdx_kernarg_touch<sizeof(RescaleParams)>();
    const StepParams& p = rp.s;
    __shared__ float part[RESCALE_THREADS / 64][4];
    const int b = blockIdx.x;
    const float f = rescale_factor(p, rp.phi, b, part);
    if (rp.factor_out && threadIdx.x == 0) rp.factor_out[b] = f;
    rescale_apply<PRED>(p, f, b);
}

// ------------------------------------------------------------------ fused sampler update, per-sample scalars from a table
// Every scalar the three kernels above take as a kernel argument comes from row b of a device table (MDX_STEP_* of mdx.h),
// so samples with different guidance scales, rescale strengths and schedules share one launch.  A workgroup works on ONE
// sample: its row is the same address in every lane.  table_row fills the StepParams of that sample, with the pointers the
// scalar entries' host code would have kept (a term whose coefficient is exactly 0 is skipped, not multiplied: what it
// points to may be NaN); the kernels then run the very bodies of the scalar kernels on them.
struct TableParams {
    StepParams s;
    const float* table;
    float* factor_out;
};

// row: the MDX_STEP_ROW floats of the sample, or nullptr for a sample that has none (a session slot outside its request)
__device__ __forceinline__ bool table_row(StepParams& p, const float* row, float& phi) {
    if (!row || row[MDX_STEP_ACTIVE] == 0.f) return false;
    p.cfg_scale = row[MDX_STEP_CFG_SCALE];
    phi = row[MDX_STEP_RESCALE];
    p.am = row[MDX_STEP_SQRT_AT_MODEL];
    p.bm = row[MDX_STEP_SQRT_ONE_MINUS_AT_MODEL];
    p.c0 = row[MDX_STEP_C0];
    p.c1 = row[MDX_STEP_C0 + 1];
    p.c2 = row[MDX_STEP_C0 + 2];
    p.c3 = row[MDX_STEP_C0 + 3];
    p.sqrt_at = row[MDX_STEP_SQRT_AT];
    p.sqrt_one_minus_at = row[MDX_STEP_SQRT_ONE_MINUS_AT];
    p.sqrt_a_prev = row[MDX_STEP_SQRT_A_PREV];
    p.dir_coef = row[MDX_STEP_DIR_COEF];
    p.sigma = row[MDX_STEP_SIGMA];
    if (p.c1 == 0.f) p.old1 = nullptr;
    if (p.c2 == 0.f) p.old2 = nullptr;
    if (p.c3 == 0.f) p.old3 = nullptr;
    if (p.sigma == 0.f) p.noise = nullptr;
    return true;
}

// An inactive row (a request whose schedule has ended): the latent travels to the other buffer, nothing else is written.
__device__ __forceinline__ void table_copy_row(const StepParams& p, int b, unsigned first, unsigned stride) {
    if (p.x_prev == p.x) return;
    const unsigned N = (unsigned)p.C * (unsigned)p.HW;
    const size_t base = (size_t)b * N;
    for (unsigned j = first + threadIdx.x; j < N; j += stride) p.x_prev[base + j] = p.x[base + j];
}

// The two launch forms as functions of (parameters, the sample's row): the table kernels hand them row b of one table, the
// slot kernels the row their slot stands on.
// No row rescales: gridDim.x workgroups share sample blockIdx.y, sampler_step_kernel's statements per element.
template <int PRED>
__device__ __forceinline__ void step_row_spread(StepParams& p, const float* row, float* factor_out) {
    const int b = blockIdx.y;
    const unsigned N = (unsigned)p.C * (unsigned)p.HW, HW = p.HW;      // the host refuses what does not fit 31 bits
    const unsigned first = blockIdx.x * 256u, stride = gridDim.x * 256u;
    float phi;
    if (!table_row(p, row, phi)) {
        table_copy_row(p, b, first, stride);
        return;
    }
    if (factor_out && blockIdx.x == 0 && threadIdx.x == 0) factor_out[b] = 1.f;
    const size_t base = (size_t)b * N;
    for (unsigned j = first + threadIdx.x; j < N; j += stride) {
        const unsigned c = j / HW;
        sampler_step_element<PRED>(p, base + j, ((size_t)b * HW + (j - c * HW)) * p.eps_ld + c);
    }
}

// Some row rescales: a workgroup owns a sample, as in sampler_step_rescale_kernel; a row with phi == 0 reads no statistics
// and runs pass 2 with f = 1, which is sampler_step_kernel's result to the bit.  That equality is NOT by construction:
// rescale_apply spells out by hand (__builtin_fmaf, fp contract(off)) the contraction the compiler currently chooses for
// sampler_step_element, so it is coupled to the compiler's choices.  tests/test_step_table_gpu.py (phi == 0 rows of a mixed
// launch against the plain entry) and test_constant_outputs_give_factor_one hold it on hardware; if a toolchain update makes
// them fail, respell rescale_apply -- do not loosen the tests.
template <int PRED>
__device__ __forceinline__ void step_row_owned(StepParams& p, const float* row, float* factor_out, float (*part)[4]) {
    const int b = blockIdx.x;
    float phi;
    if (!table_row(p, row, phi)) {
        table_copy_row(p, b, 0u, (unsigned)RESCALE_THREADS);
        return;
    }
    float f = 1.f;
    if (phi != 0.f) f = rescale_factor(p, phi, b, part);      // the row is the workgroup's: every thread takes the same side
    if (factor_out && threadIdx.x == 0) factor_out[b] = f;
    rescale_apply<PRED>(p, f, b);
}

template <int PRED>
__global__ __launch_bounds__(256) void sampler_step_table_kernel(const TableParams tp) {
    mdx_kernarg_touch<sizeof(TableParams)>();
    StepParams p = tp.s;
    step_row_spread<PRED>(p, tp.table + (size_t)blockIdx.y * MDX_STEP_ROW, tp.factor_out);
}

template <int PRED>
__global__ __launch_bounds__(RESCALE_THREADS) void sampler_step_table_rescale_kernel(const TableParams tp) {
    mdx_kernarg_touch<sizeof(TableParams)>();
    StepParams p = tp.s;
    __shared__ float part[RESCALE_THREADS / 64][4];
    step_row_owned<PRED>(p, tp.table + (size_t)blockIdx.x * MDX_STEP_ROW, tp.factor_out, part);
}

// ------------------------------------------------------------------ fused sampler update, rows looked up per session slot
// A sampling session (mdx_sampler_step_slots_f32): slot b keeps the rows of the request in it, sched[b][0 .. cap), and stands
// on row pos = tick - slot_start[b] of them.  The tick is a kernel argument and nothing on the device moves between
// admissions.  A slot outside its request has no row: the inactive row of the table entry.
struct SlotParams {
    StepParams s;
    const float* sched;       // [B][cap][MDX_STEP_ROW]
    const int* slot_start;    // [B]
    const int* slot_len;      // [B]
    int cap, tick;
    float* factor_out;
};

__device__ __forceinline__ const float* slot_row(const SlotParams& sp, int b) {
    const int pos = mdx_slot_pos(sp.slot_start, sp.slot_len, b, sp.cap, sp.tick);
    return pos < 0 ? nullptr : sp.sched + ((size_t)b * sp.cap + pos) * MDX_STEP_ROW;
}

template <int PRED>
__global__ __launch_bounds__(256) void sampler_step_slots_kernel(const SlotParams sp) {
    mdx_kernarg_touch<sizeof(SlotParams)>();
    StepParams p = sp.s;
    step_row_spread<PRED>(p, slot_row(sp, blockIdx.y), sp.factor_out);
}

template <int PRED>
__global__ __launch_bounds__(RESCALE_THREADS) void sampler_step_slots_rescale_kernel(const SlotParams sp) {
    mdx_kernarg_touch<sizeof(SlotParams)>();
    StepParams p = sp.s;
    __shared__ float part[RESCALE_THREADS / 64][4];
    step_row_owned<PRED>(p, slot_row(sp, blockIdx.x), sp.factor_out, part);
}

// ------------------------------------------------------------------ the DPM-Solver step launch (mdx_sampler_step_lin_f32)
// The model value of one evaluation (data or noise prediction, optionally thresholded) and the linear form
// x_out = A x_base + c0 val + c1 h1 + c2 h2 that every update of the solver is; include/mdx.h has the contract.  The host
// keeps a history pointer only for a non-zero coefficient and sets phi = 0 without an unconditional half, so the kernels test
// pointers and A / phi only.  No __restrict__: x_out may be x_base and / or x_model, element for element -- every kernel below
// reads element i of both before it stores element i of x_out, in the same thread.
struct LinParams {
    const float* x_base;
    const float* x_model;
    const f16* out_u;
    const f16* out_c;
    const float* h1;
    const float* h2;
    float* model_out;
    float* x_out;
    float* model_pre_out;
    float* thr_out;
    float* factor_out;
    int out_ld, B, C, HW;
    float cfg_scale, am, sm, A, c0, c1, c2, phi, max_val;
    unsigned k;               // thresholding: the rank (0-based) of the lower of the two order statistics
    int thresholding;
};

// Step 8 (mdx_sampler_step_lin_noise_f32): x_out = (step 7) + cn * z, one fma.  NOISE says where z comes from: a tensor, or
// the generator -- quad_values<MODE_NORMAL> of rng_device.h at (seeds[b], stream, draw), scale 1, the bits mdx_randn_f32 stores.
// One Philox call gives the four elements 4 q .. 4 q + 3 of a sample (counted from the sample's start: with C * HW % 4 != 0 the
// last quad is partial, with HW % 4 != 0 a quad straddles two channels -- every element finds its own channel and pixel), so
// quads are dealt, never drawn once per element: to threads in the SPREAD form, to lanes in the OWNED form (below).  Both
// noise sources run the same statements on an element but the one that fetches z, so they agree to the bit.  The
// LIN_NOISE_NONE instantiations are the kernels mdx_sampler_step_lin_f32 has always launched: they take LinParams alone.
enum { LIN_NOISE_NONE = 0, LIN_NOISE_TENSOR = 1, LIN_NOISE_SEEDED = 2 };

struct LinNoise {
    float cn;
    const float* noise;
    const unsigned long long* seeds;
    unsigned stream, draw;
};

struct LinNoiseParams {
    LinParams l;
    LinNoise n;
};

constexpr int LIN_U = 4;

// the quad that starts at element j0 (a multiple of 4) of sample b
__device__ __forceinline__ void lin_quad_z(const LinNoise& n, int b, unsigned j0, float (&z)[LIN_U]) {
    RngParams r{};
    r.stream = n.stream;
    r.scale = 1.0f;
    unsigned bits[4];
    quad_values<MODE_NORMAL>(r, n.seeds[b], n.draw, j0 >> 2, bits);
#pragma unroll
    for (int e = 0; e < 4; ++e) z[e] = __uint_as_float(bits[e]);
}

// steps 3 and 4: the CFG-combined (and rescaled) model output m to the model value
template <int PRED, int VALUE>
__device__ __forceinline__ float lin_value(const LinParams& p, float m, float xm) {
    float e = m;
    if constexpr (PRED == MDX_PRED_V) e = p.am * m + p.sm * xm;      // eps = a v + b x_m (dpm_solver.py:281-284)
    if constexpr (VALUE == MDX_VALUE_X0) return (xm - p.sm * e) / p.am;
    return e;
}

template <int PRED, int VALUE>
constexpr bool lin_reads_x_model = PRED == MDX_PRED_V || VALUE == MDX_VALUE_X0;

// step 7; a skipped term's operand is whatever the caller left in the register
__device__ __forceinline__ float lin_form(const LinParams& p, float val, float xb, float h1, float h2) {
    float xo = p.c0 * val;
    if (p.A != 0.f) xo += p.A * xb;
    if (p.h1) xo += p.c1 * h1;
    if (p.h2) xo += p.c2 * h2;
    return xo;
}

// SPREAD: sampler_step_kernel's grid and element order
template <int PRED, int VALUE>
__global__ __launch_bounds__(256) void sampler_step_lin_kernel(const LinParams p) {
    mdx_kernarg_touch<sizeof(LinParams)>();
    const size_t total = (size_t)p.B * p.C * p.HW;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int pix = (int)(i % p.HW);
        const size_t bc = i / p.HW;
        const int c = (int)(bc % p.C);
        const int b = (int)(bc / p.C);
        const size_t ei = ((size_t)b * p.HW + pix) * p.out_ld + c;
        float m = (float)p.out_c[ei];
        if (p.out_u) {
            const float eu = (float)p.out_u[ei];
            m = eu + p.cfg_scale * (m - eu);
        }
        float xm = 0.f, xb = 0.f, h1 = 0.f, h2 = 0.f;
        if constexpr (lin_reads_x_model<PRED, VALUE>) xm = p.x_model[i];
        if (p.A != 0.f) xb = p.x_base[i];
        if (p.h1) h1 = p.h1[i];
        if (p.h2) h2 = p.h2[i];
        const float val = lin_value<PRED, VALUE>(p, m, xm);
        p.model_out[i] = val;
        if (p.model_pre_out) p.model_pre_out[i] = val;
        p.x_out[i] = lin_form(p, val, xb, h1, h2);
    }
}

// SPREAD with step 8: a quad per thread and trip, all loads first (the draw's arithmetic then runs under their latency), then
// the arithmetic and the stores -- a thread stores only elements it has read, so x_out may be x_base / x_model as above.
// 64-thread workgroups: a quad is four elements, so the latent of a UNet batch still spreads over a hundred CUs and more.
constexpr int LIN_NOISE_THREADS = 64;

template <int PRED, int VALUE, int NOISE>
__global__ __launch_bounds__(LIN_NOISE_THREADS) void sampler_step_lin_noise_kernel(const LinNoiseParams q) {
    mdx_kernarg_touch<sizeof(LinNoiseParams)>();
    const LinParams& p = q.l;
    const unsigned N = (unsigned)p.C * (unsigned)p.HW, HW = p.HW;       // the host refuses what does not fit 31 bits
    const unsigned quads = (N + 3u) / 4u;
    const size_t items = (size_t)p.B * quads;
    for (size_t it = (size_t)blockIdx.x * LIN_NOISE_THREADS + threadIdx.x; it < items;
         it += (size_t)gridDim.x * LIN_NOISE_THREADS) {
        const int b = (int)(it / quads);
        const unsigned j0 = (unsigned)(it - (size_t)b * quads) * 4u;
        const size_t base = (size_t)b * N;
        float m[LIN_U], xm[LIN_U], xb[LIN_U], h1[LIN_U], h2[LIN_U], z[LIN_U];
#pragma unroll
        for (int u = 0; u < LIN_U; ++u) {
            const unsigned j = j0 + u;
            m[u] = xm[u] = xb[u] = h1[u] = h2[u] = z[u] = 0.f;
            if (j < N) {
                const size_t i = base + j;
                const unsigned c = j / HW;
                const size_t ei = ((size_t)b * HW + (j - c * HW)) * p.out_ld + c;
                m[u] = (float)p.out_c[ei];
                if (p.out_u) {
                    const float eu = (float)p.out_u[ei];
                    m[u] = eu + p.cfg_scale * (m[u] - eu);
                }
                if constexpr (lin_reads_x_model<PRED, VALUE>) xm[u] = p.x_model[i];
                if (p.A != 0.f) xb[u] = p.x_base[i];
                if (p.h1) h1[u] = p.h1[i];
                if (p.h2) h2[u] = p.h2[i];
                if constexpr (NOISE == LIN_NOISE_TENSOR) z[u] = q.n.noise[i];
            }
        }
        if constexpr (NOISE == LIN_NOISE_SEEDED) lin_quad_z(q.n, b, j0, z);
#pragma unroll
        for (int u = 0; u < LIN_U; ++u) {
            const unsigned j = j0 + u;
            if (j < N) {
                const size_t i = base + j;
                const float val = lin_value<PRED, VALUE>(p, m[u], xm[u]);
                p.model_out[i] = val;
                if (p.model_pre_out) p.model_pre_out[i] = val;
                p.x_out[i] = __builtin_fmaf(q.n.cn, z[u], lin_form(p, val, xb[u], h1[u], h2[u]));
            }
        }
    }
}

// OWNED, the passes over a sample, U elements of a thread at a time as rescale_apply does it (all loads, then the
// arithmetic and the stores).  Every pass deals element j to thread j % RESCALE_THREADS, with and without noise: a lone
// workgroup lives on coalesced loads (with quads dealt to its threads, four consecutive elements each, the launch measured
// twice the time).  So the seeded instantiations deal the quads of a trip to LANES and the values travel by shuffle: in one
// trip a wave works on LIN_U spans of 64 consecutive elements (64 apart from the sample's start: quad-aligned), 16 quads each,
// 64 in all; lane L draws quad L & 15 of span L >> 4, and the element of span u in lane l takes value l & 3 of lane
// 16 u + l / 4.  Their loops run the same trips in all lanes of a wave (the shuffles need every lane).
template <int NOISE>
__device__ __forceinline__ bool lin_owned_trip(unsigned j0, unsigned N) {
    if constexpr (NOISE == LIN_NOISE_SEEDED)
        return j0 - (threadIdx.x & 63u) < N;
    else
        return j0 < N;
}

// z of the thread's LIN_U elements j0 + u * RESCALE_THREADS of sample b
__device__ __forceinline__ void lin_owned_z(const LinNoise& n, int b, unsigned j0, unsigned N, float (&z)[LIN_U]) {
    const unsigned lane = threadIdx.x & 63u;
    const unsigned start = (j0 - lane) + (lane >> 4) * RESCALE_THREADS + (lane & 15u) * 4u;
    float zq[LIN_U] = {0.f, 0.f, 0.f, 0.f};
    if (start < N) lin_quad_z(n, b, start, zq);
#pragma unroll
    for (int u = 0; u < LIN_U; ++u) {
        const int src = u * 16 + (int)(lane >> 2);
        const float a0 = __shfl(zq[0], src, 64), a1 = __shfl(zq[1], src, 64), a2 = __shfl(zq[2], src, 64),
                    a3 = __shfl(zq[3], src, 64);
        const unsigned e = lane & 3u;
        z[u] = e == 0 ? a0 : e == 1 ? a1 : e == 2 ? a2 : a3;
    }
}

// Steps 1-4 (and, without thresholding, 6, 7 and 8).  PARK: the values wait in model_out for the selection.
template <int PRED, int VALUE, bool PARK, int NOISE>
__device__ __forceinline__ void lin_owned_values(const LinParams& p, const LinNoise& n, float f, int b) {
    const unsigned N = (unsigned)p.C * (unsigned)p.HW, HW = p.HW;
    const f16* oc = p.out_c + (size_t)b * HW * p.out_ld;
    const f16* ou = p.out_u ? p.out_u + (size_t)b * HW * p.out_ld : nullptr;
    const size_t base = (size_t)b * N;
    for (unsigned j0 = threadIdx.x; lin_owned_trip<NOISE>(j0, N); j0 += RESCALE_THREADS * LIN_U) {
        float m[LIN_U], xm[LIN_U], xb[LIN_U], h1[LIN_U], h2[LIN_U], z[LIN_U];
#pragma unroll
        for (int u = 0; u < LIN_U; ++u) {
            const unsigned j = j0 + u * RESCALE_THREADS;
            xm[u] = xb[u] = h1[u] = h2[u] = 0.f;
            if constexpr (NOISE != LIN_NOISE_NONE) z[u] = 0.f;
            if (j < N) {
                const size_t i = base + j;
                const unsigned c = j / HW;
                const size_t ei = (size_t)(j - c * HW) * p.out_ld + c;
                m[u] = (float)oc[ei];
                if (ou) {
                    const float eu = (float)ou[ei];
                    m[u] = eu + p.cfg_scale * (m[u] - eu);
                }
                if constexpr (lin_reads_x_model<PRED, VALUE>) xm[u] = p.x_model[i];
                if constexpr (!PARK) {
                    if (p.A != 0.f) xb[u] = p.x_base[i];
                    if (p.h1) h1[u] = p.h1[i];
                    if (p.h2) h2[u] = p.h2[i];
                    if constexpr (NOISE == LIN_NOISE_TENSOR) z[u] = n.noise[i];
                }
            }
        }
        if constexpr (!PARK && NOISE == LIN_NOISE_SEEDED) lin_owned_z(n, b, j0, N, z);
#pragma unroll
        for (int u = 0; u < LIN_U; ++u) {
            const unsigned j = j0 + u * RESCALE_THREADS;
            if (j < N) {
                const size_t i = base + j;
                const float val = lin_value<PRED, VALUE>(p, m[u] * f, xm[u]);
                p.model_out[i] = val;
                if (p.model_pre_out) p.model_pre_out[i] = val;
                if constexpr (!PARK) {
                    float xo = lin_form(p, val, xb[u], h1[u], h2[u]);
                    if constexpr (NOISE != LIN_NOISE_NONE) xo = __builtin_fmaf(n.cn, z[u], xo);
                    p.x_out[i] = xo;
                }
            }
        }
    }
}

// Step 5's s for the sample whose parked values are vals[0 .. N): the same bits in every thread.  |v| as a bit pattern orders
// as an unsigned integer, so the k-th smallest is found digit by digit, most significant first: a pass counts, per value of
// the digit, the candidates (the values that share the digits found so far), and wave 0 finds the digit in which the running
// count passes the rank.  Counting is exact whatever the values are, so every pass finds exactly one digit and nothing below
// is indexed by data except hist[digit], digit < 256.  Most candidates of the first pass share two or three digits (the high
// exponent bits), so a wave first counts the digit of its first live lane, twice, with one atomic each, and leaves only the
// rest to per-lane atomics.
__device__ __forceinline__ float lin_threshold_s(const LinParams& p, const float* vals, unsigned N, unsigned* hist,
                                                 unsigned* sel) {
    const int lane = threadIdx.x & 63;
    unsigned prefix = 0, rank = p.k, count_eq = 0;
    for (int shift = 24; shift >= 0; shift -= 8) {
        if (threadIdx.x < 256) hist[threadIdx.x] = 0;
        __syncthreads();
        const unsigned himask = shift == 24 ? 0u : 0xffffffffu << (shift + 8);
        for (unsigned j0 = 0; j0 < N; j0 += RESCALE_THREADS) {      // the same trips in every thread: ballots below
            const unsigned j = j0 + threadIdx.x;
            const unsigned bits = j < N ? __float_as_uint(vals[j]) & 0x7fffffffu : 0u;
            bool live = j < N && (bits & himask) == prefix;
            const unsigned digit = (bits >> shift) & 255u;
#pragma unroll
            for (int peel = 0; peel < 2; ++peel) {
                const unsigned long long any = __ballot(live);
                if (any != 0) {
                    const int first = __ffsll((long long)any) - 1;
                    const unsigned d = (unsigned)__shfl((int)digit, first, 64);
                    const unsigned long long same = __ballot(live && digit == d);
                    if (lane == first) atomicAdd(&hist[d], (unsigned)__popcll(same));
                    live = live && digit != d;
                }
            }
            if (live) atomicAdd(&hist[digit], 1u);
        }
        __syncthreads();
        if (threadIdx.x < 64) {
            const unsigned h0 = hist[4 * lane], h1 = hist[4 * lane + 1], h2 = hist[4 * lane + 2], h3 = hist[4 * lane + 3];
            const unsigned sum = h0 + h1 + h2 + h3;
            unsigned inc = sum;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const unsigned t = (unsigned)__shfl_up((int)inc, o, 64);
                if (lane >= o) inc += t;
            }
            const unsigned exc = inc - sum;
            if (exc <= rank && rank < inc) {        // one lane: the candidates number more than the rank
                unsigned r = rank - exc, d = 4 * lane, n = h0;
                if (r >= h0) {
                    r -= h0, d += 1, n = h1;
                    if (r >= h1) {
                        r -= h1, d += 1, n = h2;
                        if (r >= h2) r -= h2, d += 1, n = h3;
                    }
                }
                sel[0] = d;
                sel[1] = r;
                sel[2] = n;
            }
        }
        __syncthreads();
        prefix |= (sel[0] & 255u) << shift;
        rank = sel[1];
        count_eq = sel[2];
    }
    // a = the k-th smallest; (k - rank) values lie below it and count_eq equal it.  b, the (k+1)-th: a again if the values <= a
    // number k + 2 or more, else the smallest value above a (there is one: k + 1 <= N - 1).
    unsigned b_bits = prefix;
    if (p.k - rank + count_eq < p.k + 2) {      // the same in every thread
        unsigned lo = 0xffffffffu;
        for (unsigned j = threadIdx.x; j < N; j += RESCALE_THREADS) {
            const unsigned bits = __float_as_uint(vals[j]) & 0x7fffffffu;
            if (bits > prefix && bits < lo) lo = bits;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned t = (unsigned)__shfl_xor((int)lo, o, 64);
            lo = t < lo ? t : lo;
        }
        if (lane == 0) hist[threadIdx.x >> 6] = lo;     // (hist was last read before the barrier above)
        __syncthreads();
#pragma unroll
        for (int w = 0; w < RESCALE_THREADS / 64; ++w) lo = hist[w] < lo ? hist[w] : lo;
        b_bits = lo;
    }
    const float a = __uint_as_float(prefix), bv = __uint_as_float(b_bits);
    float s;
    {
#pragma clang fp contract(off)
        const float d = bv - a;
        const float t = d * 0.995f;
        s = a + t;
    }
    return fmaxf(s, p.max_val);
}

// Steps 5-8 on the parked values.
template <int NOISE>
__device__ __forceinline__ void lin_owned_finish(const LinParams& p, const LinNoise& n, float s, int b) {
    const unsigned N = (unsigned)p.C * (unsigned)p.HW;
    const size_t base = (size_t)b * N;
    for (unsigned j0 = threadIdx.x; lin_owned_trip<NOISE>(j0, N); j0 += RESCALE_THREADS * LIN_U) {
        float v[LIN_U], xb[LIN_U], h1[LIN_U], h2[LIN_U], z[LIN_U];
#pragma unroll
        for (int u = 0; u < LIN_U; ++u) {
            const unsigned j = j0 + u * RESCALE_THREADS;
            v[u] = xb[u] = h1[u] = h2[u] = 0.f;
            if constexpr (NOISE != LIN_NOISE_NONE) z[u] = 0.f;
            if (j < N) {
                const size_t i = base + j;
                v[u] = p.model_out[i];
                if (p.A != 0.f) xb[u] = p.x_base[i];
                if (p.h1) h1[u] = p.h1[i];
                if (p.h2) h2[u] = p.h2[i];
                if constexpr (NOISE == LIN_NOISE_TENSOR) z[u] = n.noise[i];
            }
        }
        if constexpr (NOISE == LIN_NOISE_SEEDED) lin_owned_z(n, b, j0, N, z);
#pragma unroll
        for (int u = 0; u < LIN_U; ++u) {
            const unsigned j = j0 + u * RESCALE_THREADS;
            if (j < N) {
                const size_t i = base + j;
                const float val = fminf(fmaxf(v[u], -s), s) / s;
                p.model_out[i] = val;
                float xo = lin_form(p, val, xb[u], h1[u], h2[u]);
                if constexpr (NOISE != LIN_NOISE_NONE) xo = __builtin_fmaf(n.cn, z[u], xo);
                p.x_out[i] = xo;
            }
        }
    }
}

// OWNED: one kernel for both entries.  P is LinParams (mdx_sampler_step_lin_f32: NOISE is LIN_NOISE_NONE, the kernel that
// entry has always launched) or LinNoiseParams.
__device__ __forceinline__ const LinParams& lin_of(const LinParams& p) { return p; }
__device__ __forceinline__ const LinParams& lin_of(const LinNoiseParams& q) { return q.l; }
__device__ __forceinline__ LinNoise lin_noise_of(const LinParams&) { return LinNoise{}; }
__device__ __forceinline__ LinNoise lin_noise_of(const LinNoiseParams& q) { return q.n; }

template <int PRED, int VALUE, int NOISE, class P>
__global__ __launch_bounds__(RESCALE_THREADS) void sampler_step_lin_owned_kernel(const P q) {
    mdx_kernarg_touch<sizeof(P)>();
    __shared__ float part[RESCALE_THREADS / 64][4];
    __shared__ unsigned hist[256];
    __shared__ unsigned sel[4];
    const LinParams& p = lin_of(q);
    const LinNoise n = lin_noise_of(q);
    const int b = blockIdx.x;
    float f = 1.f;
    if (p.phi != 0.f) {         // rescale_factor reads these fields only
        StepParams sp{};
        sp.eps_u = p.out_u;
        sp.eps_c = p.out_c;
        sp.eps_ld = p.out_ld;
        sp.C = p.C;
        sp.HW = p.HW;
        sp.cfg_scale = p.cfg_scale;
        f = rescale_factor(sp, p.phi, b, part);
    }
    if (p.factor_out && threadIdx.x == 0) p.factor_out[b] = f;
    if constexpr (VALUE == MDX_VALUE_X0) {
        if (p.thresholding) {
            lin_owned_values<PRED, VALUE, true, NOISE>(p, n, f, b);
            __syncthreads();        // (a thread reads back only what it parked itself; the barrier is for sel / hist)
            const unsigned N = (unsigned)p.C * (unsigned)p.HW;
            const float s = lin_threshold_s(p, p.model_out + (size_t)b * N, N, hist, sel);
            if (p.thr_out && threadIdx.x == 0) p.thr_out[b] = s;
            lin_owned_finish<NOISE>(p, n, s, b);
            return;
        }
    }
    lin_owned_values<PRED, VALUE, false, NOISE>(p, n, f, b);
}

// ------------------------------------------------------------------ per-slot row gather (mdx_slot_gather_f32)
// dst[r * B + b][:] = src[b][pos_b][:] for the active slots: gridDim.x workgroups share slot blockIdx.y.  V == 4 moves 16 bytes
// per lane (n % 4 == 0 and both bases 16-byte aligned: the host decides), V == 1 one float.
constexpr int SLOT_GATHER_THREADS = 256;

template <int V>
__global__ __launch_bounds__(SLOT_GATHER_THREADS) void slot_gather_kernel(const float* __restrict__ src,
                                                                           const int* __restrict__ slot_start,
                                                                           const int* __restrict__ slot_len, int cap, int tick,
                                                                           float* __restrict__ dst, int B, size_t n, int reps) {
    const int b = blockIdx.y;
    const int pos = mdx_slot_pos(slot_start, slot_len, b, cap, tick);
    if (pos < 0) return;
    const float* row = src + ((size_t)b * cap + pos) * n;
    const size_t items = n / V, stride = (size_t)gridDim.x * SLOT_GATHER_THREADS;
    for (size_t j = (size_t)blockIdx.x * SLOT_GATHER_THREADS + threadIdx.x; j < items; j += stride) {
        if constexpr (V == 4) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(row + j * 4);
            for (int r = 0; r < reps; ++r) *reinterpret_cast<f32x4*>(dst + ((size_t)r * B + b) * n + j * 4) = v;
        } else {
            const float v = row[j];
            for (int r = 0; r < reps; ++r) dst[((size_t)r * B + b) * n + j] = v;
        }
    }
}

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

inline int grid_for(size_t total) {
    size_t b = (total + 255) / 256;
    return (int)(b > 2048 ? 2048 : (b < 1 ? 1 : b));
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

// One host body for all entries; `fn` names the entry in its messages.  sampler_step_params refuses and fills,
// sampler_step_run launches sampler_step_kernel on filled parameters, sampler_step_launch does both.
static int sampler_step_params(StepParams& p, const char* fn, const float* x, const float* x_model, const void* out_u,
                               const void* out_c, int out_ld, float cfg_scale, int pred_type, float am, float bm,
                               const float* old1, const float* old2, const float* old3, const float* coef4, float sqrt_at,
                               float sqrt_one_minus_at, float sqrt_a_prev, float dir_coef, float sigma,
                               const float* noise, float* e_t_out, float* x_prev, float* pred_x0, int B, int C, int H,
                               int W) {
    MDX_REQUIRE(pred_type == MDX_PRED_EPS || pred_type == MDX_PRED_V, "%s: unknown pred_type %d", fn, pred_type);
    MDX_REQUIRE(x && out_c && coef4 && x_prev, "%s: null pointer", fn);
    MDX_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0 && out_ld >= C, "%s: bad extents", fn);
    MDX_REQUIRE(sigma == 0.f || noise, "%s: sigma != 0 needs a noise tensor", fn);
    MDX_REQUIRE((coef4[1] == 0.f || old1) && (coef4[2] == 0.f || old2) && (coef4[3] == 0.f || old3),
                "%s: non-zero multistep coefficient without its eps history", fn);
    p = StepParams{};
    p.x = x;
    p.x_model = x_model ? x_model : x;
    p.eps_u = (const f16*)out_u;
    p.eps_c = (const f16*)out_c;
    p.old1 = coef4[1] != 0.f ? old1 : nullptr;
    p.old2 = coef4[2] != 0.f ? old2 : nullptr;
    p.old3 = coef4[3] != 0.f ? old3 : nullptr;
    p.noise = sigma != 0.f ? noise : nullptr;
    p.e_t_out = e_t_out;
    p.x_prev = x_prev;
    p.pred_x0 = pred_x0;
    p.eps_ld = out_ld;
    p.B = B;
    p.C = C;
    p.HW = H * W;
    p.cfg_scale = cfg_scale;
    p.c0 = coef4[0];
    p.c1 = coef4[1];
    p.c2 = coef4[2];
    p.c3 = coef4[3];
    p.sqrt_at = sqrt_at;
    p.sqrt_one_minus_at = sqrt_one_minus_at;
    p.sqrt_a_prev = sqrt_a_prev;
    p.dir_coef = dir_coef;
    p.sigma = sigma;
    p.am = am;
    p.bm = bm;
    return MDX_OK;
}

static int sampler_step_run(const char* fn, const StepParams& p, int pred_type, mdx_stream_t s) {
    const dim3 grid(grid_for((size_t)p.B * p.C * p.HW));
    if (pred_type == MDX_PRED_V)
        hipLaunchKernelGGL(sampler_step_kernel<MDX_PRED_V>, grid, dim3(256), 0, (hipStream_t)s, p);
    else
        hipLaunchKernelGGL(sampler_step_kernel<MDX_PRED_EPS>, grid, dim3(256), 0, (hipStream_t)s, p);
    MDX_LAUNCH_CHECK(fn);
    return MDX_OK;
}

static int sampler_step_launch(const char* fn, const float* x, const float* x_model, const void* out_u, const void* out_c,
                               int out_ld, float cfg_scale, int pred_type, float am, float bm, const float* old1,
                               const float* old2, const float* old3, const float* coef4, float sqrt_at,
                               float sqrt_one_minus_at, float sqrt_a_prev, float dir_coef, float sigma,
                               const float* noise, float* e_t_out, float* x_prev, float* pred_x0, int B, int C, int H,
                               int W, mdx_stream_t s) {
    StepParams p;
    const int rc = sampler_step_params(p, fn, x, x_model, out_u, out_c, out_ld, cfg_scale, pred_type, am, bm, old1, old2,
                                       old3, coef4, sqrt_at, sqrt_one_minus_at, sqrt_a_prev, dir_coef, sigma, noise,
                                       e_t_out, x_prev, pred_x0, B, C, H, W);
    if (rc != MDX_OK) return rc;
    return sampler_step_run(fn, p, pred_type, s);
}

extern "C" int mdx_sampler_step_f32(const float* x, const void* eps_u, const void* eps_c, int eps_ld, float cfg_scale,
                                    const float* old1, const float* old2, const float* old3, const float* coef4,
                                    float sqrt_at, float sqrt_one_minus_at, float sqrt_a_prev, float dir_coef,
                                    float sigma, const float* noise, float* e_t_out, float* x_prev, float* pred_x0,
                                    int B, int C, int H, int W, mdx_stream_t s) {
    return sampler_step_launch("mdx_sampler_step_f32", x, nullptr, eps_u, eps_c, eps_ld, cfg_scale, MDX_PRED_EPS, 1.f, 0.f,
                               old1, old2, old3, coef4, sqrt_at, sqrt_one_minus_at, sqrt_a_prev, dir_coef, sigma, noise,
                               e_t_out, x_prev, pred_x0, B, C, H, W, s);
}

extern "C" int mdx_sampler_step_pred_f32(const float* x, const float* x_model, const void* out_u, const void* out_c,
                                         int out_ld, float cfg_scale, int pred_type, float sqrt_at_model,
                                         float sqrt_one_minus_at_model, const float* old1, const float* old2,
                                         const float* old3, const float* coef4, float sqrt_at, float sqrt_one_minus_at,
                                         float sqrt_a_prev, float dir_coef, float sigma, const float* noise,
                                         float* e_t_out, float* x_prev, float* pred_x0, int B, int C, int H, int W,
                                         mdx_stream_t s) {
    return sampler_step_launch("mdx_sampler_step_pred_f32", x, x_model, out_u, out_c, out_ld, cfg_scale, pred_type,
                               sqrt_at_model, sqrt_one_minus_at_model, old1, old2, old3, coef4, sqrt_at,
                               sqrt_one_minus_at, sqrt_a_prev, dir_coef, sigma, noise, e_t_out, x_prev, pred_x0, B, C, H, W,
                               s);
}

extern "C" int mdx_sampler_step_rescale_f32(const float* x, const float* x_model, const void* out_u, const void* out_c,
                                            int out_ld, float cfg_scale, int pred_type, float sqrt_at_model,
                                            float sqrt_one_minus_at_model, const float* old1, const float* old2,
                                            const float* old3, const float* coef4, float sqrt_at, float sqrt_one_minus_at,
                                            float sqrt_a_prev, float dir_coef, float sigma, const float* noise,
                                            float* e_t_out, float* x_prev, float* pred_x0, float guidance_rescale,
                                            float* factor_out, int B, int C, int H, int W, mdx_stream_t s) {
    const char* fn = "mdx_sampler_step_rescale_f32";
    RescaleParams rp;
    const int rc = sampler_step_params(rp.s, fn, x, x_model, out_u, out_c, out_ld, cfg_scale, pred_type, sqrt_at_model,
                                       sqrt_one_minus_at_model, old1, old2, old3, coef4, sqrt_at, sqrt_one_minus_at,
                                       sqrt_a_prev, dir_coef, sigma, noise, e_t_out, x_prev, pred_x0, B, C, H, W);
    if (rc != MDX_OK) return rc;
    MDX_REQUIRE(guidance_rescale >= 0.f && guidance_rescale <= 1.f, "%s: guidance_rescale %g is not in [0, 1]", fn,
                (double)guidance_rescale);
    MDX_REQUIRE((size_t)C * H * W >= 2, "%s: the per-sample std needs C * H * W >= 2", fn);
    MDX_REQUIRE((size_t)C * H * W <= 0x7fffffffu, "%s: bad extents (C * H * W of one sample exceeds 31 bits)", fn);
    if (guidance_rescale == 0.f || !out_u) {      // f == 1: the launch of mdx_sampler_step_pred_f32, bit for bit
        const int rc1 = sampler_step_run(fn, rp.s, pred_type, s);
        if (rc1 != MDX_OK || !factor_out) return rc1;
        const hipError_t e = hipMemsetD32Async((hipDeviceptr_t)factor_out, 0x3f800000 /* 1.0f */, (size_t)B, (hipStream_t)s);
        if (e != hipSuccess) {
            mdx_set_error("%s: factor_out fill failed: %s", fn, hipGetErrorString(e));
            return MDX_E_HIP;
        }
        return MDX_OK;
    }
    rp.phi = guidance_rescale;
    rp.factor_out = factor_out;
    if (pred_type == MDX_PRED_V)
        hipLaunchKernelGGL(sampler_step_rescale_kernel<MDX_PRED_V>, dim3(B), dim3(RESCALE_THREADS), 0, (hipStream_t)s, rp);
    else
        hipLaunchKernelGGL(sampler_step_rescale_kernel<MDX_PRED_EPS>, dim3(B), dim3(RESCALE_THREADS), 0, (hipStream_t)s, rp);
    MDX_LAUNCH_CHECK(fn);
    return MDX_OK;
}

// What the table entry and the slot entry refuse and fill alike: the pointer and extent checks of the scalar entries on
// coefficients that need none (they live on the device), the limits of the two launch forms, and the history / noise
// pointers as given -- table_row keeps or drops them by the row's coefficient.
static int step_rows_params(StepParams& p, const char* fn, const float* x, const float* x_model, const void* out_u,
                            const void* out_c, int out_ld, int pred_type, const float* old1, const float* old2,
                            const float* old3, const float* noise, float* e_t_out, float* x_prev, float* pred_x0,
                            int any_rescale, int B, int C, int H, int W) {
    const float no_history[4] = {1.f, 0.f, 0.f, 0.f};
    const int rc = sampler_step_params(p, fn, x, x_model, out_u, out_c, out_ld, 1.f, pred_type, 1.f, 0.f, old1, old2, old3,
                                       no_history, 1.f, 0.f, 1.f, 0.f, 0.f, noise, e_t_out, x_prev, pred_x0, B, C, H, W);
    if (rc != MDX_OK) return rc;
    MDX_REQUIRE(!any_rescale || out_u, "%s: any_rescale needs the unconditional output out_u", fn);
    MDX_REQUIRE(!any_rescale || (size_t)C * H * W >= 2, "%s: the per-sample std needs C * H * W >= 2", fn);
    MDX_REQUIRE((size_t)C * H * W <= 0x7fffffffu, "%s: bad extents (C * H * W of one sample exceeds 31 bits)", fn);
    MDX_REQUIRE(any_rescale || B <= 65535, "%s: bad extents (B exceeds 65535 samples)", fn);
    p.old1 = old1;
    p.old2 = old2;
    p.old3 = old3;
    p.noise = noise;
    return MDX_OK;
}

// the workgroups of sampler_step_kernel's grid for the same batch, dealt to the samples
static dim3 step_rows_spread_grid(int B, int C, int H, int W) {
    return dim3((grid_for((size_t)B * C * H * W) + B - 1) / B, B);
}

extern "C" int mdx_sampler_step_table_f32(const float* x, const float* x_model, const void* out_u, const void* out_c,
                                          int out_ld, int pred_type, const float* old1, const float* old2,
                                          const float* old3, const float* noise, float* e_t_out, float* x_prev,
                                          float* pred_x0, const float* table, int any_rescale, float* factor_out, int B,
                                          int C, int H, int W, mdx_stream_t s) {
    const char* fn = "mdx_sampler_step_table_f32";
    TableParams tp;
    const int rc = step_rows_params(tp.s, fn, x, x_model, out_u, out_c, out_ld, pred_type, old1, old2, old3, noise, e_t_out,
                                    x_prev, pred_x0, any_rescale, B, C, H, W);
    if (rc != MDX_OK) return rc;
    MDX_REQUIRE(table, "%s: null table", fn);
    tp.table = table;
    tp.factor_out = factor_out;
    const hipStream_t st = (hipStream_t)s;
    if (any_rescale) {
        if (pred_type == MDX_PRED_V)
            hipLaunchKernelGGL(sampler_step_table_rescale_kernel<MDX_PRED_V>, dim3(B), dim3(RESCALE_THREADS), 0, st, tp);
        else
            hipLaunchKernelGGL(sampler_step_table_rescale_kernel<MDX_PRED_EPS>, dim3(B), dim3(RESCALE_THREADS), 0, st, tp);
    } else {
        const dim3 grid = step_rows_spread_grid(B, C, H, W);
        if (pred_type == MDX_PRED_V)
            hipLaunchKernelGGL(sampler_step_table_kernel<MDX_PRED_V>, grid, dim3(256), 0, st, tp);
        else
            hipLaunchKernelGGL(sampler_step_table_kernel<MDX_PRED_EPS>, grid, dim3(256), 0, st, tp);
    }
    MDX_LAUNCH_CHECK(fn);
    return MDX_OK;
}

extern "C" int mdx_sampler_step_slots_f32(const float* x, const float* x_model, const void* out_u, const void* out_c,
                                          int out_ld, int pred_type, const float* old1, const float* old2,
                                          const float* old3, const float* noise, float* e_t_out, float* x_prev,
                                          float* pred_x0, const float* sched, const int* slot_start, const int* slot_len,
                                          int cap, int tick, int any_rescale, float* factor_out, int B, int C, int H, int W,
                                          mdx_stream_t s) {
    const char* fn = "mdx_sampler_step_slots_f32";
    SlotParams sp;
    const int rc = step_rows_params(sp.s, fn, x, x_model, out_u, out_c, out_ld, pred_type, old1, old2, old3, noise, e_t_out,
                                    x_prev, pred_x0, any_rescale, B, C, H, W);
    if (rc != MDX_OK) return rc;
    MDX_REQUIRE(sched && slot_start && slot_len, "%s: null slot pointer", fn);
    MDX_REQUIRE(cap > 0 && tick >= 0, "%s: bad slot extents (cap=%d tick=%d; cap > 0, tick >= 0)", fn, cap, tick);
    sp.sched = sched;
    sp.slot_start = slot_start;
    sp.slot_len = slot_len;
    sp.cap = cap;
    sp.tick = tick;
    sp.factor_out = factor_out;
    const hipStream_t st = (hipStream_t)s;
    if (any_rescale) {
        if (pred_type == MDX_PRED_V)
            hipLaunchKernelGGL(sampler_step_slots_rescale_kernel<MDX_PRED_V>, dim3(B), dim3(RESCALE_THREADS), 0, st, sp);
        else
            hipLaunchKernelGGL(sampler_step_slots_rescale_kernel<MDX_PRED_EPS>, dim3(B), dim3(RESCALE_THREADS), 0, st, sp);
    } else {
        const dim3 grid = step_rows_spread_grid(B, C, H, W);
        if (pred_type == MDX_PRED_V)
            hipLaunchKernelGGL(sampler_step_slots_kernel<MDX_PRED_V>, grid, dim3(256), 0, st, sp);
        else
            hipLaunchKernelGGL(sampler_step_slots_kernel<MDX_PRED_EPS>, grid, dim3(256), 0, st, sp);
    }
    MDX_LAUNCH_CHECK(fn);
    return MDX_OK;
}

extern "C" int mdx_slot_gather_f32(const float* src, const int* slot_start, const int* slot_len, int cap, int tick, float* dst,
                                   int B, long n, int reps, mdx_stream_t s) {
    const char* fn = "mdx_slot_gather_f32";
    MDX_REQUIRE(src && slot_start && slot_len && dst, "%s: null pointer", fn);
    MDX_REQUIRE(B > 0 && B <= 65535 && n > 0 && reps > 0, "%s: bad extents (B=%d n=%ld reps=%d)", fn, B, n, reps);
    MDX_REQUIRE(cap > 0 && tick >= 0, "%s: bad slot extents (cap=%d tick=%d; cap > 0, tick >= 0)", fn, cap, tick);
    const bool vec = n % 4 == 0 && (((uintptr_t)src | (uintptr_t)dst) & 15) == 0;
    const size_t items = vec ? (size_t)n / 4 : (size_t)n;
    size_t per_slot = (items + SLOT_GATHER_THREADS - 1) / SLOT_GATHER_THREADS;
    if (per_slot > 64) per_slot = 64;       // a row is a few tens of KB: further trips of the grid-stride loop beyond that
    const dim3 grid((unsigned)per_slot, B);
    if (vec)
        hipLaunchKernelGGL(slot_gather_kernel<4>, grid, dim3(SLOT_GATHER_THREADS), 0, (hipStream_t)s, src, slot_start, slot_len,
                           cap, tick, dst, B, (size_t)n, reps);
    else
        hipLaunchKernelGGL(slot_gather_kernel<1>, grid, dim3(SLOT_GATHER_THREADS), 0, (hipStream_t)s, src, slot_start, slot_len,
                           cap, tick, dst, B, (size_t)n, reps);
    MDX_LAUNCH_CHECK(fn);
    return MDX_OK;
}

// ---- mdx_sampler_step_lin_f32
static bool bytes_overlap(const void* a, size_t na, const void* b, size_t nb) {
    if (!a || !b || na == 0 || nb == 0) return false;
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

template <int PRED, int VALUE, int NOISE>
static void sampler_step_lin_noise_run(const LinNoiseParams& q, bool owned, hipStream_t st) {
    if (owned) {
        hipLaunchKernelGGL((sampler_step_lin_owned_kernel<PRED, VALUE, NOISE, LinNoiseParams>), dim3(q.l.B), dim3(RESCALE_THREADS), 0, st, q);
    } else {
        const size_t items = (size_t)q.l.B * (((size_t)q.l.C * q.l.HW + 3) / 4);
        const size_t blocks = (items + LIN_NOISE_THREADS - 1) / LIN_NOISE_THREADS;
        hipLaunchKernelGGL((sampler_step_lin_noise_kernel<PRED, VALUE, NOISE>), dim3((unsigned)(blocks > 8192 ? 8192 : blocks)),
                           dim3(LIN_NOISE_THREADS), 0, st, q);
    }
}

template <int PRED, int VALUE>
static void sampler_step_lin_run(const LinParams& p, const LinNoise* nz, bool owned, hipStream_t st) {
    if (nz) {
        const LinNoiseParams q{p, *nz};
        if (nz->seeds)
            sampler_step_lin_noise_run<PRED, VALUE, LIN_NOISE_SEEDED>(q, owned, st);
        else
            sampler_step_lin_noise_run<PRED, VALUE, LIN_NOISE_TENSOR>(q, owned, st);
    } else if (owned)
        hipLaunchKernelGGL((sampler_step_lin_owned_kernel<PRED, VALUE, LIN_NOISE_NONE, LinParams>), dim3(p.B), dim3(RESCALE_THREADS), 0, st, p);
    else
        hipLaunchKernelGGL((sampler_step_lin_kernel<PRED, VALUE>), dim3(grid_for((size_t)p.B * p.C * p.HW)), dim3(256), 0, st, p);
}

// Both entries: nz == nullptr is mdx_sampler_step_lin_f32's launch, kernel for kernel (the noise entry passes it for cn == 0).
static int sampler_step_lin_entry(const char* fn, const float* x_base, const float* x_model, const void* out_u,
                                  const void* out_c, int out_ld, float cfg_scale, int pred_type, float guidance_rescale,
                                  int value_type, float alpha_m, float sigma_m, int thresholding, float max_val, const float* h1,
                                  const float* h2, float A, float c0, float c1, float c2, float* model_out, float* x_out,
                                  float* model_pre_out, float* thr_out, float* factor_out, const LinNoise* nz, int B, int C,
                                  int H, int W, mdx_stream_t s) {
    MDX_REQUIRE(pred_type == MDX_PRED_EPS || pred_type == MDX_PRED_V, "%s: unknown pred_type %d", fn, pred_type);
    MDX_REQUIRE(value_type == MDX_VALUE_X0 || value_type == MDX_VALUE_EPS, "%s: unknown value_type %d", fn, value_type);
    MDX_REQUIRE(x_base && x_model && out_c && model_out && x_out, "%s: null pointer", fn);
    MDX_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0 && out_ld >= C, "%s: bad extents", fn);
    const size_t N = (size_t)C * H * W;
    MDX_REQUIRE(N <= 0x7fffffffu, "%s: bad extents (C * H * W of one sample exceeds 31 bits)", fn);
    MDX_REQUIRE((c1 == 0.f || h1) && (c2 == 0.f || h2), "%s: non-zero history coefficient without its model value", fn);
    MDX_REQUIRE(value_type != MDX_VALUE_X0 || alpha_m != 0.f, "%s: alpha_m == 0 (the data prediction divides by it)", fn);
    MDX_REQUIRE(guidance_rescale >= 0.f && guidance_rescale <= 1.f, "%s: guidance_rescale %g is not in [0, 1]", fn,
                (double)guidance_rescale);
    const bool rescale = guidance_rescale != 0.f && out_u;
    MDX_REQUIRE(!rescale || N >= 2, "%s: the per-sample std needs C * H * W >= 2", fn);
    if (thresholding) {
        MDX_REQUIRE(value_type == MDX_VALUE_X0, "%s: thresholding acts on a data prediction (MDX_VALUE_X0)", fn);
        MDX_REQUIRE(N >= 2, "%s: thresholding needs two order statistics, C * H * W >= 2", fn);
        MDX_REQUIRE(max_val > 0.f && max_val <= 3.402823466e38f, "%s: max_val %g is not a finite positive number", fn,
                    (double)max_val);
    }
    // the only aliases: x_out == x_base, x_out == x_model.  An input whose term is skipped is not read and may lie anywhere.
    const size_t nx = (size_t)B * N * sizeof(float), nh = (((size_t)B * H * W - 1) * out_ld + C) * sizeof(f16);
    const struct { const void* ptr; size_t bytes; const char* name; } outs[] = {
        {model_out, nx, "model_out"}, {x_out, nx, "x_out"}, {model_pre_out, nx, "model_pre_out"},
        {thr_out, B * sizeof(float), "thr_out"}, {factor_out, B * sizeof(float), "factor_out"}},
      ins[] = {{A != 0.f ? x_base : nullptr, nx, "x_base"}, {x_model, nx, "x_model"}, {out_u, nh, "out_u"}, {out_c, nh, "out_c"},
               {c1 != 0.f ? h1 : nullptr, nx, "h1"}, {c2 != 0.f ? h2 : nullptr, nx, "h2"},
               {nz ? nz->noise : nullptr, nx, "noise"}, {nz ? nz->seeds : nullptr, B * sizeof(unsigned long long), "seeds"}};
    for (size_t o = 0; o < sizeof(outs) / sizeof(outs[0]); ++o) {
        for (size_t i = 0; i < sizeof(ins) / sizeof(ins[0]); ++i) {
            const bool allowed = o == 1 && i < 2 && outs[o].ptr == ins[i].ptr;
            MDX_REQUIRE(allowed || !bytes_overlap(outs[o].ptr, outs[o].bytes, ins[i].ptr, ins[i].bytes),
                        "%s: %s overlaps %s (only x_out may alias x_base / x_model, element for element)", fn, outs[o].name,
                        ins[i].name);
        }
        for (size_t q = o + 1; q < sizeof(outs) / sizeof(outs[0]); ++q)
            MDX_REQUIRE(!bytes_overlap(outs[o].ptr, outs[o].bytes, outs[q].ptr, outs[q].bytes), "%s: %s overlaps %s", fn,
                        outs[o].name, outs[q].name);
    }
    LinParams p{};
    p.x_base = x_base;
    p.x_model = x_model;
    p.out_u = (const f16*)out_u;
    p.out_c = (const f16*)out_c;
    p.h1 = c1 != 0.f ? h1 : nullptr;
    p.h2 = c2 != 0.f ? h2 : nullptr;
    p.model_out = model_out;
    p.x_out = x_out;
    p.model_pre_out = model_pre_out;
    p.thr_out = thr_out;
    p.factor_out = factor_out;
    p.out_ld = out_ld;
    p.B = B;
    p.C = C;
    p.HW = H * W;
    p.cfg_scale = cfg_scale;
    p.am = alpha_m;
    p.sm = sigma_m;
    p.A = A;
    p.c0 = c0;
    p.c1 = c1;
    p.c2 = c2;
    p.phi = rescale ? guidance_rescale : 0.f;
    p.max_val = max_val;
    p.k = (unsigned)((double)(N - 1) * 0.995);
    p.thresholding = thresholding != 0;
    const bool owned = rescale || p.thresholding;
    hipStream_t st = (hipStream_t)s;
    if (pred_type == MDX_PRED_V && value_type == MDX_VALUE_X0)
        sampler_step_lin_run<MDX_PRED_V, MDX_VALUE_X0>(p, nz, owned, st);
    else if (pred_type == MDX_PRED_V)
        sampler_step_lin_run<MDX_PRED_V, MDX_VALUE_EPS>(p, nz, owned, st);
    else if (value_type == MDX_VALUE_X0)
        sampler_step_lin_run<MDX_PRED_EPS, MDX_VALUE_X0>(p, nz, owned, st);
    else
        sampler_step_lin_run<MDX_PRED_EPS, MDX_VALUE_EPS>(p, nz, owned, st);
    MDX_LAUNCH_CHECK(fn);
    if (!owned && factor_out) {      // f == 1 everywhere, as mdx_sampler_step_rescale_f32 reports it
        const hipError_t e = hipMemsetD32Async((hipDeviceptr_t)factor_out, 0x3f800000 /* 1.0f */, (size_t)B, st);
        if (e != hipSuccess) {
            mdx_set_error("%s: factor_out fill failed: %s", fn, hipGetErrorString(e));
            return MDX_E_HIP;
        }
    }
    return MDX_OK;
}

extern "C" int mdx_sampler_step_lin_f32(const float* x_base, const float* x_model, const void* out_u, const void* out_c,
                                        int out_ld, float cfg_scale, int pred_type, float guidance_rescale, int value_type,
                                        float alpha_m, float sigma_m, int thresholding, float max_val, const float* h1,
                                        const float* h2, float A, float c0, float c1, float c2, float* model_out,
                                        float* x_out, float* model_pre_out, float* thr_out, float* factor_out, int B, int C,
                                        int H, int W, mdx_stream_t s) {
    return sampler_step_lin_entry("mdx_sampler_step_lin_f32", x_base, x_model, out_u, out_c, out_ld, cfg_scale, pred_type,
                                  guidance_rescale, value_type, alpha_m, sigma_m, thresholding, max_val, h1, h2, A, c0, c1, c2,
                                  model_out, x_out, model_pre_out, thr_out, factor_out, nullptr, B, C, H, W, s);
}

extern "C" int mdx_sampler_step_lin_noise_f32(const float* x_base, const float* x_model, const void* out_u, const void* out_c,
                                              int out_ld, float cfg_scale, int pred_type, float guidance_rescale,
                                              int value_type, float alpha_m, float sigma_m, int thresholding, float max_val,
                                              const float* h1, const float* h2, float A, float c0, float c1, float c2,
                                              float* model_out, float* x_out, float* model_pre_out, float* thr_out,
                                              float* factor_out, float cn, const float* noise, const unsigned long long* seeds,
                                              unsigned stream, unsigned draw, int B, int C, int H, int W, mdx_stream_t s) {
    const char* fn = "mdx_sampler_step_lin_noise_f32";
    MDX_REQUIRE(cn >= -3.402823466e38f && cn <= 3.402823466e38f, "%s: cn %g is not finite", fn, (double)cn);
    MDX_REQUIRE(stream < DROPOUT_STREAM_BIT, "%s: stream %u is not below 2^31", fn, stream);
    MDX_REQUIRE(cn == 0.f || ((noise != nullptr) != (seeds != nullptr)),
                "%s: cn != 0 takes exactly one noise source, noise or seeds (got %s)", fn, noise ? "both" : "neither");
    const LinNoise nz{cn, noise, noise ? nullptr : seeds, stream, draw};
    return sampler_step_lin_entry(fn, x_base, x_model, out_u, out_c, out_ld, cfg_scale, pred_type, guidance_rescale, value_type,
                                  alpha_m, sigma_m, thresholding, max_val, h1, h2, A, c0, c1, c2, model_out, x_out,
                                  model_pre_out, thr_out, factor_out, cn != 0.f ? &nz : nullptr, B, C, H, W, s);
}

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
