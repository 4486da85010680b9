// The fused sampler step family and its session helpers: the eps/PLMS step (scalar, guidance-rescale, table and slot
// entries), the DPM-Solver linear step (with and without noise), the UniPC step (corrector and next predictor), and the
// per-slot row gather.
//
// The family's promise is that every launch form gives the same bits where the forms overlap: the scalar entry, a table row,
// a slot row, a phi == 0 row of a rescaling launch, cn == 0 of the noise entry, seeded and tensor noise.  THE SOURCE FIXES THE
// ROUNDING: the arithmetic of an element is written once per family (cfg_combine, step_arith, lin_value, lin_x_out), compiled
// under `#pragma clang fp contract(off)`, with __builtin_fmaf exactly where a product is fused into a sum.  Every kernel calls
// these bodies on operands it has loaded, so the forms agree by construction and not by the compiler's choice of contraction.
#include "mdx_common.h"
#include "rng_device.h"

namespace {

// ------------------------------------------------------------------ the guided pair
// The two halves of the model output (NHWC fp16, out_u == nullptr: no guidance) and what it takes to combine them.
struct GuidedPair {
    const f16* out_u;
    const f16* out_c;
    int ld, C, HW;
    float cfg_scale;
};

// u + s (c - u): the difference rounded, the product fused into the sum
__device__ __forceinline__ float cfg_combine(float u, float c, float s) {
#pragma clang fp contract(off)
    return __builtin_fmaf(s, c - u, u);
}

// The middle branch of three-branch guidance (InstructPix2Pix: [uu ; ui ; ci] = out_u, out_m, out_c), a compile-time matter:
// a kernel takes a GuidedMid only in its DUAL instantiation, whose parameter struct carries it behind the two-branch one, so a
// two-branch launch has the kernarg and the code it has always had.  out_m has out_u's layout; the host refuses it without out_u.
struct NoMid {
    static constexpr bool dual = false;
};
struct GuidedMid {
    static constexpr bool dual = true;
    const f16* out_m;
    float mid_scale;
};
__device__ __forceinline__ NoMid mid_at(const NoMid&, size_t) { return NoMid{}; }
__device__ __forceinline__ GuidedMid mid_at(const GuidedMid& m, size_t off) { return GuidedMid{m.out_m + off, m.mid_scale}; }

// u + s_i (m - u) + s_t (c - m): both differences rounded, both products fused.  m == u gives cfg_combine(u, c, s_t) and
// m == c gives cfg_combine(u, c, s_i), to the bit (a difference of exactly 0 adds exactly 0).
__device__ __forceinline__ float cfg_combine3(float u, float m, float c, float s_i, float s_t) {
#pragma clang fp contract(off)
    return __builtin_fmaf(s_t, c - m, __builtin_fmaf(s_i, m - u, u));
}

// the combined model output of one element; GUIDED: ou is known to be there (always so with a middle branch)
template <bool GUIDED, class M>
__device__ __forceinline__ float guided_value(const M& mid, const f16* ou, const f16* oc, size_t ei, float cfg_scale) {
    if constexpr (M::dual) {
        return cfg_combine3((float)ou[ei], (float)mid.out_m[ei], (float)oc[ei], mid.mid_scale, cfg_scale);
    } else {
        float m = (float)oc[ei];
        if (GUIDED || ou) m = cfg_combine((float)ou[ei], m, cfg_scale);
        return m;
    }
}

// ------------------------------------------------------------------ fused sampler update (plms.py:188-244)
struct StepParams {
    GuidedPair g;
    const float* x;
    const float* old1;
    const float* old2;
    const float* old3;
    const float* noise;
    float* e_t_out;
    float* x_prev;
    float* pred_x0;
    int B;
    float c0, c1, c2, c3;
    float sqrt_at, sqrt_one_minus_at, sqrt_a_prev, dir_coef, sigma;
    // MDX_PRED_V only: the latent the model was evaluated on, sqrt(alphas_cumprod) and sqrt(1 - alphas_cumprod) there
    const float* x_model;
    float am, bm;
};

// the DUAL instantiations' parameters
struct StepDualParams {
    StepParams s;
    GuidedMid mid;
};

// The loaded operands of one element (a skipped term's operand stays 0 and is not used) and what the step makes of them.
struct StepOperands {
    float m, x_model, x, old1, old2, old3, noise;
};
struct StepResult {
    float e_t, pred_x0, x_prev;
};

// PRED: MDX_PRED_EPS | MDX_PRED_V.  The update of ONE element: m is the CFG-combined (and rescaled) model output.
template <int PRED>
__device__ __forceinline__ StepResult step_arith(const StepParams& p, const StepOperands& v) {
#pragma clang fp contract(off)
    StepResult r;
    r.e_t = v.m;
    if constexpr (PRED == MDX_PRED_V) r.e_t = __builtin_fmaf(p.am, v.m, p.bm * v.x_model);   // eps = a v + b x_m (dpm_solver.py:281-284)
    float ep = p.c0 * r.e_t;
    if (p.old1) ep = __builtin_fmaf(p.c1, v.old1, ep);
    if (p.old2) ep = __builtin_fmaf(p.c2, v.old2, ep);
    if (p.old3) ep = __builtin_fmaf(p.c3, v.old3, ep);
    r.pred_x0 = __builtin_fmaf(-p.sqrt_one_minus_at, ep, v.x) / p.sqrt_at;
    r.x_prev = p.sqrt_a_prev * r.pred_x0 + p.dir_coef * ep;      // both products rounded
    if (p.noise) r.x_prev = __builtin_fmaf(p.sigma, v.noise, r.x_prev);
    return r;
}

// No __restrict__ anywhere below: x_prev may alias x, and for MDX_PRED_V also x_model (the second call of the PLMS first step
// writes the latent its model output was computed on).  The outputs may alias no other input, and only element for element,
// so a thread loads all operands of its elements before it stores any of them.
// ou / oc: the pair's halves from wherever the caller counts ei (the batch's start or the sample's).  GUIDED: ou is known to
// be there (a rescaling launch: the host refuses it without) -- the load then hangs on no test of the pointer, which between
// the loads of a batch would cost a memory round trip each.
// mid: the middle branch from where ou / oc start (NoMid: none).
template <int PRED, bool GUIDED, class M>
__device__ __forceinline__ StepOperands step_load(const StepParams& p, const M& mid, const f16* ou, const f16* oc, size_t ei,
                                                  size_t i) {
    StepOperands v{};
    v.m = guided_value<GUIDED>(mid, ou, oc, ei, p.g.cfg_scale);
    if constexpr (PRED == MDX_PRED_V) v.x_model = p.x_model[i];
    v.x = p.x[i];
    if (p.old1) v.old1 = p.old1[i];
    if (p.old2) v.old2 = p.old2[i];
    if (p.old3) v.old3 = p.old3[i];
    if (p.noise) v.noise = p.noise[i];
    return v;
}

__device__ __forceinline__ void step_store(const StepParams& p, size_t i, const StepResult& r) {
    if (p.e_t_out) p.e_t_out[i] = r.e_t;
    if (p.pred_x0) p.pred_x0[i] = r.pred_x0;
    p.x_prev[i] = r.x_prev;
}

// the body of sampler_step_kernel and of the spread row kernel: load, call, store
template <int PRED, class M = NoMid>
__device__ __forceinline__ void sampler_step_element(const StepParams& p, size_t i, size_t ei, const M& mid = M{}) {
    step_store(p, i, step_arith<PRED>(p, step_load<PRED, false>(p, mid, p.g.out_u, p.g.out_c, ei, i)));
}

// SPREAD: the grid-stride loop of sampler_step_kernel and of its DUAL sibling
template <int PRED, class M>
__device__ __forceinline__ void sampler_step_spread(const StepParams& p, const M& mid) {
    const size_t total = (size_t)p.B * p.g.C * p.g.HW;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int pix = (int)(i % p.g.HW);
        const size_t bc = i / p.g.HW;
        const int c = (int)(bc % p.g.C);
        const int b = (int)(bc / p.g.C);
        sampler_step_element<PRED>(p, i, ((size_t)b * p.g.HW + pix) * p.g.ld + c, mid);
    }
}

template <int PRED>
__global__ __launch_bounds__(256) void sampler_step_kernel(const StepParams p) {
    mdx_kernarg_touch<sizeof(StepParams)>();
    sampler_step_spread<PRED>(p, NoMid{});
}

template <int PRED>
__global__ __launch_bounds__(256) void sampler_step_dual_kernel(const StepDualParams q) {
    mdx_kernarg_touch<sizeof(StepDualParams)>();
    sampler_step_spread<PRED>(q.s, q.mid);
}

// ------------------------------------------------------------------ fused sampler update with guidance rescale
// Lin et al., "Common Diffusion Noise Schedules and Sample Steps are Flawed", section 3.4: the CFG-combined model output m is
// scaled by f[b] = phi * std(out_c[b]) / std(m[b]) + (1 - phi) before the step.  The statistics are per sample over C * HW,
// so ONE workgroup owns a sample: pass 1 reads only the two model outputs (which no output may alias) in their own NHWC order,
// pass 2 is the step on m' = f m.
struct RescaleParams {
    StepParams s;
    float phi;
    float* factor_out;
};

constexpr int RESCALE_THREADS = 1024;

// Sums are taken of d = v - K with K = the mean of the sample's first 64 values (the same bits in every wave), so that
// sum(d^2) - sum(d)^2 / N cancels nothing to speak of when the outputs sit on an offset far above their spread.
// Shared by the eps family and the lin family: it reads the guided pair alone.
// m is the three-branch value where a middle branch is given (mid: from the batch's start); the target std stays out_c's.
template <class M = NoMid>
__device__ __forceinline__ float rescale_factor(const GuidedPair& g, float phi, int b, float (*part)[4], const M& mid0 = M{}) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned N = (unsigned)g.C * (unsigned)g.HW;      // per sample: the host refuses what does not fit 31 bits
    const unsigned C = g.C, HW = g.HW;
    const f16* ou = g.out_u + (size_t)b * HW * g.ld;
    const f16* oc = g.out_c + (size_t)b * HW * g.ld;
    const M mid = mid_at(mid0, (size_t)b * HW * g.ld);

    // ---- pass 1: unbiased per-sample std of out_c and of m, in the outputs' own (pixel, channel) order
    float kc, km;
    {
        const unsigned j = (unsigned)lane < N ? (unsigned)lane : N - 1;
        const size_t ei = (size_t)(j / C) * g.ld + j % C;
        const float c = (float)oc[ei];
        kc = wave_sum(c) * (1.f / 64.f);
        km = wave_sum(guided_value<true>(mid, ou, oc, ei, g.cfg_scale)) * (1.f / 64.f);
    }
    float sc = 0.f, scc = 0.f, sm = 0.f, smm = 0.f;
#pragma unroll 4
    for (unsigned j = threadIdx.x; j < N; j += RESCALE_THREADS) {
        const size_t ei = (size_t)(j / C) * g.ld + j % C;
        const float c = (float)oc[ei];
        const float dc = c - kc, dm = guided_value<true>(mid, ou, oc, ei, g.cfg_scale) - km;
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

// ---- pass 2: the step on m' = f m, U elements of a thread at a time: all their loads first, then the arithmetic and the
// stores.  Without the batching every trip of the loop waits out one memory latency behind the previous trip's stores (a
// workgroup has a sample to itself, so there is no one else to hide it).  f == 1 (a phi == 0 row) multiplies exactly, so the
// result is sampler_step_kernel's: both run step_arith.
template <int PRED, class M = NoMid>
__device__ __forceinline__ void rescale_apply(const StepParams& p, float f, int b, const M& mid0 = M{}) {
    const unsigned N = (unsigned)p.g.C * (unsigned)p.g.HW;
    const unsigned HW = p.g.HW;
    const f16* ou = p.g.out_u + (size_t)b * HW * p.g.ld;
    const f16* oc = p.g.out_c + (size_t)b * HW * p.g.ld;
    const M mid = mid_at(mid0, (size_t)b * HW * p.g.ld);      // its loads go out with the batch's others, below
    constexpr int U = 4;
    const size_t base = (size_t)b * N;
    for (unsigned j0 = threadIdx.x; j0 < N; j0 += RESCALE_THREADS * U) {
        StepOperands v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const unsigned j = j0 + u * RESCALE_THREADS;
            if (j < N) {
                const unsigned c = j / HW;
                v[u] = step_load<PRED, true>(p, mid, ou, oc, (size_t)(j - c * HW) * p.g.ld + c, base + j);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const unsigned j = j0 + u * RESCALE_THREADS;
            if (j < N) {
                v[u].m *= f;
                step_store(p, base + j, step_arith<PRED>(p, v[u]));
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
    const float f = rescale_factor(p.g, rp.phi, b, part);
    if (rp.factor_out && threadIdx.x == 0) rp.factor_out[b] = f;
    rescale_apply<PRED>(p, f, b);
}

struct RescaleDualParams {
    RescaleParams r;
    GuidedMid mid;
};

template <int PRED>
__global__ __launch_bounds__(RESCALE_THREADS) void sampler_step_rescale_dual_kernel(const RescaleDualParams q) {
    mdx_kernarg_touch<sizeof(RescaleDualParams)>();
    const StepParams& p = q.r.s;
    __shared__ float part[RESCALE_THREADS / 64][4];
    const int b = blockIdx.x;
    const float f = rescale_factor(p.g, q.r.phi, b, part, q.mid);
    if (q.r.factor_out && threadIdx.x == 0) q.r.factor_out[b] = f;
    rescale_apply<PRED>(p, f, b, q.mid);
}

// ------------------------------------------------------------------ fused sampler update, per-sample scalars from a row
// Every scalar the kernels above take as a kernel argument comes from a row of MDX_STEP_ROW floats on the device (MDX_STEP_*
// of mdx.h), so samples with different guidance scales, rescale strengths and schedules share one launch.  A workgroup works
// on ONE sample: its row is the same address in every lane.  Where the row of sample b lies is the one difference between the
// two entries: row b of a table (mdx_sampler_step_table_f32: no slot arrays), or -- a sampling session,
// mdx_sampler_step_slots_f32 -- the row slot b stands on, rows[b][tick - slot_start[b]] of its request's [cap] rows; the tick
// is a kernel argument and nothing on the device moves between admissions.  A slot outside its request has no row, which is an
// inactive row.
struct RowParams {
    StepParams s;
    const float* rows;        // [B][MDX_STEP_ROW], or with slot arrays [B][cap][MDX_STEP_ROW]
    const int* slot_start;    // [B] or nullptr
    const int* slot_len;      // [B]
    int cap, tick;
    float* factor_out;
};

__device__ __forceinline__ const float* step_row(const RowParams& rp, int b) {
    if (!rp.slot_start) return rp.rows + (size_t)b * MDX_STEP_ROW;
    const int pos = mdx_slot_pos(rp.slot_start, rp.slot_len, b, rp.cap, rp.tick);
    return pos < 0 ? nullptr : rp.rows + ((size_t)b * rp.cap + pos) * MDX_STEP_ROW;
}

// table_row fills the StepParams of the row's sample, with the pointers the scalar entries' host code would have kept (a term
// whose coefficient is exactly 0 is skipped, not multiplied: what it points to may be NaN).  false: no row, or an inactive one.
__device__ __forceinline__ bool table_row(StepParams& p, const float* row, float& phi) {
    if (!row || row[MDX_STEP_ACTIVE] == 0.f) return false;
    p.g.cfg_scale = row[MDX_STEP_CFG_SCALE];
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
    const unsigned N = (unsigned)p.g.C * (unsigned)p.g.HW;
    const size_t base = (size_t)b * N;
    for (unsigned j = first + threadIdx.x; j < N; j += stride) p.x_prev[base + j] = p.x[base + j];
}

// SPREAD, no row rescales: gridDim.x workgroups share sample blockIdx.y, sampler_step_kernel's body per element.
template <int PRED>
__global__ __launch_bounds__(256) void sampler_step_rows_kernel(const RowParams rp) {
    mdx_kernarg_touch<sizeof(RowParams)>();
    StepParams p = rp.s;
    const int b = blockIdx.y;
    const unsigned N = (unsigned)p.g.C * (unsigned)p.g.HW, HW = p.g.HW;      // the host refuses what does not fit 31 bits
    const unsigned first = blockIdx.x * 256u, stride = gridDim.x * 256u;
    float phi;
    if (!table_row(p, step_row(rp, b), phi)) {
        table_copy_row(p, b, first, stride);
        return;
    }
    if (rp.factor_out && blockIdx.x == 0 && threadIdx.x == 0) rp.factor_out[b] = 1.f;
    const size_t base = (size_t)b * N;
    for (unsigned j = first + threadIdx.x; j < N; j += stride) {
        const unsigned c = j / HW;
        sampler_step_element<PRED>(p, base + j, ((size_t)b * HW + (j - c * HW)) * p.g.ld + c);
    }
}

// OWNED, some row rescales: a workgroup owns a sample, as in sampler_step_rescale_kernel; a row with phi == 0 reads no
// statistics and runs pass 2 with f = 1, which is the spread kernel's result to the bit (rescale_apply).
template <int PRED>
__global__ __launch_bounds__(RESCALE_THREADS) void sampler_step_rows_owned_kernel(const RowParams rp) {
    mdx_kernarg_touch<sizeof(RowParams)>();
    StepParams p = rp.s;
    __shared__ float part[RESCALE_THREADS / 64][4];
    const int b = blockIdx.x;
    float phi;
    if (!table_row(p, step_row(rp, b), phi)) {
        table_copy_row(p, b, 0u, (unsigned)RESCALE_THREADS);
        return;
    }
    float f = 1.f;
    if (phi != 0.f) f = rescale_factor(p.g, phi, b, part);      // the row is the workgroup's: every thread takes the same side
    if (rp.factor_out && threadIdx.x == 0) rp.factor_out[b] = f;
    rescale_apply<PRED>(p, f, b);
}

// ------------------------------------------------------------------ the DPM-Solver step launch (mdx_sampler_step_lin_f32)
// The model value of one evaluation (data or noise prediction, optionally thresholded) and the linear form
// x_out = A x_base + c0 val + c1 h1 + c2 h2 that every update of the solver is; include/mdx.h has the contract.  The host
// keeps a history pointer only for a non-zero coefficient and sets phi = 0 without an unconditional half, so the kernels test
// pointers and A / phi only.  No __restrict__: x_out may be x_base and / or x_model, element for element -- every kernel below
// reads element i of both before it stores element i of x_out, in the same thread.
struct LinParams {
    GuidedPair g;
    const float* x_base;
    const float* x_model;
    const float* h1;
    const float* h2;
    float* model_out;
    float* x_out;
    float* model_pre_out;
    float* thr_out;
    float* factor_out;
    int B;
    float am, sm, A, c0, c1, c2, phi, max_val;
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

// the DUAL instantiations' parameters, with and without noise (mdx_sampler_step_lin_dual_f32)
struct LinDualParams {
    LinParams l;
    LinNoise n;
    GuidedMid mid;
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

// The loaded operands of one element; a skipped term's operand stays 0 and is not used.
struct LinOperands {
    float m, x_model, x_base, h1, h2, z;
};

template <int PRED, int VALUE>
constexpr bool lin_reads_x_model = PRED == MDX_PRED_V || VALUE == MDX_VALUE_X0;

// what steps 1-4 read: the CFG-combined model output and the latent the model was evaluated on
// (mid: the middle branch from where ou / oc start, NoMid: none)
template <int PRED, int VALUE, class M>
__device__ __forceinline__ void lin_load_model(const LinParams& p, const M& mid, const f16* ou, const f16* oc, size_t ei,
                                               size_t i, LinOperands& v) {
    v.m = guided_value<false>(mid, ou, oc, ei, p.g.cfg_scale);
    if constexpr (lin_reads_x_model<PRED, VALUE>) v.x_model = p.x_model[i];
}

// what steps 7 and 8 read, but z from the generator
template <int NOISE>
__device__ __forceinline__ void lin_load_terms(const LinParams& p, const LinNoise& n, size_t i, LinOperands& v) {
    if (p.A != 0.f) v.x_base = p.x_base[i];
    if (p.h1) v.h1 = p.h1[i];
    if (p.h2) v.h2 = p.h2[i];
    if constexpr (NOISE == LIN_NOISE_TENSOR) v.z = n.noise[i];
}

// steps 3 and 4: the CFG-combined (and rescaled) model output m to the model value.
// PER-FORM SPELLING (the one statement of the family that has one): eps = a v + b x_m (dpm_solver.py:281-284) rounds b x_m
// and fuses a v in the SPREAD kernels, and rounds a v and fuses b x_m in the OWNED kernel.  The two forms have always
// disagreed here and nothing promises that they agree (a launch is SPREAD or OWNED for all its samples), so each keeps the
// bits it has always given.
template <int PRED, int VALUE, bool OWNED>
__device__ __forceinline__ float lin_value(const LinParams& p, float m, float xm) {
#pragma clang fp contract(off)
    float e = m;
    if constexpr (PRED == MDX_PRED_V) e = OWNED ? __builtin_fmaf(p.sm, xm, p.am * m) : __builtin_fmaf(p.am, m, p.sm * xm);
    if constexpr (VALUE == MDX_VALUE_X0) return __builtin_fmaf(-p.sm, e, xm) / p.am;
    return e;
}

// steps 7 and 8: c0 val and A x_base both rounded and added, every further term fused into the sum in this order
template <int NOISE>
__device__ __forceinline__ float lin_x_out(const LinParams& p, const LinNoise& n, float val, const LinOperands& v) {
#pragma clang fp contract(off)
    float xo = p.c0 * val;
    if (p.A != 0.f) xo = xo + p.A * v.x_base;
    if (p.h1) xo = __builtin_fmaf(p.c1, v.h1, xo);
    if (p.h2) xo = __builtin_fmaf(p.c2, v.h2, xo);
    if constexpr (NOISE != LIN_NOISE_NONE) xo = __builtin_fmaf(n.cn, v.z, xo);
    return xo;
}

// steps 3, 4, 7 and 8 of an element whose operands are loaded, and its stores
template <int PRED, int VALUE, bool OWNED, int NOISE>
__device__ __forceinline__ void lin_element(const LinParams& p, const LinNoise& n, size_t i, const LinOperands& v) {
    const float val = lin_value<PRED, VALUE, OWNED>(p, v.m, v.x_model);
    p.model_out[i] = val;
    if (p.model_pre_out) p.model_pre_out[i] = val;
    p.x_out[i] = lin_x_out<NOISE>(p, n, val, v);
}

// SPREAD: sampler_step_kernel's grid and element order
template <int PRED, int VALUE, class M>
__device__ __forceinline__ void sampler_step_lin_spread(const LinParams& p, const M& mid) {
    const size_t total = (size_t)p.B * p.g.C * p.g.HW;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int pix = (int)(i % p.g.HW);
        const size_t bc = i / p.g.HW;
        const int c = (int)(bc % p.g.C);
        const int b = (int)(bc / p.g.C);
        LinOperands v{};
        lin_load_model<PRED, VALUE>(p, mid, p.g.out_u, p.g.out_c, ((size_t)b * p.g.HW + pix) * p.g.ld + c, i, v);
        lin_load_terms<LIN_NOISE_NONE>(p, LinNoise{}, i, v);
        lin_element<PRED, VALUE, false, LIN_NOISE_NONE>(p, LinNoise{}, i, v);
    }
}

template <int PRED, int VALUE>
__global__ __launch_bounds__(256) void sampler_step_lin_kernel(const LinParams p) {
    mdx_kernarg_touch<sizeof(LinParams)>();
    sampler_step_lin_spread<PRED, VALUE>(p, NoMid{});
}

template <int PRED, int VALUE>
__global__ __launch_bounds__(256) void sampler_step_lin_dual_kernel(const LinDualParams q) {
    mdx_kernarg_touch<sizeof(LinDualParams)>();
    sampler_step_lin_spread<PRED, VALUE>(q.l, q.mid);
}

// SPREAD with step 8: a quad per thread and trip, all loads first (the draw's arithmetic then runs under their latency), then
// the arithmetic and the stores -- a thread stores only elements it has read, so x_out may be x_base / x_model as above.
// 64-thread workgroups: a quad is four elements, so the latent of a UNet batch still spreads over a hundred CUs and more.
constexpr int LIN_NOISE_THREADS = 64;

template <int PRED, int VALUE, int NOISE, class M>
__device__ __forceinline__ void sampler_step_lin_noise_spread(const LinParams& p, const LinNoise& n, const M& mid) {
    const unsigned N = (unsigned)p.g.C * (unsigned)p.g.HW, HW = p.g.HW;       // the host refuses what does not fit 31 bits
    const unsigned quads = (N + 3u) / 4u;
    const size_t items = (size_t)p.B * quads;
    for (size_t it = (size_t)blockIdx.x * LIN_NOISE_THREADS + threadIdx.x; it < items;
         it += (size_t)gridDim.x * LIN_NOISE_THREADS) {
        const int b = (int)(it / quads);
        const unsigned j0 = (unsigned)(it - (size_t)b * quads) * 4u;
        const size_t base = (size_t)b * N;
        LinOperands v[LIN_U];
#pragma unroll
        for (int u = 0; u < LIN_U; ++u) {
            const unsigned j = j0 + u;
            v[u] = LinOperands{};
            if (j < N) {
                const unsigned c = j / HW;
                lin_load_model<PRED, VALUE>(p, mid, p.g.out_u, p.g.out_c, ((size_t)b * HW + (j - c * HW)) * p.g.ld + c, base + j, v[u]);
                lin_load_terms<NOISE>(p, n, base + j, v[u]);
            }
        }
        if constexpr (NOISE == LIN_NOISE_SEEDED) {
            float z[LIN_U];
            lin_quad_z(n, b, j0, z);
#pragma unroll
            for (int u = 0; u < LIN_U; ++u) v[u].z = z[u];
        }
#pragma unroll
        for (int u = 0; u < LIN_U; ++u)
            if (j0 + u < N) lin_element<PRED, VALUE, false, NOISE>(p, n, base + j0 + u, v[u]);
    }
}

template <int PRED, int VALUE, int NOISE>
__global__ __launch_bounds__(LIN_NOISE_THREADS) void sampler_step_lin_noise_kernel(const LinNoiseParams q) {
    mdx_kernarg_touch<sizeof(LinNoiseParams)>();
    sampler_step_lin_noise_spread<PRED, VALUE, NOISE>(q.l, q.n, NoMid{});
}

template <int PRED, int VALUE, int NOISE>
__global__ __launch_bounds__(LIN_NOISE_THREADS) void sampler_step_lin_noise_dual_kernel(const LinDualParams q) {
    mdx_kernarg_touch<sizeof(LinDualParams)>();
    sampler_step_lin_noise_spread<PRED, VALUE, NOISE>(q.l, q.n, q.mid);
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
__device__ __forceinline__ void lin_owned_z(const LinNoise& n, int b, unsigned j0, unsigned N, LinOperands (&v)[LIN_U]) {
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
        v[u].z = e == 0 ? a0 : e == 1 ? a1 : e == 2 ? a2 : a3;
    }
}

// Steps 1-4 (and, without thresholding, 7 and 8).  PARK: the values wait in model_out for the selection.
template <int PRED, int VALUE, bool PARK, int NOISE, class M>
__device__ __forceinline__ void lin_owned_values(const LinParams& p, const LinNoise& n, const M& mid0, float f, int b) {
    const unsigned N = (unsigned)p.g.C * (unsigned)p.g.HW, HW = p.g.HW;
    const f16* oc = p.g.out_c + (size_t)b * HW * p.g.ld;
    const f16* ou = p.g.out_u ? p.g.out_u + (size_t)b * HW * p.g.ld : nullptr;
    const M mid = mid_at(mid0, (size_t)b * HW * p.g.ld);      // its loads go out with the batch's others, below
    const size_t base = (size_t)b * N;
    for (unsigned j0 = threadIdx.x; lin_owned_trip<NOISE>(j0, N); j0 += RESCALE_THREADS * LIN_U) {
        LinOperands v[LIN_U];
#pragma unroll
        for (int u = 0; u < LIN_U; ++u) {
            const unsigned j = j0 + u * RESCALE_THREADS;
            v[u] = LinOperands{};
            if (j < N) {
                const unsigned c = j / HW;
                lin_load_model<PRED, VALUE>(p, mid, ou, oc, (size_t)(j - c * HW) * p.g.ld + c, base + j, v[u]);
                if constexpr (!PARK) lin_load_terms<NOISE>(p, n, base + j, v[u]);
            }
        }
        if constexpr (!PARK && NOISE == LIN_NOISE_SEEDED) lin_owned_z(n, b, j0, N, v);
#pragma unroll
        for (int u = 0; u < LIN_U; ++u) {
            const unsigned j = j0 + u * RESCALE_THREADS;
            if (j < N) {
                v[u].m *= f;
                if constexpr (PARK) {
                    const float val = lin_value<PRED, VALUE, true>(p, v[u].m, v[u].x_model);
                    p.model_out[base + j] = val;
                    if (p.model_pre_out) p.model_pre_out[base + j] = val;
                } else {
                    lin_element<PRED, VALUE, true, NOISE>(p, n, base + j, v[u]);
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
    const unsigned N = (unsigned)p.g.C * (unsigned)p.g.HW;
    const size_t base = (size_t)b * N;
    for (unsigned j0 = threadIdx.x; lin_owned_trip<NOISE>(j0, N); j0 += RESCALE_THREADS * LIN_U) {
        float parked[LIN_U];
        LinOperands v[LIN_U];
#pragma unroll
        for (int u = 0; u < LIN_U; ++u) {
            const unsigned j = j0 + u * RESCALE_THREADS;
            parked[u] = 0.f;
            v[u] = LinOperands{};
            if (j < N) {
                parked[u] = p.model_out[base + j];
                lin_load_terms<NOISE>(p, n, base + j, v[u]);
            }
        }
        if constexpr (NOISE == LIN_NOISE_SEEDED) lin_owned_z(n, b, j0, N, v);
#pragma unroll
        for (int u = 0; u < LIN_U; ++u) {
            const unsigned j = j0 + u * RESCALE_THREADS;
            if (j < N) {
                const float val = fminf(fmaxf(parked[u], -s), s) / s;
                p.model_out[base + j] = val;
                p.x_out[base + j] = lin_x_out<NOISE>(p, n, val, v[u]);
            }
        }
    }
}

// OWNED: one kernel for all entries.  P is LinParams (mdx_sampler_step_lin_f32: NOISE is LIN_NOISE_NONE, the kernel that
// entry has always launched), LinNoiseParams, or LinDualParams (a middle branch, any NOISE).
__device__ __forceinline__ const LinParams& lin_of(const LinParams& p) { return p; }
__device__ __forceinline__ const LinParams& lin_of(const LinNoiseParams& q) { return q.l; }
__device__ __forceinline__ const LinParams& lin_of(const LinDualParams& q) { return q.l; }
__device__ __forceinline__ LinNoise lin_noise_of(const LinParams&) { return LinNoise{}; }
__device__ __forceinline__ LinNoise lin_noise_of(const LinNoiseParams& q) { return q.n; }
__device__ __forceinline__ LinNoise lin_noise_of(const LinDualParams& q) { return q.n; }
__device__ __forceinline__ NoMid lin_mid_of(const LinParams&) { return NoMid{}; }
__device__ __forceinline__ NoMid lin_mid_of(const LinNoiseParams&) { return NoMid{}; }
__device__ __forceinline__ GuidedMid lin_mid_of(const LinDualParams& q) { return q.mid; }

template <int PRED, int VALUE, int NOISE, class P>
__global__ __launch_bounds__(RESCALE_THREADS) void sampler_step_lin_owned_kernel(const P q) {
    mdx_kernarg_touch<sizeof(P)>();
    __shared__ float part[RESCALE_THREADS / 64][4];
    __shared__ unsigned hist[256];
    __shared__ unsigned sel[4];
    const LinParams& p = lin_of(q);
    const LinNoise n = lin_noise_of(q);
    const auto mid = lin_mid_of(q);
    const int b = blockIdx.x;
    float f = 1.f;
    if (p.phi != 0.f) f = rescale_factor(p.g, p.phi, b, part, mid);
    if (p.factor_out && threadIdx.x == 0) p.factor_out[b] = f;
    if constexpr (VALUE == MDX_VALUE_X0) {
        if (p.thresholding) {
            lin_owned_values<PRED, VALUE, true, NOISE>(p, n, mid, f, b);
            __syncthreads();        // (a thread reads back only what it parked itself; the barrier is for sel / hist)
            const unsigned N = (unsigned)p.g.C * (unsigned)p.g.HW;
            const float s = lin_threshold_s(p, p.model_out + (size_t)b * N, N, hist, sel);
            if (p.thr_out && threadIdx.x == 0) p.thr_out[b] = s;
            lin_owned_finish<NOISE>(p, n, s, b);
            return;
        }
    }
    lin_owned_values<PRED, VALUE, false, NOISE>(p, n, mid, f, b);
}

// ------------------------------------------------------------------ the UniPC step launch (mdx_sampler_step_pc_f32)
// Two linear forms over the model value of one evaluation: the CORRECTED latent at the evaluation's time,
// xc = Ac x_base + d0 val + d1 h1 + d2 h2 + d3 h3, and the PREDICTED latent at the next time, xp = Ap xc + e0 val + e1 h1 + e2 h2
// (uni_pc.unipc_plan folds the differences D_j into the coefficients); include/mdx.h has the contract.  Steps 1-6 are the lin
// family's on LinParams `c`, which also carries the corrector's form: the kernels below call lin_load_model, lin_value,
// lin_x_out, rescale_factor, lin_owned_values<PARK> and lin_threshold_s, so corrector off is the lin launch on (x_model, Ap, e)
// and d3 == 0 is the lin launch on (x_base, Ac, d), to the bit.  `p` is a LinParams for lin_x_out's sake: of it only A, c0 .. c2,
// h1, h2 and x_out (x_pred_out) are read.  A history is loaded once, if either form has a coefficient for it.
// No __restrict__: x_corr_out may be x_base and x_pred_out may be x_model, element for element -- a thread reads element i of
// everything before it stores element i of anything.
struct PcParams {
    LinParams c;
    LinParams p;
    const float* h1;
    const float* h2;
    const float* h3;
    float d3;
    int has_corrector;
};

struct PcOperands {
    LinOperands v;
    float h3;
};

// what steps 7 and 8 read.  XM: x_model is not among the operands yet (the pass did not load it, or the value needs none).
template <bool XM>
__device__ __forceinline__ void pc_load_terms(const PcParams& q, size_t i, PcOperands& o) {
    if (q.has_corrector) {
        if (q.c.A != 0.f) o.v.x_base = q.c.x_base[i];
    } else if constexpr (XM) {
        o.v.x_model = q.c.x_model[i];
    }
    if (q.h1) o.v.h1 = q.h1[i];
    if (q.h2) o.v.h2 = q.h2[i];
    if (q.h3) o.h3 = q.h3[i];
}

// steps 7 and 8 and their stores
__device__ __forceinline__ void pc_forms(const PcParams& q, size_t i, float val, const PcOperands& o) {
#pragma clang fp contract(off)
    float xc = o.v.x_model;      // no corrector: the bits of the latent the model was evaluated on
    if (q.has_corrector) {
        xc = lin_x_out<LIN_NOISE_NONE>(q.c, LinNoise{}, val, o.v);
        if (q.h3) xc = __builtin_fmaf(q.d3, o.h3, xc);
    }
    LinOperands w = o.v;
    w.x_base = xc;
    const float xp = lin_x_out<LIN_NOISE_NONE>(q.p, LinNoise{}, val, w);
    q.c.x_out[i] = xc;
    q.p.x_out[i] = xp;
}

template <int PRED, int VALUE, bool OWNED>
__device__ __forceinline__ void pc_element(const PcParams& q, size_t i, const PcOperands& o) {
    const float val = lin_value<PRED, VALUE, OWNED>(q.c, o.v.m, o.v.x_model);
    q.c.model_out[i] = val;
    if (q.c.model_pre_out) q.c.model_pre_out[i] = val;
    pc_forms(q, i, val, o);
}

// SPREAD: sampler_step_lin_kernel's grid and element order
template <int PRED, int VALUE>
__global__ __launch_bounds__(256) void sampler_step_pc_kernel(const PcParams q) {
    mdx_kernarg_touch<sizeof(PcParams)>();
    const LinParams& p = q.c;
    const size_t total = (size_t)p.B * p.g.C * p.g.HW;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int pix = (int)(i % p.g.HW);
        const size_t bc = i / p.g.HW;
        const int c = (int)(bc % p.g.C);
        const int b = (int)(bc / p.g.C);
        PcOperands o{};
        lin_load_model<PRED, VALUE>(p, NoMid{}, p.g.out_u, p.g.out_c, ((size_t)b * p.g.HW + pix) * p.g.ld + c, i, o.v);
        pc_load_terms<!lin_reads_x_model<PRED, VALUE>>(q, i, o);
        pc_element<PRED, VALUE, false>(q, i, o);
    }
}

// OWNED without thresholding: lin_owned_values' one pass (U elements of a thread at a time, all loads first)
template <int PRED, int VALUE>
__device__ __forceinline__ void pc_owned_values(const PcParams& q, float f, int b) {
    const LinParams& p = q.c;
    const unsigned N = (unsigned)p.g.C * (unsigned)p.g.HW, HW = p.g.HW;
    const f16* oc = p.g.out_c + (size_t)b * HW * p.g.ld;
    const f16* ou = p.g.out_u ? p.g.out_u + (size_t)b * HW * p.g.ld : nullptr;
    const size_t base = (size_t)b * N;
    for (unsigned j0 = threadIdx.x; j0 < N; j0 += RESCALE_THREADS * LIN_U) {
        PcOperands o[LIN_U];
#pragma unroll
        for (int u = 0; u < LIN_U; ++u) {
            const unsigned j = j0 + u * RESCALE_THREADS;
            o[u] = PcOperands{};
            if (j < N) {
                const unsigned c = j / HW;
                lin_load_model<PRED, VALUE>(p, NoMid{}, ou, oc, (size_t)(j - c * HW) * p.g.ld + c, base + j, o[u].v);
                pc_load_terms<!lin_reads_x_model<PRED, VALUE>>(q, base + j, o[u]);
            }
        }
#pragma unroll
        for (int u = 0; u < LIN_U; ++u) {
            const unsigned j = j0 + u * RESCALE_THREADS;
            if (j < N) {
                o[u].v.m *= f;
                pc_element<PRED, VALUE, true>(q, base + j, o[u]);
            }
        }
    }
}

// OWNED with thresholding, steps 5-8 on the values lin_owned_values<PARK> left in model_out (lin_owned_finish's pass)
__device__ __forceinline__ void pc_owned_finish(const PcParams& q, float s, int b) {
    const LinParams& p = q.c;
    const unsigned N = (unsigned)p.g.C * (unsigned)p.g.HW;
    const size_t base = (size_t)b * N;
    for (unsigned j0 = threadIdx.x; j0 < N; j0 += RESCALE_THREADS * LIN_U) {
        float parked[LIN_U];
        PcOperands o[LIN_U];
#pragma unroll
        for (int u = 0; u < LIN_U; ++u) {
            const unsigned j = j0 + u * RESCALE_THREADS;
            parked[u] = 0.f;
            o[u] = PcOperands{};
            if (j < N) {
                parked[u] = p.model_out[base + j];
                pc_load_terms<true>(q, base + j, o[u]);
            }
        }
#pragma unroll
        for (int u = 0; u < LIN_U; ++u) {
            const unsigned j = j0 + u * RESCALE_THREADS;
            if (j < N) {
                const float val = fminf(fmaxf(parked[u], -s), s) / s;
                p.model_out[base + j] = val;
                pc_forms(q, base + j, val, o[u]);
            }
        }
    }
}

template <int PRED, int VALUE>
__global__ __launch_bounds__(RESCALE_THREADS) void sampler_step_pc_owned_kernel(const PcParams q) {
    mdx_kernarg_touch<sizeof(PcParams)>();
    __shared__ float part[RESCALE_THREADS / 64][4];
    __shared__ unsigned hist[256];
    __shared__ unsigned sel[4];
    const LinParams& p = q.c;
    const int b = blockIdx.x;
    float f = 1.f;
    if (p.phi != 0.f) f = rescale_factor(p.g, p.phi, b, part);
    if (p.factor_out && threadIdx.x == 0) p.factor_out[b] = f;
    if constexpr (VALUE == MDX_VALUE_X0) {
        if (p.thresholding) {
            lin_owned_values<PRED, VALUE, true, LIN_NOISE_NONE>(p, LinNoise{}, NoMid{}, f, b);
            __syncthreads();        // (a thread reads back only what it parked itself; the barrier is for sel / hist)
            const unsigned N = (unsigned)p.g.C * (unsigned)p.g.HW;
            const float s = lin_threshold_s(p, p.model_out + (size_t)b * N, N, hist, sel);
            if (p.thr_out && threadIdx.x == 0) p.thr_out[b] = s;
            pc_owned_finish(q, s, b);
            return;
        }
    }
    pc_owned_values<PRED, VALUE>(q, f, b);
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

// ------------------------------------------------------------------ host helpers
// factor_out[0 .. B) = 1 for a launch form that computes no factor (f == 1 everywhere)
int fill_factor_one(const char* fn, float* factor_out, int B, hipStream_t st) {
    if (!factor_out) return MDX_OK;
    const hipError_t e = hipMemsetD32Async((hipDeviceptr_t)factor_out, 0x3f800000 /* 1.0f */, (size_t)B, st);
    if (e != hipSuccess) {
        mdx_set_error("%s: factor_out fill failed: %s", fn, hipGetErrorString(e));
        return MDX_E_HIP;
    }
    return MDX_OK;
}

// The per-sample extent refusals of every entry that indexes a sample with 32 bits; with_std: it may take a per-sample std.
int sample_extent_check(const char* fn, size_t N, bool with_std) {
    MDX_REQUIRE(!with_std || N >= 2, "%s: the per-sample std needs C * H * W >= 2", fn);
    MDX_REQUIRE(N <= 0x7fffffffu, "%s: bad extents (C * H * W of one sample exceeds 31 bits)", fn);
    return MDX_OK;
}

bool bytes_overlap(const void* a, size_t na, const void* b, size_t nb) {
    if (!a || !b || na == 0 || nb == 0) return false;
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

// What both DUAL entries refuse about the middle branch itself (out_m != nullptr); its overlaps are the entries' own.
int guided_mid_check(const char* fn, const void* out_u, float mid_scale) {
    MDX_REQUIRE(out_u, "%s: out_m without out_u (the middle branch extends a guided pair)", fn);
    MDX_REQUIRE(mid_scale >= -3.402823466e38f && mid_scale <= 3.402823466e38f, "%s: mid_scale %g is not finite", fn,
                (double)mid_scale);
    return MDX_OK;
}

}  // namespace

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
    p.g = GuidedPair{(const f16*)out_u, (const f16*)out_c, out_ld, C, H * W, cfg_scale};
    p.x = x;
    p.x_model = x_model ? x_model : x;
    p.old1 = coef4[1] != 0.f ? old1 : nullptr;
    p.old2 = coef4[2] != 0.f ? old2 : nullptr;
    p.old3 = coef4[3] != 0.f ? old3 : nullptr;
    p.noise = sigma != 0.f ? noise : nullptr;
    p.e_t_out = e_t_out;
    p.x_prev = x_prev;
    p.pred_x0 = pred_x0;
    p.B = B;
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
    const dim3 grid(grid_for((size_t)p.B * p.g.C * p.g.HW));
    const auto kernel = pred_type == MDX_PRED_V ? sampler_step_kernel<MDX_PRED_V> : sampler_step_kernel<MDX_PRED_EPS>;
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, (hipStream_t)s, p);
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

// The rescale entry and its DUAL superset: out_m == nullptr is the two-branch body, launch for launch.
static int sampler_step_rescale_entry(const char* fn, const float* x, const float* x_model, const void* out_u,
                                      const void* out_c, int out_ld, float cfg_scale, int pred_type, float sqrt_at_model,
                                      float sqrt_one_minus_at_model, const float* old1, const float* old2, const float* old3,
                                      const float* coef4, float sqrt_at, float sqrt_one_minus_at, float sqrt_a_prev,
                                      float dir_coef, float sigma, const float* noise, float* e_t_out, float* x_prev,
                                      float* pred_x0, float guidance_rescale, float* factor_out, const void* out_m,
                                      float mid_scale, int B, int C, int H, int W, mdx_stream_t s) {
    RescaleParams rp;
    int rc = sampler_step_params(rp.s, fn, x, x_model, out_u, out_c, out_ld, cfg_scale, pred_type, sqrt_at_model,
                                 sqrt_one_minus_at_model, old1, old2, old3, coef4, sqrt_at, sqrt_one_minus_at, sqrt_a_prev,
                                 dir_coef, sigma, noise, e_t_out, x_prev, pred_x0, B, C, H, W);
    if (rc != MDX_OK) return rc;
    MDX_REQUIRE(guidance_rescale >= 0.f && guidance_rescale <= 1.f, "%s: guidance_rescale %g is not in [0, 1]", fn,
                (double)guidance_rescale);
    if ((rc = sample_extent_check(fn, (size_t)C * H * W, true)) != MDX_OK) return rc;
    const bool v = pred_type == MDX_PRED_V;
    if (out_m) {
        if ((rc = guided_mid_check(fn, out_u, mid_scale)) != MDX_OK) return rc;
        const size_t nx = (size_t)B * C * H * W * sizeof(float), nh = (((size_t)B * H * W - 1) * out_ld + C) * sizeof(f16);
        const struct { const void* ptr; size_t bytes; const char* name; } outs[] = {
            {e_t_out, nx, "e_t_out"}, {x_prev, nx, "x_prev"}, {pred_x0, nx, "pred_x0"}, {factor_out, B * sizeof(float), "factor_out"}};
        for (const auto& o : outs)
            MDX_REQUIRE(!bytes_overlap(o.ptr, o.bytes, out_m, nh), "%s: %s overlaps out_m", fn, o.name);
        const GuidedMid mid{(const f16*)out_m, mid_scale};
        if (guidance_rescale == 0.f) {      // SPREAD, as the two-branch entry chooses
            const StepDualParams q{rp.s, mid};
            hipLaunchKernelGGL(v ? sampler_step_dual_kernel<MDX_PRED_V> : sampler_step_dual_kernel<MDX_PRED_EPS>,
                               dim3(grid_for((size_t)B * C * H * W)), dim3(256), 0, (hipStream_t)s, q);
            MDX_LAUNCH_CHECK(fn);
            return fill_factor_one(fn, factor_out, B, (hipStream_t)s);
        }
        rp.phi = guidance_rescale;
        rp.factor_out = factor_out;
        const RescaleDualParams q{rp, mid};
        hipLaunchKernelGGL(v ? sampler_step_rescale_dual_kernel<MDX_PRED_V> : sampler_step_rescale_dual_kernel<MDX_PRED_EPS>,
                           dim3(B), dim3(RESCALE_THREADS), 0, (hipStream_t)s, q);
        MDX_LAUNCH_CHECK(fn);
        return MDX_OK;
    }
    if (guidance_rescale == 0.f || !out_u) {      // f == 1: the launch of mdx_sampler_step_pred_f32, bit for bit
        rc = sampler_step_run(fn, rp.s, pred_type, s);
        return rc != MDX_OK ? rc : fill_factor_one(fn, factor_out, B, (hipStream_t)s);
    }
    rp.phi = guidance_rescale;
    rp.factor_out = factor_out;
    const auto kernel = v ? sampler_step_rescale_kernel<MDX_PRED_V> : sampler_step_rescale_kernel<MDX_PRED_EPS>;
    hipLaunchKernelGGL(kernel, dim3(B), dim3(RESCALE_THREADS), 0, (hipStream_t)s, rp);
    MDX_LAUNCH_CHECK(fn);
    return MDX_OK;
}

extern "C" int mdx_sampler_step_rescale_f32(const float* x, const float* x_model, const void* out_u, const void* out_c,
                                            int out_ld, float cfg_scale, int pred_type, float sqrt_at_model,
                                            float sqrt_one_minus_at_model, const float* old1, const float* old2,
                                            const float* old3, const float* coef4, float sqrt_at, float sqrt_one_minus_at,
                                            float sqrt_a_prev, float dir_coef, float sigma, const float* noise,
                                            float* e_t_out, float* x_prev, float* pred_x0, float guidance_rescale,
                                            float* factor_out, int B, int C, int H, int W, mdx_stream_t s) {
    return sampler_step_rescale_entry("mdx_sampler_step_rescale_f32", x, x_model, out_u, out_c, out_ld, cfg_scale, pred_type,
                                      sqrt_at_model, sqrt_one_minus_at_model, old1, old2, old3, coef4, sqrt_at,
                                      sqrt_one_minus_at, sqrt_a_prev, dir_coef, sigma, noise, e_t_out, x_prev, pred_x0,
                                      guidance_rescale, factor_out, nullptr, 0.f, B, C, H, W, s);
}

extern "C" int mdx_sampler_step_dual_f32(const float* x, const float* x_model, const void* out_u, const void* out_c, int out_ld,
                                         float cfg_scale, int pred_type, float sqrt_at_model, float sqrt_one_minus_at_model,
                                         const float* old1, const float* old2, const float* old3, const float* coef4,
                                         float sqrt_at, float sqrt_one_minus_at, float sqrt_a_prev, float dir_coef, float sigma,
                                         const float* noise, float* e_t_out, float* x_prev, float* pred_x0,
                                         float guidance_rescale, float* factor_out, const void* out_m, float mid_scale, int B,
                                         int C, int H, int W, mdx_stream_t s) {
    return sampler_step_rescale_entry("mdx_sampler_step_dual_f32", x, x_model, out_u, out_c, out_ld, cfg_scale, pred_type,
                                      sqrt_at_model, sqrt_one_minus_at_model, old1, old2, old3, coef4, sqrt_at,
                                      sqrt_one_minus_at, sqrt_a_prev, dir_coef, sigma, noise, e_t_out, x_prev, pred_x0,
                                      guidance_rescale, factor_out, out_m, mid_scale, B, C, H, W, s);
}

// The table entry and the slot entry (slot_start != nullptr): the pointer and extent checks of the scalar entries on
// coefficients that need none (they live on the device), the limits of the two launch forms, and the history / noise
// pointers as given -- table_row keeps or drops them by the row's coefficient.
static int step_rows_launch(const char* fn, const float* x, const float* x_model, const void* out_u, const void* out_c,
                            int out_ld, int pred_type, const float* old1, const float* old2, const float* old3,
                            const float* noise, float* e_t_out, float* x_prev, float* pred_x0, bool slots, const float* rows,
                            const int* slot_start, const int* slot_len, int cap, int tick, int any_rescale, float* factor_out,
                            int B, int C, int H, int W, mdx_stream_t s) {
    RowParams rp;
    const float no_history[4] = {1.f, 0.f, 0.f, 0.f};
    int rc = sampler_step_params(rp.s, fn, x, x_model, out_u, out_c, out_ld, 1.f, pred_type, 1.f, 0.f, old1, old2, old3,
                                 no_history, 1.f, 0.f, 1.f, 0.f, 0.f, noise, e_t_out, x_prev, pred_x0, B, C, H, W);
    if (rc != MDX_OK) return rc;
    MDX_REQUIRE(!any_rescale || out_u, "%s: any_rescale needs the unconditional output out_u", fn);
    if ((rc = sample_extent_check(fn, (size_t)C * H * W, any_rescale != 0)) != MDX_OK) return rc;
    MDX_REQUIRE(any_rescale || B <= 65535, "%s: bad extents (B exceeds 65535 samples)", fn);
    if (slots) {
        MDX_REQUIRE(rows && slot_start && slot_len, "%s: null slot pointer", fn);
        MDX_REQUIRE(cap > 0 && tick >= 0, "%s: bad slot extents (cap=%d tick=%d; cap > 0, tick >= 0)", fn, cap, tick);
    } else {
        MDX_REQUIRE(rows, "%s: null table", fn);
    }
    rp.s.old1 = old1;
    rp.s.old2 = old2;
    rp.s.old3 = old3;
    rp.s.noise = noise;
    rp.rows = rows;
    rp.slot_start = slot_start;
    rp.slot_len = slot_len;
    rp.cap = cap;
    rp.tick = tick;
    rp.factor_out = factor_out;
    const hipStream_t st = (hipStream_t)s;
    const bool v = pred_type == MDX_PRED_V;
    if (any_rescale) {
        const auto kernel = v ? sampler_step_rows_owned_kernel<MDX_PRED_V> : sampler_step_rows_owned_kernel<MDX_PRED_EPS>;
        hipLaunchKernelGGL(kernel, dim3(B), dim3(RESCALE_THREADS), 0, st, rp);
    } else {      // the workgroups of sampler_step_kernel's grid for the same batch, dealt to the samples
        const auto kernel = v ? sampler_step_rows_kernel<MDX_PRED_V> : sampler_step_rows_kernel<MDX_PRED_EPS>;
        hipLaunchKernelGGL(kernel, dim3((grid_for((size_t)B * C * H * W) + B - 1) / B, B), dim3(256), 0, st, rp);
    }
    MDX_LAUNCH_CHECK(fn);
    return MDX_OK;
}

extern "C" int mdx_sampler_step_table_f32(const float* x, const float* x_model, const void* out_u, const void* out_c,
                                          int out_ld, int pred_type, const float* old1, const float* old2,
                                          const float* old3, const float* noise, float* e_t_out, float* x_prev,
                                          float* pred_x0, const float* table, int any_rescale, float* factor_out, int B,
                                          int C, int H, int W, mdx_stream_t s) {
    return step_rows_launch("mdx_sampler_step_table_f32", x, x_model, out_u, out_c, out_ld, pred_type, old1, old2, old3, noise,
                            e_t_out, x_prev, pred_x0, false, table, nullptr, nullptr, 0, 0, any_rescale, factor_out, B, C, H, W, s);
}

extern "C" int mdx_sampler_step_slots_f32(const float* x, const float* x_model, const void* out_u, const void* out_c,
                                          int out_ld, int pred_type, const float* old1, const float* old2,
                                          const float* old3, const float* noise, float* e_t_out, float* x_prev,
                                          float* pred_x0, const float* sched, const int* slot_start, const int* slot_len,
                                          int cap, int tick, int any_rescale, float* factor_out, int B, int C, int H, int W,
                                          mdx_stream_t s) {
    return step_rows_launch("mdx_sampler_step_slots_f32", x, x_model, out_u, out_c, out_ld, pred_type, old1, old2, old3, noise,
                            e_t_out, x_prev, pred_x0, true, sched, slot_start, slot_len, cap, tick, any_rescale, factor_out, B, C, H, W, s);
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

// nz == nullptr: the kernels mdx_sampler_step_lin_f32 has always launched.  mid: the DUAL instantiations, same grids.
template <int PRED, int VALUE>
static void sampler_step_lin_run(const LinParams& p, const LinNoise* nz, const GuidedMid* mid, bool owned, hipStream_t st) {
    const dim3 own_grid(p.B), own_block(RESCALE_THREADS);
    if (mid) {
        const LinDualParams d{p, nz ? *nz : LinNoise{}, *mid};
        const int noise = !nz ? LIN_NOISE_NONE : nz->seeds ? LIN_NOISE_SEEDED : LIN_NOISE_TENSOR;
        const size_t ditems = (size_t)p.B * (((size_t)p.g.C * p.g.HW + 3) / 4);
        const size_t dblocks = (ditems + LIN_NOISE_THREADS - 1) / LIN_NOISE_THREADS;
        const dim3 dgrid((unsigned)(dblocks > 8192 ? 8192 : dblocks)), dblock(LIN_NOISE_THREADS);
        if (owned) {
            if (noise == LIN_NOISE_NONE)
                hipLaunchKernelGGL((sampler_step_lin_owned_kernel<PRED, VALUE, LIN_NOISE_NONE, LinDualParams>), own_grid, own_block, 0, st, d);
            else if (noise == LIN_NOISE_SEEDED)
                hipLaunchKernelGGL((sampler_step_lin_owned_kernel<PRED, VALUE, LIN_NOISE_SEEDED, LinDualParams>), own_grid, own_block, 0, st, d);
            else
                hipLaunchKernelGGL((sampler_step_lin_owned_kernel<PRED, VALUE, LIN_NOISE_TENSOR, LinDualParams>), own_grid, own_block, 0, st, d);
        } else if (noise == LIN_NOISE_NONE) {
            hipLaunchKernelGGL((sampler_step_lin_dual_kernel<PRED, VALUE>), dim3(grid_for((size_t)p.B * p.g.C * p.g.HW)), dim3(256), 0, st, d);
        } else if (noise == LIN_NOISE_SEEDED) {
            hipLaunchKernelGGL((sampler_step_lin_noise_dual_kernel<PRED, VALUE, LIN_NOISE_SEEDED>), dgrid, dblock, 0, st, d);
        } else {
            hipLaunchKernelGGL((sampler_step_lin_noise_dual_kernel<PRED, VALUE, LIN_NOISE_TENSOR>), dgrid, dblock, 0, st, d);
        }
        return;
    }
    if (!nz) {
        if (owned)
            hipLaunchKernelGGL((sampler_step_lin_owned_kernel<PRED, VALUE, LIN_NOISE_NONE, LinParams>), own_grid, own_block, 0, st, p);
        else
            hipLaunchKernelGGL((sampler_step_lin_kernel<PRED, VALUE>), dim3(grid_for((size_t)p.B * p.g.C * p.g.HW)), dim3(256), 0, st, p);
        return;
    }
    const LinNoiseParams q{p, *nz};
    const size_t items = (size_t)p.B * (((size_t)p.g.C * p.g.HW + 3) / 4);
    const size_t blocks = (items + LIN_NOISE_THREADS - 1) / LIN_NOISE_THREADS;
    const dim3 grid((unsigned)(blocks > 8192 ? 8192 : blocks)), block(LIN_NOISE_THREADS);
    if (nz->seeds) {
        if (owned)
            hipLaunchKernelGGL((sampler_step_lin_owned_kernel<PRED, VALUE, LIN_NOISE_SEEDED, LinNoiseParams>), own_grid, own_block, 0, st, q);
        else
            hipLaunchKernelGGL((sampler_step_lin_noise_kernel<PRED, VALUE, LIN_NOISE_SEEDED>), grid, block, 0, st, q);
    } else {
        if (owned)
            hipLaunchKernelGGL((sampler_step_lin_owned_kernel<PRED, VALUE, LIN_NOISE_TENSOR, LinNoiseParams>), own_grid, own_block, 0, st, q);
        else
            hipLaunchKernelGGL((sampler_step_lin_noise_kernel<PRED, VALUE, LIN_NOISE_TENSOR>), grid, block, 0, st, q);
    }
}

// What every entry of the lin family and the pc entry refuse about steps 1-6, in this order; pointers_ok / histories_ok: the
// entry's own required pointers and (coefficient, history) pairs.
static int lin_value_checks(const char* fn, bool pointers_ok, bool histories_ok, const void* out_u, int out_ld, int pred_type,
                            float guidance_rescale, int value_type, float alpha_m, int thresholding, float max_val,
                            const void* out_m, float mid_scale, int B, int C, int H, int W) {
    MDX_REQUIRE(pred_type == MDX_PRED_EPS || pred_type == MDX_PRED_V, "%s: unknown pred_type %d", fn, pred_type);
    MDX_REQUIRE(value_type == MDX_VALUE_X0 || value_type == MDX_VALUE_EPS, "%s: unknown value_type %d", fn, value_type);
    MDX_REQUIRE(pointers_ok, "%s: null pointer", fn);
    MDX_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0 && out_ld >= C, "%s: bad extents", fn);
    const size_t N = (size_t)C * H * W;
    int rc = sample_extent_check(fn, N, false);
    if (rc != MDX_OK) return rc;
    MDX_REQUIRE(histories_ok, "%s: non-zero history coefficient without its model value", fn);
    MDX_REQUIRE(value_type != MDX_VALUE_X0 || alpha_m != 0.f, "%s: alpha_m == 0 (the data prediction divides by it)", fn);
    MDX_REQUIRE(guidance_rescale >= 0.f && guidance_rescale <= 1.f, "%s: guidance_rescale %g is not in [0, 1]", fn,
                (double)guidance_rescale);
    if ((rc = sample_extent_check(fn, N, guidance_rescale != 0.f && out_u)) != MDX_OK) return rc;
    if (out_m && (rc = guided_mid_check(fn, out_u, mid_scale)) != MDX_OK) return rc;
    if (thresholding) {
        MDX_REQUIRE(value_type == MDX_VALUE_X0, "%s: thresholding acts on a data prediction (MDX_VALUE_X0)", fn);
        MDX_REQUIRE(N >= 2, "%s: thresholding needs two order statistics, C * H * W >= 2", fn);
        MDX_REQUIRE(max_val > 0.f && max_val <= 3.402823466e38f, "%s: max_val %g is not a finite positive number", fn,
                    (double)max_val);
    }
    return MDX_OK;
}

// Both entries: nz == nullptr is mdx_sampler_step_lin_f32's launch, kernel for kernel (the noise entry passes it for cn == 0).
static int sampler_step_lin_entry(const char* fn, const float* x_base, const float* x_model, const void* out_u,
                                  const void* out_c, int out_ld, float cfg_scale, int pred_type, float guidance_rescale,
                                  int value_type, float alpha_m, float sigma_m, int thresholding, float max_val, const float* h1,
                                  const float* h2, float A, float c0, float c1, float c2, float* model_out, float* x_out,
                                  float* model_pre_out, float* thr_out, float* factor_out, const LinNoise* nz,
                                  const void* out_m, float mid_scale, int B, int C, int H, int W, mdx_stream_t s) {
    const size_t N = (size_t)C * H * W;
    int rc = lin_value_checks(fn, x_base && x_model && out_c && model_out && x_out, (c1 == 0.f || h1) && (c2 == 0.f || h2), out_u,
                              out_ld, pred_type, guidance_rescale, value_type, alpha_m, thresholding, max_val, out_m, mid_scale,
                              B, C, H, W);
    if (rc != MDX_OK) return rc;
    const bool rescale = guidance_rescale != 0.f && out_u;
    // the only aliases: x_out == x_base, x_out == x_model.  An input whose term is skipped is not read and may lie anywhere.
    const size_t nx = (size_t)B * N * sizeof(float), nh = (((size_t)B * H * W - 1) * out_ld + C) * sizeof(f16);
    const struct { const void* ptr; size_t bytes; const char* name; } outs[] = {
        {model_out, nx, "model_out"}, {x_out, nx, "x_out"}, {model_pre_out, nx, "model_pre_out"},
        {thr_out, B * sizeof(float), "thr_out"}, {factor_out, B * sizeof(float), "factor_out"}},
      ins[] = {{A != 0.f ? x_base : nullptr, nx, "x_base"}, {x_model, nx, "x_model"}, {out_u, nh, "out_u"}, {out_c, nh, "out_c"},
               {out_m, nh, "out_m"},
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
    p.g = GuidedPair{(const f16*)out_u, (const f16*)out_c, out_ld, C, H * W, cfg_scale};
    p.x_base = x_base;
    p.x_model = x_model;
    p.h1 = c1 != 0.f ? h1 : nullptr;
    p.h2 = c2 != 0.f ? h2 : nullptr;
    p.model_out = model_out;
    p.x_out = x_out;
    p.model_pre_out = model_pre_out;
    p.thr_out = thr_out;
    p.factor_out = factor_out;
    p.B = B;
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
    const auto run = pred_type == MDX_PRED_V
                         ? (value_type == MDX_VALUE_X0 ? sampler_step_lin_run<MDX_PRED_V, MDX_VALUE_X0> : sampler_step_lin_run<MDX_PRED_V, MDX_VALUE_EPS>)
                         : (value_type == MDX_VALUE_X0 ? sampler_step_lin_run<MDX_PRED_EPS, MDX_VALUE_X0> : sampler_step_lin_run<MDX_PRED_EPS, MDX_VALUE_EPS>);
    const GuidedMid mid{(const f16*)out_m, mid_scale};
    run(p, nz, out_m ? &mid : nullptr, owned, st);
    MDX_LAUNCH_CHECK(fn);
    return owned ? MDX_OK : fill_factor_one(fn, factor_out, B, st);      // f == 1 everywhere, as mdx_sampler_step_rescale_f32 reports it
}

extern "C" int mdx_sampler_step_lin_f32(const float* x_base, const float* x_model, const void* out_u, const void* out_c,
                                        int out_ld, float cfg_scale, int pred_type, float guidance_rescale, int value_type,
                                        float alpha_m, float sigma_m, int thresholding, float max_val, const float* h1,
                                        const float* h2, float A, float c0, float c1, float c2, float* model_out,
                                        float* x_out, float* model_pre_out, float* thr_out, float* factor_out, int B, int C,
                                        int H, int W, mdx_stream_t s) {
    return sampler_step_lin_entry("mdx_sampler_step_lin_f32", x_base, x_model, out_u, out_c, out_ld, cfg_scale, pred_type,
                                  guidance_rescale, value_type, alpha_m, sigma_m, thresholding, max_val, h1, h2, A, c0, c1, c2,
                                  model_out, x_out, model_pre_out, thr_out, factor_out, nullptr, nullptr, 0.f, B, C, H, W, s);
}

// The noise entry and its DUAL superset: out_m == nullptr is the two-branch body, launch for launch.
static int sampler_step_lin_noise_entry(const char* fn, const float* x_base, const float* x_model, const void* out_u,
                                        const void* out_c, int out_ld, float cfg_scale, int pred_type, float guidance_rescale,
                                        int value_type, float alpha_m, float sigma_m, int thresholding, float max_val,
                                        const float* h1, const float* h2, float A, float c0, float c1, float c2,
                                        float* model_out, float* x_out, float* model_pre_out, float* thr_out, float* factor_out,
                                        float cn, const float* noise, const unsigned long long* seeds, unsigned stream,
                                        unsigned draw, const void* out_m, float mid_scale, int B, int C, int H, int W,
                                        mdx_stream_t s) {
    MDX_REQUIRE(cn >= -3.402823466e38f && cn <= 3.402823466e38f, "%s: cn %g is not finite", fn, (double)cn);
    MDX_REQUIRE(stream < DROPOUT_STREAM_BIT, "%s: stream %u is not below 2^31", fn, stream);
    MDX_REQUIRE(cn == 0.f || ((noise != nullptr) != (seeds != nullptr)),
                "%s: cn != 0 takes exactly one noise source, noise or seeds (got %s)", fn, noise ? "both" : "neither");
    const LinNoise nz{cn, noise, noise ? nullptr : seeds, stream, draw};
    return sampler_step_lin_entry(fn, x_base, x_model, out_u, out_c, out_ld, cfg_scale, pred_type, guidance_rescale, value_type,
                                  alpha_m, sigma_m, thresholding, max_val, h1, h2, A, c0, c1, c2, model_out, x_out,
                                  model_pre_out, thr_out, factor_out, cn != 0.f ? &nz : nullptr, out_m, mid_scale, B, C, H, W, s);
}

extern "C" int mdx_sampler_step_lin_noise_f32(const float* x_base, const float* x_model, const void* out_u, const void* out_c,
                                              int out_ld, float cfg_scale, int pred_type, float guidance_rescale,
                                              int value_type, float alpha_m, float sigma_m, int thresholding, float max_val,
                                              const float* h1, const float* h2, float A, float c0, float c1, float c2,
                                              float* model_out, float* x_out, float* model_pre_out, float* thr_out,
                                              float* factor_out, float cn, const float* noise, const unsigned long long* seeds,
                                              unsigned stream, unsigned draw, int B, int C, int H, int W, mdx_stream_t s) {
    return sampler_step_lin_noise_entry("mdx_sampler_step_lin_noise_f32", x_base, x_model, out_u, out_c, out_ld, cfg_scale,
                                        pred_type, guidance_rescale, value_type, alpha_m, sigma_m, thresholding, max_val, h1, h2,
                                        A, c0, c1, c2, model_out, x_out, model_pre_out, thr_out, factor_out, cn, noise, seeds,
                                        stream, draw, nullptr, 0.f, B, C, H, W, s);
}

extern "C" int mdx_sampler_step_lin_dual_f32(const float* x_base, const float* x_model, const void* out_u, const void* out_c,
                                             int out_ld, float cfg_scale, int pred_type, float guidance_rescale,
                                             int value_type, float alpha_m, float sigma_m, int thresholding, float max_val,
                                             const float* h1, const float* h2, float A, float c0, float c1, float c2,
                                             float* model_out, float* x_out, float* model_pre_out, float* thr_out,
                                             float* factor_out, float cn, const float* noise, const unsigned long long* seeds,
                                             unsigned stream, unsigned draw, const void* out_m, float mid_scale, int B, int C,
                                             int H, int W, mdx_stream_t s) {
    return sampler_step_lin_noise_entry("mdx_sampler_step_lin_dual_f32", x_base, x_model, out_u, out_c, out_ld, cfg_scale,
                                        pred_type, guidance_rescale, value_type, alpha_m, sigma_m, thresholding, max_val, h1, h2,
                                        A, c0, c1, c2, model_out, x_out, model_pre_out, thr_out, factor_out, cn, noise, seeds,
                                        stream, draw, out_m, mid_scale, B, C, H, W, s);
}

// ---- mdx_sampler_step_pc_f32
extern "C" int mdx_sampler_step_pc_f32(const float* x_base, const float* x_model, const void* out_u, const void* out_c,
                                       int out_ld, float cfg_scale, int pred_type, float guidance_rescale, int value_type,
                                       float alpha_m, float sigma_m, int thresholding, float max_val, const float* h1,
                                       const float* h2, const float* h3, int has_corrector, float Ac, float d0, float d1,
                                       float d2, float d3, float Ap, float e0, float e1, float e2, float* model_out,
                                       float* x_corr_out, float* x_pred_out, float* model_pre_out, float* thr_out,
                                       float* factor_out, int B, int C, int H, int W, mdx_stream_t s) {
    const char* fn = "mdx_sampler_step_pc_f32";
    if (!has_corrector) Ac = d0 = d1 = d2 = d3 = 0.f;      // not read
    const bool r1 = d1 != 0.f || e1 != 0.f, r2 = d2 != 0.f || e2 != 0.f, r3 = d3 != 0.f;
    const size_t N = (size_t)C * H * W;
    int rc = lin_value_checks(fn, x_model && out_c && model_out && x_corr_out && x_pred_out, (!r1 || h1) && (!r2 || h2) && (!r3 || h3),
                              out_u, out_ld, pred_type, guidance_rescale, value_type, alpha_m, thresholding, max_val, nullptr,
                              0.f, B, C, H, W);
    if (rc != MDX_OK) return rc;
    MDX_REQUIRE(!has_corrector || x_base, "%s: has_corrector without x_base (the latent the corrector starts from)", fn);
    const bool rescale = guidance_rescale != 0.f && out_u;
    // the only aliases: x_corr_out == x_base, x_pred_out == x_model.  An input whose term is skipped is not read.
    const size_t nx = (size_t)B * N * sizeof(float), nh = (((size_t)B * H * W - 1) * out_ld + C) * sizeof(f16);
    const struct { const void* ptr; size_t bytes; const char* name; } outs[] = {
        {x_corr_out, nx, "x_corr_out"}, {x_pred_out, nx, "x_pred_out"}, {model_out, nx, "model_out"},
        {model_pre_out, nx, "model_pre_out"}, {thr_out, B * sizeof(float), "thr_out"}, {factor_out, B * sizeof(float), "factor_out"}},
      ins[] = {{has_corrector && Ac != 0.f ? x_base : nullptr, nx, "x_base"}, {x_model, nx, "x_model"}, {out_u, nh, "out_u"},
               {out_c, nh, "out_c"}, {r1 ? h1 : nullptr, nx, "h1"}, {r2 ? h2 : nullptr, nx, "h2"}, {r3 ? h3 : nullptr, nx, "h3"}};
    for (size_t o = 0; o < sizeof(outs) / sizeof(outs[0]); ++o) {
        for (size_t i = 0; i < sizeof(ins) / sizeof(ins[0]); ++i) {
            const bool allowed = o == i && o < 2 && outs[o].ptr == ins[i].ptr;
            MDX_REQUIRE(allowed || !bytes_overlap(outs[o].ptr, outs[o].bytes, ins[i].ptr, ins[i].bytes),
                        "%s: %s overlaps %s (only x_corr_out may alias x_base and x_pred_out x_model, element for element)", fn,
                        outs[o].name, ins[i].name);
        }
        for (size_t q = o + 1; q < sizeof(outs) / sizeof(outs[0]); ++q)
            MDX_REQUIRE(!bytes_overlap(outs[o].ptr, outs[o].bytes, outs[q].ptr, outs[q].bytes), "%s: %s overlaps %s", fn,
                        outs[o].name, outs[q].name);
    }
    PcParams q{};
    LinParams& c = q.c;
    c.g = GuidedPair{(const f16*)out_u, (const f16*)out_c, out_ld, C, H * W, cfg_scale};
    c.x_base = x_base;
    c.x_model = x_model;
    c.h1 = d1 != 0.f ? h1 : nullptr;
    c.h2 = d2 != 0.f ? h2 : nullptr;
    c.model_out = model_out;
    c.x_out = x_corr_out;
    c.model_pre_out = model_pre_out;
    c.thr_out = thr_out;
    c.factor_out = factor_out;
    c.B = B;
    c.am = alpha_m;
    c.sm = sigma_m;
    c.A = Ac;
    c.c0 = d0;
    c.c1 = d1;
    c.c2 = d2;
    c.phi = rescale ? guidance_rescale : 0.f;
    c.max_val = max_val;
    c.k = (unsigned)((double)(N - 1) * 0.995);
    c.thresholding = thresholding != 0;
    q.p.h1 = e1 != 0.f ? h1 : nullptr;
    q.p.h2 = e2 != 0.f ? h2 : nullptr;
    q.p.x_out = x_pred_out;
    q.p.A = Ap;
    q.p.c0 = e0;
    q.p.c1 = e1;
    q.p.c2 = e2;
    q.h1 = r1 ? h1 : nullptr;
    q.h2 = r2 ? h2 : nullptr;
    q.h3 = r3 ? h3 : nullptr;
    q.d3 = d3;
    q.has_corrector = has_corrector != 0;
    const bool owned = rescale || c.thresholding;
    const bool v = pred_type == MDX_PRED_V, x0 = value_type == MDX_VALUE_X0;
    hipStream_t st = (hipStream_t)s;
    if (owned) {
        const auto kernel = v ? (x0 ? sampler_step_pc_owned_kernel<MDX_PRED_V, MDX_VALUE_X0> : sampler_step_pc_owned_kernel<MDX_PRED_V, MDX_VALUE_EPS>)
                              : (x0 ? sampler_step_pc_owned_kernel<MDX_PRED_EPS, MDX_VALUE_X0> : sampler_step_pc_owned_kernel<MDX_PRED_EPS, MDX_VALUE_EPS>);
        hipLaunchKernelGGL(kernel, dim3(B), dim3(RESCALE_THREADS), 0, st, q);
    } else {
        const auto kernel = v ? (x0 ? sampler_step_pc_kernel<MDX_PRED_V, MDX_VALUE_X0> : sampler_step_pc_kernel<MDX_PRED_V, MDX_VALUE_EPS>)
                              : (x0 ? sampler_step_pc_kernel<MDX_PRED_EPS, MDX_VALUE_X0> : sampler_step_pc_kernel<MDX_PRED_EPS, MDX_VALUE_EPS>);
        hipLaunchKernelGGL(kernel, dim3(grid_for((size_t)B * N)), dim3(256), 0, st, q);
    }
    MDX_LAUNCH_CHECK(fn);
    return owned ? MDX_OK : fill_factor_one(fn, factor_out, B, st);
}
