// Separable resampling of NCHW fp32 planes (include/mdx.h: mdx_resample_f32 / mdx_resample_noised_f32): the enlargement between
// the two passes of DiffusionPipeline.hires, and every other resize the pipeline needs on the device.  One table-driven kernel:
// the interpolation mode never reaches the device, only tap tables do (minddiffusion_amd/resample.py builds them in float64).
//
// The arithmetic, fixed here.  For output element (i, j) of a plane, with e() the edge rule of the axis (columns: clamp to
// [0, W_in - 1], or with wrap_x the index mod W_in, non-negative; rows: always clamp to [0, H_in - 1]):
//   1. horizontal, for every input row r the element needs:  t_r = 0; for k = 0 .. Tx - 1 ascending:
//        t_r = fmaf(x_w[j][k], in[r][e(x_start[j] + k)], t_r)
//   2. t_r stays fp32 (it is staged in LDS, never rounded to anything narrower)
//   3. vertical:  v = 0; for k = 0 .. Ty - 1 ascending:  v = fmaf(y_w[i][k], t_{e(y_start[i] + k)}, v)
//   4. no atomics; an output element depends on its own sample and plane only -- not on the batch, not on the tile that holds it,
//      not on the store width.
// The noised form continues with z0 = scale * v (one multiply) and xt = q_sample_f(z0, n, a, b), n a passed noise element or the
// value quad_values<MODE_NORMAL> (rng_device.h) gives the element's NCHW index inside its OUTPUT sample.
//
// Launch form: one launch, grid (column tiles, row tiles, B * C), 256 threads.  A block owns a 16 x 32 tile of outputs of one
// plane.  It copies the tile's slices of the four tables into LDS, stages the horizontally resampled strip -- the input rows
// min_i e(y_start[i]) .. max_i e(y_start[i] + Ty - 1) of the tile's rows, at the tile's 32 output columns -- in LDS, and runs the
// vertical pass from it.  Lanes walk the columns in both passes: LDS rows are 32 consecutive dwords, no bank conflicts.
// LDS: 6.2 KiB of tables at 32 taps plus 128 bytes per strip row, capped at RS_LDS_BUDGET = 40 KiB -- four blocks stay resident on
// a CU's 160 KiB.  A latent makes a few hundred blocks at most, so the launch is latency-bound; nothing here is pipelined.
// The strip holds `cap` rows, which the host sizes from the geometry: ceil(15 * H_in / H_out) + Ty + 2 (at most H_in).  Tables of
// resample.tap_table stay inside it (tests/test_resample_cpu.py checks every tile); for any other table the kernel clamps the row
// it reads into the strip, so a malformed table gives wrong values, never an access outside LDS or `in`.
#include "mdx_common.h"
#include "qsample_device.h"
#include "rng_device.h"

namespace {

constexpr int RS_TH = 16, RS_TW = 32;       // output tile: rows x columns
constexpr int RS_THREADS = 256;
constexpr size_t RS_LDS_BUDGET = 40 * 1024;

struct ResampleParams {
    const float* in;            // [B][C][H_in][W_in]
    float* out;                 // plain form: [B][C][H_out][W_out]
    int C, H_in, W_in, H_out, W_out;
    const int* y_start;
    const float* y_w;
    const int* x_start;
    const float* x_w;
    int Ty, Tx, wrap_x, cap;
    // the noised form
    float scale, a, b;
    const float* noise;         // [B][C][H_out][W_out] or NULL: drawn from r
    float* z0_out;
    float* xt_out;
    RngParams r;                // seeds, stream, draw; scale 1, no dropout
};

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

inline bool overlaps(const void* p, size_t pbytes, const void* q, size_t qbytes) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + qbytes && b < a + pbytes;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// V outputs of one row per item (V == 4 needs W_out % 4 == 0 and 16-byte aligned outputs and noise: the host decides)
template <int V, bool NOISED>
__global__ __launch_bounds__(RS_THREADS) void resample_kernel(const ResampleParams p) {
    extern __shared__ float rs_lds[];
    float* xw = rs_lds;                                     // [RS_TW][Tx]
    float* yw = xw + RS_TW * p.Tx;                          // [RS_TH][Ty]
    int* xs = reinterpret_cast<int*>(yw + RS_TH * p.Ty);    // [RS_TW]
    int* ys = xs + RS_TW;                                   // [RS_TH]
    float* strip = reinterpret_cast<float*>(ys + RS_TH);    // [cap][RS_TW]
    const int x0 = blockIdx.x * RS_TW, y0 = blockIdx.y * RS_TH;
    const int tw = min(RS_TW, p.W_out - x0), th = min(RS_TH, p.H_out - y0);
    const int tid = threadIdx.x;
    const size_t plane = blockIdx.z;
    const float* src = p.in + plane * p.H_in * p.W_in;

    // the tile's slices of the tables.  A start is brought into the range where e() still tells its taps apart -- the same
    // element for every tap, and no index arithmetic below can overflow: [-T, L - 1] for a clamped axis, [0, W_in) with wrap_x.
    for (int t = tid; t < tw * p.Tx; t += RS_THREADS) xw[t] = p.x_w[(size_t)x0 * p.Tx + t];
    for (int t = tid; t < th * p.Ty; t += RS_THREADS) yw[t] = p.y_w[(size_t)y0 * p.Ty + t];
    if (tid < tw) {
        const int st = p.x_start[x0 + tid];
        const int m = st % p.W_in;
        xs[tid] = p.wrap_x ? (m < 0 ? m + p.W_in : m) : clampi(st, -p.Tx, p.W_in - 1);
    }
    if (tid < th) ys[tid] = clampi(p.y_start[y0 + tid], -p.Ty, p.H_in - 1);
    __syncthreads();

    // the input rows the tile needs (every lane computes the same two numbers from LDS)
    int rmin = p.H_in - 1, rmax = 0;
    for (int i = 0; i < th; ++i) {
        rmin = min(rmin, max(ys[i], 0));
        rmax = max(rmax, min(ys[i] + p.Ty - 1, p.H_in - 1));
    }
    const int nrows = clampi(rmax - rmin + 1, 1, p.cap);

    // horizontal pass into the strip
    for (int t = tid; t < nrows * RS_TW; t += RS_THREADS) {
        const int r = t / RS_TW, c = t - r * RS_TW;
        if (c >= tw) continue;
        const float* row = src + (size_t)(rmin + r) * p.W_in;
        const float* w = xw + c * p.Tx;
        const int st = xs[c];
        float acc = 0.0f;
        for (int k = 0; k < p.Tx; ++k) {
            const int gx = p.wrap_x ? (st + k) % p.W_in : clampi(st + k, 0, p.W_in - 1);
            acc = __builtin_fmaf(w[k], row[gx], acc);
        }
        strip[t] = acc;
    }
    __syncthreads();

    // vertical pass from the strip, and the outputs
    const size_t hw_out = (size_t)p.H_out * p.W_out;
    for (int t = tid; t < RS_TH * RS_TW / V; t += RS_THREADS) {
        const int r = t / (RS_TW / V), c0 = (t - r * (RS_TW / V)) * V;
        if (r >= th || c0 >= tw) continue;
        const float* w = yw + r * p.Ty;
        const int st = ys[r];
        float v[V];
#pragma unroll
        for (int e = 0; e < V; ++e) v[e] = 0.0f;
        for (int k = 0; k < p.Ty; ++k) {
            const int rr = clampi(clampi(st + k, 0, p.H_in - 1) - rmin, 0, nrows - 1);
            const float wk = w[k];
#pragma unroll
            for (int e = 0; e < V; ++e) v[e] = __builtin_fmaf(wk, strip[rr * RS_TW + c0 + e], v[e]);
        }
        const size_t in_plane = (size_t)(y0 + r) * p.W_out + (x0 + c0);
        const size_t at = plane * hw_out + in_plane;
        if constexpr (!NOISED) {
            store_v<V>(p.out + at, v);
        } else {
            float z0[V];
#pragma unroll
            for (int e = 0; e < V; ++e) z0[e] = p.scale * v[e];
            if (p.z0_out) store_v<V>(p.z0_out + at, z0);
            if (p.xt_out) {
                float nz[V], xt[V];
                if (p.noise) {
                    load_v<V>(p.noise + at, nz);
                } else {
                    const size_t b = plane / p.C, c = plane - b * p.C;
                    const size_t el = c * hw_out + in_plane;        // the NCHW index inside the output sample
                    unsigned bits[4];
                    quad_values<MODE_NORMAL>(p.r, p.r.seeds[b], p.r.draw, (unsigned)(el >> 2), bits);
                    if constexpr (V == 4) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) nz[e] = __uint_as_float(bits[e]);
                    } else {
                        const int lane = (int)(el & 3);
                        nz[0] = __uint_as_float(lane == 0 ? bits[0] : lane == 1 ? bits[1] : lane == 2 ? bits[2] : bits[3]);
                    }
                }
#pragma unroll
                for (int e = 0; e < V; ++e) xt[e] = q_sample_f(z0[e], nz[e], p.a, p.b);
                store_v<V>(p.xt_out + at, xt);
            }
        }
    }
}

// Every check both entries share, and the launch geometry: MDX_OK with `lds` and `grid` filled, or MDX_E_INVALID.
int resample_plan(const char* fn, ResampleParams& p, int B, size_t* lds, dim3* grid) {
    MDX_REQUIRE(p.in && p.y_start && p.y_w && p.x_start && p.x_w, "%s: null pointer", fn);
    MDX_REQUIRE(B > 0 && p.C > 0 && p.H_in > 0 && p.W_in > 0 && p.H_out > 0 && p.W_out > 0,
                "%s: bad extents (B=%d C=%d H_in=%d W_in=%d H_out=%d W_out=%d)", fn, B, p.C, p.H_in, p.W_in, p.H_out, p.W_out);
    MDX_REQUIRE((long long)p.H_in * p.W_in <= (1LL << 30) && (long long)p.H_out * p.W_out <= (1LL << 30),
                "%s: bad extents (a plane of more than 2^30 pixels)", fn);
    MDX_REQUIRE(p.Tx >= 1 && p.Tx <= MDX_RESAMPLE_MAX_TAPS && p.Ty >= 1 && p.Ty <= MDX_RESAMPLE_MAX_TAPS,
                "%s: Tx and Ty must be in [1, %d], got Tx=%d Ty=%d", fn, MDX_RESAMPLE_MAX_TAPS, p.Tx, p.Ty);
    const int tiles_x = (p.W_out + RS_TW - 1) / RS_TW, tiles_y = (p.H_out + RS_TH - 1) / RS_TH;
    MDX_REQUIRE(tiles_y <= 65535 && (long long)B * p.C <= 65535,
                "%s: bad extents (grid: %d tile rows, %lld planes; at most 65535 each)", fn, tiles_y, (long long)B * p.C);
    const long long need = ((long long)(RS_TH - 1) * p.H_in + p.H_out - 1) / p.H_out + p.Ty + 2;
    p.cap = (int)(need < p.H_in ? need : p.H_in);
    *lds = ((size_t)RS_TW * p.Tx + (size_t)RS_TH * p.Ty + RS_TW + RS_TH + (size_t)p.cap * RS_TW) * sizeof(float);
    MDX_REQUIRE(*lds <= RS_LDS_BUDGET,
                "%s: a %d-row output tile needs a strip of %d input rows, %zu bytes of LDS with its tables; the kernel keeps a "
                "block under %zu (H_in=%d -> H_out=%d is a very large downscale: resample in two steps)",
                fn, RS_TH, p.cap, *lds, RS_LDS_BUDGET, p.H_in, p.H_out);
    *grid = dim3(tiles_x, tiles_y, B * p.C);
    return MDX_OK;
}

}  // namespace

extern "C" int mdx_resample_f32(const float* in, float* out, int B, int C, int H_in, int W_in, int H_out, int W_out,
                                const int* y_start, const float* y_w, int Ty, const int* x_start, const float* x_w, int Tx,
                                int wrap_x, mdx_stream_t s) {
    const char* fn = "mdx_resample_f32";
    MDX_REQUIRE(out, "%s: null pointer", fn);
    ResampleParams p = {};
    p.in = in; p.out = out;
    p.C = C; p.H_in = H_in; p.W_in = W_in; p.H_out = H_out; p.W_out = W_out;
    p.y_start = y_start; p.y_w = y_w; p.x_start = x_start; p.x_w = x_w;
    p.Ty = Ty; p.Tx = Tx; p.wrap_x = wrap_x != 0;
    size_t lds;
    dim3 grid;
    if (const int rc = resample_plan(fn, p, B, &lds, &grid)) return rc;
    const size_t planes = (size_t)B * C;
    MDX_REQUIRE(!overlaps(out, planes * H_out * W_out * sizeof(float), in, planes * H_in * W_in * sizeof(float)),
                "%s: out overlaps in", fn);
    if (W_out % 4 == 0 && aligned16(out))
        hipLaunchKernelGGL((resample_kernel<4, false>), grid, dim3(RS_THREADS), lds, (hipStream_t)s, p);
    else
        hipLaunchKernelGGL((resample_kernel<1, false>), grid, dim3(RS_THREADS), lds, (hipStream_t)s, p);
    MDX_LAUNCH_CHECK(fn);
    return MDX_OK;
}

extern "C" int mdx_resample_noised_f32(const float* in, int B, int C, int H_in, int W_in, int H_out, int W_out, const int* y_start,
                                       const float* y_w, int Ty, const int* x_start, const float* x_w, int Tx, int wrap_x,
                                       float scale, float a, float b, const float* noise, const unsigned long long* seeds,
                                       unsigned stream, unsigned draw, float* z0_out, float* xt_out, mdx_stream_t s) {
    const char* fn = "mdx_resample_noised_f32";
    MDX_REQUIRE(z0_out || xt_out, "%s: no output (z0_out and xt_out are both null)", fn);
    MDX_REQUIRE(!xt_out || noise || seeds, "%s: xt_out needs a noise source (a noise tensor, or seeds)", fn);
    ResampleParams p = {};
    p.in = in;
    p.C = C; p.H_in = H_in; p.W_in = W_in; p.H_out = H_out; p.W_out = W_out;
    p.y_start = y_start; p.y_w = y_w; p.x_start = x_start; p.x_w = x_w;
    p.Ty = Ty; p.Tx = Tx; p.wrap_x = wrap_x != 0;
    p.scale = scale; p.a = a; p.b = b;
    p.noise = xt_out ? noise : nullptr; p.z0_out = z0_out; p.xt_out = xt_out;
    size_t lds;
    dim3 grid;
    if (const int rc = resample_plan(fn, p, B, &lds, &grid)) return rc;
    MDX_REQUIRE((long long)C * H_out * W_out <= RNG_MAX_N, "%s: bad extents (C * H_out * W_out > 2^34, the generator's limit)", fn);
    p.r.seeds = seeds; p.r.out = nullptr;
    p.r.stream = stream; p.r.draw = draw;
    p.r.scale = 1.0f; p.r.dropout_p = 0.0f; p.r.inv_keep = 1.0f;
    p.r.n = (unsigned long long)C * H_out * W_out; p.r.items = 0;
    p.r.slot_start = p.r.slot_len = nullptr; p.r.tick = 0;
    const size_t planes = (size_t)B * C;
    const size_t ibytes = planes * H_in * W_in * sizeof(float), obytes = planes * H_out * W_out * sizeof(float);
    MDX_REQUIRE(!(z0_out && overlaps(z0_out, obytes, in, ibytes)) && !(xt_out && overlaps(xt_out, obytes, in, ibytes)),
                "%s: an output overlaps in", fn);
    MDX_REQUIRE(!(z0_out && xt_out && overlaps(z0_out, obytes, xt_out, obytes)), "%s: z0_out and xt_out must be different tensors",
                fn);
    MDX_REQUIRE(!(p.noise && ((z0_out && overlaps(z0_out, obytes, p.noise, obytes)) || overlaps(xt_out, obytes, p.noise, obytes))),
                "%s: an output overlaps noise", fn);
    if (W_out % 4 == 0 && (!z0_out || aligned16(z0_out)) && (!xt_out || aligned16(xt_out)) && (!p.noise || aligned16(p.noise)))
        hipLaunchKernelGGL((resample_kernel<4, true>), grid, dim3(RS_THREADS), lds, (hipStream_t)s, p);
    else
        hipLaunchKernelGGL((resample_kernel<1, true>), grid, dim3(RS_THREADS), lds, (hipStream_t)s, p);
    MDX_LAUNCH_CHECK(fn);
    return MDX_OK;
}
