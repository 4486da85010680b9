// Windowed UNet evaluation (MultiDiffusion, Bar-Tal et al. 2023): the two launches around the UNet when a large latent canvas is
// evaluated as a batch of overlapping windows of the trained size.  mdx_window_gather_f32 cuts windows k0 .. k0 + n - 1 out of the
// fp32 NCHW canvas into the UNet's input batch; mdx_window_average_f16 averages the NHWC fp16 outputs of ALL windows back onto the
// canvas, where windows overlap.  Both are memory- and launch-bound: one 16-byte access per lane where the shape allows it,
// one-wave workgroups on a capped grid with a grid-stride loop (as csrc/inpaint.hip).  Every output element has exactly one
// writer: the average is a gather per canvas pixel over its covering windows in ascending window number, no atomics.
// The window offsets are read from a device table [ny + nx] (rows, then columns); the host validates its own copy of the table
// before any launch and the kernels clamp what they read into the canvas, so a table that differs from the validated one can
// mis-place a window but not leave the buffers.
// Regions and wrap-around windows (mdx_window_gather_rows_f32 / mdx_window_average_regions_f16, further down) are kernels of their
// own beside these two: the gather takes a table of window numbers and lets a window run over the right edge of the canvas
// into its left one; the average weighs every (window, region) pair's output by the region's mask at the pixel.
#include "mdx_common.h"

namespace {

constexpr int WN_THREADS = 64;
constexpr int WN_MAX_BLOCKS = 4096;     // 256 CUs x 16 waves; larger tensors take further passes of the grid-stride loop

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

inline bool overlaps(const void* p, size_t pbytes, const void* q, size_t qbytes) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + qbytes && b < a + pbytes;
}

inline int wn_blocks(size_t items) {
    const size_t blocks = (items + WN_THREADS - 1) / WN_THREADS;
    return (int)(blocks < (size_t)WN_MAX_BLOCKS ? blocks : (size_t)WN_MAX_BLOCKS);
}

__device__ __forceinline__ int clamp_off(int o, int hi) { return min(max(o, 0), hi); }

// ---------------------------------------------------------------------------------------------------------------- gather
struct GatherParams {
    const float* canvas;        // [NB][C][Hc][Wc]
    float* out;                 // [NB * n][C][h][w], row j * n + kk
    const int* offsets;         // device, [ny + nx]
    int ny, nx, k0, n, C, Hc, Wc, h, w;
    size_t total;               // NB * n * C * h * w
};

// V consecutive pixels of one window row per lane (V == 4: w, Wc and the x-offsets of the range are multiples of 4 and both bases
// are 16-byte aligned -- the host decides).  A pure copy: both forms move the same bits.
template <int V>
__global__ __launch_bounds__(WN_THREADS) void window_gather_kernel(const GatherParams p) {
    const size_t items = p.total / V;
    const int wv = p.w / V;
    for (size_t j = (size_t)blockIdx.x * WN_THREADS + threadIdx.x; j < items; j += (size_t)gridDim.x * WN_THREADS) {
        const int xx = (int)(j % wv) * V;
        size_t r = j / wv;
        const int yy = (int)(r % p.h); r /= p.h;
        const int c = (int)(r % p.C); r /= p.C;
        const int kk = (int)(r % p.n);
        const size_t b = r / p.n;
        const int k = p.k0 + kk;
        const int iy = k / p.nx, ix = k - iy * p.nx;
        const int oy = clamp_off(p.offsets[iy], p.Hc - p.h), ox = clamp_off(p.offsets[p.ny + ix], p.Wc - p.w);
        const float* src = p.canvas + ((b * p.C + c) * p.Hc + oy + yy) * (size_t)p.Wc + ox + xx;
        if constexpr (V == 4)
            *reinterpret_cast<f32x4*>(p.out + j * 4) = *reinterpret_cast<const f32x4*>(src);
        else
            p.out[j] = *src;
    }
}

// ---------------------------------------------------------------------------------------------------------------- average
struct AverageParams {
    const f16* win;             // [NB * N][h * w][ld], row j * N + k
    f16* out;                   // [NB][Hc * Wc][ld]
    const float* weights;       // [h * w], NULL: uniform
    const int* offsets;         // device, [ny + nx]
    int ny, nx, C, ld, Hc, Wc, h, w;
    size_t total;               // NB * Hc * Wc * (ld / 8)
};

// One 16-byte chunk (8 halves) of one canvas pixel per lane; ld == 8: one pixel per lane.  The covering windows are visited in
// ascending k = iy * nx + ix.  Uniform: acc = (float)e_k0; acc += (float)e_k; acc / (float)count -- plain fp32 adds and one IEEE
// divide.  Weighted: acc = w * e_k0, then fmaf(w, e_k, acc); wsum likewise by plain adds; acc / wsum.  A pixel under ONE window
// takes that window's halves as they are.  Channels >= C are written 0.
template <bool WEIGHTED>
__global__ __launch_bounds__(WN_THREADS) void window_average_kernel(const AverageParams p) {
    const int chunks = p.ld / 8;
    const int N = p.ny * p.nx;
    const size_t hw = (size_t)p.h * p.w;
    for (size_t j = (size_t)blockIdx.x * WN_THREADS + threadIdx.x; j < p.total; j += (size_t)gridDim.x * WN_THREADS) {
        const int ch = (int)(j % chunks);
        size_t r = j / chunks;
        const int x = (int)(r % p.Wc); r /= p.Wc;
        const int y = (int)(r % p.Hc);
        const size_t b = r / p.Hc;
        float acc[8] = {};
        f16x8 one = {};
        float wsum = 0.0f;
        int count = 0;
        for (int iy = 0; iy < p.ny; ++iy) {
            const int yy = y - clamp_off(p.offsets[iy], p.Hc - p.h);
            if (yy < 0 || yy >= p.h) continue;
            for (int ix = 0; ix < p.nx; ++ix) {
                const int xx = x - clamp_off(p.offsets[p.ny + ix], p.Wc - p.w);
                if (xx < 0 || xx >= p.w) continue;
                const size_t pix = (size_t)yy * p.w + xx;
                const f16x8 e = *reinterpret_cast<const f16x8*>(p.win + ((b * N + (size_t)(iy * p.nx + ix)) * hw + pix) * p.ld + ch * 8);
                if constexpr (WEIGHTED) {
                    const float wt = p.weights[pix];
                    if (count == 0) {
#pragma unroll
                        for (int i = 0; i < 8; ++i) acc[i] = wt * (float)e[i];
                        wsum = wt;
                    } else {
#pragma unroll
                        for (int i = 0; i < 8; ++i) acc[i] = __builtin_fmaf(wt, (float)e[i], acc[i]);
                        wsum += wt;
                    }
                } else {
                    if (count == 0) {
#pragma unroll
                        for (int i = 0; i < 8; ++i) acc[i] = (float)e[i];
                    } else {
#pragma unroll
                        for (int i = 0; i < 8; ++i) acc[i] += (float)e[i];
                    }
                }
                if (count == 0) one = e;
                ++count;
            }
        }
        f16x8 o;
        const float den = WEIGHTED ? wsum : (float)count;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const f16 v = count == 1 ? one[i] : (f16)(acc[i] / den);        // (f16)float: round to nearest even
            o[i] = ch * 8 + i < p.C ? v : (f16)0.0f;
        }
        // count == 0 cannot happen for a table the host accepted (every pixel is covered); such a pixel would be written 0 / 0
        *reinterpret_cast<f16x8*>(p.out + j * 8) = o;
    }
}

// ------------------------------------------------------------------------------------------------------- gather by rows
struct GatherRowsParams {
    const float* canvas;        // [NB][C][Hc][Wc]
    float* out;                 // [NB * n][C][h][w], row j * n + i
    const int* offsets;         // device, [ny + nx]
    const int* rows;            // device, [n]: window numbers, any order, repeats allowed
    int ny, nx, n, C, Hc, Wc, h, w, wrap;
    size_t total;               // NB * n * C * h * w
};

// window_gather_kernel with the window number read from rows[i], and with wrap a window at ox covering columns (ox + i) mod Wc.
// V == 4: w, Wc and every x-offset used are multiples of 4, so the four columns of a lane never straddle the seam; the offset
// read from the table is rounded down to a multiple of 4, so that holds for a table that differs from the validated one too.
template <int V>
__global__ __launch_bounds__(WN_THREADS) void window_gather_rows_kernel(const GatherRowsParams p) {
    const size_t items = p.total / V;
    const int wv = p.w / V;
    const int N = p.ny * p.nx;
    for (size_t j = (size_t)blockIdx.x * WN_THREADS + threadIdx.x; j < items; j += (size_t)gridDim.x * WN_THREADS) {
        const int xx = (int)(j % wv) * V;
        size_t r = j / wv;
        const int yy = (int)(r % p.h); r /= p.h;
        const int c = (int)(r % p.C); r /= p.C;
        const int i = (int)(r % p.n);
        const size_t b = r / p.n;
        const int k = clamp_off(p.rows[i], N - 1);
        const int iy = k / p.nx, ix = k - iy * p.nx;
        const int oy = clamp_off(p.offsets[iy], p.Hc - p.h);
        int ox = clamp_off(p.offsets[p.ny + ix], p.wrap ? p.Wc - 1 : p.Wc - p.w);
        if constexpr (V == 4) ox &= ~3;
        int col = ox + xx;
        if (col >= p.Wc) col -= p.Wc;                                   // (only with wrap: ox + w <= Wc without)
        const float* src = p.canvas + ((b * p.C + c) * p.Hc + oy + yy) * (size_t)p.Wc + col;
        if constexpr (V == 4)
            *reinterpret_cast<f32x4*>(p.out + j * 4) = *reinterpret_cast<const f32x4*>(src);
        else
            p.out[j] = *src;
    }
}

// ------------------------------------------------------------------------------------------------------ region average
struct RegionAverageParams {
    const f16* win;             // [NB * P][h * w][ld], row j * P + p
    f16* out;                   // [NB][Hc * Wc][ld]
    const float* weights;       // [h * w], NULL: wt == 1
    const int* offsets;         // device, [ny + nx]
    const int* pair_region;     // device, [P]; REGIONS only
    const int* pair_first;      // device, [N + 1]: the pairs of window k are [pair_first[k], pair_first[k + 1]); REGIONS only
    const float* masks;         // device, [R][Hc][Wc]; REGIONS only
    int ny, nx, P, R, C, ld, Hc, Wc, h, w, wrap;
    size_t total;               // NB * Hc * Wc * (ld / 8)
};

// One 16-byte chunk of one canvas pixel per lane, as window_average_kernel.  The covering windows are visited in ascending k and
// the pairs of a window in ascending r.  A term's q = M_r(pixel) [* wt(pixel - origin_k)]; a term with M_r(pixel) == 0 is skipped
// BEFORE its window row is read.  First term: acc = q * e, qsum = q; later terms: acc = fmaf(q, e, acc), qsum += q; the result is
// fp16_rne(acc / qsum), and a pixel with exactly one term takes that term's halves as they are.  Without REGIONS pair p is window
// p and q = wt (1 without weights): 1 * e and fmaf(1, e, acc) are window_average_kernel's adds, and qsum is its count.
template <bool REGIONS, bool WEIGHTED>
__global__ __launch_bounds__(WN_THREADS) void window_average_regions_kernel(const RegionAverageParams p) {
    const int chunks = p.ld / 8;
    const size_t hw = (size_t)p.h * p.w;
    for (size_t j = (size_t)blockIdx.x * WN_THREADS + threadIdx.x; j < p.total; j += (size_t)gridDim.x * WN_THREADS) {
        const int ch = (int)(j % chunks);
        size_t r = j / chunks;
        const int x = (int)(r % p.Wc); r /= p.Wc;
        const int y = (int)(r % p.Hc);
        const size_t b = r / p.Hc;
        float acc[8] = {};
        f16x8 one = {};
        float qsum = 0.0f;
        int count = 0;
        for (int iy = 0; iy < p.ny; ++iy) {
            const int yy = y - clamp_off(p.offsets[iy], p.Hc - p.h);
            if (yy < 0 || yy >= p.h) continue;
            for (int ix = 0; ix < p.nx; ++ix) {
                int xx = x - clamp_off(p.offsets[p.ny + ix], p.wrap ? p.Wc - 1 : p.Wc - p.w);
                if (p.wrap && xx < 0) xx += p.Wc;
                if (xx < 0 || xx >= p.w) continue;
                const size_t pix = (size_t)yy * p.w + xx;
                const int k = iy * p.nx + ix;
                int p0 = k, p1 = k + 1;
                if constexpr (REGIONS) {
                    p0 = clamp_off(p.pair_first[k], p.P);
                    p1 = min(max(p.pair_first[k + 1], p0), p.P);
                }
                float wt = 1.0f;
                if constexpr (WEIGHTED) wt = p.weights[pix];
                for (int pr = p0; pr < p1; ++pr) {
                    float q = wt;
                    if constexpr (REGIONS) {
                        const int reg = clamp_off(p.pair_region[pr], p.R - 1);
                        const float m = p.masks[((size_t)reg * p.Hc + y) * p.Wc + x];
                        if (!(m > 0.0f)) continue;                          // before the window row is read
                        q = WEIGHTED ? m * wt : m;
                    }
                    const f16x8 e = *reinterpret_cast<const f16x8*>(p.win + ((b * p.P + (size_t)pr) * hw + pix) * p.ld + ch * 8);
                    if (count == 0) {
#pragma unroll
                        for (int i = 0; i < 8; ++i) acc[i] = q * (float)e[i];
                        qsum = q;
                        one = e;
                    } else {
#pragma unroll
                        for (int i = 0; i < 8; ++i) acc[i] = __builtin_fmaf(q, (float)e[i], acc[i]);
                        qsum += q;
                    }
                    ++count;
                }
            }
        }
        f16x8 o;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const f16 v = count == 1 ? one[i] : (f16)(acc[i] / qsum);       // (f16)float: round to nearest even
            o[i] = ch * 8 + i < p.C ? v : (f16)0.0f;
        }
        // count == 0 cannot happen for tables and masks the host accepted (the masks sum to > 0 at every pixel, and a region is
        // active in every window that covers a pixel of its support); such a pixel would be written 0 / 0
        *reinterpret_cast<f16x8*>(p.out + j * 8) = o;
    }
}

// One axis of the host's copy of the offset table, every offset already known to lie inside the canvas (WN_CHECK_GRID):
// ascending from 0 to L - w in steps of 1 .. w, so every pixel is covered.
const char* check_axis(const int* off, int n, int L, int w) {
    if (off[0] != 0 || off[n - 1] != L - w) return "the offsets of an axis must start at 0 and end at L - w";
    for (int i = 1; i < n; ++i) {
        if (off[i] <= off[i - 1]) return "the offsets of an axis must ascend";
        if (off[i] - off[i - 1] > w) return "the windows leave canvas pixels uncovered";
    }
    return nullptr;
}

// The x axis with wrap-around: a window at o covers columns (o + i) mod L, i < w.  Ascending from 0, every step 1 .. w, the last
// offset inside the canvas and at most w before its end, so the last window reaches (at least) column 0 again.
const char* check_axis_wrapped(const int* off, int n, int L, int w) {
    if (off[0] != 0) return "the offsets of a wrapped axis must start at 0";
    for (int i = 1; i < n; ++i) {
        if (off[i] <= off[i - 1]) return "the offsets of an axis must ascend";
        if (off[i] - off[i - 1] > w) return "the windows leave canvas pixels uncovered";
    }
    if (off[n - 1] >= L) return "the last offset of a wrapped axis must lie inside the canvas";
    if (L - off[n - 1] > w) return "the windows leave canvas pixels uncovered";
    return nullptr;
}

}  // namespace

#define WN_CHECK_GRID(name, wrap)                                                                                                \
    MDX_REQUIRE(ny > 0 && nx > 0 && NB > 0 && C > 0 && Hc > 0 && Wc > 0 && h > 0 && w > 0,                                       \
                name ": bad extents (ny=%d nx=%d NB=%d C=%d Hc=%d Wc=%d h=%d w=%d)", ny, nx, NB, C, Hc, Wc, h, w);               \
    MDX_REQUIRE(h <= Hc && w <= Wc, name ": the window (%d x %d) is larger than the canvas (%d x %d)", h, w, Hc, Wc);            \
    MDX_REQUIRE((long long)Hc * Wc <= 0x7fffffffLL && (long long)ny * nx <= 0x7fffffffLL,                                        \
                name ": bad extents (more than 2^31 - 1 pixels or windows)");                                                    \
    for (int i = 0; i < ny + nx; ++i)                                                                                            \
        MDX_REQUIRE(offsets_host[i] >= 0 && offsets_host[i] + (i < ny ? h : (wrap) ? 1 : w) <= (i < ny ? Hc : Wc),               \
                    name ": an offset leaves the canvas (%s offset %d = %d)", i < ny ? "row" : "column", i < ny ? i : i - ny,    \
                    offsets_host[i]);                                                                                            \
    {                                                                                                                            \
        const char* bad_y = check_axis(offsets_host, ny, Hc, h);                                                                 \
        const char* bad_x = ((wrap) ? check_axis_wrapped : check_axis)(offsets_host + ny, nx, Wc, w);                            \
        MDX_REQUIRE(!bad_y && !bad_x, name ": %s (%s)", bad_y ? bad_y : bad_x, bad_y ? "rows" : "columns");                      \
    }

extern "C" int mdx_window_gather_f32(const float* canvas, float* out, const int* offsets, const int* offsets_host, int ny, int nx,
                                     int k0, int n, int NB, int C, int Hc, int Wc, int h, int w, mdx_stream_t s) {
    MDX_REQUIRE(canvas && out && offsets && offsets_host, "mdx_window_gather_f32: null pointer");
    WN_CHECK_GRID("mdx_window_gather_f32", false)
    MDX_REQUIRE(k0 >= 0 && n > 0 && (long long)k0 + n <= (long long)ny * nx,
                "mdx_window_gather_f32: windows [%d, %d + %d) are not inside the grid of %d x %d", k0, k0, n, ny, nx);
    MDX_REQUIRE(!overlaps(out, (size_t)NB * n * C * h * w * sizeof(float), canvas, (size_t)NB * C * Hc * Wc * sizeof(float)),
                "mdx_window_gather_f32: out overlaps canvas");
    GatherParams p;
    p.canvas = canvas; p.out = out; p.offsets = offsets;
    p.ny = ny; p.nx = nx; p.k0 = k0; p.n = n; p.C = C; p.Hc = Hc; p.Wc = Wc; p.h = h; p.w = w;
    p.total = (size_t)NB * n * C * h * w;
    bool vec = w % 4 == 0 && Wc % 4 == 0 && aligned16(canvas) && aligned16(out);
    for (int k = k0; k < k0 + n && vec; ++k) vec = offsets_host[ny + k % nx] % 4 == 0;
    if (vec)
        hipLaunchKernelGGL(window_gather_kernel<4>, dim3(wn_blocks(p.total / 4)), dim3(WN_THREADS), 0, (hipStream_t)s, p);
    else
        hipLaunchKernelGGL(window_gather_kernel<1>, dim3(wn_blocks(p.total)), dim3(WN_THREADS), 0, (hipStream_t)s, p);
    MDX_LAUNCH_CHECK("mdx_window_gather_f32");
    return MDX_OK;
}

extern "C" int mdx_window_average_f16(const void* windows, void* out, const float* weights, int n_weights, const int* offsets,
                                      const int* offsets_host, int ny, int nx, int NB, int C, int ld, int Hc, int Wc, int h, int w,
                                      mdx_stream_t s) {
    MDX_REQUIRE(windows && out && offsets && offsets_host, "mdx_window_average_f16: null pointer");
    WN_CHECK_GRID("mdx_window_average_f16", false)
    MDX_REQUIRE(ld >= C && ld % 8 == 0, "mdx_window_average_f16: ld must be a multiple of 8 and >= C (ld=%d C=%d)", ld, C);
    MDX_REQUIRE(aligned16(windows) && aligned16(out), "mdx_window_average_f16: windows and out must be 16-byte aligned");
    MDX_REQUIRE(!overlaps(out, (size_t)NB * Hc * Wc * ld * sizeof(f16), windows, (size_t)NB * ny * nx * h * w * ld * sizeof(f16)),
                "mdx_window_average_f16: out overlaps windows");
    MDX_REQUIRE(!weights || n_weights > 0, "mdx_window_average_f16: non-positive weight count (%d)", n_weights);
    MDX_REQUIRE(!weights || n_weights == h * w, "mdx_window_average_f16: %d weights for a window of %d x %d", n_weights, h, w);
    AverageParams p;
    p.win = (const f16*)windows; p.out = (f16*)out; p.weights = weights; p.offsets = offsets;
    p.ny = ny; p.nx = nx; p.C = C; p.ld = ld; p.Hc = Hc; p.Wc = Wc; p.h = h; p.w = w;
    p.total = (size_t)NB * Hc * Wc * (ld / 8);
    if (weights)
        hipLaunchKernelGGL(window_average_kernel<true>, dim3(wn_blocks(p.total)), dim3(WN_THREADS), 0, (hipStream_t)s, p);
    else
        hipLaunchKernelGGL(window_average_kernel<false>, dim3(wn_blocks(p.total)), dim3(WN_THREADS), 0, (hipStream_t)s, p);
    MDX_LAUNCH_CHECK("mdx_window_average_f16");
    return MDX_OK;
}

extern "C" int mdx_window_gather_rows_f32(const float* canvas, float* out, const int* offsets, const int* offsets_host, int ny,
                                          int nx, const int* rows, const int* rows_host, int n, int wrap_x, int NB, int C, int Hc,
                                          int Wc, int h, int w, mdx_stream_t s) {
    MDX_REQUIRE(canvas && out && offsets && offsets_host && rows && rows_host, "mdx_window_gather_rows_f32: null pointer");
    MDX_REQUIRE(wrap_x == 0 || wrap_x == 1, "mdx_window_gather_rows_f32: wrap_x must be 0 or 1, got %d", wrap_x);
    WN_CHECK_GRID("mdx_window_gather_rows_f32", wrap_x)
    MDX_REQUIRE(n > 0, "mdx_window_gather_rows_f32: non-positive row count (%d)", n);
    for (int i = 0; i < n; ++i)
        MDX_REQUIRE(rows_host[i] >= 0 && rows_host[i] < ny * nx,
                    "mdx_window_gather_rows_f32: row %d is window %d, not inside the grid of %d x %d", i, rows_host[i], ny, nx);
    MDX_REQUIRE(!overlaps(out, (size_t)NB * n * C * h * w * sizeof(float), canvas, (size_t)NB * C * Hc * Wc * sizeof(float)),
                "mdx_window_gather_rows_f32: out overlaps canvas");
    GatherRowsParams p;
    p.canvas = canvas; p.out = out; p.offsets = offsets; p.rows = rows;
    p.ny = ny; p.nx = nx; p.n = n; p.C = C; p.Hc = Hc; p.Wc = Wc; p.h = h; p.w = w; p.wrap = wrap_x;
    p.total = (size_t)NB * n * C * h * w;
    bool vec = w % 4 == 0 && Wc % 4 == 0 && aligned16(canvas) && aligned16(out);
    for (int i = 0; i < n && vec; ++i) vec = offsets_host[ny + rows_host[i] % nx] % 4 == 0;
    if (vec)
        hipLaunchKernelGGL(window_gather_rows_kernel<4>, dim3(wn_blocks(p.total / 4)), dim3(WN_THREADS), 0, (hipStream_t)s, p);
    else
        hipLaunchKernelGGL(window_gather_rows_kernel<1>, dim3(wn_blocks(p.total)), dim3(WN_THREADS), 0, (hipStream_t)s, p);
    MDX_LAUNCH_CHECK("mdx_window_gather_rows_f32");
    return MDX_OK;
}

extern "C" int mdx_window_average_regions_f16(const void* windows, void* out, const float* weights, int n_weights,
                                              const int* offsets, const int* offsets_host, int ny, int nx, int wrap_x,
                                              const int* pair_window_host, const int* pair_region, const int* pair_region_host,
                                              const int* pair_first, const int* pair_first_host, int P, const float* masks, int R,
                                              int NB, int C, int ld, int Hc, int Wc, int h, int w, mdx_stream_t s) {
    MDX_REQUIRE(windows && out && offsets && offsets_host, "mdx_window_average_regions_f16: null pointer");
    MDX_REQUIRE(wrap_x == 0 || wrap_x == 1, "mdx_window_average_regions_f16: wrap_x must be 0 or 1, got %d", wrap_x);
    WN_CHECK_GRID("mdx_window_average_regions_f16", wrap_x)
    MDX_REQUIRE(ld >= C && ld % 8 == 0, "mdx_window_average_regions_f16: ld must be a multiple of 8 and >= C (ld=%d C=%d)", ld, C);
    MDX_REQUIRE(R >= 0 && P > 0, "mdx_window_average_regions_f16: bad pair or region count (P=%d R=%d)", P, R);
    const int N = ny * nx;
    if (R == 0) {
        MDX_REQUIRE(!masks, "mdx_window_average_regions_f16: masks without regions (R == 0)");
        MDX_REQUIRE(P == N, "mdx_window_average_regions_f16: without regions the pairs are the windows (P=%d, %d windows)", P, N);
    } else {
        MDX_REQUIRE(masks && pair_window_host && pair_region && pair_region_host && pair_first && pair_first_host,
                    "mdx_window_average_regions_f16: null pointer (masks or a pair table, R=%d)", R);
        MDX_REQUIRE((long long)R * Hc * Wc <= 0x7fffffffLL, "mdx_window_average_regions_f16: bad extents (the masks have more "
                    "than 2^31 - 1 elements)");
        MDX_REQUIRE(pair_first_host[0] == 0 && pair_first_host[N] == P,
                    "mdx_window_average_regions_f16: pair_first must run from 0 to P (%d .. %d, P=%d)", pair_first_host[0],
                    pair_first_host[N], P);
        for (int k = 0; k < N; ++k) {
            const int p0 = pair_first_host[k], p1 = pair_first_host[k + 1];
            MDX_REQUIRE(p0 <= p1 && p1 <= P, "mdx_window_average_regions_f16: pair_first must not descend (window %d)", k);
            for (int q = p0; q < p1; ++q) {
                MDX_REQUIRE(pair_window_host[q] == k, "mdx_window_average_regions_f16: pair %d is window %d, pair_first puts it "
                            "in window %d (the pairs are sorted by window)", q, pair_window_host[q], k);
                MDX_REQUIRE(pair_region_host[q] >= 0 && pair_region_host[q] < R,
                            "mdx_window_average_regions_f16: pair %d is region %d of %d", q, pair_region_host[q], R);
                MDX_REQUIRE(q == p0 || pair_region_host[q] > pair_region_host[q - 1],
                            "mdx_window_average_regions_f16: the regions of window %d must ascend (pair %d)", k, q);
            }
        }
    }
    MDX_REQUIRE(aligned16(windows) && aligned16(out), "mdx_window_average_regions_f16: windows and out must be 16-byte aligned");
    MDX_REQUIRE(!overlaps(out, (size_t)NB * Hc * Wc * ld * sizeof(f16), windows, (size_t)NB * P * h * w * ld * sizeof(f16)),
                "mdx_window_average_regions_f16: out overlaps windows");
    MDX_REQUIRE(!weights || n_weights > 0, "mdx_window_average_regions_f16: non-positive weight count (%d)", n_weights);
    MDX_REQUIRE(!weights || n_weights == h * w, "mdx_window_average_regions_f16: %d weights for a window of %d x %d", n_weights,
                h, w);
    RegionAverageParams p;
    p.win = (const f16*)windows; p.out = (f16*)out; p.weights = weights; p.offsets = offsets;
    p.pair_region = pair_region; p.pair_first = pair_first; p.masks = masks;
    p.ny = ny; p.nx = nx; p.P = P; p.R = R; p.C = C; p.ld = ld; p.Hc = Hc; p.Wc = Wc; p.h = h; p.w = w; p.wrap = wrap_x;
    p.total = (size_t)NB * Hc * Wc * (ld / 8);
    const dim3 grid(wn_blocks(p.total)), block(WN_THREADS);
    if (R > 0 && weights)
        hipLaunchKernelGGL((window_average_regions_kernel<true, true>), grid, block, 0, (hipStream_t)s, p);
    else if (R > 0)
        hipLaunchKernelGGL((window_average_regions_kernel<true, false>), grid, block, 0, (hipStream_t)s, p);
    else if (weights)
        hipLaunchKernelGGL((window_average_regions_kernel<false, true>), grid, block, 0, (hipStream_t)s, p);
    else
        hipLaunchKernelGGL((window_average_regions_kernel<false, false>), grid, block, 0, (hipStream_t)s, p);
    MDX_LAUNCH_CHECK("mdx_window_average_regions_f16");
    return MDX_OK;
}
