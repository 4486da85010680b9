// Windowed UNet evaluation (MultiDiffusion, Bar-Tal et al. 2023): the two launches around the UNet when a large latent canvas is
// evaluated as a batch of overlapping windows of the trained size.  The gather cuts windows out of the fp32 NCHW canvas into the
// UNet's input batch; the average brings the NHWC fp16 outputs of ALL windows -- or of all (window, region) pairs -- back onto the
// canvas, where windows overlap.  Both are memory- and launch-bound: one 16-byte access per lane where the shape allows it,
// one-wave workgroups on a capped grid with a grid-stride loop (as csrc/inpaint.hip).  Every output element has exactly one
// writer: the average is a gather per canvas pixel over its covering windows in ascending window number, no atomics.
// The window offsets are read from a device table [ny + nx] (rows, then columns); the host validates its own copy of the table
// before any launch and the kernels clamp what they read into the canvas, so a table that differs from the validated one can
// mis-place a window but not leave the buffers.
// ONE kernel pair and one host body each serve the four entries:
//   mdx_window_gather_f32           window_gather_kernel<4 | 1>, the windows a range: rows == NULL, k0, no wrap
//   mdx_window_gather_rows_f32      window_gather_kernel<4 | 1>, the windows named by a table; wrap_x lets a window run over the
//                                   right edge of the canvas into its left one
//   mdx_window_average_f16          window_average_kernel<false, WEIGHTED>: R == 0, the pairs are the windows, no wrap
//   mdx_window_average_regions_f16  window_average_kernel<R > 0, WEIGHTED>: every pair's output weighed by its region's mask
// and a fifth entry brings fp32 NCHW IMAGE tiles (the VAE decoder's outputs on a tiled canvas) back onto the image canvas:
//   mdx_tile_blend_f32              tile_blend_kernel<4 | 1>: the gather's row order and vector decision, the average's one
//                                   writer per pixel, min-ramp weights computed in the kernel, [0, 1] conversion fused
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
    float* out;                 // [NB * n][C][h][w], row j * n + i
    const int* offsets;         // device, [ny + nx]
    const int* rows;            // device, [n]: window numbers, any order, repeats allowed; NULL: windows k0 .. k0 + n - 1
    int ny, nx, k0, n, C, Hc, Wc, h, w, wrap;
    size_t total;               // NB * n * C * h * w
};

// V consecutive pixels of one window row per lane; output row i is window rows[i], or k0 + i without a table.  With wrap a window
// at ox covers columns (ox + i) mod Wc.  V == 4: w, Wc and every x-offset used are multiples of 4 and both bases are 16-byte
// aligned (the host decides), so the four columns of a lane never straddle the seam; the offset read from the table is rounded
// down to a multiple of 4, so that holds for a table that differs from the validated one too.  A pure copy: both forms move the
// same bits.
template <int V>
__global__ __launch_bounds__(WN_THREADS) void window_gather_kernel(const GatherParams p) {
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
        const int k = p.rows ? clamp_off(p.rows[i], N - 1) : p.k0 + i;
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

// ---------------------------------------------------------------------------------------------------------------- average
struct AverageParams {
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

// One 16-byte chunk (8 halves) of one canvas pixel per lane; ld == 8: one pixel per lane.  The covering windows are visited in
// ascending k = iy * nx + ix and the pairs of a window in ascending r.  A term's q = M_r(pixel) [* wt(pixel - origin_k)]; a term
// with M_r(pixel) == 0 is skipped BEFORE its window row is read.  First term: acc = q * e, qsum = q; later terms: acc =
// fmaf(q, e, acc), qsum += q; the result is fp16_rne(acc / qsum), and a pixel with exactly one term takes that term's halves as
// they are.  Without REGIONS pair p is window p and q = wt (1 without weights): 1 * e and fmaf(1, e, acc) are the plain mean's
// fp32 adds and qsum is its count, or its weight sum.  Channels >= C are written 0.
template <bool REGIONS, bool WEIGHTED>
__global__ __launch_bounds__(WN_THREADS) void window_average_kernel(const AverageParams p) {
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
        // count == 0 cannot happen for tables and masks the host accepted (every pixel is covered, the masks sum to > 0 at every
        // pixel, and a region is active in every window that covers a pixel of its support); such a pixel would be written 0 / 0
        *reinterpret_cast<f16x8*>(p.out + j * 8) = o;
    }
}

// ---------------------------------------------------------------------------------------------------------------- tile blend
struct BlendParams {
    const float* tiles;         // [NB * N][C][h][w], row j * N + k
    float* out;                 // [NB][C][Hc][Wc]
    const int* offsets;         // device, [ny + nx]
    int ny, nx, C, Hc, Wc, h, w, ramp_y, ramp_x, wrap, unit;
    size_t total;               // NB * C * Hc * Wc
};

// acc + q * e with the product and the sum rounded separately (never an fma: a numpy float32 restatement is bit-equal)
__device__ __forceinline__ float blend_add(float acc, float q, float e) {
#pragma clang fp contract(off)
    const float t = q * e;
    return acc + t;
}

// the bits of torch.clamp((v + 1.0) / 2.0, 0.0, 1.0), NaN kept
__device__ __forceinline__ float to_unit(float v) {
#pragma clang fp contract(off)
    const float u = (v + 1.0f) / 2.0f;
    return u < 0.0f ? 0.0f : u > 1.0f ? 1.0f : u;
}

// V consecutive columns of one (b, c, y) canvas row per lane.  The covering tiles are visited in ascending k = iy * nx + ix; the
// weight of tile-local pixel (yy, xx) is q = (float)(min(yy + 1, h - yy, ramp_y) * min(xx + 1, w - xx, ramp_x)), an integer
// <= 2^24.  First term: acc = q * e, qsum = q; later terms: acc = acc + q * e (blend_add), qsum += q; the result is acc / qsum,
// and a pixel with exactly one term takes that term's bits.  V == 4: w, Wc and every x offset are multiples of 4 and both bases
// are 16-byte aligned (the host decides; a table read is rounded down to a multiple of 4), so the four columns of a lane share
// their covering tiles and never straddle the seam; their weights differ per column.  Both forms compute the same bits.
template <int V>
__global__ __launch_bounds__(WN_THREADS) void tile_blend_kernel(const BlendParams p) {
    const size_t items = p.total / V;
    const int wv = p.Wc / V;
    const size_t N = (size_t)p.ny * p.nx;
    for (size_t j = (size_t)blockIdx.x * WN_THREADS + threadIdx.x; j < items; j += (size_t)gridDim.x * WN_THREADS) {
        const int x = (int)(j % wv) * V;
        size_t r = j / wv;
        const int y = (int)(r % p.Hc); r /= p.Hc;
        const int c = (int)(r % p.C);
        const size_t b = r / p.C;
        float acc[V] = {}, one[V] = {};
        float qsum[V] = {};
        int count = 0;
        for (int iy = 0; iy < p.ny; ++iy) {
            const int yy = y - clamp_off(p.offsets[iy], p.Hc - p.h);
            if (yy < 0 || yy >= p.h) continue;
            const int qy = min(min(yy + 1, p.h - yy), p.ramp_y);
            for (int ix = 0; ix < p.nx; ++ix) {
                int ox = clamp_off(p.offsets[p.ny + ix], p.wrap ? p.Wc - 1 : p.Wc - p.w);
                if constexpr (V == 4) ox &= ~3;
                int xx = x - ox;
                if (p.wrap && xx < 0) xx += p.Wc;
                if (xx < 0 || xx >= p.w) continue;
                const float* src = p.tiles + (((b * N + (size_t)(iy * p.nx + ix)) * p.C + c) * p.h + yy) * (size_t)p.w + xx;
                float e[V];
                if constexpr (V == 4) {
                    const f32x4 v = *reinterpret_cast<const f32x4*>(src);
#pragma unroll
                    for (int i = 0; i < 4; ++i) e[i] = v[i];
                } else {
                    e[0] = *src;
                }
#pragma unroll
                for (int i = 0; i < V; ++i) {
                    const float q = (float)(qy * min(min(xx + i + 1, p.w - xx - i), p.ramp_x));
                    if (count == 0) {
                        acc[i] = q * e[i];
                        qsum[i] = q;
                        one[i] = e[i];
                    } else {
                        acc[i] = blend_add(acc[i], q, e[i]);
                        qsum[i] += q;
                    }
                }
                ++count;
            }
        }
        // count == 0 cannot happen for a table the host accepted (every pixel is covered); such a pixel would be written 0 / 0
        float o[V];
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const float v = count == 1 ? one[i] : acc[i] / qsum[i];
            o[i] = p.unit ? to_unit(v) : v;
        }
        if constexpr (V == 4) {
            f32x4 v;
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = o[i];
            *reinterpret_cast<f32x4*>(p.out + j * 4) = v;
        } else {
            p.out[j] = o[0];
        }
    }
}

// ------------------------------------------------------------------------------------------------------------- the host
// One axis of the host's copy of the offset table, every offset already known to lie inside the canvas (check_grid):
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

// The extents and the host's copy of the offset table, for all four entries; `fn` names the entry in its messages.
int check_grid(const char* fn, const int* offsets_host, int ny, int nx, int wrap, int NB, int C, int Hc, int Wc, int h, int w) {
    MDX_REQUIRE(ny > 0 && nx > 0 && NB > 0 && C > 0 && Hc > 0 && Wc > 0 && h > 0 && w > 0,
                "%s: bad extents (ny=%d nx=%d NB=%d C=%d Hc=%d Wc=%d h=%d w=%d)", fn, ny, nx, NB, C, Hc, Wc, h, w);
    MDX_REQUIRE(h <= Hc && w <= Wc, "%s: the window (%d x %d) is larger than the canvas (%d x %d)", fn, h, w, Hc, Wc);
    MDX_REQUIRE((long long)Hc * Wc <= 0x7fffffffLL && (long long)ny * nx <= 0x7fffffffLL,
                "%s: bad extents (more than 2^31 - 1 pixels or windows)", fn);
    for (int i = 0; i < ny + nx; ++i)
        MDX_REQUIRE(offsets_host[i] >= 0 && offsets_host[i] + (i < ny ? h : wrap ? 1 : w) <= (i < ny ? Hc : Wc),
                    "%s: an offset leaves the canvas (%s offset %d = %d)", fn, i < ny ? "row" : "column", i < ny ? i : i - ny,
                    offsets_host[i]);
    const char* bad_y = check_axis(offsets_host, ny, Hc, h);
    const char* bad_x = (wrap ? check_axis_wrapped : check_axis)(offsets_host + ny, nx, Wc, w);
    MDX_REQUIRE(!bad_y && !bad_x, "%s: %s (%s)", fn, bad_y ? bad_y : bad_x, bad_y ? "rows" : "columns");
    return MDX_OK;
}

// One host body for both gather entries; `fn` names the entry in its messages.  rows_host NULL: the windows are the range
// k0 .. k0 + n - 1 (and rows is NULL); otherwise they are rows_host[0 .. n), the values the device table `rows` holds.
int gather_launch(const char* fn, const float* canvas, float* out, const int* offsets, const int* offsets_host, int ny, int nx,
                  const int* rows, const int* rows_host, int k0, int n, int wrap, int NB, int C, int Hc, int Wc, int h, int w,
                  mdx_stream_t s) {
    MDX_REQUIRE(canvas && out && offsets && offsets_host && !rows == !rows_host, "%s: null pointer", fn);
    MDX_REQUIRE(wrap == 0 || wrap == 1, "%s: wrap_x must be 0 or 1, got %d", fn, wrap);
    if (const int rc = check_grid(fn, offsets_host, ny, nx, wrap, NB, C, Hc, Wc, h, w)) return rc;
    if (!rows_host) {
        MDX_REQUIRE(k0 >= 0 && n > 0 && (long long)k0 + n <= (long long)ny * nx,
                    "%s: windows [%d, %d + %d) are not inside the grid of %d x %d", fn, k0, k0, n, ny, nx);
    } else {
        MDX_REQUIRE(n > 0, "%s: non-positive row count (%d)", fn, n);
        for (int i = 0; i < n; ++i)
            MDX_REQUIRE(rows_host[i] >= 0 && rows_host[i] < ny * nx, "%s: row %d is window %d, not inside the grid of %d x %d",
                        fn, i, rows_host[i], ny, nx);
    }
    MDX_REQUIRE(!overlaps(out, (size_t)NB * n * C * h * w * sizeof(float), canvas, (size_t)NB * C * Hc * Wc * sizeof(float)),
                "%s: out overlaps canvas", fn);
    GatherParams p;
    p.canvas = canvas; p.out = out; p.offsets = offsets; p.rows = rows;
    p.ny = ny; p.nx = nx; p.k0 = k0; p.n = n; p.C = C; p.Hc = Hc; p.Wc = Wc; p.h = h; p.w = w; p.wrap = wrap;
    p.total = (size_t)NB * n * C * h * w;
    bool vec = w % 4 == 0 && Wc % 4 == 0 && aligned16(canvas) && aligned16(out);
    for (int i = 0; i < n && vec; ++i) vec = offsets_host[ny + (rows_host ? rows_host[i] : k0 + i) % nx] % 4 == 0;
    if (vec)
        hipLaunchKernelGGL(window_gather_kernel<4>, dim3(wn_blocks(p.total / 4)), dim3(WN_THREADS), 0, (hipStream_t)s, p);
    else
        hipLaunchKernelGGL(window_gather_kernel<1>, dim3(wn_blocks(p.total)), dim3(WN_THREADS), 0, (hipStream_t)s, p);
    MDX_LAUNCH_CHECK(fn);
    return MDX_OK;
}

// One host body for both average entries; `fn` names the entry in its messages.  R == 0: no regions -- masks and the pair
// tables are NULL and the P pairs are the ny * nx windows.
int average_launch(const char* fn, const void* windows, void* out, const float* weights, int n_weights, const int* offsets,
                   const int* offsets_host, int ny, int nx, int wrap, const int* pair_window_host, const int* pair_region,
                   const int* pair_region_host, const int* pair_first, const int* pair_first_host, int P, const float* masks,
                   int R, int NB, int C, int ld, int Hc, int Wc, int h, int w, mdx_stream_t s) {
    MDX_REQUIRE(windows && out && offsets && offsets_host, "%s: null pointer", fn);
    MDX_REQUIRE(wrap == 0 || wrap == 1, "%s: wrap_x must be 0 or 1, got %d", fn, wrap);
    if (const int rc = check_grid(fn, offsets_host, ny, nx, wrap, NB, C, Hc, Wc, h, w)) return rc;
    MDX_REQUIRE(ld >= C && ld % 8 == 0, "%s: ld must be a multiple of 8 and >= C (ld=%d C=%d)", fn, ld, C);
    MDX_REQUIRE(R >= 0 && P > 0, "%s: bad pair or region count (P=%d R=%d)", fn, P, R);
    const int N = ny * nx;
    if (R == 0) {
        MDX_REQUIRE(!masks, "%s: masks without regions (R == 0)", fn);
        MDX_REQUIRE(P == N, "%s: without regions the pairs are the windows (P=%d, %d windows)", fn, P, N);
    } else {
        MDX_REQUIRE(masks && pair_window_host && pair_region && pair_region_host && pair_first && pair_first_host,
                    "%s: null pointer (masks or a pair table, R=%d)", fn, R);
        MDX_REQUIRE((long long)R * Hc * Wc <= 0x7fffffffLL, "%s: bad extents (the masks have more than 2^31 - 1 elements)", fn);
        MDX_REQUIRE(pair_first_host[0] == 0 && pair_first_host[N] == P, "%s: pair_first must run from 0 to P (%d .. %d, P=%d)",
                    fn, pair_first_host[0], pair_first_host[N], P);
        for (int k = 0; k < N; ++k) {
            const int p0 = pair_first_host[k], p1 = pair_first_host[k + 1];
            MDX_REQUIRE(p0 <= p1 && p1 <= P, "%s: pair_first must not descend (window %d)", fn, k);
            for (int q = p0; q < p1; ++q) {
                MDX_REQUIRE(pair_window_host[q] == k, "%s: pair %d is window %d, pair_first puts it in window %d (the pairs are "
                            "sorted by window)", fn, q, pair_window_host[q], k);
                MDX_REQUIRE(pair_region_host[q] >= 0 && pair_region_host[q] < R, "%s: pair %d is region %d of %d", fn, q,
                            pair_region_host[q], R);
                MDX_REQUIRE(q == p0 || pair_region_host[q] > pair_region_host[q - 1],
                            "%s: the regions of window %d must ascend (pair %d)", fn, k, q);
            }
        }
    }
    MDX_REQUIRE(aligned16(windows) && aligned16(out), "%s: windows and out must be 16-byte aligned", fn);
    MDX_REQUIRE(!overlaps(out, (size_t)NB * Hc * Wc * ld * sizeof(f16), windows, (size_t)NB * P * h * w * ld * sizeof(f16)),
                "%s: out overlaps windows", fn);
    MDX_REQUIRE(!weights || n_weights > 0, "%s: non-positive weight count (%d)", fn, n_weights);
    MDX_REQUIRE(!weights || n_weights == h * w, "%s: %d weights for a window of %d x %d", fn, n_weights, h, w);
    AverageParams p;
    p.win = (const f16*)windows; p.out = (f16*)out; p.weights = weights; p.offsets = offsets;
    p.pair_region = pair_region; p.pair_first = pair_first; p.masks = masks;
    p.ny = ny; p.nx = nx; p.P = P; p.R = R; p.C = C; p.ld = ld; p.Hc = Hc; p.Wc = Wc; p.h = h; p.w = w; p.wrap = wrap;
    p.total = (size_t)NB * Hc * Wc * (ld / 8);
    const dim3 grid(wn_blocks(p.total)), block(WN_THREADS);
    if (R > 0 && weights)
        hipLaunchKernelGGL((window_average_kernel<true, true>), grid, block, 0, (hipStream_t)s, p);
    else if (R > 0)
        hipLaunchKernelGGL((window_average_kernel<true, false>), grid, block, 0, (hipStream_t)s, p);
    else if (weights)
        hipLaunchKernelGGL((window_average_kernel<false, true>), grid, block, 0, (hipStream_t)s, p);
    else
        hipLaunchKernelGGL((window_average_kernel<false, false>), grid, block, 0, (hipStream_t)s, p);
    MDX_LAUNCH_CHECK(fn);
    return MDX_OK;
}

// The blend's host body: the gather's vector decision on the image canvas, every x offset of the table counted.
int blend_launch(const char* fn, const float* tiles, float* out, const int* offsets, const int* offsets_host, int ny, int nx,
                 int wrap, int NB, int C, int Hc, int Wc, int h, int w, int ramp_y, int ramp_x, int mode, mdx_stream_t s) {
    MDX_REQUIRE(tiles && out && offsets && offsets_host, "%s: null pointer", fn);
    MDX_REQUIRE(wrap == 0 || wrap == 1, "%s: wrap_x must be 0 or 1, got %d", fn, wrap);
    if (const int rc = check_grid(fn, offsets_host, ny, nx, wrap, NB, C, Hc, Wc, h, w)) return rc;
    MDX_REQUIRE(ramp_y >= 1 && ramp_x >= 1 && ramp_y <= 4096 && ramp_x <= 4096,
                "%s: the ramps must be in [1, 4096] (their products stay exact in fp32), got %d x %d", fn, ramp_y, ramp_x);
    MDX_REQUIRE(mode == MDX_TILE_RAW || mode == MDX_TILE_UNIT, "%s: unknown mode %d", fn, mode);
    const size_t N = (size_t)ny * nx;
    MDX_REQUIRE(!overlaps(out, (size_t)NB * C * Hc * Wc * sizeof(float), tiles, (size_t)NB * N * C * h * w * sizeof(float)),
                "%s: out overlaps tiles", fn);
    BlendParams p;
    p.tiles = tiles; p.out = out; p.offsets = offsets;
    p.ny = ny; p.nx = nx; p.C = C; p.Hc = Hc; p.Wc = Wc; p.h = h; p.w = w; p.ramp_y = ramp_y; p.ramp_x = ramp_x; p.wrap = wrap;
    p.unit = mode == MDX_TILE_UNIT;
    p.total = (size_t)NB * C * Hc * Wc;
    bool vec = w % 4 == 0 && Wc % 4 == 0 && aligned16(tiles) && aligned16(out);
    for (int i = 0; i < nx && vec; ++i) vec = offsets_host[ny + i] % 4 == 0;
    if (vec)
        hipLaunchKernelGGL(tile_blend_kernel<4>, dim3(wn_blocks(p.total / 4)), dim3(WN_THREADS), 0, (hipStream_t)s, p);
    else
        hipLaunchKernelGGL(tile_blend_kernel<1>, dim3(wn_blocks(p.total)), dim3(WN_THREADS), 0, (hipStream_t)s, p);
    MDX_LAUNCH_CHECK(fn);
    return MDX_OK;
}

}  // namespace

extern "C" int mdx_window_gather_f32(const float* canvas, float* out, const int* offsets, const int* offsets_host, int ny, int nx,
                                     int k0, int n, int NB, int C, int Hc, int Wc, int h, int w, mdx_stream_t s) {
    return gather_launch("mdx_window_gather_f32", canvas, out, offsets, offsets_host, ny, nx, nullptr, nullptr, k0, n, 0, NB, C,
                         Hc, Wc, h, w, s);
}

extern "C" int mdx_window_average_f16(const void* windows, void* out, const float* weights, int n_weights, const int* offsets,
                                      const int* offsets_host, int ny, int nx, int NB, int C, int ld, int Hc, int Wc, int h, int w,
                                      mdx_stream_t s) {
    // (ny * nx as P: not positive, or past 2^31 - 1, is check_grid's to refuse, before P is looked at)
    return average_launch("mdx_window_average_f16", windows, out, weights, n_weights, offsets, offsets_host, ny, nx, 0, nullptr,
                          nullptr, nullptr, nullptr, nullptr, (int)((long long)ny * nx), nullptr, 0, NB, C, ld, Hc, Wc, h, w, s);
}

extern "C" int mdx_window_gather_rows_f32(const float* canvas, float* out, const int* offsets, const int* offsets_host, int ny,
                                          int nx, const int* rows, const int* rows_host, int n, int wrap_x, int NB, int C, int Hc,
                                          int Wc, int h, int w, mdx_stream_t s) {
    MDX_REQUIRE(rows && rows_host, "mdx_window_gather_rows_f32: null pointer");
    return gather_launch("mdx_window_gather_rows_f32", canvas, out, offsets, offsets_host, ny, nx, rows, rows_host, 0, n, wrap_x,
                         NB, C, Hc, Wc, h, w, s);
}

extern "C" int mdx_window_average_regions_f16(const void* windows, void* out, const float* weights, int n_weights,
                                              const int* offsets, const int* offsets_host, int ny, int nx, int wrap_x,
                                              const int* pair_window_host, const int* pair_region, const int* pair_region_host,
                                              const int* pair_first, const int* pair_first_host, int P, const float* masks, int R,
                                              int NB, int C, int ld, int Hc, int Wc, int h, int w, mdx_stream_t s) {
    return average_launch("mdx_window_average_regions_f16", windows, out, weights, n_weights, offsets, offsets_host, ny, nx,
                          wrap_x, pair_window_host, pair_region, pair_region_host, pair_first, pair_first_host, P, masks, R, NB,
                          C, ld, Hc, Wc, h, w, s);
}

extern "C" int mdx_tile_blend_f32(const float* tiles, float* out, const int* offsets, const int* offsets_host, int ny, int nx,
                                  int wrap_x, int NB, int C, int Hc, int Wc, int TH, int TW, int ramp_y, int ramp_x, int mode,
                                  mdx_stream_t s) {
    return blend_launch("mdx_tile_blend_f32", tiles, out, offsets, offsets_host, ny, nx, wrap_x, NB, C, Hc, Wc, TH, TW, ramp_y,
                        ramp_x, mode, s);
}
