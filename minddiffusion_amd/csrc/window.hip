// Windowed UNet evaluation (MultiDiffusion, Bar-Tal et al. 2023): the two launches around the UNet when a large latent canvas is
// evaluated as a batch of overlapping windows of the trained size.  mdx_window_gather_f32 cuts windows k0 .. k0 + n - 1 out of the
// fp32 NCHW canvas into the UNet's input batch; mdx_window_average_f16 averages the NHWC fp16 outputs of ALL windows back onto the
// canvas, where windows overlap.  Both are memory- and launch-bound: one 16-byte access per lane where the shape allows it,
// one-wave workgroups on a capped grid with a grid-stride loop (as csrc/inpaint.hip).  Every output element has exactly one
// writer: the average is a gather per canvas pixel over its covering windows in ascending window number, no atomics.
// The window offsets are read from a device table [ny + nx] (rows, then columns); the host validates its own copy of the table
// before any launch and the kernels clamp what they read into the canvas, so a table that differs from the validated one can
// mis-place a window but not leave the buffers.
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

}  // namespace

#define WN_CHECK_GRID(name)                                                                                                  \
    MDX_REQUIRE(ny > 0 && nx > 0 && NB > 0 && C > 0 && Hc > 0 && Wc > 0 && h > 0 && w > 0,                                   \
                name ": bad extents (ny=%d nx=%d NB=%d C=%d Hc=%d Wc=%d h=%d w=%d)", ny, nx, NB, C, Hc, Wc, h, w);           \
    MDX_REQUIRE(h <= Hc && w <= Wc, name ": the window (%d x %d) is larger than the canvas (%d x %d)", h, w, Hc, Wc);        \
    MDX_REQUIRE((long long)Hc * Wc <= 0x7fffffffLL && (long long)ny * nx <= 0x7fffffffLL,                                    \
                name ": bad extents (more than 2^31 - 1 pixels or windows)");                                                \
    for (int i = 0; i < ny + nx; ++i)                                                                                        \
        MDX_REQUIRE(offsets_host[i] >= 0 && offsets_host[i] + (i < ny ? h : w) <= (i < ny ? Hc : Wc),                        \
                    name ": an offset leaves the canvas (%s offset %d = %d)", i < ny ? "row" : "column", i < ny ? i : i - ny, \
                    offsets_host[i]);                                                                                        \
    {                                                                                                                        \
        const char* bad_y = check_axis(offsets_host, ny, Hc, h);                                                             \
        const char* bad_x = check_axis(offsets_host + ny, nx, Wc, w);                                                        \
        MDX_REQUIRE(!bad_y && !bad_x, name ": %s (%s)", bad_y ? bad_y : bad_x, bad_y ? "rows" : "columns");                  \
    }

extern "C" int mdx_window_gather_f32(const float* canvas, float* out, const int* offsets, const int* offsets_host, int ny, int nx,
                                     int k0, int n, int NB, int C, int Hc, int Wc, int h, int w, mdx_stream_t s) {
    MDX_REQUIRE(canvas && out && offsets && offsets_host, "mdx_window_gather_f32: null pointer");
    WN_CHECK_GRID("mdx_window_gather_f32")
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
    WN_CHECK_GRID("mdx_window_average_f16")
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
