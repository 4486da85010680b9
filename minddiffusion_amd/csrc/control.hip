// ControlNet residual add (mdx_control_add_f16) and the in-place SiLU of the hint block (mdx_silu_f16).
//
// mdx_control_add_f16: the 13 residual tensors of a ControlNet (Zhang et al. 2023: one per UNet skip connection and one for the
// middle block's output) are added into the UNet's activations IN PLACE by one launch -- up to 16 segments {dst, src, elements per
// batch row}, four resolutions, ~6.7 M halves per batch row on the SDv2 UNet at a 64 x 64 latent.  Thirteen separate adds would be
// launch-bound; one table-driven launch streams them once.  Which source row feeds a destination row (src_row, -1 = the row is not
// touched) and the scale of every (segment, row) are DEVICE tables read when the kernel runs, and so are the source pointers: a
// captured graph serves any scales, any row mapping and a re-planned ControlNet without being captured again.
//
// Memory-bound: 2 reads + 1 write of 16 bytes per chunk.  One flat index space over (segment, row, chunk); a thread takes UNROLL
// chunks a pass with all its loads issued ahead of the first store.  The segment of a chunk is found from a prefix table in the
// kernel arguments (<= 16 scalar compares).  No atomics: every destination chunk has exactly one writer.
#include "mdx_common.h"

namespace {

constexpr int UNROLL = 4;

struct ControlParams {
    f16* dst[MDX_CONTROL_MAX_SEGS];
    long long prefix[MDX_CONTROL_MAX_SEGS + 1];     // first flat chunk of segment s; prefix[n_seg] = total
    int cpr[MDX_CONTROL_MAX_SEGS];                  // 16-byte chunks per row
    const f16* const* src;                          // device table [n_seg]
    const int* src_row;                             // device table [nb]
    const float* scale;                             // device table [n_seg][nb]
    int n_seg, nb;
};

struct Item {
    f16* d;
    f16x8 dv, sv;
    float sc;
    bool on;
};

__device__ __forceinline__ void control_load(const ControlParams& p, long long i, Item& it) {
    it.on = false;
    if (i >= p.prefix[MDX_CONTROL_MAX_SEGS]) return;
    // the segment of chunk i: constant indices only, so every table entry is a scalar read of the kernel arguments
    int s = 0, cpr = p.cpr[0];
    long long first = 0;
    f16* dst = p.dst[0];
#pragma unroll
    for (int k = 1; k < MDX_CONTROL_MAX_SEGS; ++k) {
        if (k < p.n_seg && i >= p.prefix[k]) {
            s = k;
            cpr = p.cpr[k];
            first = p.prefix[k];
            dst = p.dst[k];
        }
    }
    const long long local = i - first;
    const int r = (int)(local / cpr);
    const int c = (int)(local - (long long)r * cpr);
    const int sr = p.src_row[r];
    if (sr < 0) return;      // this destination row is not touched at all
    const size_t row_elems = (size_t)cpr * 8;
    it.d = dst + (size_t)r * row_elems + (size_t)c * 8;
    it.sv = *reinterpret_cast<const f16x8*>(p.src[s] + (size_t)sr * row_elems + (size_t)c * 8);
    it.dv = *reinterpret_cast<const f16x8*>(it.d);
    it.sc = p.scale[(size_t)s * p.nb + r];
    it.on = true;
}

__global__ __launch_bounds__(256) void control_add_kernel(const ControlParams p) {
    const long long total = p.prefix[MDX_CONTROL_MAX_SEGS];
    const long long pass = (long long)gridDim.x * 256 * UNROLL;
    for (long long base = (long long)blockIdx.x * 256 * UNROLL + threadIdx.x; base < total; base += pass) {
        Item it[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) control_load(p, base + (long long)u * 256, it[u]);
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            if (!it[u].on) continue;
            f16x8 o;
#pragma unroll
            for (int e = 0; e < 8; ++e)
                o[e] = f16_rne_from_f32_bits(__builtin_fmaf(it[u].sc, (float)it[u].sv[e], (float)it[u].dv[e]));
            *reinterpret_cast<f16x8*>(it[u].d) = o;
        }
    }
}

__global__ __launch_bounds__(256) void silu_kernel(f16* __restrict__ x, size_t chunks) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < chunks; i += (size_t)gridDim.x * 256) {
        f16x8 v = *reinterpret_cast<const f16x8*>(x + i * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = (f16)silu_f((float)v[e]);
        *reinterpret_cast<f16x8*>(x + i * 8) = v;
    }
}

}  // namespace

extern "C" int mdx_control_add_f16(const mdx_control_add_desc* d, mdx_stream_t s) {
    MDX_REQUIRE(d, "mdx_control_add_f16: null descriptor");
    MDX_REQUIRE(d->n_seg >= 1 && d->n_seg <= MDX_CONTROL_MAX_SEGS, "mdx_control_add_f16: %d segments outside [1, %d]", d->n_seg,
                MDX_CONTROL_MAX_SEGS);
    MDX_REQUIRE(d->nb >= 1, "mdx_control_add_f16: nb must be >= 1 (got %d)", d->nb);
    MDX_REQUIRE(d->src && d->src_row && d->scale, "mdx_control_add_f16: null src / src_row / scale table");
    MDX_REQUIRE((size_t)d->src % 8 == 0 && (size_t)d->src_row % 4 == 0 && (size_t)d->scale % 4 == 0,
                "mdx_control_add_f16: misaligned src / src_row / scale table");
    ControlParams p;
    p.n_seg = d->n_seg, p.nb = d->nb;
    p.src = reinterpret_cast<const f16* const*>(d->src), p.src_row = d->src_row, p.scale = d->scale;
    long long total = 0;
    for (int k = 0; k < MDX_CONTROL_MAX_SEGS; ++k) {
        p.dst[k] = nullptr, p.cpr[k] = 1, p.prefix[k] = total;
        if (k >= d->n_seg) continue;
        MDX_REQUIRE(d->dst[k], "mdx_control_add_f16: segment %d has a null dst", k);
        MDX_REQUIRE((size_t)d->dst[k] % 16 == 0, "mdx_control_add_f16: dst of segment %d is not 16-byte aligned", k);
        MDX_REQUIRE(d->elems_per_row[k] >= 8 && d->elems_per_row[k] % 8 == 0,
                    "mdx_control_add_f16: elems_per_row of segment %d must be a positive multiple of 8 (got %d)", k,
                    d->elems_per_row[k]);
        p.dst[k] = (f16*)d->dst[k];
        p.cpr[k] = d->elems_per_row[k] / 8;
        total += (long long)p.cpr[k] * d->nb;
    }
    for (int k = d->n_seg; k <= MDX_CONTROL_MAX_SEGS; ++k) p.prefix[k] = total;     // (entries past the last segment: the total)
    const int blocks = grid_for(((size_t)total + UNROLL - 1) / UNROLL);
    hipLaunchKernelGGL(control_add_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)s, p);
    MDX_LAUNCH_CHECK("mdx_control_add_f16");
    return MDX_OK;
}

extern "C" int mdx_silu_f16(void* x, size_t n, mdx_stream_t s) {
    MDX_REQUIRE(x && n > 0 && n % 8 == 0 && (size_t)x % 16 == 0,
                "mdx_silu_f16: x must be non-null and 16-byte aligned, n a positive multiple of 8");
    hipLaunchKernelGGL(silu_kernel, dim3(grid_for(n / 8)), dim3(256), 0, (hipStream_t)s, (f16*)x, n / 8);
    MDX_LAUNCH_CHECK("mdx_silu_f16");
    return MDX_OK;
}
