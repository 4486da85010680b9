// Inpainting, the work around the sampler (wukong-huahua/inpaint.py): the masked image (:55), c_concat = cat(nearest-resized
// mask, scaled posterior sample of the masked image's moments) (:76-85), a feathered compositing weight, and the output stage
// clamp((alpha decoded + (1 - alpha) image + 1) / 2, 0, 1) with its 8-bit NHWC form (:110-115).  fp32 NCHW elementwise work,
// memory-bound: one float4 (or, where a pointer or an extent does not allow it, one float) per lane and iteration, one-wave
// workgroups and a capped grid with a grid-stride loop, as csrc/qsample.hip.  The feather is the one kernel with a neighbourhood:
// a 32 x 32 output tile whose halo sits in LDS as bytes (the mask is binary), rows then columns.
// Mask convention everywhere: value >= 0.5 is the hole.  All argument checks run on the host, before any launch.
#include "mdx_common.h"

namespace {

constexpr int IP_THREADS = 64;
constexpr int IP_MAX_BLOCKS = 4096;     // 256 CUs x 16 waves; larger tensors take further passes of the grid-stride loop

template <int V>
__device__ __forceinline__ void load_v(const float* p, float (&v)[V]) {
    if constexpr (V == 4) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(p);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
        v[0] = *p;
    }
}

template <int V>
__device__ __forceinline__ void store_v(float* p, const float (&v)[V]) {
    if constexpr (V == 4) {
        f32x4 t;
        t.x = v[0]; t.y = v[1]; t.z = v[2]; t.w = v[3];
        *reinterpret_cast<f32x4*>(p) = t;
    } else {
        *p = v[0];
    }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

inline bool overlaps(const void* p, size_t pbytes, const void* q, size_t qbytes) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + qbytes && b < a + pbytes;
}

inline int ip_blocks(size_t items) {
    const size_t blocks = (items + IP_THREADS - 1) / IP_THREADS;
    return (int)(blocks < (size_t)IP_MAX_BLOCKS ? blocks : (size_t)IP_MAX_BLOCKS);
}

// ---------------------------------------------------------------------------------------------------------------- masked image
struct MaskImageParams {
    const float* image;
    const float* mask;
    float* out;
    int mask_b, C, HW;
    size_t total;           // B * C * HW
};

// V elements of one (b, c) plane per lane (V == 4 needs HW % 4 == 0 and 16-byte aligned pointers: the host decides)
template <int V>
__global__ __launch_bounds__(IP_THREADS) void mask_image_kernel(const MaskImageParams p) {
    const size_t n = p.total / V;
    for (size_t j = (size_t)blockIdx.x * IP_THREADS + threadIdx.x; j < n; j += (size_t)gridDim.x * IP_THREADS) {
        const size_t i = j * V;
        const size_t bc = i / p.HW;
        const size_t pix = i - bc * p.HW;
        const size_t b = p.mask_b == 1 ? 0 : bc / p.C;
        float x[V], m[V];
        load_v<V>(p.image + i, x);
        load_v<V>(p.mask + b * p.HW + pix, m);
#pragma unroll
        for (int e = 0; e < V; ++e) x[e] = x[e] * (m[e] < 0.5f ? 1.0f : 0.0f);     // image * (mask < 0.5), the bool as a float
        store_v<V>(p.out + i, x);
    }
}

// ---------------------------------------------------------------------------------------------------------------- c_concat
struct ConcatParams {
    const f16* mom;             // NHWC fp16 [B][hw][ld] = [mean (zc) | logvar (zc) | pad]
    const float* post_noise;    // NULL: the mode
    const float* mask;          // [mask_b][1][H][W]
    float* out;                 // [B][1 + zc][h][w]
    float scale;
    int mask_b, H, W, zc, h, w, ld;
    size_t total;               // B * (1 + zc) * h * w
};

// V consecutive pixels of one (b, c') plane of out per lane.  c' == 0: the mask at the latent grid; c' >= 1: channel c' - 1 of the
// posterior sample, read as in vae_encode_noised_kernel (qsample.hip).
template <int V>
__global__ __launch_bounds__(IP_THREADS) void concat_kernel(const ConcatParams p) {
    const size_t n = p.total / V;
    const int hw = p.h * p.w;
    for (size_t j = (size_t)blockIdx.x * IP_THREADS + threadIdx.x; j < n; j += (size_t)gridDim.x * IP_THREADS) {
        const size_t i = j * V;
        const int pix = (int)(i % hw);
        const size_t bc = i / hw;
        const int cc = (int)(bc % (p.zc + 1)), b = (int)(bc / (p.zc + 1));
        float o[V];
        if (cc == 0) {
            const float* mk = p.mask + (size_t)(p.mask_b == 1 ? 0 : b) * p.H * p.W;
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const int y = (pix + e) / p.w, x = (pix + e) - y * p.w;
                const int sy = (int)(((long long)y * p.H) / p.h), sx = (int)(((long long)x * p.W) / p.w);   // < H, < W
                o[e] = mk[(size_t)sy * p.W + sx] >= 0.5f ? 1.0f : 0.0f;
            }
        } else {
            const int c = cc - 1;
            const f16* m = p.mom + ((size_t)b * hw + pix) * p.ld;
            float pn[V];
            if (p.post_noise) load_v<V>(p.post_noise + ((size_t)b * p.zc + c) * hw + pix, pn);
#pragma unroll
            for (int e = 0; e < V; ++e) {
                // vae_encode_noised_kernel's statements (qsample.hip), in its order: z0_out there is this, bit for bit
                const float mean = (float)m[(size_t)e * p.ld + c];
                float lv = (float)m[(size_t)e * p.ld + p.zc + c];
                lv = fminf(fmaxf(lv, -30.0f), 20.0f);
                const float z = p.post_noise ? mean + __expf(0.5f * lv) * pn[e] : mean;
                o[e] = p.scale * z;
            }
        }
        store_v<V>(p.out + i, o);
    }
}

// ---------------------------------------------------------------------------------------------------------------- feather
constexpr int FT_TILE = 32;             // output tile, both directions
constexpr int FT_THREADS = 256;
constexpr int FT_MAX_RADIUS = 48;       // LDS: (32 + 96)^2 bytes + (32 + 96) * 32 floats = 32 KiB at the cap

// One block per (tile, mask).  Phase 1: the binarised tile with its halo (replicate edges = clamped source coordinates) into LDS
// as bytes.  Phase 2: rows -- tmp[r][c] = sum_k w[k] m[r][c + k] for every halo row.  Phase 3: columns, max with m, clamp, store.
// Lanes walk the fastest dimension in every phase: byte reads of 4 neighbouring lanes share a dword (broadcast), float reads are
// consecutive dwords -- no bank conflicts.
__global__ __launch_bounds__(FT_THREADS) void feather_kernel(const float* __restrict__ mask, const float* __restrict__ wts,
                                                             int R, float* __restrict__ out, int H, int W) {
    extern __shared__ unsigned char ft_lds[];
    const int span = FT_TILE + 2 * R;                   // halo tile edge
    float* tmp = reinterpret_cast<float*>(ft_lds);      // [span][FT_TILE]
    unsigned char* mt = ft_lds + (size_t)span * FT_TILE * sizeof(float);   // [span][span]
    const int x0 = blockIdx.x * FT_TILE, y0 = blockIdx.y * FT_TILE;
    const float* mk = mask + (size_t)blockIdx.z * H * W;
    float* o = out + (size_t)blockIdx.z * H * W;
    for (int t = threadIdx.x; t < span * span; t += FT_THREADS) {
        const int ly = t / span, lx = t - ly * span;
        const int gy = min(max(y0 + ly - R, 0), H - 1), gx = min(max(x0 + lx - R, 0), W - 1);
        mt[t] = mk[(size_t)gy * W + gx] >= 0.5f ? 1 : 0;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < span * FT_TILE; t += FT_THREADS) {
        const int r = t / FT_TILE, c = t - r * FT_TILE;
        const unsigned char* row = mt + r * span + c;
        float acc = 0.0f;
        for (int k = 0; k <= 2 * R; ++k) acc = __builtin_fmaf(wts[k], (float)row[k], acc);
        tmp[t] = acc;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < FT_TILE * FT_TILE; t += FT_THREADS) {
        const int r = t / FT_TILE, c = t - r * FT_TILE;
        const int gy = y0 + r, gx = x0 + c;
        if (gy >= H || gx >= W) continue;
        float acc = 0.0f;
        for (int k = 0; k <= 2 * R; ++k) acc = __builtin_fmaf(wts[k], tmp[(r + k) * FT_TILE + c], acc);
        const float m = (float)mt[(r + R) * span + c + R];
        o[(size_t)gy * W + gx] = fminf(fmaxf(m, acc), 1.0f);
    }
}

// ---------------------------------------------------------------------------------------------------------------- composite
struct CompositeParams {
    const float* dec;
    const float* image;
    const float* alpha;         // NULL: alpha == 1, image is not read
    float* out_f32;             // NCHW, may be NULL
    unsigned char* out_u8;      // NHWC, may be NULL
    int alpha_b, C, HW;
    size_t total;               // B * HW
};

// alpha d + (1 - alpha) img: alpha == 0 returns img and alpha == 1 returns d, bit for bit (finite d / img)
__device__ __forceinline__ float blend_f(float a, float d, float img) { return __builtin_fmaf(a, d, (1.0f - a) * img); }

// torch.clamp((t + 1.0) / 2.0, 0.0, 1.0): the division by two is the exact multiplication
__device__ __forceinline__ float to_unit_f(float t) { return fminf(fmaxf((t + 1.0f) * 0.5f, 0.0f), 1.0f); }

// V consecutive pixels of one sample per lane, all C channels of them: the NCHW planes move as float4, the NHWC bytes of the V
// pixels are V * C consecutive bytes.  C3: C == 3 and V == 4 with a 4-byte aligned out_u8 -- the 12 bytes leave as three dwords.
template <int V, bool C3>
__global__ __launch_bounds__(IP_THREADS) void composite_kernel(const CompositeParams p) {
    const size_t n = p.total / V;
    for (size_t j = (size_t)blockIdx.x * IP_THREADS + threadIdx.x; j < n; j += (size_t)gridDim.x * IP_THREADS) {
        const size_t i = j * V;
        const size_t b = i / p.HW;
        const size_t pix = i - b * p.HW;
        float a[V];
        if (p.alpha) load_v<V>(p.alpha + (p.alpha_b == 1 ? 0 : b) * p.HW + pix, a);
        unsigned bytes[C3 ? 12 : 1];
        const int C = C3 ? 3 : p.C;      // (a constant bound: the optimizer unrolls it and `bytes` stays in registers)
        for (int c = 0; c < C; ++c) {
            const size_t at = (b * p.C + c) * p.HW + pix;
            float d[V], v[V];
            load_v<V>(p.dec + at, d);
            if (p.alpha) {
                float im[V];
                load_v<V>(p.image + at, im);
#pragma unroll
                for (int e = 0; e < V; ++e) d[e] = blend_f(a[e], d[e], im[e]);
            }
#pragma unroll
            for (int e = 0; e < V; ++e) v[e] = to_unit_f(d[e]);
            if (p.out_f32) store_v<V>(p.out_f32 + at, v);
            if (p.out_u8) {
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    const unsigned q = (unsigned)(unsigned char)(v[e] * 255.0f);      // truncation; v is in [0, 1]
                    if constexpr (C3) {
                        if (c == 0) bytes[e * 3] = q;
                        else if (c == 1) bytes[e * 3 + 1] = q;
                        else bytes[e * 3 + 2] = q;
                    } else {
                        p.out_u8[(i + e) * p.C + c] = (unsigned char)q;
                    }
                }
            }
        }
        if constexpr (C3) {
            if (p.out_u8) {
                unsigned* o = reinterpret_cast<unsigned*>(p.out_u8 + i * 3);
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    o[k] = bytes[4 * k] | (bytes[4 * k + 1] << 8) | (bytes[4 * k + 2] << 16) | (bytes[4 * k + 3] << 24);
            }
        }
    }
}

}  // namespace

extern "C" int mdx_inpaint_mask_image_f32(const float* image, const float* mask, int mask_b, float* out, int B, int C, int HW,
                                          mdx_stream_t s) {
    MDX_REQUIRE(image && mask && out, "mdx_inpaint_mask_image_f32: null pointer");
    MDX_REQUIRE(B > 0 && C > 0 && HW > 0, "mdx_inpaint_mask_image_f32: bad extents (B=%d C=%d HW=%d)", B, C, HW);
    MDX_REQUIRE(mask_b == 1 || mask_b == B, "mdx_inpaint_mask_image_f32: mask_b must be 1 or B (mask_b=%d B=%d)", mask_b, B);
    MaskImageParams p;
    p.image = image; p.mask = mask; p.out = out;
    p.mask_b = mask_b; p.C = C; p.HW = HW;
    p.total = (size_t)B * C * HW;
    MDX_REQUIRE(!overlaps(out, p.total * sizeof(float), mask, (size_t)mask_b * HW * sizeof(float)),
                "mdx_inpaint_mask_image_f32: out overlaps mask");
    const bool vec = HW % 4 == 0 && aligned16(image) && aligned16(mask) && aligned16(out);
    if (vec)
        hipLaunchKernelGGL(mask_image_kernel<4>, dim3(ip_blocks(p.total / 4)), dim3(IP_THREADS), 0, (hipStream_t)s, p);
    else
        hipLaunchKernelGGL(mask_image_kernel<1>, dim3(ip_blocks(p.total)), dim3(IP_THREADS), 0, (hipStream_t)s, p);
    MDX_LAUNCH_CHECK("mdx_inpaint_mask_image_f32");
    return MDX_OK;
}

extern "C" int mdx_inpaint_concat_f32(const void* moments, int ld, const float* post_noise, float scale_factor,
                                      const float* mask, int mask_b, int H, int W, float* out, int B, int zc, int h, int w,
                                      mdx_stream_t s) {
    MDX_REQUIRE(mask && out && (moments || zc == 0), "mdx_inpaint_concat_f32: null pointer");
    MDX_REQUIRE(B > 0 && zc >= 0 && h > 0 && w > 0 && H > 0 && W > 0 && ld >= 2 * zc,
                "mdx_inpaint_concat_f32: bad extents (B=%d zc=%d h=%d w=%d H=%d W=%d ld=%d)", B, zc, h, w, H, W, ld);
    MDX_REQUIRE((long long)h * w <= 0x7fffffffLL && (long long)H * W <= 0x7fffffffLL,
                "mdx_inpaint_concat_f32: bad extents (a plane of more than 2^31 - 1 pixels)");
    MDX_REQUIRE(mask_b == 1 || mask_b == B, "mdx_inpaint_concat_f32: mask_b must be 1 or B (mask_b=%d B=%d)", mask_b, B);
    ConcatParams p;
    p.mom = (const f16*)moments; p.post_noise = post_noise; p.mask = mask; p.out = out;
    p.scale = scale_factor;
    p.mask_b = mask_b; p.H = H; p.W = W; p.zc = zc; p.h = h; p.w = w; p.ld = ld;
    p.total = (size_t)B * (zc + 1) * h * w;
    const bool vec = (h * w) % 4 == 0 && aligned16(post_noise) && aligned16(out);
    if (vec)
        hipLaunchKernelGGL(concat_kernel<4>, dim3(ip_blocks(p.total / 4)), dim3(IP_THREADS), 0, (hipStream_t)s, p);
    else
        hipLaunchKernelGGL(concat_kernel<1>, dim3(ip_blocks(p.total)), dim3(IP_THREADS), 0, (hipStream_t)s, p);
    MDX_LAUNCH_CHECK("mdx_inpaint_concat_f32");
    return MDX_OK;
}

extern "C" int mdx_mask_feather_f32(const float* mask, const float* weights, int radius, float* out, int Bm, int H, int W,
                                    mdx_stream_t s) {
    MDX_REQUIRE(mask && weights && out, "mdx_mask_feather_f32: null pointer");
    MDX_REQUIRE(Bm > 0 && H > 0 && W > 0, "mdx_mask_feather_f32: bad extents (Bm=%d H=%d W=%d)", Bm, H, W);
    MDX_REQUIRE((long long)H * W <= 0x7fffffffLL, "mdx_mask_feather_f32: bad extents (a plane of more than 2^31 - 1 pixels)");
    MDX_REQUIRE(radius >= 0 && radius <= FT_MAX_RADIUS, "mdx_mask_feather_f32: radius must be in [0, %d], got %d", FT_MAX_RADIUS,
                radius);
    const int tiles_x = (W + FT_TILE - 1) / FT_TILE, tiles_y = (H + FT_TILE - 1) / FT_TILE;
    MDX_REQUIRE(tiles_y <= 65535 && Bm <= 65535, "mdx_mask_feather_f32: bad extents (grid: %d tile rows, %d masks)", tiles_y, Bm);
    const size_t bytes = (size_t)Bm * H * W * sizeof(float);
    MDX_REQUIRE(!overlaps(out, bytes, mask, bytes), "mdx_mask_feather_f32: out overlaps mask");
    const int span = FT_TILE + 2 * radius;
    const size_t lds = (size_t)span * FT_TILE * sizeof(float) + (size_t)span * span;
    hipLaunchKernelGGL(feather_kernel, dim3(tiles_x, tiles_y, Bm), dim3(FT_THREADS), lds, (hipStream_t)s, mask, weights, radius,
                       out, H, W);
    MDX_LAUNCH_CHECK("mdx_mask_feather_f32");
    return MDX_OK;
}

extern "C" int mdx_inpaint_composite_f32(const float* decoded, const float* image, const float* alpha, int alpha_b,
                                         float* out_f32, unsigned char* out_u8, int B, int C, int H, int W, mdx_stream_t s) {
    MDX_REQUIRE(decoded && (image || !alpha), "mdx_inpaint_composite_f32: null pointer");
    MDX_REQUIRE(out_f32 || out_u8, "mdx_inpaint_composite_f32: no output (out_f32 and out_u8 are both null)");
    MDX_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0, "mdx_inpaint_composite_f32: bad extents (B=%d C=%d H=%d W=%d)", B, C, H, W);
    MDX_REQUIRE((long long)H * W <= 0x7fffffffLL, "mdx_inpaint_composite_f32: bad extents (a plane of more than 2^31 - 1 pixels)");
    MDX_REQUIRE(!alpha || alpha_b == 1 || alpha_b == B, "mdx_inpaint_composite_f32: alpha_b must be 1 or B (alpha_b=%d B=%d)",
                alpha_b, B);
    const int HW = H * W;
    const size_t bytes = (size_t)B * C * HW * sizeof(float);
    MDX_REQUIRE(!out_f32 || (!overlaps(out_f32, bytes, decoded, bytes) && !(alpha && overlaps(out_f32, bytes, image, bytes)) &&
                             !(alpha && overlaps(out_f32, bytes, alpha, (size_t)alpha_b * HW * sizeof(float)))),
                "mdx_inpaint_composite_f32: out_f32 overlaps an input");
    CompositeParams p;
    p.dec = decoded; p.image = alpha ? image : nullptr; p.alpha = alpha; p.out_f32 = out_f32; p.out_u8 = out_u8;
    p.alpha_b = alpha_b; p.C = C; p.HW = HW;
    p.total = (size_t)B * HW;
    const bool vec = HW % 4 == 0 && aligned16(decoded) && aligned16(p.image) && aligned16(alpha) && aligned16(out_f32);
    const bool c3 = vec && C == 3 && ((uintptr_t)out_u8 & 3) == 0;
    if (c3)
        hipLaunchKernelGGL((composite_kernel<4, true>), dim3(ip_blocks(p.total / 4)), dim3(IP_THREADS), 0, (hipStream_t)s, p);
    else if (vec)
        hipLaunchKernelGGL((composite_kernel<4, false>), dim3(ip_blocks(p.total / 4)), dim3(IP_THREADS), 0, (hipStream_t)s, p);
    else
        hipLaunchKernelGGL((composite_kernel<1, false>), dim3(ip_blocks(p.total)), dim3(IP_THREADS), 0, (hipStream_t)s, p);
    MDX_LAUNCH_CHECK("mdx_inpaint_composite_f32");
    return MDX_OK;
}
