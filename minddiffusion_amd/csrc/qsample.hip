// Forward-process sampling for img2img: q(x_t | x_0) = a x0 + b noise (ddpm.py:197-200), optionally blended into a running
// latent under a mask (plms.py:153-157), and the same statement fused onto AutoencoderKL.encode's posterior sample
// (autoencoder.py:70-78).  fp32 NCHW elementwise work: memory-bound, one float4 (or, where a pointer or an extent does not
// allow it, one float) per lane and iteration, one-wave workgroups so that a 2 x 4 x 64 x 64 latent already spreads over 128 CUs.
#include "mdx_common.h"
#include "qsample_device.h"

namespace {

constexpr int QS_THREADS = 64;
constexpr int QS_MAX_BLOCKS = 4096;     // 256 CUs x 16 waves; larger tensors take further passes of the grid-stride loop

// q_sample_f, blend_f, load_v and store_v live in qsample_device.h: the per-slot blend of rng.hip runs the same bodies.

struct QSampleParams {
    const float* x0;
    const float* noise;
    const float* mask;      // NULL: no blend
    const float* img;
    float* out;
    float a, b;
    int mask_c, C, HW;
    size_t total;           // B * C * HW
};

// V elements of one (b, c) plane per lane (V == 4 needs HW % 4 == 0 and 16-byte aligned pointers: the host decides).
// No __restrict__ on img / out: out may alias img element for element -- img's V values are read before out's are stored.
template <int V>
__global__ __launch_bounds__(QS_THREADS) void q_sample_kernel(const QSampleParams p) {
    const size_t n = p.total / V;
    for (size_t j = (size_t)blockIdx.x * QS_THREADS + threadIdx.x; j < n; j += (size_t)gridDim.x * QS_THREADS) {
        const size_t i = j * V;
        float x[V], nz[V], q[V];
        load_v<V>(p.x0 + i, x);
        load_v<V>(p.noise + i, nz);
#pragma unroll
        for (int e = 0; e < V; ++e) q[e] = q_sample_f(x[e], nz[e], p.a, p.b);
        if (p.mask) {
            size_t mi = i;                                      // mask_c == C: the mask has the latent's own shape
            if (p.mask_c == 1) {                                // one mask plane per sample
                const size_t bc = i / p.HW;
                mi = (bc / p.C) * p.HW + (i - bc * p.HW);
            }
            float m[V], im[V];
            load_v<V>(p.mask + mi, m);
            load_v<V>(p.img + i, im);
#pragma unroll
            for (int e = 0; e < V; ++e) q[e] = blend_f(m[e], q[e], im[e]);
        }
        store_v<V>(p.out + i, q);
    }
}

struct EncodeNoisedParams {
    const f16* mom;             // NHWC fp16 [B][HW][ld] = [mean (zc) | logvar (zc) | pad]
    const float* post_noise;    // NULL: the mode
    const float* noise;
    float* z0;
    float* xt;
    float scale, a, b;
    int zc, HW, ld;
    size_t total;               // B * zc * HW
};

// V consecutive pixels of one (b, c) plane per lane: the fp32 NCHW tensors move as float4, the moments -- whose channel
// dimension lies across that direction -- as the 2 V halves the lane needs (neighbouring channels share their cache lines).
template <int V>
__global__ __launch_bounds__(QS_THREADS) void vae_encode_noised_kernel(const EncodeNoisedParams p) {
    const size_t n = p.total / V;
    for (size_t j = (size_t)blockIdx.x * QS_THREADS + threadIdx.x; j < n; j += (size_t)gridDim.x * QS_THREADS) {
        const size_t i = j * V;
        const int pix = (int)(i % p.HW);
        const size_t bc = i / p.HW;
        const int c = (int)(bc % p.zc), b = (int)(bc / p.zc);
        const f16* m = p.mom + ((size_t)b * p.HW + pix) * p.ld;
        float pn[V], z0[V];
        if (p.post_noise) load_v<V>(p.post_noise + i, pn);
#pragma unroll
        for (int e = 0; e < V; ++e) {
            // gaussian_sample_kernel's statements (vae.hip)
            const float mean = (float)m[(size_t)e * p.ld + c];
            float lv = (float)m[(size_t)e * p.ld + p.zc + c];
            lv = fminf(fmaxf(lv, -30.0f), 20.0f);
            const float z = p.post_noise ? mean + __expf(0.5f * lv) * pn[e] : mean;
            z0[e] = p.scale * z;
        }
        if (p.z0) store_v<V>(p.z0 + i, z0);
        if (p.xt) {
            float nz[V], xt[V];
            load_v<V>(p.noise + i, nz);
#pragma unroll
            for (int e = 0; e < V; ++e) xt[e] = q_sample_f(z0[e], nz[e], p.a, p.b);
            store_v<V>(p.xt + i, xt);
        }
    }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

inline bool overlaps(const void* p, size_t pbytes, const void* q, size_t qbytes) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + qbytes && b < a + pbytes;
}

inline int qs_blocks(size_t items) {
    const size_t blocks = (items + QS_THREADS - 1) / QS_THREADS;
    return (int)(blocks < (size_t)QS_MAX_BLOCKS ? blocks : (size_t)QS_MAX_BLOCKS);
}

}  // namespace

extern "C" int mdx_q_sample_f32(const float* x0, const float* noise, float a, float b, const float* mask, int mask_c,
                                const float* img, float* out, int B, int C, int HW, mdx_stream_t s) {
    MDX_REQUIRE(x0 && noise && out, "mdx_q_sample_f32: null pointer");
    MDX_REQUIRE(B > 0 && C > 0 && HW > 0, "mdx_q_sample_f32: bad extents (B=%d C=%d HW=%d)", B, C, HW);
    MDX_REQUIRE(!mask || img, "mdx_q_sample_f32: mask needs img");
    MDX_REQUIRE(!mask || mask_c == 1 || mask_c == C, "mdx_q_sample_f32: mask_c must be 1 or C (mask_c=%d C=%d)", mask_c, C);
    const size_t total = (size_t)B * C * HW, bytes = total * sizeof(float);
    MDX_REQUIRE(!overlaps(out, bytes, x0, bytes) && !overlaps(out, bytes, noise, bytes) &&
                    !(mask && overlaps(out, bytes, mask, (size_t)B * mask_c * HW * sizeof(float))) &&
                    !(mask && img != out && overlaps(out, bytes, img, bytes)),
                "mdx_q_sample_f32: out may alias img element for element and nothing else");
    QSampleParams p;
    p.x0 = x0; p.noise = noise; p.mask = mask; p.img = mask ? img : nullptr; p.out = out;
    p.a = a; p.b = b;
    p.mask_c = mask_c; p.C = C; p.HW = HW;
    p.total = total;
    const bool vec = HW % 4 == 0 && aligned16(x0) && aligned16(noise) && aligned16(out) &&
                     (!mask || (aligned16(mask) && aligned16(img)));
    if (vec)
        hipLaunchKernelGGL(q_sample_kernel<4>, dim3(qs_blocks(total / 4)), dim3(QS_THREADS), 0, (hipStream_t)s, p);
    else
        hipLaunchKernelGGL(q_sample_kernel<1>, dim3(qs_blocks(total)), dim3(QS_THREADS), 0, (hipStream_t)s, p);
    MDX_LAUNCH_CHECK("mdx_q_sample_f32");
    return MDX_OK;
}

extern "C" int mdx_vae_encode_noised_f32(const void* moments, int ld, const float* post_noise, float scale_factor, float a,
                                         float b, const float* noise, float* z0_out, float* xt_out, int B, int zc, int HW,
                                         mdx_stream_t s) {
    MDX_REQUIRE(moments, "mdx_vae_encode_noised_f32: null pointer");
    MDX_REQUIRE(B > 0 && zc > 0 && HW > 0 && ld >= 2 * zc, "mdx_vae_encode_noised_f32: bad extents (B=%d zc=%d HW=%d ld=%d)", B,
                zc, HW, ld);
    MDX_REQUIRE(z0_out || xt_out, "mdx_vae_encode_noised_f32: no output (z0_out and xt_out are both null)");
    MDX_REQUIRE(!xt_out || noise, "mdx_vae_encode_noised_f32: xt_out needs a noise tensor");
    MDX_REQUIRE(z0_out != xt_out, "mdx_vae_encode_noised_f32: z0_out and xt_out must be different tensors");
    EncodeNoisedParams p;
    p.mom = (const f16*)moments; p.post_noise = post_noise; p.noise = xt_out ? noise : nullptr;
    p.z0 = z0_out; p.xt = xt_out;
    p.scale = scale_factor; p.a = a; p.b = b;
    p.zc = zc; p.HW = HW; p.ld = ld;
    p.total = (size_t)B * zc * HW;
    const bool vec = HW % 4 == 0 && aligned16(post_noise) && aligned16(p.noise) && aligned16(z0_out) && aligned16(xt_out);
    if (vec)
        hipLaunchKernelGGL(vae_encode_noised_kernel<4>, dim3(qs_blocks(p.total / 4)), dim3(QS_THREADS), 0, (hipStream_t)s, p);
    else
        hipLaunchKernelGGL(vae_encode_noised_kernel<1>, dim3(qs_blocks(p.total)), dim3(QS_THREADS), 0, (hipStream_t)s, p);
    MDX_LAUNCH_CHECK("mdx_vae_encode_noised_f32");
    return MDX_OK;
}
