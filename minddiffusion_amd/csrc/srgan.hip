// SRGAN x2 / x4 / x8 post-upscaler of Taichu-GLIDE (vision/Taichu-GLIDE/model/glide_text2im/model/srgan.py:75-117): the two 9 x 9
// convolutions at the ends of the Generator.  Everything between them -- the 3 x 3 trunk, conv2 with its residual and the
// sub-pixel layers -- runs on mdx_gemm_f16 (MDX_EPI_PRELU, MDX_OUT_D2S2).
//
//   conv_in  = PReLU_64(Conv9x9(3 -> 64)(x))          srgan.py:83-85   fp32 NCHW image in, NHWC fp16 out (no layout launch)
//   conv_out = tanh(Conv9x9(64 -> 3)(t))               srgan.py:115-116 NHWC fp16 in, fp32 NCHW out (what sr_handle returns)
//
// Both are direct convolutions on the vector ALU with fp32 accumulation over fp16-rounded operands (docs/KERNELS.md has the
// rooflines).  conv_out uses v_dot2_f32_f16: two channels per instruction, 8 pixels x 3 outputs per thread, the input halo
// streamed through LDS in 8-channel chunks.
#include "mdx_common.h"

namespace {

constexpr int CI_TY = 32, CI_TX = 16;                 // conv_in output tile: 32 x 16 pixels, 2 per thread (rows ty, ty + 16)
constexpr int CI_HY = CI_TY + 8, CI_HX = CI_TX + 8;    // its input halo (pad 4 each side)

__global__ __launch_bounds__(256) void srgan_conv_in_kernel(const float* __restrict__ x, const f16* __restrict__ w,
                                                            const float* __restrict__ bias, const float* __restrict__ slope,
                                                            f16* __restrict__ out, int H, int W) {
    __shared__ float4 ws4[243 * 16];                   // [k = (ky * 9 + kx) * 3 + c][64 outputs] fp32 (fp16-rounded weights)
    __shared__ float xs[3][CI_HY][CI_HX];              // fp16-rounded input halo
    const int tid = threadIdx.x;
    const int b = blockIdx.z, y0 = blockIdx.y * CI_TY, x0 = blockIdx.x * CI_TX;
    float* wsf = reinterpret_cast<float*>(ws4);
    for (int i = tid; i < 243 * 64; i += 256) {        // reference layout [o][c][ky][kx] -> [(ky, kx, c)][o]
        const int o = i & 63, k = i >> 6;
        const int c = k % 3, t = k / 3;
        wsf[i] = (float)w[(o * 3 + c) * 81 + t];
    }
    for (int i = tid; i < 3 * CI_HY * CI_HX; i += 256) {
        const int c = i / (CI_HY * CI_HX), r = i - c * (CI_HY * CI_HX);
        const int yy = r / CI_HX, xx = r - yy * CI_HX;
        const int gy = y0 + yy - 4, gx = x0 + xx - 4;
        float v = 0.f;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = (float)(f16)x[(((size_t)b * 3 + c) * H + gy) * W + gx];
        xs[c][yy][xx] = v;
    }
    __syncthreads();
    const int ty = tid >> 4, tx = tid & 15;
    float acc0[64], acc1[64];
#pragma unroll
    for (int o = 0; o < 64; ++o) acc0[o] = acc1[o] = 0.f;
    for (int ky = 0; ky < 9; ++ky)
        for (int kx = 0; kx < 9; ++kx)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float a0 = xs[c][ty + ky][tx + kx], a1 = xs[c][ty + 16 + ky][tx + kx];
                const float4* wk = ws4 + ((ky * 9 + kx) * 3 + c) * 16;
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const float4 wv = wk[q];
                    acc0[4 * q] += a0 * wv.x; acc0[4 * q + 1] += a0 * wv.y; acc0[4 * q + 2] += a0 * wv.z; acc0[4 * q + 3] += a0 * wv.w;
                    acc1[4 * q] += a1 * wv.x; acc1[4 * q + 1] += a1 * wv.y; acc1[4 * q + 2] += a1 * wv.z; acc1[4 * q + 3] += a1 * wv.w;
                }
            }
    const int gx = x0 + tx;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int gy = y0 + ty + 16 * h;
        if (gy >= H || gx >= W) continue;
        f16* dst = out + (((size_t)b * H + gy) * W + gx) * 64;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            f16x8 o;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int n = 8 * q + e;
                const float v = (h ? acc1[n] : acc0[n]) + bias[n];
                o[e] = (f16)(v > 0.f ? v : slope[n] * v);
            }
            *reinterpret_cast<f16x8*>(dst + 8 * q) = o;
        }
    }
}

// conv_out: 32 x 64 output pixels per block; thread = (row, 8-pixel strip).  The halo of one 8-channel chunk sits in LDS as
// [40 rows][81 slots][8 ch] fp16 -- 72 pixels plus one pad slot per 8 pixels, so that the b128 reads of lanes 8 pixels apart
// fall on distinct banks.
constexpr int CO_TY = 32, CO_TX = 64;
constexpr int CO_HY = CO_TY + 8, CO_HX = CO_TX + 8;
constexpr int CO_SLOTS = CO_HX + CO_HX / 8;          // 81

__device__ __forceinline__ int co_slot(int xx) { return xx + (xx >> 3); }

__global__ __launch_bounds__(256) void srgan_conv_out_kernel(const f16* __restrict__ x, const f16* __restrict__ w,
                                                             const float* __restrict__ bias, float* __restrict__ out, int H, int W) {
    __shared__ f16x8 hs[CO_HY * CO_SLOTS];           // 51.8 KB
    __shared__ f16x8 wsm[81 * 3];                    // [tap][o] 8 channels of the chunk
    const int tid = threadIdx.x;
    const int b = blockIdx.z, y0 = blockIdx.y * CO_TY, x0 = blockIdx.x * CO_TX;
    const int ty = tid >> 3, sx = (tid & 7) * 8;
    float acc[3][8];
#pragma unroll
    for (int o = 0; o < 3; ++o)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[o][j] = 0.f;
    for (int ch = 0; ch < 64; ch += 8) {
        __syncthreads();                             // the previous chunk's reads are done
        for (int i = tid; i < CO_HY * CO_HX; i += 256) {
            const int yy = i / CO_HX, xx = i - yy * CO_HX;
            const int gy = y0 + yy - 4, gx = x0 + xx - 4;
            f16x8 v;
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = (f16)0.f;
            if (gy >= 0 && gy < H && gx >= 0 && gx < W)
                v = *reinterpret_cast<const f16x8*>(x + (((size_t)b * H + gy) * W + gx) * 64 + ch);
            hs[yy * CO_SLOTS + co_slot(xx)] = v;
        }
        if (tid < 243) {                             // reference layout [o][c][ky][kx] -> [tap][o][8 c]
            const int o = tid % 3, t = tid / 3;
            f16x8 v;
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = w[(o * 64 + ch + e) * 81 + t];
            wsm[tid] = v;
        }
        __syncthreads();
        for (int ky = 0; ky < 9; ++ky) {
            f16x8 row[16];
            const f16x8* hr = hs + (ty + ky) * CO_SLOTS;
#pragma unroll
            for (int j = 0; j < 16; ++j) row[j] = hr[co_slot(sx + j)];
#pragma unroll
            for (int kx = 0; kx < 9; ++kx)
#pragma unroll
                for (int o = 0; o < 3; ++o) {
                    const f16x8 wv = wsm[(ky * 9 + kx) * 3 + o];
#pragma unroll
                    for (int pr = 0; pr < 4; ++pr) {
                        const f16x2 wp = {wv[2 * pr], wv[2 * pr + 1]};
#pragma unroll
                        for (int j = 0; j < 8; ++j) {
                            const f16x2 ap = {row[j + kx][2 * pr], row[j + kx][2 * pr + 1]};
                            acc[o][j] = __builtin_amdgcn_fdot2(ap, wp, acc[o][j], false);
                        }
                    }
                }
        }
    }
    const int gy = y0 + ty;
    if (gy >= H) return;
#pragma unroll
    for (int o = 0; o < 3; ++o) {
        float* dst = out + (((size_t)b * 3 + o) * H + gy) * W + x0 + sx;
        const float bo = bias[o];
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (x0 + sx + j < W) dst[j] = tanhf(acc[o][j] + bo);
    }
}

}  // namespace

extern "C" int mdx_srgan_conv_in_f16(const float* x, const void* w, const float* bias, const float* slope, void* out, int B, int H,
                                     int W, mdx_stream_t s) {
    MDX_REQUIRE(x && w && bias && slope && out, "mdx_srgan_conv_in_f16: null pointer");
    // (every index is size_t: the x8 upscale of 8 x 256^2 reads / writes 4 GiB tensors)
    MDX_REQUIRE(B > 0 && H > 0 && W > 0 && B <= 65535 && (long)H * W < 0x80000000l,
                "mdx_srgan_conv_in_f16: bad extents (B=%d H=%d W=%d)", B, H, W);
    const dim3 grid((W + CI_TX - 1) / CI_TX, (H + CI_TY - 1) / CI_TY, B);
    hipLaunchKernelGGL(srgan_conv_in_kernel, grid, dim3(256), 0, (hipStream_t)s, x, (const f16*)w, bias, slope, (f16*)out, H, W);
    MDX_LAUNCH_CHECK("mdx_srgan_conv_in_f16");
    return MDX_OK;
}

extern "C" int mdx_srgan_conv_out_f32(const void* x, const void* w, const float* bias, float* out, int B, int H, int W,
                                      mdx_stream_t s) {
    MDX_REQUIRE(x && w && bias && out, "mdx_srgan_conv_out_f32: null pointer");
    // (every index is size_t: the x8 upscale of 8 x 256^2 reads / writes 4 GiB tensors)
    MDX_REQUIRE(B > 0 && H > 0 && W > 0 && B <= 65535 && (long)H * W < 0x80000000l,
                "mdx_srgan_conv_out_f32: bad extents (B=%d H=%d W=%d)", B, H, W);
    const dim3 grid((W + CO_TX - 1) / CO_TX, (H + CO_TY - 1) / CO_TY, B);
    hipLaunchKernelGGL(srgan_conv_out_kernel, grid, dim3(256), 0, (hipStream_t)s, (const f16*)x, (const f16*)w, bias, out, H, W);
    MDX_LAUNCH_CHECK("mdx_srgan_conv_out_f32");
    return MDX_OK;
}
