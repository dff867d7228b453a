// lpips.hip -- the pieces of the LPIPS (AlexNet, v0.1) perceptual distance that are not convolutions.
//
// The sender's decision rule compares generated frames with the originals by LPIPS (reference city_sender.py:302 builds
// lpips.LPIPS(net='alex'), :376-406 decide_5to5_lpips keeps a frame while the distance stays under the threshold).  The
// algorithm as the reference vendors it (models/networks_basic.py:62-93 PNetLin.forward + ScalingLayer, models/eval_models.py:35-37
// normalize_tensor, models/pretrained_networks.py:56-94 AlexNet slices; restated in oracle/lpips.py):
//     x -> (x - shift) / scale                                            (ScalingLayer, per RGB channel)
//     AlexNet features: conv 11x11 s4 p2 (3->64) ReLU | maxpool 3 s2, conv 5x5 p2 (64->192) ReLU |
//                       maxpool 3 s2, conv 3x3 (192->384) ReLU | conv 3x3 (384->256) ReLU | conv 3x3 (256->256) ReLU
//     per tap k of the five ReLU outputs: unit-normalise over channels (x / (|x|_2 + 1e-10)), squared difference of the two
//     images, 1x1 convolution with the learned non-negative weights lin_k (one output channel), spatial mean; sum over k.
// The convolutions run on evc_conv2d_nhwc_f32 (exact bf16 split: the inputs are not normalised); this file holds
//   * evc_im2col_nchw_f32: the stride-4 11x11 first convolution as patches -> rows of a matrix (the scaling layer fused in, zero
//     padding applied AFTER the scaling as the convolution does), so that it becomes a 1x1 convolution over 363 (padded 368) channels;
//   * evc_maxpool3s2_nhwc_f32: MaxPool2d(kernel 3, stride 2), floor mode, no padding;
//   * evc_lpips_layer_f32: normalise + squared difference + lin_k + spatial mean of one tap, accumulated into the distance.
// The whole family (models/networks_basic.py:25-88 PNetLin with vgg / alex / squeeze, models/pretrained_networks.py:5-134) and
// its spatial form (fvd_utils/calculate_lpips.py:9-58, LPIPS(spatial=True)) add
//   * evc_maxpool2d_nhwc_f32: MaxPool2d(2, 2) of VGG16 and MaxPool2d(3, 2, ceil_mode=True) of SqueezeNet 1.1;
//   * evc_lpips_map_f32: the per-pixel distance of one tap, a grid over all N*HW pixels (VGG's first tap is 128x128x64 per image);
//   * evc_lpips_map_mean_f32: its spatial mean, accumulated into the distance;
//   * evc_lpips_upsample_add_f32: its bilinear up-sampling to the image size, accumulated into the spatial map.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/evc_hip.h"

namespace {

// Running max that keeps a NaN, as torch's max_pool does (fmaxf returns the operand that is not NaN).
__device__ __forceinline__ float max_nan(float m, float v) { return (v > m || v != v) ? v : m; }

// out[n][oy][ox][(c*KH + ky)*KW + kx] = in-range ? (x[n][c][oy*s - pad + ky][ox*s - pad + kx] - shift[c]) / scale[c] : 0;
// channels K = C*KH*KW .. ld_out-1 are zero.  One thread per output element (coalesced writes along the patch axis).
__global__ void im2col_kernel(const float* __restrict__ x, float* __restrict__ out, int C, int H, int W, int KH, int KW,
                              int stride, int pad, int Ho, int Wo, int ld_out, const float* __restrict__ shift,
                              const float* __restrict__ scale, size_t total) {
    const int K = C * KH * KW;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int k = (int)(i % ld_out);
        const size_t pix = i / ld_out;
        const int ox = (int)(pix % Wo);
        const int oy = (int)((pix / Wo) % Ho);
        const size_t n = pix / ((size_t)Wo * Ho);
        float v = 0.f;
        if (k < K) {
            const int c = k / (KH * KW), r = k - c * KH * KW;
            const int ky = r / KW, kx = r - ky * KW;
            const int yy = oy * stride - pad + ky, xx = ox * stride - pad + kx;
            if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
                v = x[((n * C + c) * H + yy) * W + xx];
                if (shift) v = (v - shift[c]) / scale[c];
            }
        }
        out[i] = v;
    }
}

__global__ void maxpool3s2_kernel(const float4* __restrict__ x, float4* __restrict__ out, int H, int W, int C4, int Ho, int Wo,
                                  size_t total) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % C4);
        const size_t pix = i / C4;
        const int ox = (int)(pix % Wo);
        const int oy = (int)((pix / Wo) % Ho);
        const size_t n = pix / ((size_t)Wo * Ho);
        float4 m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const float4 v = x[((n * H + (2 * oy + ky)) * W + (2 * ox + kx)) * C4 + c];
                m.x = max_nan(m.x, v.x); m.y = max_nan(m.y, v.y); m.z = max_nan(m.z, v.z); m.w = max_nan(m.w, v.w);
            }
        out[i] = m;
    }
}

// One workgroup (256 threads = 4 waves) per image pair; a wave takes pixels wave, wave + 4, ...; its lanes stride the channels.
// Fixed assignment and fixed reduction trees: deterministic.
__global__ __launch_bounds__(256) void lpips_layer_kernel(const float* __restrict__ f0, const float* __restrict__ f1,
                                                          const float* __restrict__ w, float* __restrict__ dist, int HW, int C,
                                                          int accumulate) {
    __shared__ float red[4];
    const int n = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* a = f0 + (size_t)n * HW * C;
    const float* b = f1 + (size_t)n * HW * C;
    float acc = 0.f;
    for (int p = wave; p < HW; p += 4) {
        const float* ap = a + (size_t)p * C;
        const float* bp = b + (size_t)p * C;
        float sa = 0.f, sb = 0.f;
        for (int c = lane; c < C; c += 64) { const float u = ap[c], v = bp[c]; sa += u * u; sb += v * v; }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { sa += __shfl_xor(sa, off); sb += __shfl_xor(sb, off); }
        const float ia = 1.0f / (sqrtf(sa) + 1e-10f), ib = 1.0f / (sqrtf(sb) + 1e-10f);
        float d = 0.f;
        for (int c = lane; c < C; c += 64) { const float t = ap[c] * ia - bp[c] * ib; d += w[c] * t * t; }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) d += __shfl_xor(d, off);
        acc += d;                                  // identical in every lane
    }
    if (lane == 0) red[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        const float v = (red[0] + red[1] + red[2] + red[3]) / (float)HW;
        dist[n] = accumulate ? dist[n] + v : v;
    }
}

// MaxPool2d(k, stride), no padding, floor or ceil mode: window elements beyond the input are skipped (a ceil-mode window
// always starts inside, so it holds at least one element).  K is a template argument so that the window unrolls.
template <int K>
__global__ void maxpool2d_kernel(const float4* __restrict__ x, float4* __restrict__ out, int H, int W, int C4, int stride, int Ho,
                                 int Wo, size_t total) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % C4);
        const size_t pix = i / C4;
        const int ox = (int)(pix % Wo);
        const int oy = (int)((pix / Wo) % Ho);
        const size_t n = pix / ((size_t)Wo * Ho);
        float4 m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
#pragma unroll
        for (int ky = 0; ky < K; ++ky)
#pragma unroll
            for (int kx = 0; kx < K; ++kx) {
                const int yy = oy * stride + ky, xx = ox * stride + kx;
                if (yy < H && xx < W) {
                    const float4 v = x[((n * H + yy) * W + xx) * C4 + c];
                    m.x = max_nan(m.x, v.x); m.y = max_nan(m.y, v.y); m.z = max_nan(m.z, v.z); m.w = max_nan(m.w, v.w);
                }
            }
        out[i] = m;
    }
}

// map[g] = sum_c w[c] * (f0[g][c] / (|f0[g]|_2 + 1e-10) - f1[g][c] / (|f1[g]|_2 + 1e-10))^2 for the pixels g of all pairs.
// Lanes per pixel: 16, for every C.  The taps have 64 ... 512 channels, i.e. 16 ... 128 float4 per pixel and image: with 16-byte
// loads a 64-channel pixel fills exactly 16 lanes (a full wave would leave 48 of them idle or fall back to 4-byte loads), and a
// 512-channel pixel puts V = 8 float4 per image into each lane -- 64 registers for both images and 32 for the weights: 127 VGPRs
// and 4 waves per SIMD by the compiler's report, no scratch; the 64-channel taps, which carry most of the bytes, take 39 VGPRs
// and 8 waves.  A wave so covers 4 pixels whatever C is, each load instruction reads 256 contiguous bytes per pixel (1 KiB contiguous at
// C = 64), the reductions stay inside a 16-lane row (four xor steps, no LDS), and at HW = 1 a batch of N pairs still needs only
// N / 4 waves instead of N.  Both passes (norms, weighted difference) run on the registers: every element is read once.
// The assignment of channels to lanes and the reduction tree depend on C only: deterministic.
template <int V>
__global__ __launch_bounds__(256) void lpips_map_kernel(const float4* __restrict__ f0, const float4* __restrict__ f1,
                                                        const float4* __restrict__ w, float* __restrict__ map, size_t pixels) {
    const int sub = threadIdx.x & 15;
    const size_t first = (size_t)blockIdx.x * 16 + (threadIdx.x >> 4), step = (size_t)gridDim.x * 16;
    float4 wv[V];
#pragma unroll
    for (int j = 0; j < V; ++j) wv[j] = w[sub + 16 * j];
    for (size_t g = first; g < pixels; g += step) {
        const float4* a = f0 + g * (16 * V);
        const float4* b = f1 + g * (16 * V);
        float4 u[V], v[V];
#pragma unroll
        for (int j = 0; j < V; ++j) { u[j] = a[sub + 16 * j]; v[j] = b[sub + 16 * j]; }
        float sa = 0.f, sb = 0.f;
#pragma unroll
        for (int j = 0; j < V; ++j) {
            sa += u[j].x * u[j].x + u[j].y * u[j].y + u[j].z * u[j].z + u[j].w * u[j].w;
            sb += v[j].x * v[j].x + v[j].y * v[j].y + v[j].z * v[j].z + v[j].w * v[j].w;
        }
#pragma unroll
        for (int off = 8; off > 0; off >>= 1) { sa += __shfl_xor(sa, off); sb += __shfl_xor(sb, off); }
        const float ia = 1.0f / (sqrtf(sa) + 1e-10f), ib = 1.0f / (sqrtf(sb) + 1e-10f);
        float d = 0.f;
#pragma unroll
        for (int j = 0; j < V; ++j) {
            float tx, ty, tz, tw;
            {   // both products rounded before the subtraction: a contracted fma(u, ia, -(v * ib)) would leave a residue on
                // identical images, and d(x, x) must be exactly 0
#pragma clang fp contract(off)
                tx = u[j].x * ia - v[j].x * ib; ty = u[j].y * ia - v[j].y * ib;
                tz = u[j].z * ia - v[j].z * ib; tw = u[j].w * ia - v[j].w * ib;
            }
            d += wv[j].x * tx * tx + wv[j].y * ty * ty + wv[j].z * tz * tz + wv[j].w * tw * tw;
        }
#pragma unroll
        for (int off = 8; off > 0; off >>= 1) d += __shfl_xor(d, off);
        if (sub == 0) map[g] = d;
    }
}

// dist[n] (+)= mean_p map[n][p].  One workgroup per pair; thread t adds pixels t, t + 256, ... in order, then a fixed xor tree
// per wave and the four wave sums in order: the order depends on HW only.
__global__ __launch_bounds__(256) void lpips_map_mean_kernel(const float* __restrict__ map, float* __restrict__ dist, int HW,
                                                             int accumulate) {
    __shared__ float red[4];
    const int n = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* m = map + (size_t)n * HW;
    float acc = 0.f;
    for (int p = threadIdx.x; p < HW; p += 256) acc += m[p];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
    if (lane == 0) red[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        const float v = (red[0] + red[1] + red[2] + red[3]) / (float)HW;
        dist[n] = accumulate ? dist[n] + v : v;
    }
}

// torch's upsample_bilinear2d, align_corners = False, float32: source index max((dst + 0.5) * scale - 0.5, 0) with
// scale = in / out, the upper neighbour clamped to the last row / column, weights 1 - l and l.  One thread per output pixel.
// The operations are spelled out (contraction off, fmaf where torch's device kernel has a fused multiply-add: the source
// index, the first product of each row's sum and of the sum of the two rows), which reproduces that kernel bit for bit.
__global__ void lpips_upsample_add_kernel(const float* __restrict__ map, float* __restrict__ out, int h, int w, int H, int W,
                                          float sy, float sx, int accumulate, size_t total) {
#pragma clang fp contract(off)
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int ox = (int)(i % W);
        const int oy = (int)((i / W) % H);
        const size_t n = i / ((size_t)W * H);
        const float fy = fmaxf(fmaf(sy, (float)oy + 0.5f, -0.5f), 0.f), fx = fmaxf(fmaf(sx, (float)ox + 0.5f, -0.5f), 0.f);
        const int y0 = min((int)fy, h - 1), x0 = min((int)fx, w - 1);
        const int y1 = y0 + (y0 < h - 1 ? 1 : 0), x1 = x0 + (x0 < w - 1 ? 1 : 0);
        const float ly1 = fy - (float)y0, lx1 = fx - (float)x0;
        const float ly0 = 1.f - ly1, lx0 = 1.f - lx1;
        const float* m = map + n * ((size_t)h * w);
        const float r0 = fmaf(lx0, m[(size_t)y0 * w + x0], lx1 * m[(size_t)y0 * w + x1]);
        const float r1 = fmaf(lx0, m[(size_t)y1 * w + x0], lx1 * m[(size_t)y1 * w + x1]);
        const float v = fmaf(ly0, r0, ly1 * r1);
        out[i] = accumulate ? out[i] + v : v;
    }
}

}  // namespace

extern "C" int evc_im2col_nchw_f32(const float* x, float* out, int N, int C, int H, int W, int KH, int KW, int stride, int pad,
                                   int ld_out, const float* shift, const float* scale, void* stream) {
    if (!x || !out || N <= 0 || C <= 0 || H <= 0 || W <= 0 || KH <= 0 || KW <= 0 || stride <= 0 || pad < 0) return EVC_EINVAL;
    if ((shift == nullptr) != (scale == nullptr)) return EVC_EINVAL;
    const int Ho = (H + 2 * pad - KH) / stride + 1, Wo = (W + 2 * pad - KW) / stride + 1;
    if (Ho <= 0 || Wo <= 0 || ld_out < C * KH * KW) return EVC_EINVAL;
    const size_t total = (size_t)N * Ho * Wo * ld_out;
    const int grid = (int)((total + 255) / 256 > 8192 ? 8192 : (total + 255) / 256);
    hipLaunchKernelGGL(im2col_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, out, C, H, W, KH, KW, stride, pad, Ho, Wo,
                       ld_out, shift, scale, total);
    return hipGetLastError() == hipSuccess ? EVC_OK : EVC_ELAUNCH;
}

extern "C" int evc_maxpool3s2_nhwc_f32(const float* x, float* out, int N, int H, int W, int C, void* stream) {
    if (!x || !out || N <= 0 || H < 3 || W < 3 || C <= 0 || (C & 3)) return EVC_EINVAL;
    const int Ho = (H - 3) / 2 + 1, Wo = (W - 3) / 2 + 1;
    const size_t total = (size_t)N * Ho * Wo * (C / 4);
    const int grid = (int)((total + 255) / 256 > 8192 ? 8192 : (total + 255) / 256);
    hipLaunchKernelGGL(maxpool3s2_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const float4*>(x),
                       reinterpret_cast<float4*>(out), H, W, C / 4, Ho, Wo, total);
    return hipGetLastError() == hipSuccess ? EVC_OK : EVC_ELAUNCH;
}

extern "C" int evc_lpips_layer_f32(const float* f0, const float* f1, const float* lin_w, float* dist, int N, int HW, int C,
                                   int accumulate, void* stream) {
    if (!f0 || !f1 || !lin_w || !dist || N <= 0 || HW <= 0 || C <= 0) return EVC_EINVAL;
    hipLaunchKernelGGL(lpips_layer_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream, f0, f1, lin_w, dist, HW, C, accumulate);
    return hipGetLastError() == hipSuccess ? EVC_OK : EVC_ELAUNCH;
}

extern "C" int evc_maxpool2d_nhwc_f32(const float* x, float* out, int N, int H, int W, int C, int k, int stride, int ceil_mode,
                                      void* stream) {
    if (!x || !out || N <= 0 || C <= 0 || (C & 3) || (k != 2 && k != 3) || stride <= 0 || H <= 0 || W <= 0) return EVC_EINVAL;
    if (ceil_mode != 0 && ceil_mode != 1) return EVC_EINVAL;
    // torch's pooling_output_shape without padding: the last window of ceil mode must start inside the input.  A side shorter
    // than the window is legal in ceil mode as long as one window starts inside it (SqueezeNet's 2 x 1 tap pools to 1 x 1).
    const int round_up = ceil_mode ? stride - 1 : 0;
    if (H - k + round_up < 0 || W - k + round_up < 0) return EVC_EINVAL;
    int Ho = (H - k + round_up) / stride + 1, Wo = (W - k + round_up) / stride + 1;
    if (ceil_mode && (Ho - 1) * stride >= H) --Ho;
    if (ceil_mode && (Wo - 1) * stride >= W) --Wo;
    const size_t total = (size_t)N * Ho * Wo * (C / 4);
    const int grid = (int)((total + 255) / 256 > 8192 ? 8192 : (total + 255) / 256);
    auto kern = k == 2 ? maxpool2d_kernel<2> : maxpool2d_kernel<3>;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const float4*>(x),
                       reinterpret_cast<float4*>(out), H, W, C / 4, stride, Ho, Wo, total);
    return hipGetLastError() == hipSuccess ? EVC_OK : EVC_ELAUNCH;
}

extern "C" int evc_lpips_map_f32(const float* f0, const float* f1, const float* lin_w, float* map, int N, int HW, int C,
                                 void* stream) {
    if (!f0 || !f1 || !lin_w || !map || N <= 0 || HW <= 0 || C < 64 || C > 512 || (C & 63)) return EVC_EINVAL;
    if ((((uintptr_t)f0 | (uintptr_t)f1 | (uintptr_t)lin_w) & 15) != 0) return EVC_EINVAL;
    const size_t pixels = (size_t)N * HW;
    const size_t blocks = (pixels + 15) / 16;
    const dim3 grid((unsigned)(blocks > 16384 ? 16384 : blocks)), block(256);
    const float4* a = reinterpret_cast<const float4*>(f0);
    const float4* b = reinterpret_cast<const float4*>(f1);
    const float4* w = reinterpret_cast<const float4*>(lin_w);
    hipStream_t st = (hipStream_t)stream;
    switch (C / 64) {
        case 1: hipLaunchKernelGGL(lpips_map_kernel<1>, grid, block, 0, st, a, b, w, map, pixels); break;
        case 2: hipLaunchKernelGGL(lpips_map_kernel<2>, grid, block, 0, st, a, b, w, map, pixels); break;
        case 3: hipLaunchKernelGGL(lpips_map_kernel<3>, grid, block, 0, st, a, b, w, map, pixels); break;
        case 4: hipLaunchKernelGGL(lpips_map_kernel<4>, grid, block, 0, st, a, b, w, map, pixels); break;
        case 5: hipLaunchKernelGGL(lpips_map_kernel<5>, grid, block, 0, st, a, b, w, map, pixels); break;
        case 6: hipLaunchKernelGGL(lpips_map_kernel<6>, grid, block, 0, st, a, b, w, map, pixels); break;
        case 7: hipLaunchKernelGGL(lpips_map_kernel<7>, grid, block, 0, st, a, b, w, map, pixels); break;
        default: hipLaunchKernelGGL(lpips_map_kernel<8>, grid, block, 0, st, a, b, w, map, pixels); break;
    }
    return hipGetLastError() == hipSuccess ? EVC_OK : EVC_ELAUNCH;
}

extern "C" int evc_lpips_map_mean_f32(const float* map, float* dist, int N, int HW, int accumulate, void* stream) {
    if (!map || !dist || N <= 0 || HW <= 0) return EVC_EINVAL;
    hipLaunchKernelGGL(lpips_map_mean_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream, map, dist, HW, accumulate);
    return hipGetLastError() == hipSuccess ? EVC_OK : EVC_ELAUNCH;
}

extern "C" int evc_lpips_upsample_add_f32(const float* map, float* out, int N, int h, int w, int H, int W, int accumulate,
                                          void* stream) {
    if (!map || !out || N <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0) return EVC_EINVAL;
    const size_t total = (size_t)N * H * W;
    const int grid = (int)((total + 255) / 256 > 8192 ? 8192 : (total + 255) / 256);
    hipLaunchKernelGGL(lpips_upsample_add_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, map, out, h, w, H, W,
                       (float)h / (float)H, (float)w / (float)W, accumulate, total);
    return hipGetLastError() == hipSuccess ? EVC_OK : EVC_ELAUNCH;
}
