// i3d.hip -- the pieces of the I3D feature network (FVD) that are not convolutions.
//
// For each (video, q, threshold) job the reference reports the Frechet video distance between the decoded and the original
// clip (city_sender.py:264-279, :575-589): InceptionI3d(400) (models/fvd/pytorch_i3d.py) on preprocess_single's input
// (models/fvd/fvd.py: bilinear resize of the shorter side to 224, centre crop, (x - 0.5) * 2).  Every Unit3D and every
// MaxPool3dSamePadding pads TensorFlow-"same" with zeros (pytorch_i3d.py:9-34, :71-99).  Activations are NTHWC (B*T images of
// H x W x C); the 1x1x1 and 3x3x3 convolutions run on evc_conv2d_nhwc_f32 (3x3x3 via evc_frame_taps_f32).  This file holds
//   * evc_i3d_stem_im2col_f32: resize + crop + scale + same padding fused into the rows of the 7x7x7 stride-2 first convolution,
//     which then is a 1x1 convolution over 3*7*7*7 (padded) channels -- the resized video is never written;
//   * evc_maxpool3d_same_nthwc_f32: MaxPool3dSamePadding for any window / strides;
//   * evc_i3d_head_f32: AvgPool3d((kt, H, W), stride 1), the 1x1x1 logits unit with bias and the mean over the windows.
#include <hip/hip_runtime.h>
#include "../../include/evc_hip.h"

namespace {

// Running max that keeps a NaN, as torch's max_pool does (fmaxf returns the operand that is not NaN).
__device__ __forceinline__ float max_nan(float m, float v) { return (v > m || v != v) ? v : m; }

// PyTorch's bilinear source index, align_corners=False, output size given (area_pixel_compute_source_index).
struct Lin { int i0, i1; float l0, l1; };
__device__ inline Lin lin_src(int dst, float scale, int in) {
    float s = scale * (dst + 0.5f) - 0.5f;
    if (s < 0.f) s = 0.f;
    Lin r;
    r.i0 = (int)s;
    r.i1 = r.i0 + (r.i0 < in - 1 ? 1 : 0);
    r.l1 = s - (float)r.i0;
    r.l0 = 1.f - r.l1;
    return r;
}

// out[f - f_begin][oy][ox][((c*KT + kt)*KH + ky)*KW + kx] for the flattened output frames f = b*To + ot:
//   padded-video coordinate (t, y, x) = (ot*ST - pt + kt, oy*SH - ph + ky, ox*SW - pw + kx) of the R x R crop;
//   inside: (bilinear(x[b][t][c], h0 + y, w0 + x) - 0.5) * 2 on the Hr x Wr resize; outside: 0; columns >= C*KT*KH*KW: 0.
__global__ void i3d_stem_kernel(const float* __restrict__ x, float* __restrict__ out, int T, int C, int H, int W, int Hr, int Wr,
                                int h0, int w0, int R, int KT, int KH, int KW, int ST, int SH, int SW, int pt, int ph, int pw,
                                int To, int Ho, int Wo, int f_begin, int ld_out, size_t total) {
    const int K = C * KT * KH * KW;
    const float sh = (float)H / (float)Hr, sw = (float)W / (float)Wr;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int k = (int)(i % ld_out);
        const size_t pix = i / ld_out;
        const int ox = (int)(pix % Wo);
        const int oy = (int)((pix / Wo) % Ho);
        const int f = f_begin + (int)(pix / ((size_t)Wo * Ho));
        float v = 0.f;
        if (k < K) {
            const int kx = k % KW, ky = (k / KW) % KH, kt = (k / (KW * KH)) % KT, c = k / (KW * KH * KT);
            const int b = f / To, ot = f - b * To;
            const int t = ot * ST - pt + kt, yy = oy * SH - ph + ky, xx = ox * SW - pw + kx;
            if (t >= 0 && t < T && yy >= 0 && yy < R && xx >= 0 && xx < R) {
                const Lin ly = lin_src(h0 + yy, sh, H), lx = lin_src(w0 + xx, sw, W);
                const float* p = x + (((size_t)b * T + t) * C + c) * H * W;
                const float top = lx.l0 * p[ly.i0 * W + lx.i0] + lx.l1 * p[ly.i0 * W + lx.i1];
                const float bot = lx.l0 * p[ly.i1 * W + lx.i0] + lx.l1 * p[ly.i1 * W + lx.i1];
                v = ((ly.l0 * top + ly.l1 * bot) - 0.5f) * 2.f;
            }
        }
        out[i] = v;
    }
}

// One thread per (output voxel, 4 channels); positions in the padding count as zeros, as F.pad + max_pool3d sees them.
__global__ void maxpool3d_same_kernel(const float4* __restrict__ x, float4* __restrict__ out, int T, int H, int W, int C4,
                                      int To, int Ho, int Wo, int KT, int KH, int KW, int ST, int SH, int SW, int pt, int ph,
                                      int pw, size_t total) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % C4);
        size_t r = i / C4;
        const int ox = (int)(r % Wo); r /= Wo;
        const int oy = (int)(r % Ho); r /= Ho;
        const int ot = (int)(r % To);
        const size_t b = r / To;
        float4 m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
        for (int kt = 0; kt < KT; ++kt) {
            const int t = ot * ST - pt + kt;
            for (int ky = 0; ky < KH; ++ky) {
                const int y = oy * SH - ph + ky;
                for (int kx = 0; kx < KW; ++kx) {
                    const int xx = ox * SW - pw + kx;
                    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (t >= 0 && t < T && y >= 0 && y < H && xx >= 0 && xx < W)
                        v = x[(((b * T + t) * H + y) * W + xx) * C4 + c];
                    m.x = max_nan(m.x, v.x); m.y = max_nan(m.y, v.y); m.z = max_nan(m.z, v.z); m.w = max_nan(m.w, v.w);
                }
            }
        }
        out[i] = m;
    }
}

constexpr int HEAD_MAX_C = 2048;

// One workgroup (256 threads = 4 waves) per clip.  pooled[c] = sum_t wt(t) * sum_pixels x[b][t][p][c] with
// wt(t) = (number of the T - KT + 1 windows holding frame t) / (KT * HW * (T - KT + 1)): AvgPool3d((KT, H, W), stride 1) followed
// by the mean over the windows.  Then one wave per logit: out[b][o] = bias[o] + w[o] . pooled (the logits unit is linear, so
// it commutes with the mean).  Fixed assignment and reduction trees: deterministic.
__global__ __launch_bounds__(256) void i3d_head_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                       const float* __restrict__ bias, float* __restrict__ out, int T, int HW,
                                                       int C, int Co, int KT) {
    __shared__ float pooled[HEAD_MAX_C];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nwin = T - KT + 1;
    const float norm = 1.f / ((float)KT * (float)HW * (float)nwin);
    const float* xb = x + (size_t)b * T * HW * C;
    for (int c = threadIdx.x; c < C; c += 256) {
        float acc = 0.f;
        for (int t = 0; t < T; ++t) {
            const int lo = t - KT + 1 > 0 ? t - KT + 1 : 0, hi = t < nwin - 1 ? t : nwin - 1;   // windows s in [lo, hi]
            float s = 0.f;
            for (int p = 0; p < HW; ++p) s += xb[((size_t)t * HW + p) * C + c];
            acc += (float)(hi - lo + 1) * s;
        }
        pooled[c] = acc * norm;
    }
    __syncthreads();
    for (int o = wave; o < Co; o += 4) {
        const float* wo = w + (size_t)o * C;
        float d = 0.f;
        for (int c = lane; c < C; c += 64) d += wo[c] * pooled[c];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) d += __shfl_xor(d, off);
        if (lane == 0) out[(size_t)b * Co + o] = d + (bias ? bias[o] : 0.f);
    }
}

inline int grid_for(size_t total) { return (int)((total + 255) / 256 > 8192 ? 8192 : (total + 255) / 256); }

// TensorFlow "same" padding of pytorch_i3d.py compute_pad: the front gets pad / 2, the back the rest.
inline int same_pad(int size, int k, int s) {
    const int p = (size % s == 0) ? k - s : k - size % s;
    return p > 0 ? p : 0;
}

}  // namespace

extern "C" int evc_i3d_stem_im2col_f32(const float* x, float* out, int B, int T, int C, int H, int W, int Hr, int Wr, int R,
                                       int KT, int KH, int KW, int ST, int SH, int SW, int f_begin, int nf, int ld_out,
                                       void* stream) {
    if (!x || !out || B <= 0 || T <= 0 || C <= 0 || H <= 0 || W <= 0 || R <= 0 || Hr < R || Wr < R) return EVC_EINVAL;
    if (KT <= 0 || KH <= 0 || KW <= 0 || ST <= 0 || SH <= 0 || SW <= 0 || ld_out < C * KT * KH * KW) return EVC_EINVAL;
    const int pt = same_pad(T, KT, ST), ph = same_pad(R, KH, SH), pw = same_pad(R, KW, SW);
    const int To = (T + pt - KT) / ST + 1, Ho = (R + ph - KH) / SH + 1, Wo = (R + pw - KW) / SW + 1;
    if (To <= 0 || Ho <= 0 || Wo <= 0 || f_begin < 0 || nf <= 0 || (long long)f_begin + nf > (long long)B * To) return EVC_EINVAL;
    const size_t total = (size_t)nf * Ho * Wo * ld_out;
    hipLaunchKernelGGL(i3d_stem_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, x, out, T, C, H, W, Hr, Wr,
                       (Hr - R) / 2, (Wr - R) / 2, R, KT, KH, KW, ST, SH, SW, pt / 2, ph / 2, pw / 2, To, Ho, Wo, f_begin,
                       ld_out, total);
    return hipGetLastError() == hipSuccess ? EVC_OK : EVC_ELAUNCH;
}

extern "C" int evc_maxpool3d_same_nthwc_f32(const float* x, float* out, int B, int T, int H, int W, int C, int KT, int KH, int KW,
                                            int ST, int SH, int SW, void* stream) {
    if (!x || !out || B <= 0 || T <= 0 || H <= 0 || W <= 0 || C <= 0 || (C & 3)) return EVC_EINVAL;
    if (KT <= 0 || KH <= 0 || KW <= 0 || ST <= 0 || SH <= 0 || SW <= 0) return EVC_EINVAL;
    const int pt = same_pad(T, KT, ST), ph = same_pad(H, KH, SH), pw = same_pad(W, KW, SW);
    const int To = (T + pt - KT) / ST + 1, Ho = (H + ph - KH) / SH + 1, Wo = (W + pw - KW) / SW + 1;
    if (To <= 0 || Ho <= 0 || Wo <= 0) return EVC_EINVAL;
    const size_t total = (size_t)B * To * Ho * Wo * (C / 4);
    hipLaunchKernelGGL(maxpool3d_same_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const float4*>(x), reinterpret_cast<float4*>(out), T, H, W, C / 4, To, Ho, Wo, KT, KH,
                       KW, ST, SH, SW, pt / 2, ph / 2, pw / 2, total);
    return hipGetLastError() == hipSuccess ? EVC_OK : EVC_ELAUNCH;
}

extern "C" int evc_i3d_head_f32(const float* x, const float* w, const float* bias, float* out, int B, int T, int HW, int C, int Co,
                                int KT, void* stream) {
    if (!x || !w || !out || B <= 0 || HW <= 0 || C <= 0 || C > HEAD_MAX_C || Co <= 0 || KT <= 0 || T < KT) return EVC_EINVAL;
    hipLaunchKernelGGL(i3d_head_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, x, w, bias, out, T, HW, C, Co, KT);
    return hipGetLastError() == hipSuccess ? EVC_OK : EVC_ELAUNCH;
}
