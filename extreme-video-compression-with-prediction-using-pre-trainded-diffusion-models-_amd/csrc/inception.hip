// inception.hip -- the pieces of the FID Inception-v3 feature network and of the k-NN precision / recall that are not
// convolutions.
//
// The reference's evaluation/ package (inception.py, fid_PR.py, pr.py) computes the Frechet Inception distance and the
// precision / recall of Kynkaanniemi et al. over the features of pytorch-fid's Inception-v3.  The convolutions run on
// evc_conv2d_nhwc_f32 (activations NHWC, BatchNorm folded, ReLU in the epilogue); this file holds
//   * evc_inception_stem_im2col_f32: bilinear resize to 299 x 299 + 2x - 1 fused into the patch rows of Conv2d_1a_3x3
//     (stride 2, no padding) -- the resized image is never written;
//   * evc_im2col_nhwc_f32: patch rows of an NHWC tensor for any window / strides / zero padding (the stride-2 and unpadded
//     3x3 convolutions, and any filter shape the convolution dispatch refuses, become 1x1 convolutions);
//   * evc_pool3x3s1p1_nhwc_f32: the 3x3 stride-1 padded pools of the Inception blocks (average over the in-image elements, max);
//   * evc_spatial_mean_nhwc_f32: AdaptiveAvgPool2d((1, 1));
//   * evc_knn_radius_f32 / evc_manifold_hits_f32: the two set kernels of precision / recall, fp64, no n x m matrix.
// All are bandwidth- or latency-bound: 16-byte accesses, no LDS beyond the small fixed-order reductions.
#include <hip/hip_runtime.h>
#include "../../include/evc_hip.h"

namespace {

// Running max that keeps a NaN, as torch's max_pool does (fmaxf returns the operand that is not NaN).
__device__ __forceinline__ float max_nan(float m, float v) { return (v > m || v != v) ? v : m; }

// Bilinear source of output index dst, align_corners=False, size given: the rational ((2 dst + 1) in - out) / (2 out), clamped
// at 0, in integers; the two weights are the correctly rounded fp32 values of the exact fraction and of one minus it (the
// quotient of two integers below 2^31 in double, rounded once more to float, is the correctly rounded float: a double that
// sits on a float midpoint is exact, and any other quotient is further from the midpoint than a double's rounding).
struct Lin { int i0, i1; float l0, l1; };
__device__ inline Lin lin_src(int dst, int in, int out) {
    const long long den = 2LL * out;
    long long num = (2LL * dst + 1) * in - out;
    if (num < 0) num = 0;
    const long long q = num / den, r = num - q * den;
    Lin s;
    s.i0 = (int)q;
    s.i1 = s.i0 + (s.i0 < in - 1 ? 1 : 0);
    s.l1 = (float)((double)r / (double)den);
    s.l0 = (float)((double)(den - r) / (double)den);
    return s;
}

constexpr int STEM_R = 299, STEM_O = 149, STEM_K = 27;

// One thread per four columns of a patch row: out[f - f_begin][oy][ox][(c*3 + ky)*3 + kx] = the resized, 2x - 1 mapped image at
// (2 oy + ky, 2 ox + kx).  The mapping is applied to the four source pixels (2p is exact and 2p - 1 rounds once), then
// top = l0x a + l1x b, bot likewise, v = l0y top + l1y bot: with the weights that is at most seven roundings per output, and
// weight 1 / weight 0 give the mapped pixel itself (in = 299).  0 * inf = NaN as in torch.
__global__ void inception_stem_kernel(const float* __restrict__ x, float4* __restrict__ out, int H, int W, int f_begin, int ld4,
                                      size_t total) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int k4 = (int)(i % ld4);
        const size_t pix = i / ld4;
        const int ox = (int)(pix % STEM_O);
        const int oy = (int)((pix / STEM_O) % STEM_O);
        const size_t f = (size_t)f_begin + pix / ((size_t)STEM_O * STEM_O);
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = 4 * k4 + j;
            v[j] = 0.f;
            if (k < STEM_K) {
                const int kx = k % 3, ky = (k / 3) % 3, c = k / 9;
                const Lin ly = lin_src(2 * oy + ky, H, STEM_R), lx = lin_src(2 * ox + kx, W, STEM_R);
                const float* p = x + (f * 3 + c) * (size_t)H * W;
                const float a = 2.f * p[(size_t)ly.i0 * W + lx.i0] - 1.f, b = 2.f * p[(size_t)ly.i0 * W + lx.i1] - 1.f;
                const float cc = 2.f * p[(size_t)ly.i1 * W + lx.i0] - 1.f, d = 2.f * p[(size_t)ly.i1 * W + lx.i1] - 1.f;
                const float top = lx.l0 * a + lx.l1 * b;
                const float bot = lx.l0 * cc + lx.l1 * d;
                v[j] = ly.l0 * top + ly.l1 * bot;
            }
        }
        out[i] = make_float4(v[0], v[1], v[2], v[3]);
    }
}

// One thread per four columns of a patch row, (ky, kx, c) order: a 16-byte copy or zeros.
__global__ void im2col_nhwc_kernel(const float4* __restrict__ x, float4* __restrict__ out, int H, int W, int C4, int Ho, int Wo,
                                   int KH, int KW, int SH, int SW, int PH, int PW, int ld4, size_t total) {
    const int K4 = KH * KW * C4;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int k4 = (int)(i % ld4);
        size_t r = i / ld4;
        const int ox = (int)(r % Wo); r /= Wo;
        const int oy = (int)(r % Ho);
        const size_t n = r / Ho;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (k4 < K4) {
            const int c4 = k4 % C4, tap = k4 / C4;
            const int y = oy * SH - PH + tap / KW, xx = ox * SW - PW + tap % KW;
            if (y >= 0 && y < H && xx >= 0 && xx < W) v = x[((n * H + y) * W + xx) * C4 + c4];
        }
        out[i] = v;
    }
}

// One thread per (pixel, 4 channels).  MAX: the padding does not take part.  Average: the in-image elements of the window are
// added in row-major order and divided by their count (count_include_pad=False).
template <bool MAX>
__global__ void pool3x3s1p1_kernel(const float4* __restrict__ x, float4* __restrict__ out, int H, int W, int C4, size_t total) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % C4);
        size_t r = i / C4;
        const int ox = (int)(r % W); r /= W;
        const int oy = (int)(r % H);
        const size_t n = r / H;
        float4 m = MAX ? make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY) : make_float4(0.f, 0.f, 0.f, 0.f);
        int count = 0;
        for (int y = oy - 1; y <= oy + 1; ++y) {
            if (y < 0 || y >= H) continue;
            for (int xx = ox - 1; xx <= ox + 1; ++xx) {
                if (xx < 0 || xx >= W) continue;
                const float4 v = x[((n * H + y) * W + xx) * C4 + c];
                if (MAX) {
                    m.x = max_nan(m.x, v.x); m.y = max_nan(m.y, v.y); m.z = max_nan(m.z, v.z); m.w = max_nan(m.w, v.w);
                } else {
                    m.x += v.x; m.y += v.y; m.z += v.z; m.w += v.w;
                }
                ++count;
            }
        }
        if (!MAX) {
            const float d = (float)count;
            m.x /= d; m.y /= d; m.z /= d; m.w /= d;
        }
        out[i] = m;
    }
}

// One workgroup of 256 threads per (image, 64 channels): 16 lanes across the channels (one float4 each, 256 contiguous bytes per
// pixel), 16 pixel lanes that stride over the pixels; the 16 partial sums of a channel are added in lane order.  The sums are
// kept in fp64 (a serial fp32 sum over 73 x 73 pixels would lose more than the convolutions before it), the quotient is rounded
// to fp32 once.  The order of the additions depends on HW only.
struct Sum4 { double x, y, z, w; };
__global__ __launch_bounds__(256) void spatial_mean_kernel(const float4* __restrict__ x, float4* __restrict__ out, int HW, int C4) {
    __shared__ Sum4 part[16][16];
    const int cl = threadIdx.x & 15, pl = threadIdx.x >> 4;
    const int c4 = blockIdx.x * 16 + cl;
    const size_t n = blockIdx.y;
    Sum4 s = {0.0, 0.0, 0.0, 0.0};
    if (c4 < C4) {
        const float4* xn = x + n * (size_t)HW * C4 + c4;
        for (int p = pl; p < HW; p += 16) {
            const float4 v = xn[(size_t)p * C4];
            s.x += (double)v.x; s.y += (double)v.y; s.z += (double)v.z; s.w += (double)v.w;
        }
    }
    part[pl][cl] = s;
    __syncthreads();
    if (pl == 0 && c4 < C4) {
        Sum4 t = part[0][cl];
        for (int j = 1; j < 16; ++j) {
            const Sum4 v = part[j][cl];
            t.x += v.x; t.y += v.y; t.z += v.z; t.w += v.w;
        }
        const double d = (double)HW;
        out[n * C4 + c4] = make_float4((float)(t.x / d), (float)(t.y / d), (float)(t.z / d), (float)(t.w / d));
    }
}

// Squared distance of two fp32 rows of d = 4 d4 values by a group of 16 adjacent lanes: lane l adds the squares of the exact
// differences (double)a - (double)b of the float4s l, l + 16, ... in fp64, the 16 partial sums meet in a butterfly (fp addition
// is commutative, so every lane of the group ends with the same bits).  The order depends on d only.
__device__ __forceinline__ double dist2_group(const float4* __restrict__ a, const float4* __restrict__ b, int d4, int l) {
    double s = 0.0;
    for (int c = l; c < d4; c += 16) {
        const float4 p = a[c], q = b[c];
        const double e0 = (double)p.x - (double)q.x, e1 = (double)p.y - (double)q.y;
        const double e2 = (double)p.z - (double)q.z, e3 = (double)p.w - (double)q.w;
        s += e0 * e0; s += e1 * e1; s += e2 * e2; s += e3 * e3;
    }
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) s += __shfl_xor(s, off, 16);
    return s;
}

constexpr int KNN_MAX = 9;     // k + 1 <= 9

// One workgroup (256 threads = 16 groups of 16 lanes) per row i of X.  Group g visits the rows j = g, g + 16, ... and keeps the
// k + 1 smallest squared distances it has seen, sorted; the 16 lists are merged by one thread.  out[i] = the (k + 1)-th smallest
// squared distance from row i to the rows of X, row i itself (distance 0) included.
__global__ __launch_bounds__(256) void knn_radius_kernel(const float4* __restrict__ x, double* __restrict__ out, int n, int d4,
                                                         int k1) {
    __shared__ double lists[16][KNN_MAX];
    __shared__ int head[16];
    const int l = threadIdx.x & 15, g = threadIdx.x >> 4;
    const float4* xi = x + (size_t)blockIdx.x * d4;
    double best[KNN_MAX];
#pragma unroll
    for (int t = 0; t < KNN_MAX; ++t) best[t] = INFINITY;
    for (int j = g; j < n; j += 16) {
        double v = dist2_group(xi, x + (size_t)j * d4, d4, l);
#pragma unroll
        for (int t = 0; t < KNN_MAX; ++t) {      // insertion into the sorted list; slots >= k1 are never read
            const double lo = v < best[t] ? v : best[t];
            v = v < best[t] ? best[t] : v;
            best[t] = lo;
        }
    }
    if (l == 0) {
#pragma unroll
        for (int t = 0; t < KNN_MAX; ++t) lists[g][t] = best[t];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int q = 0; q < 16; ++q) head[q] = 0;
        double v = INFINITY;
        for (int t = 0; t < k1; ++t) {           // k1 times: take the smallest head of the 16 sorted lists
            int arg = 0;
            v = INFINITY;
            for (int q = 0; q < 16; ++q) {
                const double h = head[q] < k1 ? lists[q][head[q]] : INFINITY;
                if (h < v) { v = h; arg = q; }
            }
            ++head[arg];
        }
        out[blockIdx.x] = v;
    }
}

// One workgroup per row y of Y: flag[y] = 1 when some row j of X has squared distance to y <= radius2[j].
__global__ __launch_bounds__(256) void manifold_hits_kernel(const float4* __restrict__ y, const float4* __restrict__ x,
                                                            const double* __restrict__ radius2, int* __restrict__ flag, int n,
                                                            int d4) {
    const int l = threadIdx.x & 15, g = threadIdx.x >> 4;
    const float4* yi = y + (size_t)blockIdx.x * d4;
    int hit = 0;
    for (int j = g; j < n; j += 16) hit |= dist2_group(yi, x + (size_t)j * d4, d4, l) <= radius2[j] ? 1 : 0;
    hit = __syncthreads_or(hit);
    if (threadIdx.x == 0) flag[blockIdx.x] = hit ? 1 : 0;
}

inline int grid_for(size_t total) { return (int)((total + 255) / 256 > 8192 ? 8192 : (total + 255) / 256); }

}  // namespace

extern "C" int evc_inception_stem_im2col_f32(const float* x, float* out, int N, int C, int H, int W, int f_begin, int nf,
                                             int ld_out, void* stream) {
    if (!x || !out || N <= 0 || C != 3 || H <= 0 || W <= 0 || ld_out < STEM_K || (ld_out & 3)) return EVC_EINVAL;
    if (f_begin < 0 || nf <= 0 || (long long)f_begin + nf > N) return EVC_EINVAL;
    const size_t total = (size_t)nf * STEM_O * STEM_O * (ld_out / 4);
    hipLaunchKernelGGL(inception_stem_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, x,
                       reinterpret_cast<float4*>(out), H, W, f_begin, ld_out / 4, total);
    return hipGetLastError() == hipSuccess ? EVC_OK : EVC_ELAUNCH;
}

extern "C" int evc_im2col_nhwc_f32(const float* x, float* out, int N, int H, int W, int C, int KH, int KW, int SH, int SW, int PH,
                                   int PW, int ld_out, void* stream) {
    if (!x || !out || N <= 0 || H <= 0 || W <= 0 || C <= 0 || (C & 3)) return EVC_EINVAL;
    if (KH <= 0 || KW <= 0 || SH <= 0 || SW <= 0 || PH < 0 || PW < 0) return EVC_EINVAL;
    if ((long long)KH * KW * C > ld_out || (ld_out & 3) || H + 2 * PH < KH || W + 2 * PW < KW) return EVC_EINVAL;
    const int Ho = (H + 2 * PH - KH) / SH + 1, Wo = (W + 2 * PW - KW) / SW + 1;
    const size_t total = (size_t)N * Ho * Wo * (ld_out / 4);
    hipLaunchKernelGGL(im2col_nhwc_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const float4*>(x), reinterpret_cast<float4*>(out), H, W, C / 4, Ho, Wo, KH, KW, SH, SW,
                       PH, PW, ld_out / 4, total);
    return hipGetLastError() == hipSuccess ? EVC_OK : EVC_ELAUNCH;
}

extern "C" int evc_pool3x3s1p1_nhwc_f32(const float* x, float* out, int N, int H, int W, int C, int mode, void* stream) {
    if (!x || !out || N <= 0 || H <= 0 || W <= 0 || C <= 0 || (C & 3)) return EVC_EINVAL;
    if (mode != EVC_POOL_AVG && mode != EVC_POOL_MAX) return EVC_EINVAL;
    const size_t total = (size_t)N * H * W * (C / 4);
    auto kern = mode == EVC_POOL_MAX ? pool3x3s1p1_kernel<true> : pool3x3s1p1_kernel<false>;
    hipLaunchKernelGGL(kern, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const float4*>(x),
                       reinterpret_cast<float4*>(out), H, W, C / 4, total);
    return hipGetLastError() == hipSuccess ? EVC_OK : EVC_ELAUNCH;
}

extern "C" int evc_spatial_mean_nhwc_f32(const float* x, float* out, int N, int HW, int C, void* stream) {
    if (!x || !out || N <= 0 || N > 65535 || HW <= 0 || C <= 0 || (C & 3)) return EVC_EINVAL;
    const int C4 = C / 4;
    hipLaunchKernelGGL(spatial_mean_kernel, dim3((C4 + 15) / 16, N), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const float4*>(x), reinterpret_cast<float4*>(out), HW, C4);
    return hipGetLastError() == hipSuccess ? EVC_OK : EVC_ELAUNCH;
}

extern "C" int evc_knn_radius_f32(const float* x, double* radius2, int n, int d, int k, void* stream) {
    if (!x || !radius2 || d <= 0 || (d & 3) || k < 1 || k + 1 > KNN_MAX || n <= k) return EVC_EINVAL;
    hipLaunchKernelGGL(knn_radius_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const float4*>(x), radius2,
                       n, d / 4, k + 1);
    return hipGetLastError() == hipSuccess ? EVC_OK : EVC_ELAUNCH;
}

extern "C" int evc_manifold_hits_f32(const float* y, const float* x, const double* radius2, int* flags, int m, int n, int d,
                                     void* stream) {
    if (!y || !x || !radius2 || !flags || m <= 0 || n <= 0 || d <= 0 || (d & 3)) return EVC_EINVAL;
    hipLaunchKernelGGL(manifold_hits_kernel, dim3(m), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const float4*>(y),
                       reinterpret_cast<const float4*>(x), radius2, flags, n, d / 4);
    return hipGetLastError() == hipSuccess ? EVC_OK : EVC_ELAUNCH;
}
