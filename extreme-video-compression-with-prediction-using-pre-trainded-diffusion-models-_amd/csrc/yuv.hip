// yuv.hip -- planar YUV 4:2:0 <-> RGB, the conventions of the reference's codec benchmark.
//
//   evc_yuv420_to_rgb   benchmark/fvd_utils/bench_uvg.py:479: ycbcr2rgb(yuv_420_to_444(frame, mode).true_divide(max_val)) --
//                       up-sample the RAW chroma samples x2 (torch F.interpolate, align_corners=False, border indices
//                       clamped), divide by maxv = 2^bits - 1, ycbcr2rgb (benchmark/transform.py:47-65, BT.709 full range).
//   evc_rgb_to_yuv420   rgb2ycbcr (transform.py:26-44), yuv_444_to_420 (:78-107, the 2x2 average), rint(clamp(v * maxv)).
//
// At scale 2 all three up-sampling modes are one 4-tap filter per axis with two fixed phases: luma column 2c reads chroma
// columns c-2 .. c+1 with the taps w[0..3], column 2c+1 reads c-1 .. c+2 with the mirror w[3..0] (the same along rows):
//   nearest  {0, 0, 1, 0}     bilinear  {0, 0.25, 0.75, 0}     bicubic (A = -0.75)  {-0.03515625, 0.26171875, 0.87890625, -0.10546875}
// All exact in fp32; a zero tap adds an exact zero, so one kernel serves the three modes.  Columns first, then rows.
//
// Both are element-wise passes bound by the fp32 RGB side (12 B per pixel against 1.5 B of samples).  A thread owns one chroma
// row x RUN = 4 chroma columns, i.e. a 2 x 8 luma block: every chroma sample is written once, and the RGB side moves as two
// 16-byte accesses per row and channel, consecutive lanes on consecutive 32-byte runs.  That needs W % 8 == 0 and a 16-byte
// aligned RGB pointer; any other even W (34: the last thread of a row owns 2 columns) takes the same code with scalar,
// bounds-checked accesses.  The sample side is a byte buffer at arbitrary offsets (a Y4M file has a "FRAME\n" marker between
// frames): it is read byte-wise through the cache and written as one aligned word per run where the address allows it.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/evc_hip.h"

namespace {

constexpr int RUN = 4;            // chroma columns per thread
constexpr int LUMA = 2 * RUN;     // luma columns per thread
// BT.709 (transform.py:8-11).  The reference forms 2 - 2 K and 1 - K in double before they meet an fp32 tensor.
constexpr float KR = 0.2126f, KG = 0.7152f, KB = 0.0722f;
constexpr float R_CR = (float)(2.0 - 2.0 * 0.2126), B_CB = (float)(2.0 - 2.0 * 0.0722), ONE_KB = (float)(1.0 - 0.0722), ONE_KR = (float)(1.0 - 0.2126);

struct Layout {                   // where the samples of frame n lie: base + first + n * stride + off_{y,u,v}
    long long first, stride, off_y, off_u, off_v;
};

struct Taps { float w[4]; };

template <bool WIDE> __device__ __forceinline__ float sample(const uint8_t* plane, long long i) {
    if (WIDE) return (float)((unsigned)plane[2 * i] | ((unsigned)plane[2 * i + 1] << 8));
    return (float)plane[i];
}

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// One chroma plane up-sampled for the thread's block: up[dy][x], x = 0 .. LUMA-1, raw sample units.
template <bool WIDE>
__device__ __forceinline__ void upsample_block(const uint8_t* plane, int Hc, int Wc, int cy, int cx0, const Taps& t, float (&up)[2][LUMA]) {
    float h[5][LUMA];             // chroma rows cy-2 .. cy+2, filtered along columns
#pragma unroll
    for (int r = 0; r < 5; ++r) {
        const long long row = (long long)clampi(cy - 2 + r, Hc - 1) * Wc;
        float v[RUN + 4];         // chroma columns cx0-2 .. cx0+RUN+1
#pragma unroll
        for (int j = 0; j < RUN + 4; ++j) v[j] = sample<WIDE>(plane, row + clampi(cx0 - 2 + j, Wc - 1));
#pragma unroll
        for (int k = 0; k < RUN; ++k) {
            h[r][2 * k] = t.w[0] * v[k] + t.w[1] * v[k + 1] + t.w[2] * v[k + 2] + t.w[3] * v[k + 3];
            h[r][2 * k + 1] = t.w[3] * v[k + 1] + t.w[2] * v[k + 2] + t.w[1] * v[k + 3] + t.w[0] * v[k + 4];
        }
    }
#pragma unroll
    for (int x = 0; x < LUMA; ++x) {
        up[0][x] = t.w[0] * h[0][x] + t.w[1] * h[1][x] + t.w[2] * h[2][x] + t.w[3] * h[3][x];
        up[1][x] = t.w[3] * h[1][x] + t.w[2] * h[2][x] + t.w[1] * h[3][x] + t.w[0] * h[4][x];
    }
}

__device__ __forceinline__ unsigned code_of(float v, float maxv) { return (unsigned)rintf(fminf(fmaxf(v * maxv, 0.0f), maxv)); }

// `vec`: W % 8 == 0 and `out` 16-byte aligned (8-byte for the uint8 form) -- uniform over the launch.
template <bool WIDE, bool U8>
__global__ void __launch_bounds__(256)
yuv420_to_rgb_kernel(const uint8_t* __restrict__ src, Layout lay, int H, int W, int groups, Taps taps, float maxv, void* __restrict__ out,
                     int vec) {
    const int Hc = H / 2, Wc = W / 2;
    const unsigned tid = blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= (unsigned)Hc * (unsigned)groups) return;
    const int cy = tid / groups, cx0 = (tid % groups) * RUN;
    const size_t n = blockIdx.y;
    const uint8_t* frame = src + lay.first + (long long)n * lay.stride;
    float u[2][LUMA], v[2][LUMA];
    upsample_block<WIDE>(frame + lay.off_u, Hc, Wc, cy, cx0, taps, u);
    upsample_block<WIDE>(frame + lay.off_v, Hc, Wc, cy, cx0, taps, v);
    const int x0 = 2 * cx0, cols = min(LUMA, W - x0);
    const size_t plane = (size_t)H * W;
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
        const int y = 2 * cy + dy;
        float rgb[3][LUMA];
#pragma unroll
        for (int x = 0; x < LUMA; ++x) {
            const float Y = sample<WIDE>(frame + lay.off_y, (long long)y * W + min(x0 + x, W - 1)) / maxv;
            const float cb = u[dy][x] / maxv, cr = v[dy][x] / maxv;
            const float r = Y + R_CR * (cr - 0.5f);
            const float b = Y + B_CB * (cb - 0.5f);
            rgb[0][x] = r;
            rgb[1][x] = (Y - KR * r - KB * b) / KG;
            rgb[2][x] = b;
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const size_t at = (n * 3 + c) * plane + (size_t)y * W + x0;
            if (U8) {
                uint8_t* o = static_cast<uint8_t*>(out) + at;
                unsigned q[LUMA];
#pragma unroll
                for (int x = 0; x < LUMA; ++x) q[x] = code_of(rgb[c][x], 255.0f);
                if (vec) {
                    *reinterpret_cast<uint2*>(o) = make_uint2(q[0] | (q[1] << 8) | (q[2] << 16) | (q[3] << 24),
                                                              q[4] | (q[5] << 8) | (q[6] << 16) | (q[7] << 24));
                } else {
#pragma unroll
                    for (int x = 0; x < LUMA; ++x) if (x < cols) o[x] = (uint8_t)q[x];
                }
            } else {
                float* o = static_cast<float*>(out) + at;
                if (vec) {
                    reinterpret_cast<float4*>(o)[0] = make_float4(rgb[c][0], rgb[c][1], rgb[c][2], rgb[c][3]);
                    reinterpret_cast<float4*>(o)[1] = make_float4(rgb[c][4], rgb[c][5], rgb[c][6], rgb[c][7]);
                } else {
#pragma unroll
                    for (int x = 0; x < LUMA; ++x) if (x < cols) o[x] = rgb[c][x];
                }
            }
        }
    }
}

// K codes -> K samples at p: one aligned word when all K are wanted and p allows it, else byte stores.
template <bool WIDE, int K>
__device__ __forceinline__ void store_codes(uint8_t* p, const unsigned (&c)[K], int count) {
    constexpr int BYTES = K * (WIDE ? 2 : 1);          // 4, 8 or 16
    if (count == K && (reinterpret_cast<uintptr_t>(p) & (BYTES - 1)) == 0) {
        uint32_t w[BYTES / 4];
#pragma unroll
        for (int i = 0; i < BYTES / 4; ++i) {
            if constexpr (WIDE) w[i] = c[2 * i] | (c[2 * i + 1] << 16);
            else w[i] = c[4 * i] | (c[4 * i + 1] << 8) | (c[4 * i + 2] << 16) | (c[4 * i + 3] << 24);
        }
        if constexpr (BYTES == 4) *reinterpret_cast<uint32_t*>(p) = w[0];
        else if constexpr (BYTES == 8) *reinterpret_cast<uint2*>(p) = make_uint2(w[0], w[1]);
        else *reinterpret_cast<uint4*>(p) = make_uint4(w[0], w[1], w[2], w[3]);
        return;
    }
#pragma unroll
    for (int i = 0; i < K; ++i) {
        if (i >= count) break;
        if (WIDE) { p[2 * i] = (uint8_t)(c[i] & 255u); p[2 * i + 1] = (uint8_t)(c[i] >> 8); }
        else p[i] = (uint8_t)c[i];
    }
}

template <bool WIDE>
__global__ void __launch_bounds__(256)
rgb_to_yuv420_kernel(const float* __restrict__ rgb, uint8_t* __restrict__ dst, Layout lay, int H, int W, int groups, float maxv,
                     unsigned* __restrict__ events, int vec) {
    constexpr int BPS = WIDE ? 2 : 1;
    const int Hc = H / 2, Wc = W / 2;
    const unsigned tid = blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= (unsigned)Hc * (unsigned)groups) return;
    const int cy = tid / groups, cx0 = (tid % groups) * RUN;
    const size_t n = blockIdx.y;
    uint8_t* frame = dst + lay.first + (long long)n * lay.stride;
    const int x0 = 2 * cx0, cols = min(LUMA, W - x0);
    const size_t plane = (size_t)H * W;
    float cb[2][LUMA], cr[2][LUMA];
    bool bad[2][LUMA];
    bool any_bad = false;
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
        const int y = 2 * cy + dy;
        float in[3][LUMA];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float* p = rgb + (n * 3 + c) * plane + (size_t)y * W + x0;
            if (vec) {
                const float4 a = reinterpret_cast<const float4*>(p)[0], b = reinterpret_cast<const float4*>(p)[1];
                in[c][0] = a.x; in[c][1] = a.y; in[c][2] = a.z; in[c][3] = a.w;
                in[c][4] = b.x; in[c][5] = b.y; in[c][6] = b.z; in[c][7] = b.w;
            } else {
#pragma unroll
                for (int x = 0; x < LUMA; ++x) in[c][x] = x < cols ? p[x] : 0.0f;
            }
        }
        unsigned q[LUMA];
#pragma unroll
        for (int x = 0; x < LUMA; ++x) {
            const float r = in[0][x], g = in[1][x], b = in[2][x];
            const float Y = KR * r + KG * g + KB * b;
            cb[dy][x] = 0.5f * (b - Y) / ONE_KB + 0.5f;
            cr[dy][x] = 0.5f * (r - Y) / ONE_KR + 0.5f;
            bad[dy][x] = !(isfinite(r) && isfinite(g) && isfinite(b));
            any_bad |= bad[dy][x];
            q[x] = bad[dy][x] ? 0u : code_of(Y, maxv);
        }
        store_codes<WIDE, LUMA>(frame + lay.off_y + ((long long)y * W + x0) * BPS, q, cols);
    }
    unsigned qu[RUN], qv[RUN];
#pragma unroll
    for (int k = 0; k < RUN; ++k) {
        const bool b = bad[0][2 * k] || bad[0][2 * k + 1] || bad[1][2 * k] || bad[1][2 * k + 1];
        const float mu = (cb[0][2 * k] + cb[0][2 * k + 1] + cb[1][2 * k] + cb[1][2 * k + 1]) * 0.25f;
        const float mv = (cr[0][2 * k] + cr[0][2 * k + 1] + cr[1][2 * k] + cr[1][2 * k + 1]) * 0.25f;
        qu[k] = b ? 0u : code_of(mu, maxv);
        qv[k] = b ? 0u : code_of(mv, maxv);
    }
    const long long cat = ((long long)cy * Wc + cx0) * BPS;
    store_codes<WIDE, RUN>(frame + lay.off_u + cat, qu, min(RUN, Wc - cx0));
    store_codes<WIDE, RUN>(frame + lay.off_v + cat, qv, min(RUN, Wc - cx0));
    if (any_bad) atomicOr(events, EVC_RANGE_NONFINITE);
}

// The frames' geometry against the buffer: every plane of every frame inside [0, bytes).  -> thread groups per chroma row, 0 = refuse.
int checked_groups(long long bytes, const Layout& l, int N, int H, int W, int bits) {
    if (N <= 0 || N > 65535 || H < 2 || W < 2 || (H & 1) || (W & 1) || (bits != 8 && bits != 10)) return 0;
    if (l.first < 0 || l.stride < 0 || l.off_y < 0 || l.off_u < 0 || l.off_v < 0 || bytes <= 0) return 0;
    const long long bps = bits > 8 ? 2 : 1, luma = (long long)H * W * bps, chroma = luma / 4;
    long long end = l.off_y + luma;
    if (l.off_u + chroma > end) end = l.off_u + chroma;
    if (l.off_v + chroma > end) end = l.off_v + chroma;
    if (bytes < end || l.first > bytes - end) return 0;
    if (N > 1 && l.stride > (bytes - end - l.first) / (N - 1)) return 0;
    const long long groups = (W / 2 + RUN - 1) / RUN;
    if (groups * (H / 2) > 0x7FFFFFFFLL) return 0;
    return (int)groups;
}

}  // namespace

extern "C" int evc_yuv420_to_rgb(const unsigned char* src, long long src_bytes, long long first, long long frame_stride, long long off_y,
                                 long long off_u, long long off_v, int N, int H, int W, int bits, int mode, void* out, int out_u8,
                                 void* stream) {
    const Layout lay{first, frame_stride, off_y, off_u, off_v};
    if (!src || !out || mode < EVC_YUV_NEAREST || mode > EVC_YUV_BICUBIC) return EVC_EINVAL;
    const int groups = checked_groups(src_bytes, lay, N, H, W, bits);
    if (!groups) return EVC_EINVAL;
    static const Taps kTaps[3] = {{{0.0f, 0.0f, 1.0f, 0.0f}}, {{0.0f, 0.25f, 0.75f, 0.0f}}, {{-0.03515625f, 0.26171875f, 0.87890625f, -0.10546875f}}};
    const float maxv = (float)((1 << bits) - 1);
    const int vec = W % LUMA == 0 && (reinterpret_cast<uintptr_t>(out) & (out_u8 ? 7 : 15)) == 0;
    const dim3 grid(((unsigned)groups * (unsigned)(H / 2) + 255) / 256, (unsigned)N);
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, (hipStream_t)stream, src, lay, H, W, groups, kTaps[mode], maxv, out, vec);
    };
    if (bits > 8) { if (out_u8) launch(yuv420_to_rgb_kernel<true, true>); else launch(yuv420_to_rgb_kernel<true, false>); }
    else { if (out_u8) launch(yuv420_to_rgb_kernel<false, true>); else launch(yuv420_to_rgb_kernel<false, false>); }
    return hipGetLastError() == hipSuccess ? EVC_OK : EVC_ELAUNCH;
}

extern "C" int evc_rgb_to_yuv420(const float* rgb, unsigned char* dst, long long dst_bytes, long long first, long long frame_stride,
                                 long long off_y, long long off_u, long long off_v, int N, int H, int W, int bits, unsigned* events,
                                 void* stream) {
    const Layout lay{first, frame_stride, off_y, off_u, off_v};
    if (!rgb || !dst || !events) return EVC_EINVAL;
    const int groups = checked_groups(dst_bytes, lay, N, H, W, bits);
    if (!groups) return EVC_EINVAL;
    const float maxv = (float)((1 << bits) - 1);
    const int vec = W % LUMA == 0 && (reinterpret_cast<uintptr_t>(rgb) & 15) == 0;
    const dim3 grid(((unsigned)groups * (unsigned)(H / 2) + 255) / 256, (unsigned)N);
    if (bits > 8)
        hipLaunchKernelGGL(rgb_to_yuv420_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, rgb, dst, lay, H, W, groups, maxv, events, vec);
    else
        hipLaunchKernelGGL(rgb_to_yuv420_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, rgb, dst, lay, H, W, groups, maxv, events, vec);
    return hipGetLastError() == hipSuccess ? EVC_OK : EVC_ELAUNCH;
}
