// metric.hip -- the sender's decision metric on the device: per-frame squared error in double, the sum under the PSNR of
// decide_5to5 (cal_psnr: mse = mean((a - b)^2) in float64).  A sweep with noise trials judges K times the candidates, and the
// host path copies every one of them to the host first.
//
// Sums are deterministic and independent of the launch: ONE workgroup per frame; the frame's elements are cut into chunks of
// four by their INDEX IN THE FRAME (not by address), thread t takes chunks t, t + 1024, ... in that order and keeps one
// partial sum per position in the chunk; a last short chunk belongs to the thread its index names.  The four partials are
// added as (0 + 1) + (2 + 3), then a wave shuffle tree and a fixed-order pass over the sixteen wave totals in LDS (rate.hip's
// block_sum), and the total leaves with a plain store: no atomics, no workspace.  The order depends on `elems` only -- not on
// n, on the frame's row or on where the row starts -- so a frame's value is the same bit pattern in any launch.  The alignment of
// a row only decides HOW a chunk is fetched: one 16-byte load where the chunk's address allows it, four 4-byte loads where
// it does not (odd `elems` puts every other row off a 16-byte boundary).
//
// Nothing is clamped or dropped: a NaN, or inf - inf, makes that frame's sum NaN; inf against a finite value makes it inf.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/evc_hip.h"

namespace {

constexpr int SQ_THREADS = 1024;
constexpr int SQ_WAVES = SQ_THREADS / 64;
#define EVC_LAUNCH_OK() (hipGetLastError() == hipSuccess ? EVC_OK : EVC_ELAUNCH)

__device__ __forceinline__ float4 load_chunk(const float* __restrict__ p, bool aligned) {
    if (aligned) return *reinterpret_cast<const float4*>(p);
    return make_float4(p[0], p[1], p[2], p[3]);
}

__device__ __forceinline__ double sqdiff(float a, float b) {
    const double d = (double)a - (double)b;
    return d * d;
}

__global__ void __launch_bounds__(SQ_THREADS)
frame_sqerr_kernel(const float* __restrict__ a, const float* __restrict__ b, long long elems, double* __restrict__ out) {
    __shared__ double wave_total[SQ_WAVES];
    const float* __restrict__ pa = a + (long long)blockIdx.x * elems;
    const float* __restrict__ pb = b + (long long)blockIdx.x * elems;
    const bool va = ((uintptr_t)pa & 15) == 0, vb = ((uintptr_t)pb & 15) == 0;      // uniform over the workgroup
    const long long chunks = elems >> 2;                                              // full chunks; elems & 3 elements remain
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    if (va && vb) {
#pragma unroll 4
        for (long long c = threadIdx.x; c < chunks; c += SQ_THREADS) {
            const float4 x = *reinterpret_cast<const float4*>(pa + 4 * c);
            const float4 y = *reinterpret_cast<const float4*>(pb + 4 * c);
            s0 += sqdiff(x.x, y.x); s1 += sqdiff(x.y, y.y); s2 += sqdiff(x.z, y.z); s3 += sqdiff(x.w, y.w);
        }
    } else {
#pragma unroll 2
        for (long long c = threadIdx.x; c < chunks; c += SQ_THREADS) {
            const float4 x = load_chunk(pa + 4 * c, va);
            const float4 y = load_chunk(pb + 4 * c, vb);
            s0 += sqdiff(x.x, y.x); s1 += sqdiff(x.y, y.y); s2 += sqdiff(x.z, y.z); s3 += sqdiff(x.w, y.w);
        }
    }
    const int rest = (int)(elems & 3);
    if (rest && (long long)threadIdx.x == chunks % SQ_THREADS) {          // the short chunk: after the owner's full ones
        const long long i = 4 * chunks;
        s0 += sqdiff(pa[i], pb[i]);
        if (rest > 1) s1 += sqdiff(pa[i + 1], pb[i + 1]);
        if (rest > 2) s2 += sqdiff(pa[i + 2], pb[i + 2]);
    }
    double v = (s0 + s1) + (s2 + s3);
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((threadIdx.x & 63) == 0) wave_total[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = wave_total[0];
        for (int w = 1; w < SQ_WAVES; ++w) s += wave_total[w];
        out[blockIdx.x] = s;
    }
}

}  // namespace

extern "C" int evc_frame_sqerr_f64(const float* a, const float* b, int n, long long elems, double* out, void* stream) {
    if (!a || !b || !out || n <= 0 || elems <= 0) return EVC_EINVAL;
    hipLaunchKernelGGL(frame_sqerr_kernel, dim3((unsigned)n), dim3(SQ_THREADS), 0, (hipStream_t)stream, a, b, elems, out);
    return EVC_LAUNCH_OK();
}
