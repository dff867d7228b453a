// rate.hip -- rate estimation of the ELIC codec without an entropy coder (TestModel.inference, Network.py:534-640):
// quantise, evaluate the likelihood of every quantised latent and add up -log2 of it per sample, all on the device.
//
// Sums are deterministic and batch-invariant: ONE workgroup per sample, lane t takes the sample's sites t, t + 256, ... in
// that order, then a wave shuffle tree and a fixed-order pass over the four wave totals in LDS.  The order depends on
// (C, H, W) only, and the total leaves with a plain store: no atomics.  Partial sums are kept in double, so the total
// carries the rounding of its terms and none of its own.
//
// Non-finite values follow torch: compressai's bounds are torch.max(x, bound), which keeps a NaN (fmaxf would drop it).
#include <hip/hip_runtime.h>
#include "../../include/evc_hip.h"

namespace {

constexpr int RATE_THREADS = 256;
constexpr int RATE_WAVES = RATE_THREADS / 64;
constexpr int DENSITY_FLOATS = 58;     // per channel: 3+3+3, 3 x (9+3+3), 3+1  (EntropyBottleneck, filters (3,3,3,3))
#define EVC_LAUNCH_OK() (hipGetLastError() == hipSuccess ? EVC_OK : EVC_ELAUNCH)

// same site convention as elementwise.hip: anchors (parity 0) at w = 2j + (h & 1), non-anchors at w = 2j + 1 - (h & 1)
__device__ __forceinline__ int cb_col(int h, int j, int parity) { return 2 * j + ((h & 1) ^ parity); }

// torch.max(x, bound) of compressai's LowerBound: a NaN passes through
__device__ __forceinline__ float lower_bound(float x, float bound) { return x < bound ? bound : x; }
__device__ __forceinline__ double lower_bound(double x, double bound) { return x < bound ? bound : x; }

// total of v over the workgroup, valid in thread 0
__device__ __forceinline__ double block_sum(double v, double* wave_total) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((threadIdx.x & 63) == 0) wave_total[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = wave_total[0];
    for (int w = 1; w < RATE_WAVES; ++w) s += wave_total[w];
    return s;
}

// GaussianConditional.forward in eval mode (compressai 1.1.5): quantize "dequantize", _likelihood, both lower bounds.
// The fp32 operations are compressai's, in its order: values = |.|, (0.5 - v) / s, const * ., 0.5 * erfc(.), upper - lower.
// erfc and log2 are evaluated in double and rounded once, i.e. they are correctly rounded fp32 functions: the distance of a
// term to the exact value is then the format's, not a math library's.
__global__ void __launch_bounds__(RATE_THREADS)
elic_rate_pass_kernel(const float* __restrict__ ms, int ld, int mean_off, int scale_off, int C,
                      const float* __restrict__ y, int ld_y, int c0, int H, int W, int parity,
                      float* __restrict__ y_hat, double* __restrict__ bits) {
    __shared__ double wave_total[RATE_WAVES];
    const int b = blockIdx.x;
    const int Wh = W >> 1;
    const size_t n = (size_t)C * H * Wh;
    const float k = -0.70710678118654752440f;      // -(2 ** -0.5)
    double acc = 0.0;
    for (size_t i = threadIdx.x; i < n; i += RATE_THREADS) {
        const int c = (int)(i % C);                  // channels fastest: a wave reads and writes contiguous NHWC rows
        const size_t r = i / C;
        const int j = (int)(r % Wh);
        const int h = (int)(r / Wh);
        const size_t pix = ((size_t)b * H + h) * W + cb_col(h, j, parity);
        const float mu = ms[pix * ld + mean_off + c];
        const float sigma = ms[pix * ld + scale_off + c];
        const float sym = rintf(y[pix * ld_y + c0 + c] - mu);          // round half to even
        y_hat[pix * ld_y + c0 + c] = sym + mu;                         // = (float)symbol + mean of elic_scatter_symbols_kernel
        const float v = fabsf(sym);
        const float s = lower_bound(sigma, 0.11f);
        const float upper = 0.5f * (float)erfc((double)(k * ((0.5f - v) / s)));
        const float lower = 0.5f * (float)erfc((double)(k * ((-0.5f - v) / s)));
        const float p = lower_bound(upper - lower, 1e-9f);
        acc += -log2((double)p);
    }
    const double total = block_sum(acc, wave_total);
    if (threadIdx.x == 0) bits[b] = total;
}

// logits-cumulative chain of EntropyBottleneck for one channel: widths 1 -> 3 -> 3 -> 3 -> 3 -> 1; q holds softplus(matrix),
// bias and tanh(factor) of every layer, already transformed (no transcendental on a parameter here).
__device__ __forceinline__ double logits_cumulative(const float* __restrict__ q, double x) {
    double a[3], t[3];
    for (int o = 0; o < 3; ++o) {
        const double l = (double)q[o] * x + (double)q[3 + o];
        a[o] = l + (double)q[6 + o] * tanh(l);
    }
    q += 9;
    for (int layer = 1; layer < 4; ++layer, q += 15) {
        for (int o = 0; o < 3; ++o) {
            const double l = (double)q[3 * o] * a[0] + (double)q[3 * o + 1] * a[1] + (double)q[3 * o + 2] * a[2] + (double)q[9 + o];
            t[o] = l + (double)q[12 + o] * tanh(l);
        }
        a[0] = t[0]; a[1] = t[1]; a[2] = t[2];
    }
    return (double)q[0] * a[0] + (double)q[1] * a[1] + (double)q[2] * a[2] + (double)q[3];
}

__device__ __forceinline__ double sigmoid(double x) { return 1.0 / (1.0 + exp(-x)); }

// EntropyBottleneck.forward in eval mode (compressai 1.1.5): quantize "dequantize" with the medians, _likelihood, lower bound.
// z_hat is fp32 as in the coded path; the density itself is evaluated in double from the fp32 parameters.
__global__ void __launch_bounds__(RATE_THREADS)
bottleneck_rate_kernel(const float* __restrict__ z, int ld, int C, int HW, const float* __restrict__ medians,
                       const float* __restrict__ density, float* __restrict__ z_hat, double* __restrict__ bits) {
    __shared__ double wave_total[RATE_WAVES];
    const int b = blockIdx.x;
    const size_t n = (size_t)C * HW;
    double acc = 0.0;
    for (size_t i = threadIdx.x; i < n; i += RATE_THREADS) {
        const int c = (int)(i % C);
        const size_t at = ((size_t)b * HW + i / C) * ld + c;
        const float med = medians[c];
        const float zq = rintf(z[at] - med) + med;
        z_hat[at] = zq;
        const float* q = density + (size_t)c * DENSITY_FLOATS;
        const double lower = logits_cumulative(q, (double)zq - 0.5);
        const double upper = logits_cumulative(q, (double)zq + 0.5);
        const double t = lower + upper;
        const double sgn = t == 0.0 ? 0.0 : (t > 0.0 ? -1.0 : (t < 0.0 ? 1.0 : t));      // -torch.sign: 0 at 0, NaN at NaN
        const double p = lower_bound(fabs(sigmoid(sgn * upper) - sigmoid(sgn * lower)), (double)1e-9f);
        acc += -log2(p);
    }
    const double total = block_sum(acc, wave_total);
    if (threadIdx.x == 0) bits[b] = total;
}

}  // namespace

extern "C" int evc_elic_rate_pass_f32(const float* ms, int ld, int mean_off, int scale_off, int C, const float* y,
                                      int ld_y, int c0, int B, int H, int W, int parity, float* y_hat, double* bits,
                                      void* stream) {
    if (!ms || !y || !y_hat || !bits || C <= 0 || B <= 0 || H <= 0 || W <= 0 || (W & 1) || parity < 0 || parity > 1 ||
        mean_off < 0 || scale_off < 0 || mean_off + C > ld || scale_off + C > ld || c0 < 0 || c0 + C > ld_y)
        return EVC_EINVAL;
    hipLaunchKernelGGL(elic_rate_pass_kernel, dim3(B), dim3(RATE_THREADS), 0, (hipStream_t)stream, ms, ld, mean_off,
                       scale_off, C, y, ld_y, c0, H, W, parity, y_hat, bits);
    return EVC_LAUNCH_OK();
}

extern "C" int evc_bottleneck_rate_f32(const float* z, int ld, int C, int B, int H, int W, const float* medians,
                                       const float* density, float* z_hat, double* bits, void* stream) {
    if (!z || !medians || !density || !z_hat || !bits || C <= 0 || ld < C || B <= 0 || H <= 0 || W <= 0) return EVC_EINVAL;
    if ((long long)H * W > 0x7fffffffLL) return EVC_EUNSUPPORTED;
    hipLaunchKernelGGL(bottleneck_rate_kernel, dim3(B), dim3(RATE_THREADS), 0, (hipStream_t)stream, z, ld, C, H * W,
                       medians, density, z_hat, bits);
    return EVC_LAUNCH_OK();
}
