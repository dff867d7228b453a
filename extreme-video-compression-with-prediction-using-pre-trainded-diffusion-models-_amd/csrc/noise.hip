// noise.hip -- the specified noise generator of the job streams (noise specification N1).
//
// The score network is a generator: a receiver reproduces the sender's frames only if it draws the sender's noise.  So the
// noise is not "whatever the installed torch yields for a seed" but a function of a key the stream carries:
//
//   Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; multipliers 0xD2511F53, 0xCD9E8D57,
//   key increments 0x9E3779B9, 0xBB67AE85), key = (seed low, seed high), counter = (j, step, start frame, stream id);
//   the four words of block j give elements 4j .. 4j+3 of the sample: u = ((w >> 9) + 0.5) * 2^-23 in (0, 1),
//   r = sqrt(-2 ln u(w0)), theta = 2 pi u(w1) -> r cos theta, r sin theta; the same from (w2, w3).
//
// One launch fills one sampler step for the whole batch: blockIdx.y is the sample (its key: two loads, uniform over the
// block), one thread per 4-element block -> one 16-byte store per thread, consecutive lanes consecutive addresses.  A sample's
// numbers depend on its key only, not on its row or on B.  logf / sincosf / sqrtf are the accurate library functions on purpose
// (no fast intrinsics): sender and receiver must agree.  Measured at B = 32 (31.5 MB): 14 us per launch, 9 us with raw = 1 -- the
// arithmetic, not the HBM write (5 us), is the limit (profiles/NOTES.md).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/evc_hip.h"

namespace {

struct Words { uint32_t w0, w1, w2, w3; };

__device__ __forceinline__ Words philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
    constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r) { k0 += W0; k1 += W1; }
        const uint32_t hi0 = __umulhi(M0, c0), lo0 = M0 * c0;
        const uint32_t hi1 = __umulhi(M1, c2), lo1 = M1 * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1;
        c2 = hi0 ^ c3 ^ k1; c3 = lo0;
    }
    return {c0, c1, c2, c3};
}

__device__ __forceinline__ float unit_open(uint32_t w) { return ((float)(w >> 9) + 0.5f) * 0x1p-23f; }   // exact in fp32

__device__ __forceinline__ void box_muller(uint32_t wa, uint32_t wb, float& z0, float& z1) {
    const float r = sqrtf(-2.0f * logf(unit_open(wa)));
    float s, c;
    sincosf(6.283185307179586f * unit_open(wb), &s, &c);
    z0 = r * c;
    z1 = r * s;
}

__global__ void __launch_bounds__(256)
noise_normal_kernel(float4* __restrict__ out, const uint32_t* __restrict__ keys, uint32_t n4, uint32_t seed_lo, uint32_t seed_hi,
                    uint32_t step, int raw) {
    const uint32_t b = blockIdx.y;
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n4) return;
    const uint32_t stream_id = keys[2 * b], start = keys[2 * b + 1];
    const Words w = philox4x32_10(j, step, start, stream_id, seed_lo, seed_hi);
    float4 v;
    if (raw) {
        v = make_float4(__uint_as_float(w.w0), __uint_as_float(w.w1), __uint_as_float(w.w2), __uint_as_float(w.w3));
    } else {
        box_muller(w.w0, w.w1, v.x, v.y);
        box_muller(w.w2, w.w3, v.z, v.w);
    }
    out[(size_t)b * n4 + j] = v;
}

}  // namespace

extern "C" int evc_noise_normal_f32(float* out, const unsigned* keys, int B, long long n, unsigned long long seed, unsigned step,
                                    int raw, void* stream) {
    if (!out || !keys || B <= 0 || B > 65535 || n <= 0 || n % 4 != 0 || n / 4 > 0x7FFFFFFFLL) return EVC_EINVAL;
    const uint32_t n4 = (uint32_t)(n / 4);
    const dim3 grid((n4 + 255) / 256, (unsigned)B);
    hipLaunchKernelGGL(noise_normal_kernel, grid, dim3(256), 0, (hipStream_t)stream, reinterpret_cast<float4*>(out), keys, n4,
                       (uint32_t)(seed & 0xFFFFFFFFull), (uint32_t)(seed >> 32), step, raw);
    return hipGetLastError() == hipSuccess ? EVC_OK : EVC_ELAUNCH;
}
