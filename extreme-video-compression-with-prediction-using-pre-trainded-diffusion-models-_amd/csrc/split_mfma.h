// split_mfma.h -- device helpers shared by the kernels that run fp32 GEMMs on the 16-bit matrix cores (conv_igemm.hip,
// nin_gemm.hip): the MFMA fragment types, the exact bf16 / scaled fp16 operand splits with their cross-product order, and the
// power-of-two scale of a raw operand from its element bound.  The arithmetic itself is described in conv_igemm.hip.
#pragma once
#include <hip/hip_runtime.h>

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// f16x3 on a source with no GroupNorm in front of it (raw residual stream, attention output): the caller supplies a bound
// on the tensor's elements, taken from its per-channel moments (evc_gn_coeffs_bound_f32 / evc_moments_bound_f32), and the
// whole tensor is scaled by the power of two that brings that bound into [2^6, 2^7) before the fp16 split: nothing can
// overflow (<= 2^7 * 8 = 1024), typical elements sit far above fp16's subnormals, and the exact inverse goes into the
// accumulator scale.  Wave-uniform, evaluated once per kernel.
// A bound that is not finite (the NaN pattern the bound kernels write when a moment is NaN / inf) gives a NaN scale: the
// operands, the accumulator scale and so the whole output are NaN -- a non-finite input never becomes finite numbers.
__device__ __forceinline__ float bound_scale(unsigned bits) {
    const float b = sqrtf(__uint_as_float(bits));
    if (!(b < 3.0e38f)) return __builtin_nanf("");
    return b > 0.f ? ldexpf(1.0f, 6 - ilogbf(b)) : 1.0f;
}

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ void split3_bf16(const float4& v0, const float4& v1, bf16x8& p1, bf16x8& p2, bf16x8& p3) {
    const float x[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const __bf16 a = (__bf16)x[j];
        const float r = x[j] - (float)a;
        const __bf16 b = (__bf16)r;
        p1[j] = a; p2[j] = b; p3[j] = (__bf16)(r - (float)b);
    }
}

constexpr float F16_ACT_SCALE = 8.0f;
constexpr int F16_HDR_BYTES = 256;   // header of an f16x3 weight pack: [0] = 1 / (S_a * S_w), [1] = S_w; the planes follow

__device__ __forceinline__ void split2_f16(const float4& v0, const float4& v1, float xscale, f16x8& p1, f16x8& p2) {
    const float x[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        // no clamp: an element beyond fp16's range becomes (inf, -inf) and NaN in the accumulator -- loud, never a silently
        // saturated value; a NaN stays a NaN.  Whether it can happen is reported by evc_gn_coeffs_bound_f32 (EVC_RANGE_*).
        const float v = x[j] * xscale;
        const _Float16 a = (_Float16)v;
        p1[j] = a; p2[j] = (_Float16)(v - (float)a);
    }
}

// The two split arithmetics share their kernels: NP = planes per operand (3: bf16x6, 2: f16x3).
template <int NP> struct Split;
template <> struct Split<3> {
    typedef bf16x8 vec;
    static constexpr int NTERM = 6;
    // cross products, smallest first: (a plane, b plane)
    static __device__ __forceinline__ constexpr int qa(int t) { return t == 0 ? 2 : (t == 1 || t == 3) ? 1 : 0; }
    static __device__ __forceinline__ constexpr int qb(int t) { return t == 2 ? 2 : (t == 1 || t == 4) ? 1 : 0; }
    static __device__ __forceinline__ f32x16 mfma(const vec& a, const vec& b, const f32x16& c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
    }
    static __device__ __forceinline__ void split(const float4& v0, const float4& v1, float, vec (&pl)[3]) {
        split3_bf16(v0, v1, pl[0], pl[1], pl[2]);
    }
};
template <> struct Split<2> {
    typedef f16x8 vec;
    static constexpr int NTERM = 3;
    static __device__ __forceinline__ constexpr int qa(int t) { return t == 0 ? 1 : 0; }
    static __device__ __forceinline__ constexpr int qb(int t) { return t == 1 ? 1 : 0; }
    static __device__ __forceinline__ f32x16 mfma(const vec& a, const vec& b, const f32x16& c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
    }
    static __device__ __forceinline__ void split(const float4& v0, const float4& v1, float xscale, vec (&pl)[2]) {
        split2_f16(v0, v1, xscale, pl[0], pl[1]);
    }
};

}  // namespace
