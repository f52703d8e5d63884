// One correctly rounded operation at a time, never contracted into an FMA: what the kernels
// that reproduce a sequential host loop bit for bit are written in (the monotonic sweep of
// operators_pybind11.cc:14-36, the tap loop of apply_filter, NumPy's elementwise arithmetic).
#pragma once

#include <hip/hip_runtime.h>

namespace smi {

__device__ __forceinline__ float mul_rn(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ double mul_rn(double a, double b) { return __dmul_rn(a, b); }
__device__ __forceinline__ float add_rn(float a, float b) { return __fadd_rn(a, b); }
__device__ __forceinline__ double add_rn(double a, double b) { return __dadd_rn(a, b); }
// correctly rounded quotient (IEEE division, not the reciprocal approximation)
__device__ __forceinline__ float div_rn(float a, float b) { return __fdiv_rn(a, b); }
__device__ __forceinline__ double div_rn(double a, double b) { return __ddiv_rn(a, b); }

// The compiler's correctly rounded sqrtf multiplies an operand below kSqrtNormalMin = 2^-96
// (0x0f800000, the constant it compares with before v_sqrt_f32) by 2^32 first, so that the
// residuals below stay normal, scales the root back by 2^-16, and hands zero and +inf through a
// class test.  sqrt_rn_normal is what is left for an operand at or above kSqrtNormalMin: the
// hardware root (within one ulp) and the same two-sided correction from the signs of the exact
// residuals x - s * prev(s) and x - s * next(s).  Same bits as sqrtf there.  +inf gives +inf
// (both residuals are NaN and select nothing); NaN gives NaN.  Not for zero or negative operands.
constexpr float kSqrtNormalMin = 0x1p-96f;
__device__ __forceinline__ float sqrt_rn_normal(float x) {
    const float s = __builtin_amdgcn_sqrtf(x);
    const float dn = __uint_as_float(__float_as_uint(s) - 1u);
    const float up = __uint_as_float(__float_as_uint(s) + 1u);
    const float r_dn = fmaf(-dn, s, x), r_up = fmaf(-up, s, x);
    float r = r_dn <= 0.f ? dn : s;
    r = r_up > 0.f ? up : r;
    return r;
}

}  // namespace smi
