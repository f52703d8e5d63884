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

}  // namespace smi
