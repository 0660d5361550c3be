// 16-byte loads and stores of the streaming kernels (norm.hip, perceptual.hip, spectral.hip): four consecutive floats
// at a 16-byte aligned address, one access per lane.
#pragma once
#include <hip/hip_runtime.h>

namespace csg {

__device__ __forceinline__ float4 ld4(const float* p) { return *(const float4*)p; }
__device__ __forceinline__ void st4(float* p, float4 v) { *(float4*)p = v; }

}  // namespace csg
