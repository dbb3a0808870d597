// dis_half.h -- the f16 flow format (DIS_FLOW_F16, include/dis_abi.h): the one
// narrowing every flow writer and dis_flow_convert's kernel use, the exact
// widening of the readers, and the flow stores overloaded on the output type.
//
// narrow2 is the packed f32 -> f16 conversion in round-to-nearest-even with
// f16 denormals on (the gfx950 default mode): subnormals kept, |v| >= 65520 to
// +-inf, NaN stays NaN -- numpy's astype(float16), bit for bit on non-NaN
// values (tests/test_gpu_f16.py walks every rounding boundary). Never the
// round-toward-zero pack conversion.
#pragma once

#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

namespace dis {

__device__ __forceinline__ __half2 narrow2(float2 v) { return __floats2half2_rn(v.x, v.y); }
__device__ __forceinline__ float2 widen2(__half2 h) { return __half22float2(h); }

// two adjacent f16 vectors: one 8-byte access
struct alignas(8) half2x2 {
    __half2 a, b;
};

// one flow vector in the output's type
__device__ __forceinline__ void store_flow1(float2* dst, float2 o) { *dst = o; }
__device__ __forceinline__ void store_flow1(__half2* dst, float2 o) { *dst = narrow2(o); }

}  // namespace dis
