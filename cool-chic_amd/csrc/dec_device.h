// dec_device.h -- device helpers shared by the decoder's kernel files (dec_arm.hip, dec_tail.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ccmi {
namespace {

__device__ __forceinline__ int32_t tshift(int32_t s, int p) { return s < 0 ? -((-s) >> p) : s >> p; }
__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// int32 multiply with two's-complement wrap; the 24-bit form (v_mad_i32_i24, full rate)
// is exact whenever both operands fit in 24 signed bits.
template <bool F24>
__device__ __forceinline__ int32_t imul(int32_t a, int32_t b)
{
    if constexpr (F24) return __mul24(a, b);
    else return (int32_t)((uint32_t)a * (uint32_t)b);
}

} // namespace
} // namespace ccmi
