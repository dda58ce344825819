// ccmi_noise.h -- the counter-based generator of ccmi.h (ccmi_train_args.seed, and step 4e of ccmi_mix):
// splitmix64's finaliser, the 24-bit uniform in (0, 1] and the Box-Muller draw.  Included by train.hip
// (t_quant) and dec_mix.hip; tests/noise_ref.py restates it in numpy.
#pragma once

#include <stdint.h>

#include <hip/hip_runtime.h>

namespace ccmi {

__device__ __forceinline__ uint64_t mix64(uint64_t z)
{
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__device__ __forceinline__ float unif(uint64_t r) { return ((float)(r >> 40) + 0.5f) * 5.9604644775390625e-08f; }

// the unit Gaussian of the 64-bit word r: sqrtf(-2 logf(u1)) cospif(2 u2), u1 = unif(r),
// u2 = unif(mix64(r + 0x632BE59BD9B4E019)); the caller multiplies by its sigma
__device__ __forceinline__ float gauss_unit(uint64_t r)
{
    const float u1 = unif(r);
    const float u2 = unif(mix64(r + 0x632BE59BD9B4E019ull));
    return sqrtf(-2.f * logf(u1)) * cospif(2.f * u2);
}

} // namespace ccmi
