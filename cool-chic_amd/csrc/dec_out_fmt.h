// dec_out_fmt.h -- path B: what the kernels of the formatted sink (ccmi_tensor_fmt) share: the
// float32 operations that stay uncontracted, the element types, and steps 4-6 of the contract for a
// thread's 4 destination pixels.  Included by dec_out.hip (the output stage) and dec_filter.hip (the
// filter stage); everything is internal to the including file.
#pragma once

#include "dec_device.h"
#include "dec_internal.h"

namespace ccmi {
namespace {

constexpr int kOutThreads = 256; // threads of an output-stage block

// Every product and sum below is its own float32 operation: the library is built with the
// compiler's default contraction, under which a * b + c may become one fused operation -- also
// through __fmul_rn / __fadd_rn, which are plain inline operators in this toolchain's headers --
// so the two helpers switch contraction off for their own instruction.
__device__ __forceinline__ float fmt_mul(float a, float b)
{
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ float fmt_add(float a, float b)
{
#pragma clang fp contract(off)
    return a + b;
}

struct F16 {
    _Float16 v;
};
struct Bf16 {
    uint16_t bits;
};
template <typename T> struct FmtVec;
template <> struct FmtVec<float> { using type = float4; };
template <> struct FmtVec<F16> { using type = uint2; };
template <> struct FmtVec<Bf16> { using type = uint2; };

template <typename T> __device__ __forceinline__ T fmt_elem(float r);
template <> __device__ __forceinline__ float fmt_elem<float>(float r) { return r; }
template <> __device__ __forceinline__ F16 fmt_elem<F16>(float r) { return F16{(_Float16)r}; } // v_cvt_f16_f32, RNE
template <> __device__ __forceinline__ Bf16 fmt_elem<Bf16>(float r)
{
    uint32_t u = __float_as_uint(r);
    if ((u & 0x7fffffffu) > 0x7f800000u) return Bf16{0x7fc0}; // NaN (a finite scale and bias make none)
    u += 0x7fffu + ((u >> 16) & 1u); // round to nearest even
    return Bf16{(uint16_t)(u >> 16)};
}

struct DecFmtCall { // one value per launch
    float scale[3], bias[3];
    int64_t sc, sy, sx;
};

// groups of 4 destination pixels that cover one row plus the up to 3 lead-in slots
__host__ __device__ inline int fmt_row_groups(int w) { return (w + 3 + 3) / 4; }

// step 6 for a thread's 4 destination pixels d0 .. d0 + 3 of the row at `row` elements (w pixels
// wide): the packed stores where the layout and the alignment allow them
template <typename T>
__device__ __forceinline__ void fmt_store(const T (&v)[3][4], T *__restrict__ dst, const DecFmtCall &C, int64_t row,
                                          int d0, int w, bool nchw, bool nhwc)
{
    using Vec = typename FmtVec<T>::type;
    const bool full = d0 >= 0 && d0 + 4 <= w;
    if (nchw) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            T *p = dst + c * C.sc + row + d0;
            if (full && reinterpret_cast<uintptr_t>(p) % sizeof(Vec) == 0) {
                Vec pk;
                __builtin_memcpy(&pk, v[c], sizeof pk);
                *reinterpret_cast<Vec *>(p) = pk;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (d0 + k >= 0 && d0 + k < w) p[k] = v[c][k];
            }
        }
    } else if (nhwc && full) { // aligned by the choice of mis
        T e[12];
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int c = 0; c < 3; ++c) e[3 * k + c] = v[c][k];
        Vec *p = reinterpret_cast<Vec *>(dst + row + 3 * (int64_t)d0);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            Vec pk;
            __builtin_memcpy(&pk, e + 4 * j, sizeof pk);
            p[j] = pk;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (d0 + k < 0 || d0 + k >= w) continue;
#pragma unroll
            for (int c = 0; c < 3; ++c) dst[c * C.sc + row + (d0 + k) * C.sx] = v[c][k];
        }
    }
}

// group gi of row y of a w-wide frame at dst: its first destination pixel d0 (the groups of a row
// start at the naturally aligned address at or below the row's channel-0 element), the row's offset
// and the layout; false: the group lies past the row
template <typename T>
__device__ __forceinline__ bool fmt_group_at(const T *dst, const DecFmtCall &C, int y, int gi, int w, int &d0, int64_t &row,
                                             bool &nchw, bool &nhwc)
{
    nchw = C.sx == 1, nhwc = !nchw && C.sc == 1 && C.sx == 3;
    row = (int64_t)y * C.sy;
    // elements from address 0 to (channel 0, y, x' = 0); group k starts mis slots before it, where
    // the address of its first pixel is a multiple of 4 elements (NHWC: 3 mis == a0 mod 4)
    const uint64_t a0 = (uint64_t)(reinterpret_cast<uintptr_t>(dst) / sizeof(T)) + (uint64_t)row;
    const int mis = nchw ? (int)(a0 & 3) : nhwc ? (int)((3 * a0) & 3) : 0;
    d0 = 4 * gi - mis;
    return d0 < w;
}

// the thread's row y and first destination pixel d0 of a w-wide row (see above); false: no work
template <typename T>
__device__ __forceinline__ bool fmt_group(const T *dst, const DecFmtCall &C, int h, int w, int &y, int &d0, int64_t &row,
                                          bool &nchw, bool &nhwc)
{
    const int gpr = fmt_row_groups(w);
    const int64_t g = (int64_t)blockIdx.x * kOutThreads + threadIdx.x;
    y = (int)(g / gpr);
    if (y >= h) return false;
    return fmt_group_at<T>(dst, C, y, (int)(g - (int64_t)y * gpr), w, d0, row, nchw, nhwc);
}

inline DecFmtCall fmt_call(const DecFmt &f)
{
    DecFmtCall C;
    for (int c = 0; c < 3; ++c) C.scale[c] = f.scale[c], C.bias[c] = f.bias[c];
    C.sc = f.stride_c, C.sy = f.stride_y, C.sx = f.stride_x;
    return C;
}

// launch(T{}) for the element type T of a formatted-output kernel
template <typename Launch>
int with_elem_type(int elem, Launch &&launch)
{
    switch (elem) {
    case CCMI_ELEM_F32: launch(float{}); break;
    case CCMI_ELEM_F16: launch(F16{}); break;
    case CCMI_ELEM_BF16: launch(Bf16{}); break;
    default: return ccmi_set_error(CCMI_ERR_ARG, "dec: element type %d", elem);
    }
    CCMI_HIP_CHECK(hipGetLastError());
    return CCMI_OK;
}

} // namespace
} // namespace ccmi
