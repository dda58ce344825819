// dec_out.hip -- path B: the output stage of the bit-exact fixed-point .cool decoder: the 12-bit
// synthesis output of dec_tail.hip to file bytes, planar tensors or the formatted tensor, every
// sink for one frame (the per-frame tail: the frame is the kernel's argument) and for a tail group
// (frame blockIdx.y of the group's tables).
//
//  dec_output       444 -> 420/444 8/10-bit or PPM payload (ccdecapi.cpp:59-240).
//  dec_output_tensor  the same samples as planar u8 / u16 / f32 device tensors (no file
//                   layout): one packed store per 4 destination samples, any sample alignment.
//  The formatted tensor of a ccmi_tensor_fmt has seven geometries, each a description (a struct)
//  that three kernel templates are instantiated over -- dec_fmt<G, T, TABLE>, its colour form
//  dec_fmt_col<G, T, TABLE> (ccmi_colour) and the statistics pass dec_fmt_stat<G, TABLE>:
//  Plain            the same samples as three full-size channels, YUV -> RGB, scale / bias, f32 /
//                   f16 / bf16, strides, mirror.
//  Resize<CUBIC>    with a ccmi_resample: the region through an antialiased triangle filter to the
//                   output size, horizontal (dec_resize_h<CUBIC>, dec_resize_h_batch<CUBIC>) then
//                   vertical pass; CUBIC (CCMI_FILTER_CUBIC): the Keys cubic, a = -0.5.
//  Warp<CUBIC, PERSP>  with a ccmi_warp: every output pixel a bilinear sample of the frame at the
//                   position the frame's 2 x 3 matrix gives, fill or edge padding; CUBIC
//                   (CCMI_WARP_CUBIC): cubic convolution, A = -0.75, 16 taps; PERSP
//                   (CCMI_WARP_PROJECTIVE): a 3 x 3 matrix per frame, the position the quotient by
//                   its third row.  The cubic forms have the optional clamp of r' to [0, 1].
//
// The tail sees four functions (dec_internal.h): the size and the filling of an entry of a group's
// output section, launch_dec_out_group and launch_dec_out_frame.  Both launchers choose the
// geometry once (with_geometry) and hand its grid and its frame or tables to launch_fmt_forms,
// which is the only place that knows the colour protocol and the element types.  A new formatted
// sink is one more geometry struct and one more row of with_geometry; a new element type one more
// case of with_elem_type.
#include <stdlib.h>

#include <tuple>
#include <type_traits>

#include "dec_device.h"
#include "dec_internal.h"
#include "dec_out_fmt.h"

namespace ccmi {
namespace {

constexpr int kThreads = kOutThreads;

// a 12-bit synthesis value as a sample in 0 .. maxv: the rounding and the clamp of ccdecapi.cpp
__device__ __forceinline__ int32_t smp(int32_t v, int maxv)
{
    const int32_t s = (v * maxv + (1 << (kSynPrec - 1))) >> kSynPrec;
    return s < 0 ? 0 : (s > maxv ? maxv : s);
}

// ------------------------------------------------------------------ output bytes
struct DecOut {
    const int32_t *syn;
    int H, W, maxv, kind;
    int bps_or_flags; // the byte output: bytes per sample; a formatted group: the frame's kFmt* flags; else unused
    uint8_t *dst;
};

__device__ __forceinline__ void output_body(const int32_t *__restrict__ syn, int H, int W, int maxv, int kind, int bps,
                                            uint8_t *__restrict__ dst);

__global__ __launch_bounds__(kThreads) void dec_output_kernel(const int32_t *__restrict__ syn, int H, int W, int maxv,
                                                              int kind, int bps, uint8_t *__restrict__ dst)
{
    output_body(syn, H, W, maxv, kind, bps, dst);
}

__global__ __launch_bounds__(kThreads) void dec_output_batch(const DecOut *__restrict__ Os)
{
    const DecOut O = Os[blockIdx.y];
    output_body(O.syn, O.H, O.W, O.maxv, O.kind, O.bps_or_flags, O.dst);
}

__device__ __forceinline__ void output_body(const int32_t *__restrict__ syn, int H, int W, int maxv, int kind, int bps,
                                            uint8_t *__restrict__ dst)
{
    const int64_t plane = (int64_t)H * W;
    const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (p >= plane) return;
    auto put = [&](int64_t idx, int32_t s, bool big_endian) {
        if (bps == 1) dst[idx] = (uint8_t)s;
        else if (big_endian) { dst[2 * idx] = (uint8_t)(s >> 8); dst[2 * idx + 1] = (uint8_t)s; }
        else { dst[2 * idx] = (uint8_t)s; dst[2 * idx + 1] = (uint8_t)(s >> 8); }
    };
    const int y = (int)(p / W), x = (int)(p - (int64_t)y * W);
    if (kind == 2) { // PPM: interleaved RGB, 16-bit big endian
        for (int c = 0; c < 3; ++c) put(3 * p + c, smp(syn[c * plane + p], maxv), true);
        return;
    }
    put(p, smp(syn[p], maxv), false);
    if (kind == 1) {
        put(plane + p, smp(syn[plane + p], maxv), false);
        put(2 * plane + p, smp(syn[2 * plane + p], maxv), false);
    } else if (!(y & 1) && !(x & 1) && (y >> 1) < H / 2 && (x >> 1) < W / 2) {
        const int64_t cp = (int64_t)(H / 2) * (W / 2), ci = (int64_t)(y >> 1) * (W / 2) + (x >> 1);
        put(plane + ci, smp(syn[plane + p], maxv), false);
        put(plane + cp + ci, smp(syn[2 * plane + p], maxv), false);
    }
}

// ------------------------------------------------------------------ output tensors
// Device sink: the same samples as output_body (smp(), same 420 subsampling) in planar
// tensor layout, never interleaved.  Both layouts are ONE flat array of samples:
//   444: [3][H][W], sample j is smp(syn[j]);
//   420: Y[H][W] then U, V [H/2][W/2], contiguous: j < HW as above, the rest a stride-2 gather.
// A thread owns one naturally aligned group of 4 destination samples (one 32 / 64 / 128-bit
// store for u8 / u16 / f32).  dst only has the alignment of one sample, so the groups are
// laid out from the aligned address at or below dst: the first and the last group of a frame
// are partial and take scalar stores, every other group one packed store -- the chroma
// samples too, which the byte path writes one byte per thread.  DecOut::bps_or_flags is unused here
// (the sample type is the template argument).
template <typename T> struct OutVec;
template <> struct OutVec<uint8_t> { using type = uint32_t; };
template <> struct OutVec<uint16_t> { using type = uint2; };
template <> struct OutVec<float> { using type = float4; };

template <typename T> __device__ __forceinline__ T out_sample(int32_t s, float fmax);
template <> __device__ __forceinline__ uint8_t out_sample<uint8_t>(int32_t s, float) { return (uint8_t)s; }
template <> __device__ __forceinline__ uint16_t out_sample<uint16_t>(int32_t s, float) { return (uint16_t)s; }
// one correctly rounded division: what torch's u.to(float32) / maxv computes
template <> __device__ __forceinline__ float out_sample<float>(int32_t s, float fmax) { return __fdiv_rn((float)s, fmax); }

// CROP (the per-frame tail of a region decode): H x W is the region, whose sample (y, x) of
// plane c is syn[c * splane + (oy + y) * spitch + ox + x] of the whole-frame synthesis output
// (oy, ox even for 420, so the chroma's even rows and columns are the frame's).
template <typename T, bool CROP>
__device__ __forceinline__ void output_tensor_body(const int32_t *__restrict__ syn, int H, int W, int maxv, int kind,
                                                   T *__restrict__ dst, int64_t splane = 0, int spitch = 0, int oy = 0,
                                                   int ox = 0)
{
    const int64_t plane = (int64_t)H * W;
    auto direct_at = [&](int64_t j) { // flat sample j of the [.][H][W] prefix
        if (!CROP) return j;
        const int64_t c = j / plane, rem = j - c * plane;
        const int y = (int)(rem / W), x = (int)(rem - (int64_t)y * W);
        return c * splane + (int64_t)(oy + y) * spitch + ox + x;
    };
    const int ch = H / 2, cw = W / 2;
    const int64_t cp = (int64_t)ch * cw;
    const int64_t elems = kind == 1 ? 3 * plane : plane + 2 * cp;
    const int64_t direct = kind == 1 ? elems : plane; // samples below this index read syn[j]
    const int mis = (int)((reinterpret_cast<uintptr_t>(dst) / sizeof(T)) & 3); // samples past the aligned address
    const int64_t j0 = ((int64_t)blockIdx.x * kThreads + threadIdx.x) * 4 - mis;
    if (j0 >= elems) return;
    const float fmax = (float)maxv;
    T v[4];
    if (j0 >= 0 && j0 + 4 <= direct) { // the common case: 4 samples of the flat prefix
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = out_sample<T>(smp(syn[direct_at(j0 + k)], maxv), fmax);
    } else {
        // a group that is partial, crosses into the chroma planes or lies in them: one
        // division for its first chroma sample, the others step along the row
        int64_t c = 0;
        int cy = 0, cx = 0;
        const int64_t jc = (j0 > direct ? j0 : direct) - direct; // first chroma index of the group
        if (kind != 1 && cp > 0) {
            c = jc / cp;
            const int64_t ci = jc - c * cp;
            cy = (int)(ci / cw);
            cx = (int)(ci - (int64_t)cy * cw);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t j = j0 + k;
            v[k] = T(0);
            if (j < 0 || j >= elems) continue;
            if (j < direct) {
                v[k] = out_sample<T>(smp(syn[direct_at(j)], maxv), fmax);
                continue;
            }
            v[k] = out_sample<T>(smp(syn[CROP ? (1 + c) * splane + (int64_t)(oy + 2 * cy) * spitch + ox + 2 * cx
                                              : (1 + c) * plane + (int64_t)(2 * cy) * W + 2 * cx],
                                     maxv),
                                 fmax);
            if (++cx == cw) {
                cx = 0;
                if (++cy == ch) {
                    cy = 0;
                    ++c;
                }
            }
        }
    }
    if (j0 >= 0 && j0 + 4 <= elems) {
        typename OutVec<T>::type pk;
        __builtin_memcpy(&pk, v, sizeof pk);
        *reinterpret_cast<typename OutVec<T>::type *>(dst + j0) = pk;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (j0 + k >= 0 && j0 + k < elems) dst[j0 + k] = v[k];
    }
}

template <typename T>
__global__ __launch_bounds__(kThreads) void dec_output_tensor(const int32_t *__restrict__ syn, int H, int W, int maxv,
                                                              int kind, T *__restrict__ dst)
{
    output_tensor_body<T, false>(syn, H, W, maxv, kind, dst);
}

// h x w = the region at (oy, ox) of the H x W frame
template <typename T>
__global__ __launch_bounds__(kThreads) void dec_output_tensor_crop(const int32_t *__restrict__ syn, int H, int W, int oy,
                                                                   int ox, int h, int w, int maxv, int kind,
                                                                   T *__restrict__ dst)
{
    output_tensor_body<T, true>(syn, h, w, maxv, kind, dst, (int64_t)H * W, W, oy, ox);
}

template <typename T> __global__ __launch_bounds__(kThreads) void dec_output_tensor_batch(const DecOut *__restrict__ Os)
{
    const DecOut O = Os[blockIdx.y];
    output_tensor_body<T, false>(O.syn, O.H, O.W, O.maxv, O.kind, reinterpret_cast<T *>(O.dst));
}

// blocks that cover the samples of one frame plus the up to 3 lead-in slots of an unaligned dst
unsigned output_tensor_blocks(int h, int w, int kind)
{
    const int64_t plane = (int64_t)h * w;
    const int64_t elems = kind == 1 ? 3 * plane : plane + 2 * (int64_t)(h / 2) * (w / 2);
    const int64_t groups = (elems + 3 + 3) / 4;
    return (unsigned)((groups + kThreads - 1) / kThreads);
}

// ------------------------------------------------------------------ formatted output tensors
// Device sink with a ccmi_tensor_fmt (the contract is in ccmi.h): per region pixel the three
// samples of output_tensor_body (420: planes 1 and 2 at the even row and column, the nearest x2
// upsample), normalised, optionally through the YUV -> RGB matrix, scaled and biased, converted
// to float / half / bfloat16 and stored at dst + c sc + y sy + x' sx.  A thread owns 4
// consecutive destination pixels x' of one row with all three channels in registers; mirror
// reads them from x = w - 1 - x'.  The groups of a row start at the naturally aligned address at
// or below the row's channel-0 element (as output_tensor_body lays them out per frame), so with
// sx == 1 (NCHW) a full group of an aligned channel is one packed store, and with sc == 1,
// sx == 3 (NHWC) a full group's 12 elements are three; partial groups, channels whose rows are
// not aligned alike, and every other stride set take one store per element.
// The uncontracted float32 operations (fmt_mul, fmt_add), the element types and steps 4-6 for a
// thread's group (fmt_group, fmt_store) are in dec_out_fmt.h, shared with the filter stage.

// the float32 roundings of yuv2rgb's matrix (ccmi/io.py) and of its offsets / 255: R, G, B
__device__ constexpr float kFmtA[3] = {(float)-0.000007154783816076815, (float)-0.3441331386566162, (float)1.7720025777816772};
__device__ constexpr float kFmtB[3] = {(float)1.4019975662231445, (float)-0.7141380310058594, (float)0.00001542569043522235};
__device__ constexpr float kFmtO[3] = {(float)(-179.45477266423404 / 255.0), (float)(135.45870971679688 / 255.0),
                                       (float)(-226.8183044444304 / 255.0)};

// per-frame flags (DecOut::bps_or_flags of a formatted group); kFmtClamp is a cubic call's (one per
// call): its kernels clamp r' to [0, 1], the others never see it
enum { kFmtMirror = 1, kFmtMatrix = 2, kFmtClamp = 4 };

// steps 1-3 of the contract for one pixel: lrow / crow point at the pixel's luma row and at the
// row its chroma is taken from, x / xc are its luma and chroma columns
__device__ __forceinline__ void fmt_pixel(const int32_t *__restrict__ lrow, const int32_t *__restrict__ crow,
                                          int64_t splane, int x, int xc, int maxv, float fmax, bool matrix, float (&q)[3])
{
    auto unit = [maxv, fmax](int32_t v) { return __fdiv_rn((float)smp(v, maxv), fmax); };
    const float p0 = unit(lrow[x]), p1 = unit(crow[splane + xc]), p2 = unit(crow[2 * splane + xc]);
    q[0] = p0, q[1] = p1, q[2] = p2;
    if (matrix) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float t = fmt_add(fmt_add(fmt_add(p0, fmt_mul(kFmtA[c], p1)), fmt_mul(kFmtB[c], p2)), kFmtO[c]);
            q[c] = fminf(fmaxf(t, 0.f), 1.f);
        }
    }
}

// ---- the colour stage (step 3z of the contract in ccmi.h, ccmi_colour)
// The three output bodies below take a mode: kColNone is the body as it always was (the kernels
// without colour instantiate it, and nothing of the stage is compiled into them); kColWrite puts
// the pixel through its frame's ops between the geometry and scale / bias; kColStat is the
// statistics pass of the frames with a contrast op: the same pixels through the ops that precede
// the contrast op, their integer grey terms summed per thread, per wave and, by one 64-bit atomic
// add per wave, per frame.  Nothing is stored in that mode and no thread leaves before the wave's
// reduction.  The pass evaluates the geometry a second time and stages nothing: what it would stage
// is three float32 per output pixel written and read again, more traffic than the taps it re-reads
// from a synthesis output that the stage before has just left in the cache.
// The op table is one DecCol per frame in the tail's argument tables, or the kernel's own argument
// (the per-frame tail): uniform per block, so the loop over the ops branches on scalars.
enum { kColNone = 0, kColWrite = 1, kColStat = 2 };

__device__ __forceinline__ float col_clamp(float t) { return fminf(fmaxf(t, 0.f), 1.f); }

__device__ __forceinline__ float col_grey(const float (&x)[3])
{
    return fmt_add(fmt_add(fmt_mul(0.2989f, x[0]), fmt_mul(0.587f, x[1])), fmt_mul(0.114f, x[2]));
}

// ops [first, last) of the frame on one pixel; mean = m_j (read by a contrast op only)
__device__ __forceinline__ void col_ops(const DecCol &K, int first, int last, float mean, float (&x)[3])
{
    for (int i = first; i < last; ++i) {
        const DecColOp &P = K.ops[i];
        if (P.op == CCMI_COL_MATRIX) {
            float y[3];
#pragma unroll
            for (int c = 0; c < 3; ++c)
                y[c] = col_clamp(fmt_add(
                    fmt_add(fmt_add(fmt_mul(P.v[4 * c], x[0]), fmt_mul(P.v[4 * c + 1], x[1])), fmt_mul(P.v[4 * c + 2], x[2])),
                    P.v[4 * c + 3]));
#pragma unroll
            for (int c = 0; c < 3; ++c) x[c] = y[c];
        } else if (P.op == CCMI_COL_BRIGHTNESS) {
#pragma unroll
            for (int c = 0; c < 3; ++c) x[c] = col_clamp(fmt_mul(P.v[0], x[c]));
        } else { // towards the pixel's grey (saturation) or the frame's mean grey (contrast)
            const float b = fmt_mul(P.v[1], P.op == CCMI_COL_SATURATION ? col_grey(x) : mean);
#pragma unroll
            for (int c = 0; c < 3; ++c) x[c] = col_clamp(fmt_add(fmt_mul(P.v[0], x[c]), b));
        }
    }
}

// kColWrite: m_j of a frame of npix output pixels from the sum the statistics pass left
__device__ __forceinline__ float col_mean(const DecCol &K, int npix)
{
    if (K.contrast < 0) return 0.f;
    const float m = (float)((double)*K.acc / ((double)npix * 65535.0));
    return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(m))); // one value per block: kept in a scalar
}

// kColStat: one pixel's term of S_j, at most 65535
__device__ __forceinline__ uint32_t col_term(const DecCol &K, float (&x)[3])
{
    col_ops(K, 0, K.contrast, 0.f, x);
    return (uint32_t)rintf(fmt_mul(col_clamp(col_grey(x)), 65535.0f));
}

// kColStat: the thread's sum (4 pixels) -> the wave's (at most 2^24) -> the frame's; every lane of
// the wave arrives here.  Integer additions: the order of the waves does not show in the sum.
__device__ __forceinline__ void col_accumulate(const DecCol &K, uint32_t sum)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    if ((threadIdx.x & 63) == 0 && sum) atomicAdd(K.acc, (unsigned long long)sum);
}

// the format of a statistics pass: its groups of 4 pixels start at pixel 0 of every row
__device__ __forceinline__ DecFmtCall col_stat_call()
{
    DecFmtCall C{};
    return C;
}

// h x w = the region at (oy, ox) of the synthesis output syn (planes splane apart, pitch spitch;
// oy, ox even for kind 0)
template <typename T, int COL = kColNone>
__device__ __forceinline__ uint32_t output_fmt_body(const int32_t *__restrict__ syn, int64_t splane, int spitch, int oy,
                                                    int ox, int h, int w, int maxv, int kind, int flags,
                                                    T *__restrict__ dst, const DecFmtCall &C, const DecCol *K = nullptr)
{
    int y, d0;
    int64_t row;
    bool nchw, nhwc;
    if (!fmt_group<T>(dst, C, h, w, y, d0, row, nchw, nhwc)) return 0;
    float mean = 0.f;
    uint32_t sum = 0;
    if constexpr (COL == kColWrite) mean = col_mean(*K, h * w);
    const float fmax = (float)maxv;
    const bool mirror = flags & kFmtMirror, matrix = flags & kFmtMatrix;
    const int32_t *__restrict__ lrow = syn + (int64_t)(oy + y) * spitch + ox;
    const int32_t *__restrict__ crow = syn + (int64_t)(oy + (kind == 1 ? y : y & ~1)) * spitch + ox;
    T v[3][4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int d = d0 + k;
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c][k] = fmt_elem<T>(0.f);
        if (d < 0 || d >= w) continue;
        const int x = mirror ? w - 1 - d : d;
        float q[3];
        fmt_pixel(lrow, crow, splane, x, kind == 1 ? x : x & ~1, maxv, fmax, matrix, q);
        if constexpr (COL == kColStat) {
            sum += col_term(*K, q);
            continue;
        }
        if constexpr (COL == kColWrite) col_ops(*K, 0, K->n, mean, q);
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c][k] = fmt_elem<T>(fmt_add(fmt_mul(q[c], C.scale[c]), C.bias[c]));
    }
    if constexpr (COL != kColStat) fmt_store<T>(v, dst, C, row, d0, w, nchw, nhwc);
    return sum;
}

unsigned output_fmt_blocks(int h, int w)
{
    return (unsigned)(((int64_t)h * fmt_row_groups(w) + kThreads - 1) / kThreads);
}

int fmt_flags(const DecFmt &f)
{
    return (f.mirror ? kFmtMirror : 0) | (f.matrix ? kFmtMatrix : 0) | (f.cubic && f.clamp ? kFmtClamp : 0);
}

// ------------------------------------------------------------------ resampled formatted output
// The formatted sink with a ccmi_resample (steps 3a-3c of the contract in ccmi.h): the region,
// h x w, goes through an antialiased triangle filter to oh x ow between the colour step and
// scale / bias.  Two launches:
//   dec_resize_h       thread = (region row y, output column i), three channels: q per tap from
//                      the synthesis output, t[c][y][i] (float32, [3][h][ow]) to the workspace;
//   dec_fmt<Resize, T> thread = (output row, 4 destination pixels), as the formatted output stage:
//                      the vertical pass over t (loads coalesced along the row), then scale / bias,
//                      element conversion and the stores of fmt_store.  mirror reads column
//                      ow - 1 - x'.

// The weights are recomputed per thread from integers: RsTaps holds the run j0 .. j1 of output
// index i and what u(i, j) = 2D - |(2j + 1) O - (2i + 1) I| needs; everything fits int32 for
// I, O <= 16384 (the plan's bound).
struct RsTaps {
    int j0, j1, c, O, D2;
    float fU;
    __device__ __forceinline__ int u(int j) const { return D2 - abs((2 * j + 1) * O - c); }
    __device__ __forceinline__ float w(int j) const { return __fdiv_rn((float)u(j), fU); }
};

__device__ __forceinline__ RsTaps rs_taps(int i, int I, int O)
{
    RsTaps t;
    t.O = O;
    t.D2 = 2 * max(I, O);
    t.c = (2 * i + 1) * I;
    // u > 0: (c - 2D - O) / 2O < j < (c + 2D - O) / 2O, clipped to the region
    const int a = t.c - t.D2 - O, b = t.c + t.D2 - O; // b >= 1
    t.j0 = a >= 0 ? a / (2 * O) + 1 : 0;
    t.j1 = min((b - 1) / (2 * O), I - 1);
    int U = 0;
    for (int j = t.j0; j <= t.j1; ++j) U += t.u(j);
    t.fU = (float)U;
    return t;
}

// CCMI_FILTER_CUBIC (step 3a of its contract in ccmi.h): the Keys cubic, a = -0.5, in the same
// integers.  n = |(2j + 1) O - c| < 2 D2 <= 2^16 over the run, so u takes int64: Horner, every
// intermediate below 2^51; U below 2^61.  A tap at the end of the run may have u = 0.
struct CubTaps {
    int j0, j1, c, O, D2;
    float fU;
    __device__ __forceinline__ int64_t u(int j) const
    {
        const int64_t n = abs((2 * j + 1) * O - c), d = D2;
        return n < d ? ((3 * n - 5 * d) * n) * n + 2 * d * d * d : (((5 * d - n) * n - 8 * d * d) * n) + 4 * d * d * d;
    }
    __device__ __forceinline__ float w(int j) const { return __fdiv_rn((float)u(j), fU); }
};

__device__ __forceinline__ CubTaps cub_taps(int i, int I, int O)
{
    CubTaps t;
    t.O = O;
    t.D2 = 2 * max(I, O);
    t.c = (2 * i + 1) * I;
    // n < 2 D2: (c - 2 D2 - O) / 2O < j < (c + 2 D2 - O) / 2O, clipped to the region
    const int a = t.c - 2 * t.D2 - O, b = t.c + 2 * t.D2 - O; // b >= 1
    t.j0 = a >= 0 ? a / (2 * O) + 1 : 0;
    t.j1 = min((b - 1) / (2 * O), I - 1);
    int64_t U = 0;
    for (int j = t.j0; j <= t.j1; ++j) U += t.u(j);
    t.fU = (float)U;
    return t;
}

// the taps of output index i of an axis resampled from I to O: the triangle's, or the cubic's
template <bool CUBIC> __device__ __forceinline__ auto axis_taps(int i, int I, int O)
{
    if constexpr (CUBIC) return cub_taps(i, I, O);
    else return rs_taps(i, I, O);
}

// one frame of a resampling group: DecOut as Plain's entry (H x W = the region, compact)
struct DecOutRs {
    DecOut o;
    float *tmp;
};

// h x w = the region at (oy, ox) of the synthesis output, as for output_fmt_body
template <bool CUBIC = false>
__device__ __forceinline__ void resample_h_body(const int32_t *__restrict__ syn, int64_t splane, int spitch, int oy, int ox,
                                                int h, int w, int ow, int maxv, int kind, int flags,
                                                float *__restrict__ tmp)
{
    const int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int y = (int)(g / ow);
    if (y >= h) return;
    const int i = (int)(g - (int64_t)y * ow);
    const auto T = axis_taps<CUBIC>(i, w, ow);
    const float fmax = (float)maxv;
    const bool matrix = flags & kFmtMatrix;
    const int32_t *__restrict__ lrow = syn + (int64_t)(oy + y) * spitch + ox;
    const int32_t *__restrict__ crow = syn + (int64_t)(oy + (kind == 1 ? y : y & ~1)) * spitch + ox;
    float acc[3] = {0.f, 0.f, 0.f};
    for (int j = T.j0; j <= T.j1; ++j) {
        const float wj = T.w(j);
        float q[3];
        fmt_pixel(lrow, crow, splane, j, kind == 1 ? j : j & ~1, maxv, fmax, matrix, q);
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] = fmt_add(acc[c], fmt_mul(wj, q[c]));
    }
    const int64_t tplane = (int64_t)h * ow;
#pragma unroll
    for (int c = 0; c < 3; ++c) tmp[c * tplane + g] = acc[c];
}

// tmp = [3][h][ow] of resample_h_body; the frame at dst is oh x ow
template <typename T, int COL = kColNone, bool CUBIC = false>
__device__ __forceinline__ uint32_t resample_v_body(const float *__restrict__ tmp, int h, int oh, int ow, int flags,
                                                    T *__restrict__ dst, const DecFmtCall &C, const DecCol *K = nullptr)
{
    int y, d0;
    int64_t row;
    bool nchw, nhwc;
    if (!fmt_group<T>(dst, C, oh, ow, y, d0, row, nchw, nhwc)) return 0;
    const auto R = axis_taps<CUBIC>(y, h, oh);
    const bool mirror = flags & kFmtMirror;
    // element indices of tmp fit 32 bits (3 h ow <= 3 * 2^28): one base and 32-bit offsets
    const unsigned tplane = (unsigned)h * (unsigned)ow;
    unsigned x[4];
    float acc[3][4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int d = min(max(d0 + k, 0), ow - 1); // the surplus slots of a partial group are never stored
        x[k] = (unsigned)(mirror ? ow - 1 - d : d);
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c][k] = 0.f;
    }
    for (int j = R.j0; j <= R.j1; ++j) {
        const float wj = R.w(j);
        const unsigned r0 = (unsigned)j * (unsigned)ow;
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[c][k] = fmt_add(acc[c][k], fmt_mul(wj, tmp[c * tplane + r0 + x[k]]));
    }
    if constexpr (CUBIC) {
        if (flags & kFmtClamp) {
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[c][k] = col_clamp(acc[c][k]);
        }
    }
    if constexpr (COL != kColNone) {
        const float mean = COL == kColWrite ? col_mean(*K, oh * ow) : 0.f;
        uint32_t sum = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float q[3] = {acc[0][k], acc[1][k], acc[2][k]};
            if constexpr (COL == kColStat) {
                if (d0 + k >= 0 && d0 + k < ow) sum += col_term(*K, q); // a surplus slot repeats a pixel
            } else {
                col_ops(*K, 0, K->n, mean, q);
#pragma unroll
                for (int c = 0; c < 3; ++c) acc[c][k] = q[c];
            }
        }
        if constexpr (COL == kColStat) return sum;
    }
    T v[3][4];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int k = 0; k < 4; ++k) v[c][k] = fmt_elem<T>(fmt_add(fmt_mul(acc[c][k], C.scale[c]), C.bias[c]));
    fmt_store<T>(v, dst, C, row, d0, ow, nchw, nhwc);
    return 0;
}

unsigned resample_h_blocks(int h, int ow) { return (unsigned)(((int64_t)h * ow + kThreads - 1) / kThreads); }

// ------------------------------------------------------------------ warped formatted output
// The formatted sink with a ccmi_warp (steps 3a-3d of its contract in ccmi.h): every pixel of the
// oh x ow frame at dst is a bilinear sample of q over the WHOLE frame, fh x fw, at the position
// the frame's 2 x 3 matrix gives, between the colour step and scale / bias.  One launch, a thread
// = (output row, 4 destination pixels) as in the formatted output stage; the pixels go one at a
// time, so 12 tap values are live and not 48.  Each pixel gathers 4 taps x 3 channels through
// fmt_pixel (the colour step per tap).
// The synthesis output holds the window the plan derived from the matrix, h x w at (oy, ox) of
// the frame, compact (the per-frame tail: the whole frame at 0, 0).  A tap is tested and clamped
// against the FRAME, as the contract has it, then addressed relative to the window and clamped to
// it as well: the window holds every in-frame tap, so that clamp changes nothing unless the plan
// is wrong, and then it shows as a wrong value and never as a read outside the workspace.
struct DecWarpCall { // one value per launch
    int oh, ow, pad;
    float fill[3];
};

// one frame of a warping group: DecOut as Plain's entry (H x W = the window, compact)
struct DecOutWarp {
    DecOut o;
    float m[6];
    int oy, ox, fh, fw; // the window's origin in the frame, and the frame
};

template <typename T, int COL = kColNone, bool PERSP = false>
__device__ __forceinline__ uint32_t warp_body(const int32_t *__restrict__ syn, int h, int w, int oy, int ox, int fh, int fw,
                                              const float (&m)[PERSP ? 9 : 6], int maxv, int kind, int flags, T *__restrict__ dst,
                                              const DecFmtCall &C, const DecWarpCall &Wc, const DecCol *K = nullptr)
{
    int y, d0;
    int64_t row;
    bool nchw, nhwc;
    if (!fmt_group<T>(dst, C, Wc.oh, Wc.ow, y, d0, row, nchw, nhwc)) return 0;
    float mean = 0.f;
    uint32_t sum = 0;
    if constexpr (COL == kColWrite) mean = col_mean(*K, Wc.oh * Wc.ow);
    const float fmax = (float)maxv;
    const bool mirror = flags & kFmtMirror, matrix = flags & kFmtMatrix;
    const int64_t splane = (int64_t)h * w;
    const float cy = (float)y + 0.5f;
    const float xr = fmt_mul(m[1], cy), yr = fmt_mul(m[4], cy); // the row's share of the position
    float wr = 0.f; // PERSP: and of the denominator
    if constexpr (PERSP) wr = fmt_mul(m[7], cy);
    T v[3][4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int d = d0 + k;
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c][k] = fmt_elem<T>(0.f);
        if (d < 0 || d >= Wc.ow) continue;
        const float cx = (float)(mirror ? Wc.ow - 1 - d : d) + 0.5f;
        float xs = fmt_add(fmt_add(fmt_mul(m[0], cx), xr), m[2]);
        float ys = fmt_add(fmt_add(fmt_mul(m[3], cx), yr), m[5]);
        if constexpr (PERSP) { // step 3a': the plan has wn > 0 and |xs|, |ys| <= 2^22 after the division
            const float wn = fmt_add(fmt_add(fmt_mul(m[6], cx), wr), m[8]);
            xs = __fdiv_rn(xs, wn), ys = __fdiv_rn(ys, wn);
        }
        const float u = xs - 0.5f, vv = ys - 0.5f;
        const float uf = floorf(u), vf = floorf(vv); // |u|, |v| <= 2^22 + 1: exact in an int
        const float fx = u - uf, fy = vv - vf;
        const int x0 = (int)uf, y0 = (int)vf;
        const float gx = 1.f - fx, gy = 1.f - fy;
        float line[2][3]; // top, bot
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const int yy = y0 + a;
            const bool yin = yy >= 0 && yy < fh;
            const int ry = min(max(min(max(yy, 0), fh - 1) - oy, 0), h - 1);
            const int32_t *__restrict__ lrow = syn + (int64_t)ry * w;
            const int32_t *__restrict__ crow = syn + (int64_t)(kind == 1 ? ry : ry & ~1) * w;
            float t[2][3];
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const int xx = x0 + b;
                const bool in = yin && xx >= 0 && xx < fw;
                const int rx = min(max(min(max(xx, 0), fw - 1) - ox, 0), w - 1);
                fmt_pixel(lrow, crow, splane, rx, kind == 1 ? rx : rx & ~1, maxv, fmax, matrix, t[b]);
                if (!in && Wc.pad == CCMI_PAD_FILL) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) t[b][c] = Wc.fill[c];
                }
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) line[a][c] = fmt_add(fmt_mul(t[0][c], gx), fmt_mul(t[1][c], fx));
        }
        if constexpr (COL == kColNone) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float r = fmt_add(fmt_mul(line[0][c], gy), fmt_mul(line[1][c], fy));
                v[c][k] = fmt_elem<T>(fmt_add(fmt_mul(r, C.scale[c]), C.bias[c]));
            }
        } else {
            float r[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) r[c] = fmt_add(fmt_mul(line[0][c], gy), fmt_mul(line[1][c], fy));
            if constexpr (COL == kColStat) {
                sum += col_term(*K, r);
            } else {
                col_ops(*K, 0, K->n, mean, r);
#pragma unroll
                for (int c = 0; c < 3; ++c) v[c][k] = fmt_elem<T>(fmt_add(fmt_mul(r[c], C.scale[c]), C.bias[c]));
            }
        }
    }
    if constexpr (COL != kColStat) fmt_store<T>(v, dst, C, row, d0, Wc.ow, nchw, nhwc);
    return sum;
}

// ---- the cubic warp (CCMI_WARP_CUBIC: steps 3c-3d of its contract in ccmi.h)
// The same thread layout, positions and tap rule as warp_body, 16 taps per pixel: cubic convolution
// with A = -0.75 in the contract's operation order.  The four tap rows go one at a time (the loop
// over a is kept rolled, its coefficient picked by selects): 8 coefficients, 3 row sums and 3
// accumulators are live next to one tap, and the code holds 4 x 4 copies of fmt_pixel, as warp_body's.
__device__ __forceinline__ float fmt_sub(float a, float b)
{
#pragma clang fp contract(off)
    return a - b;
}
__device__ __forceinline__ float cub_in(float t) // |t| <= 1
{
    return fmt_add(fmt_mul(fmt_mul(fmt_sub(fmt_mul(1.25f, t), 2.25f), t), t), 1.f);
}
__device__ __forceinline__ float cub_out(float s) // 1 <= |s| <= 2
{
    return fmt_sub(fmt_mul(fmt_add(fmt_mul(fmt_sub(fmt_mul(-0.75f, s), -3.75f), s), -6.f), s), -3.f);
}

template <typename T, int COL = kColNone, bool PERSP = false>
__device__ __forceinline__ uint32_t wcubic_body(const int32_t *__restrict__ syn, int h, int w, int oy, int ox, int fh, int fw,
                                                const float (&m)[PERSP ? 9 : 6], int maxv, int kind, int flags, T *__restrict__ dst,
                                                const DecFmtCall &C, const DecWarpCall &Wc, const DecCol *K = nullptr)
{
    int y, d0;
    int64_t row;
    bool nchw, nhwc;
    if (!fmt_group<T>(dst, C, Wc.oh, Wc.ow, y, d0, row, nchw, nhwc)) return 0;
    float mean = 0.f;
    uint32_t sum = 0;
    if constexpr (COL == kColWrite) mean = col_mean(*K, Wc.oh * Wc.ow);
    const float fmax = (float)maxv;
    const bool mirror = flags & kFmtMirror, matrix = flags & kFmtMatrix, clamp = flags & kFmtClamp;
    const int64_t splane = (int64_t)h * w;
    const float cy = (float)y + 0.5f;
    const float xr = fmt_mul(m[1], cy), yr = fmt_mul(m[4], cy); // the row's share of the position
    float wr = 0.f; // PERSP: and of the denominator
    if constexpr (PERSP) wr = fmt_mul(m[7], cy);
    T v[3][4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int d = d0 + k;
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c][k] = fmt_elem<T>(0.f);
        if (d < 0 || d >= Wc.ow) continue;
        const float cx = (float)(mirror ? Wc.ow - 1 - d : d) + 0.5f;
        float xs = fmt_add(fmt_add(fmt_mul(m[0], cx), xr), m[2]);
        float ys = fmt_add(fmt_add(fmt_mul(m[3], cx), yr), m[5]);
        if constexpr (PERSP) { // step 3a': the plan has wn > 0 and |xs|, |ys| <= 2^22 after the division
            const float wn = fmt_add(fmt_add(fmt_mul(m[6], cx), wr), m[8]);
            xs = __fdiv_rn(xs, wn), ys = __fdiv_rn(ys, wn);
        }
        const float u = xs - 0.5f, vv = ys - 0.5f;
        const float uf = floorf(u), vf = floorf(vv); // |u|, |v| <= 2^22 + 1: exact in an int
        const float fx = u - uf, fy = vv - vf;
        const int x0 = (int)uf, y0 = (int)vf;
        const float gx = 1.f - fx, gy = 1.f - fy;
        const float wx[4] = {cub_out(fmt_add(fx, 1.f)), cub_in(fx), cub_in(gx), cub_out(fmt_add(gx, 1.f))};
        const float wy0 = cub_out(fmt_add(fy, 1.f)), wy1 = cub_in(fy), wy2 = cub_in(gy), wy3 = cub_out(fmt_add(gy, 1.f));
        float r[3] = {0.f, 0.f, 0.f};
#pragma unroll 1
        for (int a = 0; a < 4; ++a) {
            const int yy = y0 - 1 + a;
            const bool yin = yy >= 0 && yy < fh;
            const int ry = min(max(min(max(yy, 0), fh - 1) - oy, 0), h - 1);
            const int32_t *__restrict__ lrow = syn + (int64_t)ry * w;
            const int32_t *__restrict__ crow = syn + (int64_t)(kind == 1 ? ry : ry & ~1) * w;
            float line[3] = {0.f, 0.f, 0.f};
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int xx = x0 - 1 + b;
                const bool in = yin && xx >= 0 && xx < fw;
                const int rx = min(max(min(max(xx, 0), fw - 1) - ox, 0), w - 1);
                float t[3];
                fmt_pixel(lrow, crow, splane, rx, kind == 1 ? rx : rx & ~1, maxv, fmax, matrix, t);
                if (!in && Wc.pad == CCMI_PAD_FILL) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) t[c] = Wc.fill[c];
                }
#pragma unroll
                for (int c = 0; c < 3; ++c) line[c] = fmt_add(line[c], fmt_mul(t[c], wx[b]));
            }
            const float wya = a == 0 ? wy0 : a == 1 ? wy1 : a == 2 ? wy2 : wy3;
#pragma unroll
            for (int c = 0; c < 3; ++c) r[c] = fmt_add(r[c], fmt_mul(line[c], wya));
        }
        if (clamp) {
#pragma unroll
            for (int c = 0; c < 3; ++c) r[c] = col_clamp(r[c]);
        }
        if constexpr (COL == kColStat) {
            sum += col_term(*K, r);
        } else {
            if constexpr (COL == kColWrite) col_ops(*K, 0, K->n, mean, r);
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c][k] = fmt_elem<T>(fmt_add(fmt_mul(r[c], C.scale[c]), C.bias[c]));
        }
    }
    if constexpr (COL != kColStat) fmt_store<T>(v, dst, C, row, d0, Wc.ow, nchw, nhwc);
    return sum;
}

// ---- the projective warp (CCMI_WARP_PROJECTIVE: step 3a' of its contract in ccmi.h)
// The same two bodies with PERSP: the position is the quotient of the two numerators by the third
// row's denominator, two IEEE divisions per pixel; taps, padding, colour and statistics are the
// affine kernels'.  The frame's record carries nine floats and is a form of its own (kOutPersp), so
// the affine kernels keep their argument layout.
struct DecOutPersp {
    DecOut o;
    float m[9];
    int oy, ox, fh, fw; // as DecOutWarp's
};

DecWarpCall warp_call(const DecFmt &f)
{
    DecWarpCall Wc;
    Wc.oh = f.out_h, Wc.ow = f.out_w, Wc.pad = f.pad;
    for (int c = 0; c < 3; ++c) Wc.fill[c] = f.fill[c];
    return Wc;
}

// ------------------------------------------------------------------ the geometries and their kernels
// The formatted sink has seven geometries: Plain, Resize<CUBIC> and Warp<CUBIC, PERSP>.  Each is a
// description that the kernel templates and launch_geometry below are written over:
//   Frame, Out  what the per-frame tail passes by value: the statistics pass takes the Frame, the
//               typed forms the Out, which is the Frame with the destination; value() makes it
//   Entry       the frame's record in a tail group's output section; entry() makes it
//   Table       what a group's launch passes, the section and, for a resize, the output size;
//               table() makes it, at() is its entry blockIdx.y as an Out
//   call()      the values per launch that follow the format in the argument list: none, or DecWarpCall
//   body()      the geometry's body of above, from a Frame
//   kWaves, kStatWaves  the waves per SIMD the typed forms and the statistics pass ask of the compiler, or
//               0.  The int64 weights take the cubic resize kernels a few registers past 64; asked for 8
//               waves the compiler keeps them at 60 or below without a spill, and so it does the cubic
//               warp's statistics pass.  The typed cubic warp kernels spill at 64 and are left to the
//               allocator (72 - 91, 5 - 7 waves), as is the projective cubic statistics pass, whose
//               division's temporaries spill two registers under that request
//               (tests/test_decode_cubic_resources.py, tests/test_decode_persp_resources.py).
// The argument lists are laid out as the hand-written kernels' were that these replace.
template <typename F> struct WithDst : F {
    void *dst;
};

struct Plain {
    struct Frame { // h x w = the region at (oy, ox) of the H x W synthesis output
        const int32_t *syn;
        int H, W, oy, ox, h, w, maxv, kind, flags;
    };
    using Out = WithDst<Frame>;
    using Entry = DecOut; // the frame's compact H x W synthesis output (bps_or_flags = its kFmt* flags)
    using Table = const DecOut *__restrict__;
    static constexpr int kWaves = 0, kStatWaves = 0;
    static constexpr bool kHPass = false;

    static std::tuple<> call(const DecFmt &) { return {}; }
    static Out value(const DecOut &o, const DecTailFrame &f)
    {
        const DecWindow &r = f.roi.rect;
        return {{o.syn, o.H, o.W, r.y0, r.x0, r.h(), r.w(), o.maxv, o.kind, o.bps_or_flags}, o.dst};
    }
    static Entry entry(const DecOut &o, const DecTailFrame &, int, int) { return o; }
    static Table table(const void *sec, const DecFmt &) { return static_cast<const DecOut *>(sec); }
    static __device__ __forceinline__ Out at(Table Os)
    {
        const DecOut O = Os[blockIdx.y];
        return {{O.syn, O.H, O.W, 0, 0, O.H, O.W, O.maxv, O.kind, O.bps_or_flags}, O.dst};
    }
    template <typename T, int COL>
    static __device__ __forceinline__ uint32_t body(const Frame &F, T *dst, const DecFmtCall &C, const DecCol *K)
    {
        return output_fmt_body<T, COL>(F.syn, (int64_t)F.H * F.W, F.W, F.oy, F.ox, F.h, F.w, F.maxv, F.kind, F.flags, dst, C, K);
    }
};

// the horizontal pass of a resize runs first, into the frame's tmp: a kernel of its own (dec_resize_h)
struct RsHFrame { // as Plain::Frame, with the output width and tmp
    const int32_t *syn;
    int H, W, oy, ox, h, w, ow, maxv, kind, flags;
    float *tmp;
};

template <bool CUBIC> struct Resize {
    struct Frame { // tmp = [3][h][ow] of the horizontal pass
        const float *tmp;
        int h, oh, ow, flags;
    };
    using Out = WithDst<Frame>;
    using Entry = DecOutRs;
    struct Table {
        const DecOutRs *__restrict__ Os;
        int oh, ow;
    };
    static constexpr int kWaves = CUBIC ? 8 : 0, kStatWaves = kWaves;
    static constexpr bool kHPass = true, kCubic = CUBIC;

    static std::tuple<> call(const DecFmt &) { return {}; }
    static Out value(const DecOut &o, const DecTailFrame &f)
    {
        return {{f.rs_tmp, f.roi.rect.h(), f.fmt.out_h, f.fmt.out_w, o.bps_or_flags}, o.dst};
    }
    static Entry entry(const DecOut &o, const DecTailFrame &f, int, int) { return {o, f.rs_tmp}; }
    static Table table(const void *sec, const DecFmt &fmt) { return {static_cast<const DecOutRs *>(sec), fmt.out_h, fmt.out_w}; }
    static __device__ __forceinline__ Out at(const Table &S)
    {
        const DecOutRs R = S.Os[blockIdx.y];
        return {{R.tmp, R.o.H, S.oh, S.ow, R.o.bps_or_flags}, R.o.dst};
    }
    template <typename T, int COL>
    static __device__ __forceinline__ uint32_t body(const Frame &F, T *dst, const DecFmtCall &C, const DecCol *K)
    {
        return resample_v_body<T, COL, CUBIC>(F.tmp, F.h, F.oh, F.ow, F.flags, dst, C, K);
    }
};

template <bool CUBIC, bool PERSP> struct Warp {
    using Frame = std::conditional_t<PERSP, DecOutPersp, DecOutWarp>; // o.dst is the destination
    using Out = Frame;
    using Entry = Frame;
    using Table = const Frame *__restrict__;
    static constexpr int kWaves = 0, kStatWaves = CUBIC && !PERSP ? 8 : 0;
    static constexpr bool kHPass = false;

    static std::tuple<DecWarpCall> call(const DecFmt &fmt) { return {warp_call(fmt)}; }
    // the window h x w at (oy, ox) of the fh x fw frame
    static Frame make(const DecOut &o, const DecFmt &fmt, int oy, int ox, int fh, int fw)
    {
        Frame A{o, {}, oy, ox, fh, fw};
        for (int k = 0; k < (PERSP ? 9 : 6); ++k) A.m[k] = fmt.m[k];
        return A;
    }
    static Out value(const DecOut &o, const DecTailFrame &f) { return make(o, f.fmt, 0, 0, o.H, o.W); } // the whole frame
    static Entry entry(const DecOut &o, const DecTailFrame &f, int oy, int ox) { return make(o, f.fmt, oy, ox, f.syn.h, f.syn.w); }
    static Table table(const void *sec, const DecFmt &) { return static_cast<const Frame *>(sec); }
    static __device__ __forceinline__ Out at(Table Os) { return Os[blockIdx.y]; }
    template <typename T, int COL>
    static __device__ __forceinline__ uint32_t body(const Frame &A, T *dst, const DecFmtCall &C, const DecWarpCall &Wc,
                                                    const DecCol *K)
    {
        if constexpr (CUBIC)
            return wcubic_body<T, COL, PERSP>(A.o.syn, A.o.H, A.o.W, A.oy, A.ox, A.fh, A.fw, A.m, A.o.maxv, A.o.kind,
                                              A.o.bps_or_flags, dst, C, Wc, K);
        else
            return warp_body<T, COL, PERSP>(A.o.syn, A.o.H, A.o.W, A.oy, A.ox, A.fh, A.fw, A.m, A.o.maxv, A.o.kind,
                                            A.o.bps_or_flags, dst, C, Wc, K);
    }
};

__device__ __forceinline__ void *out_dst(const DecOutWarp &A) { return A.o.dst; }
__device__ __forceinline__ void *out_dst(const DecOutPersp &A) { return A.o.dst; }
template <typename F> __device__ __forceinline__ void *out_dst(const WithDst<F> &A) { return A.dst; }

// Where a kernel's frame and its op table come from is the template argument TABLE: its own arguments
// (the per-frame tail) or, TABLE, entry blockIdx.y of the group's tables.
template <typename G, bool TABLE> using OutArg = std::conditional_t<TABLE, typename G::Table, typename G::Out>;
template <typename G, bool TABLE> using StatArg = std::conditional_t<TABLE, typename G::Table, typename G::Frame>;
template <bool TABLE> using ColArg = std::conditional_t<TABLE, const DecCol *__restrict__, DecCol>;

template <typename G, bool TABLE, typename S> __device__ __forceinline__ decltype(auto) frame_of(const S &s)
{
    if constexpr (TABLE) return G::at(s);
    else return (s); // the argument itself
}
template <bool TABLE> __device__ __forceinline__ const DecCol *col_of(const ColArg<TABLE> &K)
{
    if constexpr (TABLE) return K + blockIdx.y;
    else return &K;
}

#define WAVES_PER_EU(N) __attribute__((amdgpu_waves_per_eu(N))) // 0: no request

// the typed forms: without colour ops, and with the frame's ops K.  Call = the types G::call() holds
template <typename G, typename T, bool TABLE, typename... Call>
__global__ __launch_bounds__(kThreads) WAVES_PER_EU(G::kWaves) void dec_fmt(OutArg<G, TABLE> S, DecFmtCall C, Call... L)
{
    const auto &F = frame_of<G, TABLE>(S);
    G::template body<T, kColNone>(F, static_cast<T *>(out_dst(F)), C, L..., nullptr);
}

template <typename G, typename T, bool TABLE, typename... Call>
__global__ __launch_bounds__(kThreads) WAVES_PER_EU(G::kWaves) void dec_fmt_col(OutArg<G, TABLE> S, DecFmtCall C, Call... L,
                                                                                ColArg<TABLE> K)
{
    const auto &F = frame_of<G, TABLE>(S);
    G::template body<T, kColWrite>(F, static_cast<T *>(out_dst(F)), C, L..., col_of<TABLE>(K));
}

// the statistics pass of a frame with a contrast op; of a group only those frames take part
template <typename G, bool TABLE, typename... Call>
__global__ __launch_bounds__(kThreads) WAVES_PER_EU(G::kStatWaves) void dec_fmt_stat(StatArg<G, TABLE> S, Call... L,
                                                                                     ColArg<TABLE> K)
{
    const DecCol &Kf = *col_of<TABLE>(K);
    if constexpr (TABLE)
        if (Kf.contrast < 0) return;
    const auto &F = frame_of<G, TABLE>(S);
    col_accumulate(Kf, G::template body<float, kColStat>(F, (float *)nullptr, col_stat_call(), L..., &Kf));
}

// the horizontal pass of a resize, per frame and of a tail group, whose grid covers the group's largest region
template <bool CUBIC>
__global__ __launch_bounds__(kThreads) WAVES_PER_EU(Resize<CUBIC>::kWaves) void dec_resize_h(RsHFrame S)
{
    resample_h_body<CUBIC>(S.syn, (int64_t)S.H * S.W, S.W, S.oy, S.ox, S.h, S.w, S.ow, S.maxv, S.kind, S.flags, S.tmp);
}

template <bool CUBIC>
__global__ __launch_bounds__(kThreads) WAVES_PER_EU(Resize<CUBIC>::kWaves) void dec_resize_h_batch(
    const DecOutRs *__restrict__ Os, int ow)
{
    const DecOutRs R = Os[blockIdx.y];
    const DecOut &O = R.o;
    resample_h_body<CUBIC>(O.syn, (int64_t)O.H * O.W, O.W, 0, 0, O.H, O.W, ow, O.maxv, O.kind, O.bps_or_flags, R.tmp);
}
#undef WAVES_PER_EU

} // namespace

// one launch of blocks of kThreads
template <typename Kernel, typename... A>
static void launch(Kernel kernel, dim3 grid, hipStream_t s, const A &...a)
{
    hipLaunchKernelGGL(kernel, grid, dim3(kThreads), 0, s, a...);
}

// launch(T{}) for the sample type T of a tensor-output kernel
template <typename Launch>
static int with_sample_type(int sample, Launch &&launch)
{
    switch (sample) {
    case CCMI_SAMPLE_U8: launch(uint8_t{}); break;
    case CCMI_SAMPLE_U16: launch(uint16_t{}); break;
    case CCMI_SAMPLE_F32: launch(float{}); break;
    default: return ccmi_set_error(CCMI_ERR_ARG, "dec: sample type %d", sample);
    }
    CCMI_HIP_CHECK(hipGetLastError());
    return CCMI_OK;
}

// dst as the kernel's element type: as(t, dst) inside a with_*_type launch
template <typename T> static T *as(T, void *p) { return static_cast<T *>(p); }

// f(G{}) for the geometry G of a formatted call
template <typename F> static int with_geometry(const DecFmt &fmt, F &&f)
{
    if (fmt.warp && fmt.persp) return fmt.cubic ? f(Warp<true, true>{}) : f(Warp<false, true>{});
    if (fmt.warp) return fmt.cubic ? f(Warp<true, false>{}) : f(Warp<false, false>{});
    if (fmt.rs) return fmt.cubic ? f(Resize<true>{}) : f(Resize<false>{});
    return f(Plain{});
}

// The colour protocol of the formatted sinks, for every geometry G and both launchers: src is the
// frame by value and K its op table (the per-frame tail) or, TABLE, the group's two tables.  A call
// without colour ops runs the plain form on the output grid; a call with them the statistics pass, if
// a frame has a contrast op (stat), and then the colour form.  K is read only where fmt.col is set.
template <typename G, bool TABLE>
static int launch_fmt_forms(const DecFmt &fmt, bool stat, dim3 grid, hipStream_t s, const OutArg<G, TABLE> &src, const DecCol *K)
{
    const DecFmtCall C = fmt_call(fmt);
    return std::apply(
        [&](auto... call) {
            auto col = [K]() -> ColArg<TABLE> {
                if constexpr (TABLE) return K;
                else return *K;
            };
            if (!fmt.col)
                return with_elem_type(fmt.elem, [&](auto t) {
                    launch(dec_fmt<G, decltype(t), TABLE, decltype(call)...>, grid, s, src, C, call...);
                });
            if (stat) {
                launch(dec_fmt_stat<G, TABLE, decltype(call)...>, grid, s, StatArg<G, TABLE>(src), call..., col());
                CCMI_HIP_CHECK(hipGetLastError());
            }
            return with_elem_type(fmt.elem, [&](auto t) {
                launch(dec_fmt_col<G, decltype(t), TABLE, decltype(call)...>, grid, s, src, C, call..., col());
            });
        },
        G::call(fmt));
}

// the output grid of a formatted sink, n frames: a resample's and a warp's cover the output size,
// the plain one's the h x w region
static dim3 fmt_grid(const DecFmt &fmt, int h, int w, int n)
{
    const bool sized = fmt.rs || fmt.warp;
    return dim3(output_fmt_blocks(sized ? fmt.out_h : h, sized ? fmt.out_w : w), n);
}

// what the cropping launchers ask of a region of an h x w frame: a known kind, inside the frame, not
// empty and, where the kernel reads 420 chroma at the even row and column, an even origin
static int check_region(const DecWindow &rect, int h, int w, int kind, bool even_origin)
{
    if (kind != 0 && kind != 1) return ccmi_set_error(CCMI_ERR_ARG, "dec: tensor output kind %d", kind);
    if (rect.y0 < 0 || rect.x0 < 0 || rect.y1 > h || rect.x1 > w || rect.h() < 1 || rect.w() < 1)
        return ccmi_set_error(CCMI_ERR_ARG, "dec: region outside the frame");
    if (even_origin && kind == 0 && ((rect.y0 | rect.x0) & 1))
        return ccmi_set_error(CCMI_ERR_ARG, "dec: a 420 region needs an even origin");
    return CCMI_OK;
}

// a per-frame tail's colour form needs the frame's op table (and a contrast op its accumulator)
static int col_frame(const DecFmt &fmt, const DecCol *col)
{
    if (fmt.col && (!col || (col->contrast >= 0 && !col->acc)))
        return ccmi_set_error(CCMI_ERR_ARG, "dec: colour without its op table");
    return CCMI_OK;
}

size_t dec_resample_tmp_elems(int region_h, int out_w) { return 3 * (size_t)region_h * out_w; }

static unsigned output_blocks(int h, int w) { return (unsigned)(((int64_t)h * w + kThreads - 1) / kThreads); }

int launch_dec_out_frame(const DecTailFrame &f, const int32_t *syn, int h, int w, bool crop, bool device, hipStream_t s)
{
    const DecFmt &fmt = f.fmt;
    const DecWindow &rect = f.roi.rect;
    const int kind = f.kind, maxv = (1 << f.bitdepth) - 1;
    void *dst = f.dst;
    if (!fmt.on) {
        if (crop) {
            if (int rc = check_region(rect, h, w, kind, false)) return rc;
            const dim3 grid(output_tensor_blocks(rect.h(), rect.w(), kind));
            return with_sample_type(f.sample, [&](auto t) {
                launch(dec_output_tensor_crop<decltype(t)>, grid, s, syn, h, w, rect.y0, rect.x0, rect.h(), rect.w(), maxv,
                       kind, as(t, dst));
            });
        }
        if (device) {
            if (kind != 0 && kind != 1) return ccmi_set_error(CCMI_ERR_ARG, "dec: tensor output kind %d", kind);
            const dim3 grid(output_tensor_blocks(h, w, kind));
            return with_sample_type(f.sample, [&](auto t) {
                launch(dec_output_tensor<decltype(t)>, grid, s, syn, h, w, maxv, kind, as(t, dst));
            });
        }
        launch(dec_output_kernel, dim3(output_blocks(h, w)), s, syn, h, w, maxv, kind, f.bitdepth <= 8 ? 1 : 2, f.dst);
        CCMI_HIP_CHECK(hipGetLastError());
        return CCMI_OK;
    }
    // the formatted sinks: a warp samples the whole frame, the others read roi.rect (the region, or the whole frame)
    if (int rc = check_region(fmt.warp ? DecWindow{0, h, 0, w} : rect, h, w, kind, true)) return rc;
    if (fmt.warp) {
        if (fmt.out_h < 1 || fmt.out_w < 1) return ccmi_set_error(CCMI_ERR_ARG, "dec: warp without a size");
        if (kind == 0 && ((h | w) & 1)) return ccmi_set_error(CCMI_ERR_ARG, "dec: a 420 warp needs an even frame size");
    } else if (fmt.rs && (fmt.out_h < 1 || fmt.out_w < 1 || !f.rs_tmp)) {
        return ccmi_set_error(CCMI_ERR_ARG, "dec: resample without a size");
    }
    if (int rc = col_frame(fmt, f.col)) return rc;
    const bool stat = fmt.col && f.col->contrast >= 0; // the colour forms take the frame's op table by value
    const DecOut o{syn, h, w, maxv, kind, fmt_flags(fmt), f.dst};
    return with_geometry(fmt, [&](auto g) {
        using G = decltype(g);
        if constexpr (G::kHPass) { // into rs_tmp
            launch(dec_resize_h<G::kCubic>, dim3(resample_h_blocks(rect.h(), fmt.out_w)), s,
                   RsHFrame{syn, h, w, rect.y0, rect.x0, rect.h(), rect.w(), fmt.out_w, maxv, kind, o.bps_or_flags, f.rs_tmp});
            CCMI_HIP_CHECK(hipGetLastError());
        }
        return launch_fmt_forms<G, false>(fmt, stat, fmt_grid(fmt, rect.h(), rect.w(), 1), s, G::value(o, f), f.col);
    });
}

// ------------------------------------------------------------------ a tail group's output section
// a staged frame's share of the filter stage's tables holds its entry here, rounded to 16, and its
// 96-byte filter entry (dec_filter.hip)
static_assert(sizeof(DecOut) <= sizeof(DecOutWarp) && sizeof(DecOutRs) <= sizeof(DecOutWarp) &&
                  sizeof(DecOutWarp) <= sizeof(DecOutPersp) && sizeof(DecOutPersp) + 16 + 96 <= kFltTableBytes,
              "kFltTableBytes per staged frame");

size_t dec_out_entry_bytes(int out_form)
{
    return out_form == kOutRs     ? sizeof(DecOutRs)
           : out_form == kOutWarp  ? sizeof(DecOutWarp)
           : out_form == kOutPersp ? sizeof(DecOutPersp)
                                   : sizeof(DecOut);
}

void dec_out_fill(void *out_sec, void *col_sec, int i, const DecTailFrame &f, int h, int w, int oy, int ox)
{
    const DecOut o{f.syn.out, h, w, (1 << f.bitdepth) - 1, f.kind, f.fmt.on ? fmt_flags(f.fmt) : f.bitdepth <= 8 ? 1 : 2,
                   f.dst};
    with_geometry(f.fmt, [&](auto g) {
        using G = decltype(g);
        static_cast<typename G::Entry *>(out_sec)[i] = G::entry(o, f, oy, ox);
        return 0;
    });
    if (f.fmt.col) static_cast<DecCol *>(col_sec)[i] = *f.col;
}

int launch_dec_out_group(const DecTailFrame &f0, int h, int w, int n, const void *out_sec, const DecCol *kk, bool stat,
                         hipStream_t s)
{
    const DecFmt &fmt = f0.fmt;
    if (!fmt.on) {
        const DecOut *oo = static_cast<const DecOut *>(out_sec);
        if (f0.sample < 0) { // file bytes
            launch(dec_output_batch, dim3(output_blocks(h, w), n), s, oo);
            CCMI_HIP_CHECK(hipGetLastError());
            return CCMI_OK;
        }
        const dim3 grid(output_tensor_blocks(h, w, f0.kind), n); // one kind per group
        return with_sample_type(f0.sample, [&](auto t) { launch(dec_output_tensor_batch<decltype(t)>, grid, s, oo); });
    }
    // the format but its per-frame flags (in the table) is the call's; the section holds G::Entry
    return with_geometry(fmt, [&](auto g) {
        using G = decltype(g);
        if constexpr (G::kHPass) { // h = the group's tallest region
            launch(dec_resize_h_batch<G::kCubic>, dim3(resample_h_blocks(h, fmt.out_w), n), s,
                   static_cast<const DecOutRs *>(out_sec), fmt.out_w);
            CCMI_HIP_CHECK(hipGetLastError());
        }
        return launch_fmt_forms<G, true>(fmt, stat, fmt_grid(fmt, h, w, n), s, G::table(out_sec, fmt), kk);
    });
}

} // namespace ccmi
