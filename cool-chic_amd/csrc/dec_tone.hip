// dec_tone.hip -- path B: the tone stage of the decoder's output stage (ccmi_tone, step 3x of the
// contract in ccmi.h): a per-frame list of tone ops on the staged float32 frame [3][oh][ow], between
// the staging launches of the filter stage (dec_filter.hip) and its filter kernel, which formats
// the result.
//
// A frame's list is cut into segments by the plan (DecToneSeg): a run of pointwise ops (brightness,
// saturation, matrix, solarize, posterize) ended by a whole-frame op or by the end of the list.
// Segment p of all staged frames of a tail group shares its launches; a frame with fewer segments,
// or whose segment p needs no such pass, leaves at once (one scalar branch per block):
//
//  dec_tone_stat(_batch)   reads the frame, puts the pixel through the segment's pointwise ops in
//                   registers and accumulates the terminator's statistic in the frame's accumulator
//                   block: contrast the 64-bit sum S_j (one atomic per wave), autocontrast min / max
//                   as unsigned atomics on the float bits (the values are clamped and + 0.0f, so
//                   unsigned order is float order; the minimum is kept complemented, so that the
//                   block is cleared with zeros), one per wave and channel, equalize a 3 x 256
//                   histogram in LDS, flushed bin by bin, non-empty bins only;
//  dec_tone_apply(_batch)  redoes the pointwise ops and applies contrast / autocontrast / equalize
//                   (or nothing: the list's tail), in place.  For equalize each block rebuilds the
//                   three LUTs in LDS from the global histogram with a prefix sum;
//  dec_tone_sharp(_batch)  sharpness cannot run in place: a 32 x 32 tile with its one-pixel halo
//                   goes through LDS (pointwise ops applied to the halo too) and the result into
//                   the frame's other buffer; the plan has swapped the source of the later passes.
//
// A block of the first two owns kPixPerBlock consecutive pixels of a plane, a thread every 256th.
// Every product, sum and difference is its own float32 operation (fmt_mul / fmt_add); integer sums
// and min / max make every statistic independent of the order of the blocks.
#include <algorithm>

#include "dec_out_fmt.h"

namespace ccmi {
namespace {

constexpr int kThreads = kOutThreads;
constexpr int kPixPerThread = 8, kPixPerBlock = kThreads * kPixPerThread;
constexpr int kSharpTile = 32, kSharpIn = kSharpTile + 2; // the tile and its halo
static_assert(kThreads == 256, "one thread per bin; four rows of eight in a sharpness tile");

__device__ __forceinline__ float tone_sub(float a, float b)
{
#pragma clang fp contract(off)
    return a - b;
}
__device__ __forceinline__ float tone_clamp(float t) { return fminf(fmaxf(t, 0.f), 1.f); } // NaN -> 0
__device__ __forceinline__ float tone_grey(const float (&x)[3])
{
    return fmt_add(fmt_add(fmt_mul(0.2989f, x[0]), fmt_mul(0.587f, x[1])), fmt_mul(0.114f, x[2]));
}

// the pointwise ops [first, end) of the frame on one pixel (uniform per block: scalar branches)
__device__ __forceinline__ void tone_point(const DecTone &E, int first, int end, float (&x)[3])
{
    for (int i = first; i < end; ++i) {
        const DecToneOp &P = E.ops[i];
        if (P.op == CCMI_TONE_MATRIX) {
            float y[3];
#pragma unroll
            for (int c = 0; c < 3; ++c)
                y[c] = tone_clamp(fmt_add(
                    fmt_add(fmt_add(fmt_mul(P.v[4 * c], x[0]), fmt_mul(P.v[4 * c + 1], x[1])), fmt_mul(P.v[4 * c + 2], x[2])),
                    P.v[4 * c + 3]));
#pragma unroll
            for (int c = 0; c < 3; ++c) x[c] = y[c];
        } else if (P.op == CCMI_TONE_BRIGHTNESS) {
#pragma unroll
            for (int c = 0; c < 3; ++c) x[c] = tone_clamp(fmt_mul(P.v[0], x[c]));
        } else if (P.op == CCMI_TONE_SATURATION) {
            const float b = fmt_mul(P.v[1], tone_grey(x));
#pragma unroll
            for (int c = 0; c < 3; ++c) x[c] = tone_clamp(fmt_add(fmt_mul(P.v[0], x[c]), b));
        } else if (P.op == CCMI_TONE_SOLARIZE) {
#pragma unroll
            for (int c = 0; c < 3; ++c) x[c] = x[c] >= P.v[0] ? tone_sub(1.0f, x[c]) : x[c];
        } else { // CCMI_TONE_POSTERIZE: v = L, 1 / L, L - 1
#pragma unroll
            for (int c = 0; c < 3; ++c)
                x[c] = fmt_mul(fminf(fmaxf(floorf(fmt_mul(tone_clamp(x[c]), P.v[0])), 0.f), P.v[2]), P.v[1]);
        }
    }
}

__device__ __forceinline__ uint32_t *acc_words(const DecTone &E, const DecToneSeg &S, size_t byte_off)
{
    return reinterpret_cast<uint32_t *>(E.acc + (size_t)S.acc * kToneAccBytes + byte_off);
}

__device__ __forceinline__ int tone_quant(float x) { return (int)rintf(fmt_mul(tone_clamp(x), 255.0f)); }

__device__ __forceinline__ void stat_body(const DecTone &E, int p, int oh, int ow)
{
    __shared__ uint32_t s_hist[3 * 256];
    if (p >= E.nseg) return;
    const DecToneSeg S = E.seg[p];
    if (S.term != CCMI_TONE_CONTRAST && S.term != CCMI_TONE_AUTOCONTRAST && S.term != CCMI_TONE_EQUALIZE) return;
    const int tid = threadIdx.x;
    const unsigned plane = (unsigned)oh * (unsigned)ow; // <= 2^28
    const float *__restrict__ src = E.buf[S.src];
    const unsigned base = blockIdx.x * (unsigned)kPixPerBlock + tid;
    if (S.term == CCMI_TONE_EQUALIZE) {
        for (int i = tid; i < 3 * 256; i += kThreads) s_hist[i] = 0;
        __syncthreads();
    }
    uint32_t sum = 0, lo[3] = {~0u, ~0u, ~0u}, hi[3] = {0, 0, 0};
#pragma unroll
    for (int it = 0; it < kPixPerThread; ++it) {
        const unsigned at = base + it * kThreads;
        if (at >= plane) break;
        float x[3] = {src[at], src[plane + at], src[2 * plane + at]};
        tone_point(E, S.first, S.end, x);
        if (S.term == CCMI_TONE_CONTRAST) {
            sum += (uint32_t)rintf(fmt_mul(tone_clamp(tone_grey(x)), 65535.0f));
        } else if (S.term == CCMI_TONE_AUTOCONTRAST) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const uint32_t b = __float_as_uint(fmt_add(tone_clamp(x[c]), 0.0f));
                lo[c] = min(lo[c], b), hi[c] = max(hi[c], b);
            }
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) atomicAdd(&s_hist[256 * c + tone_quant(x[c])], 1u);
        }
    }
    // every lane of the wave arrives here
    if (S.term == CCMI_TONE_CONTRAST) { // a thread's sum <= 8 * 65535, a wave's < 2^26
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
        if ((tid & 63) == 0 && sum)
            atomicAdd(reinterpret_cast<unsigned long long *>(acc_words(E, S, kToneAccSum)), (unsigned long long)sum);
    } else if (S.term == CCMI_TONE_AUTOCONTRAST) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                lo[c] = min(lo[c], (uint32_t)__shfl_xor(lo[c], o));
                hi[c] = max(hi[c], (uint32_t)__shfl_xor(hi[c], o));
            }
        }
        if ((tid & 63) == 0 && lo[0] != ~0u) { // the wave had a pixel
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                atomicMax(acc_words(E, S, kToneAccMin) + c, ~lo[c]);
                atomicMax(acc_words(E, S, kToneAccMax) + c, hi[c]);
            }
        }
    } else {
        __syncthreads();
        uint32_t *H = acc_words(E, S, kToneAccHist);
        for (int i = tid; i < 3 * 256; i += kThreads)
            if (const uint32_t n = s_hist[i]) atomicAdd(H + i, n);
    }
}

// equalize: the three LUTs of the frame from its histogram; thread t owns bin t of every channel
__device__ __forceinline__ void build_luts(const uint32_t *__restrict__ H, uint32_t npix, uint8_t *s_lut, uint32_t *s_wave,
                                           uint32_t *s_step)
{
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    uint32_t h[3], inc[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        h[c] = H[256 * c + t];
        inc[c] = h[c];
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t up = __shfl_up(inc[c], o);
            if (lane >= o) inc[c] += up;
        }
        if (lane == 63) s_wave[4 * c + wv] = inc[c];
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        for (int k = 0; k < wv; ++k) inc[c] += s_wave[4 * c + k];
        // the highest non-empty bin: the one non-empty bin at which the running sum reaches N
        if (h[c] && inc[c] == npix) s_step[c] = (npix - h[c]) / 255u;
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const uint32_t step = s_step[c];
        s_lut[256 * c + t] = (uint8_t)(step == 0 ? (uint32_t)t : min(255u, (inc[c] - h[c] + step / 2) / step));
    }
    __syncthreads();
}

__device__ __forceinline__ void apply_body(const DecTone &E, int p, int oh, int ow)
{
    __shared__ uint8_t s_lut[3 * 256];
    __shared__ uint32_t s_wave[12], s_step[3];
    if (p >= E.nseg) return;
    const DecToneSeg S = E.seg[p];
    if (S.term == CCMI_TONE_SHARPNESS) return;
    const int tid = threadIdx.x;
    const unsigned plane = (unsigned)oh * (unsigned)ow;
    float *__restrict__ buf = E.buf[S.src];
    const unsigned base = blockIdx.x * (unsigned)kPixPerBlock + tid;
    float mean_b = 0.f, lo[3] = {0.f, 0.f, 0.f}, sc[3] = {0.f, 0.f, 0.f};
    bool act[3] = {false, false, false};
    if (S.term == CCMI_TONE_CONTRAST) {
        const unsigned long long sj = *reinterpret_cast<const unsigned long long *>(acc_words(E, S, kToneAccSum));
        const float m = (float)((double)sj / ((double)plane * 65535.0));
        mean_b = fmt_mul(E.ops[S.end].v[1], m);
    } else if (S.term == CCMI_TONE_AUTOCONTRAST) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            lo[c] = __uint_as_float(~acc_words(E, S, kToneAccMin)[c]);
            const float hi = __uint_as_float(acc_words(E, S, kToneAccMax)[c]);
            act[c] = hi != lo[c];
            sc[c] = act[c] ? 1.0f / tone_sub(hi, lo[c]) : 0.f;
        }
    } else if (S.term == CCMI_TONE_EQUALIZE) {
        build_luts(acc_words(E, S, kToneAccHist), plane, s_lut, s_wave, s_step);
    }
#pragma unroll
    for (int it = 0; it < kPixPerThread; ++it) {
        const unsigned at = base + it * kThreads;
        if (at >= plane) break;
        float x[3] = {buf[at], buf[plane + at], buf[2 * plane + at]};
        tone_point(E, S.first, S.end, x);
        if (S.term == CCMI_TONE_CONTRAST) {
            const float f = E.ops[S.end].v[0];
#pragma unroll
            for (int c = 0; c < 3; ++c) x[c] = tone_clamp(fmt_add(fmt_mul(f, x[c]), mean_b));
        } else if (S.term == CCMI_TONE_AUTOCONTRAST) {
#pragma unroll
            for (int c = 0; c < 3; ++c)
                if (act[c]) x[c] = tone_clamp(fmt_mul(tone_sub(x[c], lo[c]), sc[c]));
        } else if (S.term == CCMI_TONE_EQUALIZE) {
#pragma unroll
            for (int c = 0; c < 3; ++c) x[c] = (float)s_lut[256 * c + tone_quant(x[c])] / 255.0f;
        }
        buf[at] = x[0], buf[plane + at] = x[1], buf[2 * plane + at] = x[2];
    }
}

__device__ __forceinline__ void sharp_body(const DecTone &E, int p, int oh, int ow, int tiles_x)
{
    __shared__ float s_in[3][kSharpIn * kSharpIn];
    if (p >= E.nseg) return;
    const DecToneSeg S = E.seg[p];
    if (S.term != CCMI_TONE_SHARPNESS) return;
    const int tid = threadIdx.x;
    const int ty = (int)blockIdx.x / tiles_x, tx = (int)blockIdx.x - ty * tiles_x;
    const int y0 = ty * kSharpTile, x0 = tx * kSharpTile;
    const unsigned plane = (unsigned)oh * (unsigned)ow;
    const float *__restrict__ src = E.buf[S.src];
    float *__restrict__ dst = E.buf[S.src ^ 1];
    // the tile and its halo, clamped to the frame: the weights never reach a clamped copy, since the
    // border pixels that would read one keep b = x
    for (int i = tid; i < kSharpIn * kSharpIn; i += kThreads) {
        const int ly = i / kSharpIn, lx = i - ly * kSharpIn;
        const int y = min(max(y0 - 1 + ly, 0), oh - 1), k = min(max(x0 - 1 + lx, 0), ow - 1);
        const unsigned at = (unsigned)y * (unsigned)ow + (unsigned)k;
        float x[3] = {src[at], src[plane + at], src[2 * plane + at]};
        tone_point(E, S.first, S.end, x);
#pragma unroll
        for (int c = 0; c < 3; ++c) s_in[c][i] = x[c];
    }
    __syncthreads();
    const float f = E.ops[S.end].v[0], g = E.ops[S.end].v[1];
    const float wc = (float)(5.0 / 13.0), wo = (float)(1.0 / 13.0);
    const bool small = oh <= 2 || ow <= 2;
    const int lx = tid & (kSharpTile - 1), k = x0 + lx;
    if (k >= ow) return;
#pragma unroll
    for (int j = 0; j < kSharpTile * kSharpTile / kThreads; ++j) {
        const int ly = (tid >> 5) + 8 * j, y = y0 + ly;
        if (y >= oh) break;
        const bool inner = y > 0 && y < oh - 1 && k > 0 && k < ow - 1;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float *__restrict__ q = &s_in[c][(ly + 1) * kSharpIn + lx + 1];
            const float x = q[0];
            float b = x;
            if (inner) {
                b = 0.f;
#pragma unroll
                for (int di = -1; di <= 1; ++di)
#pragma unroll
                    for (int dk = -1; dk <= 1; ++dk)
                        b = fmt_add(b, fmt_mul(di == 0 && dk == 0 ? wc : wo, q[di * kSharpIn + dk]));
            }
            // a frame of side <= 2 is left as it is (the pointwise ops before the sharpness op still act)
            dst[c * plane + (unsigned)y * (unsigned)ow + (unsigned)k] =
                small ? x : tone_clamp(fmt_add(fmt_mul(f, x), fmt_mul(g, b)));
        }
    }
}

// one frame, its entry as the kernel's own argument (the per-frame tail)
__global__ __launch_bounds__(kThreads) void dec_tone_stat(DecTone E, int p, int oh, int ow) { stat_body(E, p, oh, ow); }
__global__ __launch_bounds__(kThreads) void dec_tone_apply(DecTone E, int p, int oh, int ow) { apply_body(E, p, oh, ow); }
__global__ __launch_bounds__(kThreads) void dec_tone_sharp(DecTone E, int p, int oh, int ow, int tiles_x)
{
    sharp_body(E, p, oh, ow, tiles_x);
}

// the staged frames of a tail group: frame blockIdx.y's entry
__global__ __launch_bounds__(kThreads) void dec_tone_stat_batch(const DecTone *__restrict__ Es, int p, int oh, int ow)
{
    stat_body(Es[blockIdx.y], p, oh, ow);
}
__global__ __launch_bounds__(kThreads) void dec_tone_apply_batch(const DecTone *__restrict__ Es, int p, int oh, int ow)
{
    apply_body(Es[blockIdx.y], p, oh, ow);
}
__global__ __launch_bounds__(kThreads) void dec_tone_sharp_batch(const DecTone *__restrict__ Es, int p, int oh, int ow,
                                                                 int tiles_x)
{
    sharp_body(Es[blockIdx.y], p, oh, ow, tiles_x);
}

// which passes segment p of these frames needs
struct TonePasses {
    bool stat = false, apply = false, sharp = false;
};
TonePasses tone_passes(const DecTone *const *es, int m, int p)
{
    TonePasses t;
    for (int i = 0; i < m; ++i) {
        if (p >= es[i]->nseg) continue;
        const int term = es[i]->seg[p].term;
        t.stat = t.stat || term == CCMI_TONE_CONTRAST || term == CCMI_TONE_AUTOCONTRAST || term == CCMI_TONE_EQUALIZE;
        (term == CCMI_TONE_SHARPNESS ? t.sharp : t.apply) = true;
    }
    return t;
}

int check_tone(const DecTone &e)
{
    if (e.n < 0 || e.n > CCMI_TONE_MAX_OPS || e.nseg < 0 || e.nseg > CCMI_TONE_MAX_OPS || (e.n > 0 && !e.buf[0]))
        return ccmi_set_error(CCMI_ERR_ARG, "dec: a tone list without its staging frame");
    if ((dec_tone_sharps(e) && !e.buf[1]) || (dec_tone_stats(e) && !e.acc))
        return ccmi_set_error(CCMI_ERR_ARG, "dec: a tone list without its second frame or its accumulators");
    return CCMI_OK;
}

} // namespace

int launch_dec_tone_group(const DecTone *dev_es, const DecTone *const *host, int m, int oh, int ow, hipStream_t s)
{
    int nseg = 0;
    for (int i = 0; i < m; ++i) {
        if (int rc = check_tone(*host[i])) return rc;
        nseg = std::max(nseg, host[i]->nseg);
    }
    const size_t plane = (size_t)oh * (size_t)ow;
    const dim3 gp((unsigned)((plane + kPixPerBlock - 1) / kPixPerBlock), (unsigned)m);
    const int tiles_x = (ow + kSharpTile - 1) / kSharpTile;
    const dim3 gs((unsigned)(tiles_x * ((oh + kSharpTile - 1) / kSharpTile)), (unsigned)m);
    for (int p = 0; p < nseg; ++p) {
        const TonePasses t = tone_passes(host, m, p);
        if (t.stat) hipLaunchKernelGGL(dec_tone_stat_batch, gp, dim3(kThreads), 0, s, dev_es, p, oh, ow);
        if (t.apply) hipLaunchKernelGGL(dec_tone_apply_batch, gp, dim3(kThreads), 0, s, dev_es, p, oh, ow);
        if (t.sharp) hipLaunchKernelGGL(dec_tone_sharp_batch, gs, dim3(kThreads), 0, s, dev_es, p, oh, ow, tiles_x);
    }
    CCMI_HIP_CHECK(hipGetLastError());
    return CCMI_OK;
}

int launch_dec_tone_frame(const DecTone &e, int oh, int ow, hipStream_t s)
{
    if (int rc = check_tone(e)) return rc;
    const DecTone *es[1] = {&e};
    const size_t plane = (size_t)oh * (size_t)ow;
    const dim3 gp((unsigned)((plane + kPixPerBlock - 1) / kPixPerBlock));
    const int tiles_x = (ow + kSharpTile - 1) / kSharpTile;
    const dim3 gs((unsigned)(tiles_x * ((oh + kSharpTile - 1) / kSharpTile)));
    for (int p = 0; p < e.nseg; ++p) {
        const TonePasses t = tone_passes(es, 1, p);
        if (t.stat) hipLaunchKernelGGL(dec_tone_stat, gp, dim3(kThreads), 0, s, e, p, oh, ow);
        if (t.apply) hipLaunchKernelGGL(dec_tone_apply, gp, dim3(kThreads), 0, s, e, p, oh, ow);
        if (t.sharp) hipLaunchKernelGGL(dec_tone_sharp, gs, dim3(kThreads), 0, s, e, p, oh, ow, tiles_x);
    }
    CCMI_HIP_CHECK(hipGetLastError());
    return CCMI_OK;
}

} // namespace ccmi
