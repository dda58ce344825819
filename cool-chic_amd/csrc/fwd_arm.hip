// fwd_arm.hip -- path A ARM: causal context gather + MLP + Laplace rate, float32.
//
// Replaces, for every latent of every grid of every frame in one launch:
//   quantize (quantizer.py:231-232, eval = torch.round(gain * y)),
//   _get_neighbor (arm.py:308-352: zero pad 4, 9x9 unfold, index_select of the
//                  causal context pixels, _get_non_zero_pixel_ctx_index arm.py:373-506),
//   Arm.forward (arm.py:227-268: residual Linear+ReLU x n_hidden, Linear -> (mu, log_scale),
//                scale = exp(clamp(log_scale - 4, -4.6, 5))),
//   rate (coolchic.py:419-424 with _laplace_cdf arm.py:355-370).
//
// Layout: one workgroup (256 threads, 4 waves) owns a (4 NL) x 64 tile of one grid of one
// frame.  The quantised tile plus its causal halo (4 rows above, 4 columns either
// side) is staged once in LDS, a wave taking whole rows of it through buffer descriptors made on
// the scalar unit (arm_stage_tile); each thread evaluates the MLP for NL = 2 latents of the
// same column as one packed pair, so every weight (wave-uniform, held in SGPRs via
// scalar loads) feeds one v_pk_fma_f32 (two FMAs).  NL = 4 (two pairs per weight) was
// measured 13 % slower: 132 VGPRs, 3 waves per SIMD instead of 7.  LDS reads are lane-consecutive (conflict-free).  Grids of all resolutions
// share one launch through a tile prefix table (no per-grid launches).
//
// Two forms of the MLP, bit for bit the same (ccmi_arm_forward_f32_form): the row form above
// (arm_fwd_kernel, every dim_arm, reads the caller's parameters) and the pairs form
// (arm_fwd_pairs_kernel, dim_arm 8 and 16, the default): a packed register is two output units
// of one latent, the weights come from a transposed copy written by arm_pack_kernel.
#include <stdlib.h>

#include <algorithm>

#include "fwd_common.h"

using ccmi_fwd::cfloat_ptr;
using ccmi_fwd::f2;

namespace {

constexpr int kThreads = 256;
constexpr int kTX = 64;
constexpr int kRowsPerPass = kThreads / kTX; // 4
#ifndef CCMI_ARM_NL
#define CCMI_ARM_NL 2
#endif
constexpr int kNL = CCMI_ARM_NL;              // latents per thread (packed pairs)
constexpr int kNP = kNL / 2;
constexpr int kTY = kRowsPerPass * kNL;       // 8
constexpr int kHalo = 4;
constexpr int kLW = kTX + 2 * kHalo;          // 72
constexpr int kLH = kTY + kHalo;              // 12


// scaled ReLU of the pairs form: activations travel times 2^-32
constexpr float kArmDown = 0x1p-32f, kArmUp = 0x1p+32f;

// floor(n / d) for 0 <= n < 2^31 and 1 <= d < 2^31 as a multiply-high and a shift, so that a
// wave-uniform division stays on the scalar unit (s_mul_hi_u32; the compiler expands n / d into a
// float reciprocal on the VALU).  Granlund and Montgomery's constants for 31-bit n: with
// L = ceil(log2 d) and m = ceil(2^(31 + L) / d), which is in [2^31, 2^32), m d = 2^(31 + L) + e with
// 0 <= e < d <= 2^L, so n m / 2^(31 + L) = n / d + n e / (d 2^(31 + L)) and the second term is below
// 1 / d: the floors agree.  (2 n) m >> 32 >> L is that floor, and 2 n < 2^32.  Exact over the whole
// range; ccmi_launch_arm_f32 refuses a launch with 2^31 tiles or more.
struct ArmDiv {
    unsigned m, s;
};
inline ArmDiv arm_div_of(unsigned d)
{
    unsigned L = 0;
    while ((1u << L) < d) ++L;
    return ArmDiv{(unsigned)(((1ull << (31 + L)) + d - 1) / d), L};
}
__host__ __device__ __forceinline__ unsigned arm_div(unsigned n, ArmDiv d)
{
    return (unsigned)(((uint64_t)(n << 1) * d.m) >> 32) >> d.s;
}

struct ArmGeom {
    int n;
    int h[CCMI_MAX_GRIDS], w[CCMI_MAX_GRIDS], off[CCMI_MAX_GRIDS];
    int tiles_x[CCMI_MAX_GRIDS];
    int tile_start[CCMI_MAX_GRIDS];  // first tile of a grid in its frame; INT32_MAX past the last grid
    int ntl;                         // tiles of a frame
    ArmDiv by_ntl, by_tiles_x[CCMI_MAX_GRIDS];
};

// The tile a workgroup owns: grid l of frame b, rows y0.., columns x0.. of its H x W latents;
// wave and lane of the thread (the wave as a scalar) and what staging leaves for the stores.
struct ArmTile {
    int b, l, H, W, y0, x0;
    int wave, lane, xm;  // xm: the lane's first staged column, x0 - kHalo + lane
};

// Tile wt of a launch (the frames' tiles one after the other, a frame's by grid, a grid's row by
// row).  Everything is wave-uniform 32-bit arithmetic, so on the device it runs on the scalar unit.
__host__ __device__ __forceinline__ ArmTile arm_tile_of(const ArmGeom &g, unsigned wt)
{
    ArmTile T{};
    T.b = (int)arm_div(wt, g.by_ntl);
    const int t = (int)(wt - (unsigned)T.b * (unsigned)g.ntl);
    // the starts rise strictly (a grid has a tile) and those past the last grid are INT32_MAX
    int l = 0;
#pragma unroll
    for (int k = 1; k < CCMI_MAX_GRIDS; ++k) l += (int)((unsigned)(g.tile_start[k] - 1 - t) >> 31); // t >= start
    const unsigned lt = (unsigned)(t - g.tile_start[l]);
    const unsigned ty = arm_div(lt, g.by_tiles_x[l]);
    T.l = l;
    T.H = g.h[l];
    T.W = g.w[l];
    T.y0 = (int)ty * kTY;
    T.x0 = (int)(lt - ty * (unsigned)g.tiles_x[l]) * kTX;
    return T;
}

// Context pixel offsets (dy, dx) in the reference's gather order: flattened 9x9
// mask index k -> (k / 9 - 4, k % 9 - 4) for the indices of arm.py:373-506.
template <int D>
__device__ __forceinline__ void ctx_offset(int i, int &dy, int &dx)
{
    // clang-format off
    constexpr signed char k8[8] = {13, 22, 30, 31, 32, 37, 38, 39};
    constexpr signed char k16[16] = {13, 14, 20, 21, 22, 23, 24, 28, 29, 30, 31, 32, 33, 37, 38, 39};
    constexpr signed char k24[24] = {4, 11, 12, 13, 14, 15, 19, 20, 21, 22, 23, 24, 25, 28, 29, 30, 31, 32, 33, 34,
                                     36, 37, 38, 39};
    constexpr signed char k32[32] = {2, 3, 4, 5, 10, 11, 12, 13, 14, 15, 16, 19, 20, 21, 22, 23, 24, 25, 26, 27,
                                     28, 29, 30, 31, 32, 33, 34, 35, 36, 37, 38, 39};
    // clang-format on
    int k = D == 8 ? k8[i] : D == 16 ? k16[i] : D == 24 ? k24[i] : k32[i];
    dy = k / 9 - 4;
    dx = k % 9 - 4;
}

// inv_scale = 1 / scale (v_rcp_f32, shared by both CDF evaluations of a latent instead
// of two IEEE divisions).  expm1 of the reference is evaluated as v_exp_f32 - 1: its
// absolute error (~1 ulp of 1) is below the fp32 cancellation the reference formula
// already has in p = F(q + 1/2) - F(q - 1/2); worst rate error / tolerance of
// tests/test_forward.py over the goldens and random 720p / 1080p frames: 0.432 with
// either form (tools/rate_margin.py), ARM 5 % faster.
__device__ __forceinline__ float laplace_cdf(float x, float mu, float inv_scale)
{
    float s = x - mu;
    float sg = s > 0.f ? 1.f : (s < 0.f ? -1.f : 0.f);
    return 0.5f - 0.5f * sg * (__expf(-fabsf(s) * inv_scale) - 1.f);
}

// A frame's latents at most: the stores address an output of grid l as a wave-uniform base plus
// a 32-bit byte offset
constexpr int64_t kArmMaxLatents = (int64_t)1 << 30;

// Finds the workgroup's tile and stages it, quantised, with its causal halo in LDS.  SC: the
// quantised values are stored times 2^-32 (arm_fwd_pairs_kernel's scaled ReLU).
//
// A wave owns the rows wave, wave + 4, ... of the kLH x kLW tile: lane = column for the first 64
// columns, and lanes 0 .. kLW - 65 take the remaining columns in a second load per row.  A load
// goes through a buffer descriptor made on the scalar unit: the W floats of the row for the first
// load, the (at most) kLW - 64 floats from column x0 + 60 on that the image still has for the
// second, and no records at all for a row outside the image.  The hardware's range check then
// gives 0 for every column outside the image and touches no memory for it, and no load has a
// predicate, a branch or 64-bit address arithmetic of its own.
template <bool SC = false>
__device__ __forceinline__ ArmTile arm_stage_tile(float (&tile)[kLH][kLW], const float *__restrict__ lat,
                                                  int64_t lat_stride, const ArmGeom &g, float gain, int quantize)
{
    constexpr int kWaves = kThreads / 64, NR = kLH / kWaves, XC = kLW - 64;
    static_assert(kLH % kWaves == 0 && XC >= 0 && XC <= 64, "whole rows per wave, at most two loads per row");
    // XCD-aware tile order (ccmi_fwd::xcd_order): vertically adjacent tiles, which share the
    // 4 causal halo rows, meet in one L2
    ArmTile T = arm_tile_of(g, (unsigned)ccmi_fwd::xcd_order(blockIdx.x, gridDim.x));
    T.wave = __builtin_amdgcn_readfirstlane(threadIdx.x / 64);
    T.lane = threadIdx.x % 64;
    const float *src = lat + (int64_t)T.b * lat_stride + g.off[T.l];

    // a column left of the image goes past every row's records (with room for the four bytes of
    // the access), one at or past W is past them as it is
    T.xm = T.x0 - kHalo + T.lane;
    const unsigned col = 4u * (unsigned)max(T.xm, -2), colx = 4u * (unsigned)T.lane;
    const int xx = min(T.x0 - kHalo + 64, T.W); // the second loads' first column (x0 + 60: never negative)
    // every load of the thread is in flight before the first LDS store waits on one
    float lv[NR], lx[NR];
#pragma unroll
    for (int k = 0; k < NR; ++k) {
        const int y = T.y0 - kHalo + T.wave + k * kWaves;
        const bool in = (unsigned)y < (unsigned)T.H;
        float *at = const_cast<float *>(src + (in ? y * T.W : 0));
        lv[k] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(
            __builtin_amdgcn_make_buffer_rsrc(at, 0, in ? 4 * T.W : 0, 0x00020000), col, 0, 0));
        // the row's XC columns from xx on, as far as the image goes: lanes XC and up read nothing
        if constexpr (XC > 0)
            lx[k] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(
                __builtin_amdgcn_make_buffer_rsrc(at + (in ? xx : 0), 0, in ? 4 * min(T.W - xx, XC) : 0, 0x00020000), colx,
                0, 0));
    }
    const auto quantised = [&](float v) {
        if constexpr (SC) return rintf(gain * v) * kArmDown;
        else return quantize ? rintf(gain * v) : v;
    };
    float *dst = &tile[T.wave][T.lane];
#pragma unroll
    for (int k = 0; k < NR; ++k) dst[k * kWaves * kLW] = quantised(lv[k]);
    if constexpr (XC > 0) {
        // (the second loads stay up there: left alone, the compiler sinks them into this branch,
        // behind the waits of the stores above)
#pragma unroll
        for (int k = 0; k < NR; ++k) asm volatile("" : "+v"(lx[k]));
        if (T.lane < XC) {
#pragma unroll
            for (int k = 0; k < NR; ++k) dst[k * kWaves * kLW + 64] = quantised(lx[k]);
        }
    }
    __syncthreads();
    return T;
}

// The context gather: the byte offset in the tile of the top row that latent n of the thread
// (row wave + n * kRowsPerPass) reads, at the thread's own column, and the context value at
// (dy, dx) from it.  The offset is opaque, one register per latent: every read is then that
// register plus a constant that a ds_read2_b32 can hold, where from one base for both latents the
// compiler makes a new base register for most pairs of reads.
template <int D>
constexpr int arm_ctx_rows = D <= 16 ? 3 : 4; // rows above its own that a context of D reaches
template <int D>
__device__ __forceinline__ unsigned arm_ctx_base(const ArmTile &T, int n)
{
    unsigned at = 4u * (unsigned)((T.wave + n * kRowsPerPass + kHalo - arm_ctx_rows<D>) * kLW + T.lane);
    asm volatile("" : "+v"(at));
    return at;
}
template <int D>
__device__ __forceinline__ float arm_ctx_at(const float (&tile)[kLH][kLW], unsigned base, int dy, int dx)
{
    return *(const float *)((const char *)&tile[0][0] + base + 4u * (unsigned)((arm_ctx_rows<D> + dy) * kLW + kHalo + dx));
}

// Where a thread's outputs go: the requested outputs of the tile's frame and grid (wave-uniform,
// null where not asked for), the byte offset of the thread's first latent in them and whether
// its column is inside the image.
struct ArmOut {
    float *mu, *scale, *log_scale, *rate;
    unsigned at;
    bool col;
};
__device__ __forceinline__ ArmOut arm_out_of(const ArmTile &T, const ArmGeom &g, float *__restrict__ o_mu,
                                             float *__restrict__ o_scale, float *__restrict__ o_log_scale,
                                             float *__restrict__ o_rate, int64_t ostride)
{
    const int64_t base = (int64_t)T.b * ostride + g.off[T.l];
    const int x = T.xm + kHalo;
    return ArmOut{o_mu ? o_mu + base : nullptr, o_scale ? o_scale + base : nullptr,
                  o_log_scale ? o_log_scale + base : nullptr, o_rate ? o_rate + base : nullptr,
                  4u * (unsigned)((T.y0 + T.wave) * T.W + x), x < T.W};
}
__device__ __forceinline__ float *arm_at(float *base, unsigned byte) { return (float *)((char *)base + byte); }

// Scale, rate and the stores of the thread's latent n (row wave + n * kRowsPerPass of the tile)
// from its mu mn and log-scale lsn; q is the latent's own quantised value.
__device__ __forceinline__ void arm_emit(const ArmTile &T, const ArmOut &O, int n, float mn, float lsn, float q)
{
    const int y = T.y0 + T.wave + n * kRowsPerPass;
    if (y < T.H && O.col) {
        // v_exp_f32 / v_log_f32 directly (the clamped exponent and p in [2^-16, 1] are far
        // from the ranges the library forms guard; errors well inside the rate tolerance)
        const float sc = __expf(fminf(fmaxf(lsn - 4.f, -4.6f), 5.0f));
        const unsigned at = O.at + 4u * (unsigned)(n * kRowsPerPass * T.W);
        if (O.mu) *arm_at(O.mu, at) = mn;
        if (O.scale) *arm_at(O.scale, at) = sc;
        if (O.log_scale) *arm_at(O.log_scale, at) = lsn;
        if (O.rate) {
            const float is = __builtin_amdgcn_rcpf(sc);
            const float pr = fmaxf(laplace_cdf(q + 0.5f, mn, is) - laplace_cdf(q - 0.5f, mn, is), 1.52587890625e-05f);
            *arm_at(O.rate, at) = -__log2f(pr);
        }
    }
}

// NH >= 0: the hidden-layer count fixed at compile time (the layer loop unrolled, so the
// next layer's scalar weight loads can be scheduled under the current layer's FMAs)
template <int D, int NH = -1>
__global__ __launch_bounds__(kThreads) void arm_fwd_kernel(
    const float *__restrict__ lat, int64_t lat_stride, ArmGeom g, float gain, int quantize, int nh,
    const float *__restrict__ params, int64_t pstride, float *__restrict__ o_mu, float *__restrict__ o_scale,
    float *__restrict__ o_log_scale, float *__restrict__ o_rate, int64_t ostride)
{
    __shared__ float tile[kLH][kLW];
    const ArmTile T = arm_stage_tile(tile, lat, lat_stride, g, gain, quantize);

    const cfloat_ptr p = (cfloat_ptr)(size_t)(params + (int64_t)T.b * pstride);
    const ArmOut O = arm_out_of(T, g, o_mu, o_scale, o_log_scale, o_rate, ostride);

    // the two latents of a thread travel as one packed pair (v_pk_fma_f32): every
    // wave-uniform weight feeds both with one instruction
    // pair q = rows wave + (2q) * kRowsPerPass and wave + (2q + 1) * kRowsPerPass
    static_assert(kNL % 2 == 0, "packed pair layout");
    unsigned cb[kNL];
#pragma unroll
    for (int n = 0; n < kNL; ++n) cb[n] = arm_ctx_base<D>(T, n);
    f2 a[kNP][D];
#pragma unroll
    for (int i = 0; i < D; ++i) {
        int dy, dx;
        ctx_offset<D>(i, dy, dx);
#pragma unroll
        for (int q = 0; q < kNP; ++q)
            a[q][i] = f2{arm_ctx_at<D>(tile, cb[2 * q], dy, dx), arm_ctx_at<D>(tile, cb[2 * q + 1], dy, dx)};
    }

    if constexpr (NH >= 0) nh = NH;
#pragma unroll
    for (int layer = 0; layer < nh; ++layer) {
        const cfloat_ptr Wl = p + layer * (D * D + D);
        const cfloat_ptr bl = Wl + D * D;
        f2 o[kNP][D];
#pragma unroll
        for (int j = 0; j < D; ++j) {
            // F.linear(x) + x, then ReLU: the accumulator starts at bias + residual (one packed
            // add instead of two after the products; a different fp32 summation order, inside
            // the forward's tolerance)
            f2 acc[kNP];
#pragma unroll
            for (int q = 0; q < kNP; ++q) acc[q] = a[q][j] + f2(bl[j]);
#pragma unroll
            for (int i = 0; i < D; ++i) {
                const f2 wji = f2(Wl[j * D + i]);
#pragma unroll
                for (int q = 0; q < kNP; ++q) acc[q] = __builtin_elementwise_fma(wji, a[q][i], acc[q]);
            }
#pragma unroll
            for (int q = 0; q < kNP; ++q) o[q][j] = __builtin_elementwise_max(acc[q], f2(0.f));
        }
#pragma unroll
        for (int q = 0; q < kNP; ++q)
#pragma unroll
            for (int j = 0; j < D; ++j) a[q][j] = o[q][j];
    }

    const cfloat_ptr Wo = p + nh * (D * D + D);
    f2 m[kNP], ls[kNP];
#pragma unroll
    for (int q = 0; q < kNP; ++q) {
        m[q] = f2(Wo[2 * D]);
        ls[q] = f2(Wo[2 * D + 1]);
    }
#pragma unroll
    for (int i = 0; i < D; ++i) {
        const f2 w0 = f2(Wo[i]), w1 = f2(Wo[D + i]);
#pragma unroll
        for (int q = 0; q < kNP; ++q) {
            m[q] = __builtin_elementwise_fma(w0, a[q][i], m[q]);
            ls[q] = __builtin_elementwise_fma(w1, a[q][i], ls[q]);
        }
    }
#pragma unroll
    for (int n = 0; n < kNL; ++n)
        arm_emit(T, O, n, (n & 1) ? m[n >> 1].y : m[n >> 1].x, (n & 1) ? ls[n >> 1].y : ls[n >> 1].x,
                 arm_ctx_at<D>(tile, cb[n], 0, 0));
}

// The transposed copy of every frame's ARM parameters the pairs form reads (layout:
// fwd_common.h, arm_pack_src).  One workgroup per frame.
__global__ __launch_bounds__(kThreads) void arm_pack_kernel(const float *__restrict__ params, int64_t pstride, int d,
                                                            int nh, float *__restrict__ out, int ostride)
{
    const float *p = params + (int64_t)blockIdx.x * pstride;
    float *o = out + (int64_t)blockIdx.x * ostride;
    for (int t = threadIdx.x; t < ostride; t += kThreads) {
        const int s = ccmi_fwd::arm_pack_src(d, nh, t);
        o[t] = s >= 0 ? p[s] : 0.f;
    }
}

template <int D>
using arm_row = float __attribute__((ext_vector_type(D)));

// One row of D packed weights, `at` floats into the frame's block, as one scalar load with the
// offset in an SGPR.  The offset is made opaque so that the load stays where it is written:
// left to itself the compiler hoists every row load of an unrolled layer to its top and
// spills the SGPRs through VGPR lanes.
template <int D>
__device__ __forceinline__ arm_row<D> arm_load_row(cfloat_ptr base, unsigned at, const arm_row<D> *landed = nullptr)
{
    // scalar loads return out of order, so every wait is for all of them: the wait for the row
    // in use (`landed`, issued a row of FMAs ago) goes in front of this load, not behind it
    if (landed) asm volatile("" ::"s"((*landed)[0]));
    unsigned off = at * (unsigned)sizeof(float);
    asm volatile("" : "+s"(off));
    const arm_row<D> r =
        *(const __attribute__((address_space(4))) arm_row<D> *)((const __attribute__((address_space(4))) char *)base + off);
    // and the scheduler may not sink the load below the FMAs that follow it: it is issued
    // here and waited for at its first use, a row of FMAs later
    __builtin_amdgcn_sched_barrier(0);
    return r;
}

// Keeps the row loads one row ahead of the FMAs: no FMA of a later row (and so no load of the
// row after it) moves above this point.
template <int N>
__device__ __forceinline__ void arm_fence(f2 (&o)[kNL][N])
{
    static_assert(N == 4 || N == 8, "accumulator pairs per latent");
#pragma unroll
    for (int n = 0; n < kNL; ++n) {
        if constexpr (N == 8)
            asm volatile("" : "+v"(o[n][0]), "+v"(o[n][1]), "+v"(o[n][2]), "+v"(o[n][3]), "+v"(o[n][4]), "+v"(o[n][5]),
                         "+v"(o[n][6]), "+v"(o[n][7]));
        else
            asm volatile("" : "+v"(o[n][0]), "+v"(o[n][1]), "+v"(o[n][2]), "+v"(o[n][3]));
    }
}

// The pairs form of arm_fwd_kernel: same tile, same arithmetic, bit for bit, other packing.
// A packed register holds two neighbouring output units (j, j + 1) of ONE latent, so the weight
// operand of a v_pk_fma_f32 is the pair (W[j][i], W[j + 1][i]): with the transposed copy of
// arm_pack_kernel an aligned SGPR pair straight out of the row's scalar load, where the row
// form moves every odd-indexed weight into a scratch pair first.  The activation a_i is one
// half of a VGPR pair, selected by op_sel.  A layer is D / 2 independent accumulator chains
// per latent walked over i; each output is still (a_j + b_j) and then the products for
// i = 0 .. D-1 in order.  The rows are consumed in the order they are stored (layer: bias
// row first, then rows 0 .. D-1; then the output block in two halves), each loaded while the
// one before it is used.
//
// SC (quantize = 1 only), the scaled ReLU: the tile is staged as q 2^-32, the accumulators start
// at b 2^-32 + a' (one v_pk_fma_f32 where the unscaled form has a v_pk_add_f32), so a
// pre-activation arrives as h 2^-32 and max(h, 0) is the clamp-to-[0, 1] modifier of the layer's
// last fma: no v_max_f32 per unit and latent (gfx950 has no packed f32 max).  mu, log_scale
// and the latent's own value are multiplied back by 2^32 at the end.  Nothing is rescaled on
// the scalar unit: the weights are used as they are.  A power-of-two scaling commutes with
// every rounding of the chain, so the bits are the unscaled form's, under the conditions
// written at the fused head (fwd_syn.hip, "Scaled ReLU"): every bias, activation and
// partial sum is 0 or at least 2^-94 in magnitude, and no pre-activation exceeds 2^32.
template <int D, int NH = -1, bool SC = false>
__global__ __launch_bounds__(kThreads) void arm_fwd_pairs_kernel(
    const float *__restrict__ lat, int64_t lat_stride, ArmGeom g, float gain, int quantize, int nh,
    const float *__restrict__ packed, int pkstride, float *__restrict__ o_mu, float *__restrict__ o_scale,
    float *__restrict__ o_log_scale, float *__restrict__ o_rate, int64_t ostride)
{
    static_assert(kNL == 2 && (D == 8 || D == 16), "pairs form: two latents per thread, dim_arm 8 or 16");
    constexpr int RS = ccmi_fwd::arm_pack_row(D), LS = ccmi_fwd::arm_pack_layer(D), HP = D / 2;
    __shared__ float tile[kLH][kLW];
    const ArmTile T = arm_stage_tile<SC>(tile, lat, lat_stride, g, gain, quantize);

    const cfloat_ptr P = (cfloat_ptr)(size_t)(packed + (int64_t)T.b * pkstride);
    const ArmOut O = arm_out_of(T, g, o_mu, o_scale, o_log_scale, o_rate, ostride);
    if constexpr (NH >= 0) nh = NH;

    // a[n][jp] = activations (2 jp, 2 jp + 1) of latent n (row wave + n * kRowsPerPass)
    unsigned cb[kNL];
#pragma unroll
    for (int n = 0; n < kNL; ++n) cb[n] = arm_ctx_base<D>(T, n);
    f2 a[kNL][HP];
#pragma unroll
    for (int i = 0; i < D; ++i) {
        int dy, dx;
        ctx_offset<D>(i, dy, dx);
#pragma unroll
        for (int n = 0; n < kNL; ++n) a[n][i >> 1][i & 1] = arm_ctx_at<D>(tile, cb[n], dy, dx);
    }

    const unsigned Wo = nh * LS;
    const f2 bo = *(const __attribute__((address_space(4))) f2 *)(P + Wo + 2 * D);
    arm_row<D> cur = arm_load_row<D>(P, nh > 0 ? D * RS : 0);
#pragma unroll
    for (int layer = 0; layer < nh; ++layer) {
        const unsigned Wl = layer * LS;
        // F.linear(x) + x, then ReLU: the accumulators start at bias + residual
        f2 o[kNL][HP];
        arm_row<D> nxt = arm_load_row<D>(P, Wl, &cur);
#pragma unroll
        for (int n = 0; n < kNL; ++n)
#pragma unroll
            for (int jp = 0; jp < HP; ++jp) {
                const f2 bp = f2{cur[2 * jp], cur[2 * jp + 1]};
                o[n][jp] = SC ? __builtin_elementwise_fma(bp, f2(kArmDown), a[n][jp]) : a[n][jp] + bp;
            }
        arm_fence(o);
        cur = nxt;
#pragma unroll
        for (int i = 0; i < D; ++i) {
            // after the last row: the next layer's bias row, or the first half of the output block
            nxt = arm_load_row<D>(P, i + 1 < D ? Wl + (i + 1) * RS : layer + 1 < nh ? Wl + LS + D * RS : Wl + LS, &cur);
#pragma unroll
            for (int n = 0; n < kNL; ++n) {
                const f2 ai = f2(a[n][i >> 1][i & 1]);
#pragma unroll
                for (int jp = 0; jp < HP; ++jp) {
                    const f2 wp = f2{cur[2 * jp], cur[2 * jp + 1]};
                    if constexpr (SC && (D & 1) == 0) {
                        if (i == D - 1) { // the odd half of the last activation pair, clamped to [0, 1]
                            asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[0,1,0] op_sel_hi:[1,1,1] clamp"
                                : "=v"(o[n][jp])
                                : "s"(wp), "v"(a[n][HP - 1]), "v"(o[n][jp]));
                            continue;
                        }
                    }
                    o[n][jp] = __builtin_elementwise_fma(wp, ai, o[n][jp]);
                }
            }
            // not after the last row: the ReLU would get a canonicalising v_max in front of it
            if (i + 1 < D) arm_fence(o);
            cur = nxt;
        }
#pragma unroll
        for (int n = 0; n < kNL; ++n)
#pragma unroll
            for (int jp = 0; jp < HP; ++jp) a[n][jp] = SC ? o[n][jp] : __builtin_elementwise_max(o[n][jp], f2(0.f));
    }

    // output layer: one pair (mu, log_scale) per latent; cur holds WoT[0 .. D/2)
    f2 ml[kNL];
#pragma unroll
    for (int n = 0; n < kNL; ++n) ml[n] = SC ? bo * kArmDown : bo;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        arm_row<D> nxt = cur;
        if (half == 0) nxt = arm_load_row<D>(P, Wo + D, &cur);
#pragma unroll
        for (int k = 0; k < HP; ++k) {
            const int i = half * HP + k;
#pragma unroll
            for (int n = 0; n < kNL; ++n)
                ml[n] = __builtin_elementwise_fma(f2{cur[2 * k], cur[2 * k + 1]}, f2(a[n][i >> 1][i & 1]), ml[n]);
        }
        cur = nxt;
    }
#pragma unroll
    for (int n = 0; n < kNL; ++n) {
        float q = arm_ctx_at<D>(tile, cb[n], 0, 0);
        if constexpr (SC) {
            ml[n] *= kArmUp;
            q *= kArmUp;
        }
        arm_emit(T, O, n, ml[n].x, ml[n].y, q);
    }
}

template <int D>
__global__ __launch_bounds__(kThreads) void arm_context_kernel(const float *__restrict__ grid, int H, int W,
                                                               float *__restrict__ out)
{
    const int b = blockIdx.y;
    const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (p >= (int64_t)H * W) return;
    const int y = (int)(p / W), x = (int)(p - (int64_t)y * W);
    const float *g = grid + (int64_t)b * H * W;
    float *o = out + ((int64_t)b * H * W + p) * D;
#pragma unroll
    for (int i = 0; i < D; ++i) {
        int dy, dx;
        ctx_offset<D>(i, dy, dx);
        const int yy = y + dy, xx = x + dx;
        o[i] = (yy >= 0 && xx >= 0 && xx < W) ? g[yy * W + xx] : 0.f;
    }
}

template <int D>
__global__ __launch_bounds__(kThreads) void arm_mlp_kernel(const float *__restrict__ ctx, int64_t M, int nh,
                                                           const float *__restrict__ p, float *__restrict__ o_mu,
                                                           float *__restrict__ o_scale, float *__restrict__ o_ls)
{
    const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (r >= M) return;
    float a[D];
#pragma unroll
    for (int i = 0; i < D; ++i) a[i] = ctx[r * D + i];
    for (int layer = 0; layer < nh; ++layer) {
        const float *Wl = p + layer * (D * D + D);
        float o[D];
#pragma unroll
        for (int j = 0; j < D; ++j) {
            float acc = 0.f;
#pragma unroll
            for (int i = 0; i < D; ++i) acc = fmaf(Wl[j * D + i], a[i], acc);
            o[j] = fmaxf((acc + Wl[D * D + j]) + a[j], 0.f);
        }
#pragma unroll
        for (int j = 0; j < D; ++j) a[j] = o[j];
    }
    const float *Wo = p + nh * (D * D + D);
    float m = 0.f, ls = 0.f;
#pragma unroll
    for (int i = 0; i < D; ++i) {
        m = fmaf(Wo[i], a[i], m);
        ls = fmaf(Wo[D + i], a[i], ls);
    }
    m += Wo[2 * D];
    ls += Wo[2 * D + 1];
    if (o_mu) o_mu[r] = m;
    if (o_ls) o_ls[r] = ls;
    if (o_scale) o_scale[r] = expf(fminf(fmaxf(ls - 4.f, -4.6f), 5.0f));
}

} // namespace

extern "C" int ccmi_arm_context_f32(const float *grid, int batch, int h, int w, int dim_arm, float *out, void *stream)
{
    if (!grid || !out || batch < 1 || h < 1 || w < 1) return ccmi_set_error(CCMI_ERR_ARG, "arm_context: bad argument");
    dim3 g((unsigned)(((int64_t)h * w + kThreads - 1) / kThreads), batch);
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (dim_arm) {
    case 8: hipLaunchKernelGGL(arm_context_kernel<8>, g, dim3(kThreads), 0, s, grid, h, w, out); break;
    case 16: hipLaunchKernelGGL(arm_context_kernel<16>, g, dim3(kThreads), 0, s, grid, h, w, out); break;
    case 24: hipLaunchKernelGGL(arm_context_kernel<24>, g, dim3(kThreads), 0, s, grid, h, w, out); break;
    case 32: hipLaunchKernelGGL(arm_context_kernel<32>, g, dim3(kThreads), 0, s, grid, h, w, out); break;
    default: return ccmi_set_error(CCMI_ERR_UNSUPPORTED, "arm_context: dim_arm %d", dim_arm);
    }
    CCMI_HIP_CHECK(hipGetLastError());
    return CCMI_OK;
}

extern "C" int ccmi_arm_mlp_f32(const float *ctx, int64_t m, int dim_arm, int n_hidden, const float *params, float *mu,
                                float *scale, float *log_scale, void *stream)
{
    if (!ctx || !params || m < 0 || n_hidden < 0 || n_hidden > 4) return ccmi_set_error(CCMI_ERR_ARG, "arm_mlp: bad argument");
    if (m == 0) return CCMI_OK;
    dim3 g((unsigned)((m + kThreads - 1) / kThreads));
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (dim_arm) {
    case 8: hipLaunchKernelGGL(arm_mlp_kernel<8>, g, dim3(kThreads), 0, s, ctx, m, n_hidden, params, mu, scale, log_scale); break;
    case 16: hipLaunchKernelGGL(arm_mlp_kernel<16>, g, dim3(kThreads), 0, s, ctx, m, n_hidden, params, mu, scale, log_scale); break;
    case 24: hipLaunchKernelGGL(arm_mlp_kernel<24>, g, dim3(kThreads), 0, s, ctx, m, n_hidden, params, mu, scale, log_scale); break;
    case 32: hipLaunchKernelGGL(arm_mlp_kernel<32>, g, dim3(kThreads), 0, s, ctx, m, n_hidden, params, mu, scale, log_scale); break;
    default: return ccmi_set_error(CCMI_ERR_UNSUPPORTED, "arm_mlp: dim_arm %d", dim_arm);
    }
    CCMI_HIP_CHECK(hipGetLastError());
    return CCMI_OK;
}

extern "C" int ccmi_arm_pack_host(const float *params, int dim_arm, int n_hidden, float *out)
{
    if (!params || !out || dim_arm < 1 || n_hidden < 0) return -1;
    const int n = ccmi_fwd::arm_pack_stride(dim_arm, n_hidden);
    for (int t = 0; t < n; ++t) {
        const int s = ccmi_fwd::arm_pack_src(dim_arm, n_hidden, t);
        out[t] = s >= 0 ? params[s] : 0.f;
    }
    return n;
}

// The geometry of a launch over `batch` frames and its tile count; refuses what the kernels'
// 32-bit arithmetic does not cover.
static int arm_geometry(int n_grids, const int *h, const int *w, int batch, ArmGeom *out, int64_t *n_tiles)
{
    if (n_grids < 1 || n_grids > CCMI_MAX_GRIDS || !h || !w || batch < 1)
        return ccmi_set_error(CCMI_ERR_ARG, "arm: bad grids or batch");
    ArmGeom g{};
    g.n = n_grids;
    int64_t off = 0, tiles = 0;
    for (int l = 0; l < n_grids; ++l) {
        if (h[l] < 1 || w[l] < 1) return ccmi_set_error(CCMI_ERR_ARG, "arm: grid %d has size %dx%d", l, h[l], w[l]);
        if (off + (int64_t)h[l] * w[l] > kArmMaxLatents)
            return ccmi_set_error(CCMI_ERR_ARG, "arm: more than 2^30 latents in a frame");
        g.h[l] = h[l];
        g.w[l] = w[l];
        g.off[l] = (int)off;
        g.tiles_x[l] = ccmi_div_up(w[l], kTX);
        g.by_tiles_x[l] = arm_div_of((unsigned)g.tiles_x[l]);
        g.tile_start[l] = (int)tiles;
        tiles += (int64_t)g.tiles_x[l] * ccmi_div_up(h[l], kTY);
        off += (int64_t)h[l] * w[l];
    }
    for (int l = n_grids; l < CCMI_MAX_GRIDS; ++l) g.tile_start[l] = INT32_MAX;
    g.ntl = (int)tiles;
    g.by_ntl = arm_div_of((unsigned)tiles);
    // the tile id is a 31-bit number (arm_div), and so is the grid's x dimension
    if (tiles * batch > INT32_MAX) return ccmi_set_error(CCMI_ERR_ARG, "arm: 2^31 tiles or more in a launch");
    *out = g;
    *n_tiles = tiles * batch;
    return CCMI_OK;
}

extern "C" int ccmi_arm_tile_map(int n_grids, const int *h, const int *w, int batch, int64_t first, int count,
                                 int *out, int64_t *n_tiles)
{
    ArmGeom g;
    int64_t total = 0;
    if (int rc = arm_geometry(n_grids, h, w, batch, &g, &total)) return rc;
    if (n_tiles) *n_tiles = total;
    if (count < 0 || first < 0 || first + count > total || (count > 0 && !out))
        return ccmi_set_error(CCMI_ERR_ARG, "arm_tile_map: tiles outside the launch's %lld", (long long)total);
    for (int i = 0; i < count; ++i) {
        const ArmTile T = arm_tile_of(g, (unsigned)(first + i));
        out[4 * i] = T.b;
        out[4 * i + 1] = T.l;
        out[4 * i + 2] = T.y0;
        out[4 * i + 3] = T.x0;
    }
    return CCMI_OK;
}

int ccmi_launch_arm_f32(const ccmi_arm_args *a, hipStream_t s, int form)
{
    ArmGeom g;
    int64_t tiles = 0;
    if (int rc = arm_geometry(a->n_grids, a->h, a->w, a->batch, &g, &tiles)) return rc;
    const int off = g.off[g.n - 1] + g.h[g.n - 1] * g.w[g.n - 1];
    if ((a->latent_stride != 0 && a->latent_stride < off) || a->out_stride < off)
        return ccmi_set_error(CCMI_ERR_ARG, "arm: stride smaller than the %d latents of a frame", off);
    dim3 grid((unsigned)tiles);

    // pairs form (dim_arm 8 and 16): pack the weights on this stream, then the kernel that reads
    // the copy.  Without a buffer (none may be allocated while the stream captures) form 0 runs
    // the row form below.
    const bool has_pairs = a->dim_arm == 8 || a->dim_arm == 16;
    if (form == CCMI_ARM_FORM_PAIRS && !has_pairs)
        return ccmi_set_error(CCMI_ERR_UNSUPPORTED, "arm: the pairs form needs dim_arm 8 or 16 (got %d)", a->dim_arm);
    if (form != CCMI_ARM_FORM_ROWS && has_pairs) {
        const int pks = ccmi_fwd::arm_pack_stride(a->dim_arm, a->n_hidden);
        const int frames = a->param_stride ? a->batch : 1; // stride 0: one model shared by all frames
        float *pk = nullptr;
        if (int rc = ccmi_arm_pack_buffer((size_t)frames * pks * sizeof(float), s, &pk)) return rc;
        if (!pk && form == CCMI_ARM_FORM_PAIRS)
            return ccmi_set_error(CCMI_ERR_UNSUPPORTED, "arm: no packed-weight buffer for this stream while it captures");
        if (pk) {
            hipLaunchKernelGGL(arm_pack_kernel, dim3(frames), dim3(kThreads), 0, s, a->params, a->param_stride, a->dim_arm,
                               a->n_hidden, pk, pks);
#define CCMI_ARM_PAIRS(DD, NN)                                                                                        \
    do {                                                                                                              \
        auto kern = a->quantize ? arm_fwd_pairs_kernel<DD, NN, true> : arm_fwd_pairs_kernel<DD, NN, false>;          \
        hipLaunchKernelGGL(kern, grid, dim3(kThreads), 0, s, a->latent, a->latent_stride, g, a->gain, a->quantize,   \
                           a->n_hidden, pk, a->param_stride ? pks : 0, a->mu, a->scale, a->log_scale, a->rate,       \
                           a->out_stride);                                                                           \
    } while (0)
            // quantised latents (integers): the scaled ReLU
            if (a->dim_arm == 8) {
                if (a->n_hidden == 2) CCMI_ARM_PAIRS(8, 2);
                else CCMI_ARM_PAIRS(8, -1);
            } else {
                if (a->n_hidden == 2) CCMI_ARM_PAIRS(16, 2);
                else CCMI_ARM_PAIRS(16, -1);
            }
#undef CCMI_ARM_PAIRS
            CCMI_HIP_CHECK(hipGetLastError());
            return CCMI_OK;
        }
    }

#define CCMI_ARM_LAUNCH(DD)                                                                                     \
    hipLaunchKernelGGL(arm_fwd_kernel<DD>, grid, dim3(kThreads), 0, s, a->latent, a->latent_stride, g, a->gain, \
                       a->quantize, a->n_hidden, a->params, a->param_stride, a->mu, a->scale, a->log_scale,     \
                       a->rate, a->out_stride)
    switch (a->dim_arm) {
    case 8: CCMI_ARM_LAUNCH(8); break;
    case 16:
        // the presets' ARM (2 hidden layers): layer loop unrolled
        if (a->n_hidden == 2) {
            hipLaunchKernelGGL((arm_fwd_kernel<16, 2>), grid, dim3(kThreads), 0, s, a->latent, a->latent_stride, g, a->gain,
                               a->quantize, a->n_hidden, a->params, a->param_stride, a->mu, a->scale, a->log_scale,
                               a->rate, a->out_stride);
        } else {
            CCMI_ARM_LAUNCH(16);
        }
        break;
    case 24: CCMI_ARM_LAUNCH(24); break;
    case 32: CCMI_ARM_LAUNCH(32); break;
    default: return ccmi_set_error(CCMI_ERR_UNSUPPORTED, "arm: dim_arm must be 8, 16, 24 or 32 (got %d)", a->dim_arm);
    }
#undef CCMI_ARM_LAUNCH
    CCMI_HIP_CHECK(hipGetLastError());
    return CCMI_OK;
}
