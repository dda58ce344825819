// dec_tail.hip -- path B: the decoder tail of the bit-exact fixed-point .cool decoder: pyramid,
// synthesis, blend and output kernels, their launchers and the batched tail (the ARM + CABAC
// kernels are dec_arm.hip).
//
// Compiled with -fwrapv: every accumulation is int32 with two's-complement wrap,
// every right shift of a sum is the reference's truncation toward zero
// (s < 0 ? -((-s) >> p) : s >> p) unless the reference rounds.
//
//  dec_ups_level    one launch per pyramid level (ups_refine_cpu.hpp:11-79,
//                   ups_upsample_cpu.hpp:12-91): integer refine + 2x polyphase upsample
//                   with the reference's per-pass truncations, LDS-tiled.
//  dec_syn_fused    1x1+1x1 fused head (synfused_cpu.hpp:17-109 semantics) + 3x3 layers
//                   (syn_cpu.hpp / synlb_cpu.hpp) with replicate padding, one launch.
//  dec_syn_layer    generic per-layer integer conv (any ks / widths).
//  dec_output       444 -> 420/444 8/10-bit or PPM payload (ccdecapi.cpp:59-240).
//  dec_output_tensor  the same samples as planar u8 / u16 / f32 device tensors (no file
//                   layout): one packed store per 4 destination samples, any sample alignment.
//  dec_output_fmt   the same samples as the formatted tensor of a ccmi_tensor_fmt: three
//                   full-size channels, YUV -> RGB, scale / bias, f32 / f16 / bf16, strides, mirror.
//  dec_resample_h, dec_resample_v  the formatted tensor with a ccmi_resample: the region through an
//                   antialiased triangle filter to the output size, horizontal then vertical pass.
//  dec_warp         the formatted tensor with a ccmi_warp: every output pixel a bilinear sample of
//                   the frame at the position the frame's 2 x 3 matrix gives, fill or edge padding.
#include <stdlib.h>

#include <algorithm>
#include <type_traits>
#include <utility>

#include "dec_device.h"
#include "dec_internal.h"

namespace ccmi {
namespace {

// ------------------------------------------------------------------ upsampling (integer)
constexpr int kThreads = 256;
constexpr int kTY = 16, kTX = 64;
constexpr int kMaxKs = 16;

struct DecLevel {
    const int32_t *src;      // level-k stack (or the raw coarsest latent plane)
    int C, hs, ws, src_prec;
    const int32_t *ref;      // latent plane of level k-1 (ARM precision)
    int32_t *dst;            // level k-1 stack: C + 1 channels
    int hd, wd;
    const int32_t *kup;      // ksx2 taps
    int ksx2;
    const int32_t *kpre;     // ks taps
    int ks;
    int tiles_x;
};

// Window form (region decode): the step computes the window [dy0, dy1) x [dx0, dx1) of the
// destination level and stores it compactly (pitch = the window's width).  The source stack
// holds the window [sy0, sy1] x [sx0, sx1] of its level at pitch `spitch` from the storage
// origin (soy, sox) (a compact stack: the window's own origin; the raw coarsest latent plane:
// 0, 0 at the frame pitch); the reference plane keeps the frame pitch and holds ref_rows rows.
// Border rules use the true plane sizes of DecLevel (replicate for the source, zero for the
// refine); source reads are clamped to the stored window on top, which changes nothing the
// window's samples depend on (the host planned the windows from these very taps) and keeps
// the surplus lanes of an edge tile inside the allocation.
struct DecLevelWin {
    DecLevel L;
    int dy0, dy1, dx0, dx1;
    int soy, sox, spitch;
    int sy0, sy1, sx0, sx1; // inclusive clamp bounds
    int64_t splane;
    int ref_rows;
};

template <bool WIN>
__device__ __forceinline__ void ups_level_body(const DecLevel &A, const DecLevelWin *Wn, int gtx, int32_t *s_in,
                                               int32_t *s_tmp);

__global__ __launch_bounds__(kThreads) void dec_ups_level(DecLevel A)
{
    __shared__ int32_t s_in[(kTY + kMaxKs) * (kTX + kMaxKs)];
    __shared__ int32_t s_tmp[(kTY + kMaxKs) * kTX];
    ups_level_body<false>(A, nullptr, A.tiles_x, s_in, s_tmp);
}

// frames of a batch (identical geometry): blockIdx.y = frame
__global__ __launch_bounds__(kThreads) void dec_ups_level_batch(const DecLevel *__restrict__ As)
{
    __shared__ int32_t s_in[(kTY + kMaxKs) * (kTX + kMaxKs)];
    __shared__ int32_t s_tmp[(kTY + kMaxKs) * kTX];
    const DecLevel A = As[blockIdx.y];
    ups_level_body<false>(A, nullptr, A.tiles_x, s_in, s_tmp);
}

// region decode: blockIdx.y = frame, the grid's tiles cover the group's largest window
// (gtx tiles across); a frame's blocks past its own window leave at once
__global__ __launch_bounds__(kThreads) void dec_ups_level_win_batch(const DecLevelWin *__restrict__ As, int gtx)
{
    __shared__ int32_t s_in[(kTY + kMaxKs) * (kTX + kMaxKs)];
    __shared__ int32_t s_tmp[(kTY + kMaxKs) * kTX];
    const DecLevelWin *Wn = As + blockIdx.y;
    const DecLevel A = Wn->L;
    ups_level_body<true>(A, Wn, gtx, s_in, s_tmp);
}

template <bool WIN>
__device__ __forceinline__ void ups_level_body(const DecLevel &A, const DecLevelWin *Wn, int gtx, int32_t *s_in,
                                               int32_t *s_tmp)
{
    // window form: tiles from the window's origin rounded down to even (the upsampling phase
    // of a tile row / column is its parity, as with the whole frame's multiples of 16 / 64)
    int y0 = (blockIdx.x / gtx) * kTY;
    int x0 = (blockIdx.x % gtx) * kTX;
    int dy0 = 0, dy1 = A.hd, dx0 = 0, dx1 = A.wd, dpitch = A.wd, ref_rows = A.hd;
    if (WIN) {
        dy0 = Wn->dy0, dy1 = Wn->dy1, dx0 = Wn->dx0, dx1 = Wn->dx1;
        dpitch = dx1 - dx0;
        ref_rows = Wn->ref_rows;
        y0 += dy0 & ~1;
        x0 += dx0 & ~1;
        if (y0 >= dy1 || x0 >= dx1) return;
    }
    const int tid = threadIdx.x;
    const int64_t dplane = WIN ? (int64_t)(dy1 - dy0) * dpitch : (int64_t)A.hd * A.wd;
    auto dst_ok = [&](int y, int x) { return WIN ? (y >= dy0 && y < dy1 && x >= dx0 && x < dx1) : (y < A.hd && x < A.wd); };
    auto dst_at = [&](int y, int x) { return WIN ? (int64_t)(y - dy0) * dpitch + (x - dx0) : (int64_t)y * A.wd + x; };

    // refine (ups_refine_cpu.hpp): zero padding, two passes with truncation, residual
    {
        const int pad = A.ks / 2;
        const int rh = kTY + 2 * pad, rw = kTX + 2 * pad, pitch = kTX + kMaxKs;
        for (int i = tid; i < rh * rw; i += kThreads) {
            const int r = i / rw, c = i - r * rw;
            const int y = y0 - pad + r, x = x0 - pad + c;
            s_in[r * pitch + c] = (y >= 0 && y < ref_rows && x >= 0 && x < A.wd) ? A.ref[y * A.wd + x] : 0;
        }
        __syncthreads();
        for (int i = tid; i < rh * kTX; i += kThreads) {
            const int r = i / kTX, c = i - r * kTX;
            const int y = y0 - pad + r;
            int32_t acc = 0;
            for (int k = 0; k < A.ks; ++k) acc += s_in[r * pitch + c + k] * A.kpre[k];
            // rows outside the plane are the zero padding of the vertical pass
            s_tmp[r * kTX + c] = (y >= 0 && y < A.hd) ? tshift(acc, kArmPrec) : 0;
        }
        __syncthreads();
        for (int i = tid; i < kTY * kTX; i += kThreads) {
            const int r = i / kTX, c = i - r * kTX;
            const int y = y0 + r, x = x0 + c;
            if (dst_ok(y, x)) {
                int32_t acc = 0;
                for (int k = 0; k < A.ks; ++k) acc += s_tmp[(r + k) * kTX + c] * A.kpre[k];
                acc += (int32_t)((uint32_t)s_in[(r + pad) * pitch + c + pad] << (kUpsPrec - kArmPrec) << kUpsPrec);
                A.dst[dst_at(y, x)] = tshift(acc, kUpsPrec);
            }
        }
        __syncthreads();
    }

    // 2x upsample of every source channel (ups_upsample_cpu.hpp): replicate padding,
    // horizontal pass >> src_prec into tmp (2*ws wide), vertical pass >> 12.
    const int ks = A.ksx2 / 2, pad = ks / 2;
    const int sy0 = y0 / 2 - pad, sx0 = x0 / 2 - pad;
    const int sh = kTY / 2 + ks, sw = kTX / 2 + ks, pitch = kTX / 2 + kMaxKs;
    for (int c = 0; c < A.C; ++c) {
        const int32_t *sp = A.src + (WIN ? (int64_t)c * Wn->splane : (int64_t)c * A.hs * A.ws);
        for (int i = tid; i < sh * sw; i += kThreads) {
            const int r = i / sw, cc = i - r * sw;
            if (WIN) {
                const int yy = min(max(sy0 + r, Wn->sy0), Wn->sy1), xx = min(max(sx0 + cc, Wn->sx0), Wn->sx1);
                s_in[r * pitch + cc] = sp[(int64_t)(yy - Wn->soy) * Wn->spitch + (xx - Wn->sox)];
            } else {
                s_in[r * pitch + cc] = sp[clampi(sy0 + r, A.hs - 1) * A.ws + clampi(sx0 + cc, A.ws - 1)];
            }
        }
        __syncthreads();
        for (int i = tid; i < sh * kTX; i += kThreads) {
            const int r = i / kTX, cc = i - r * kTX;
            const int X = x0 + cc, xs = X >> 1, ph = X & 1;
            int32_t acc = 0;
            for (int k = 0; k < ks; ++k) acc += s_in[r * pitch + (xs - pad + ph + k - sx0)] * A.kup[2 * k + ph];
            s_tmp[r * kTX + cc] = tshift(acc, A.src_prec);
        }
        __syncthreads();
        for (int i = tid; i < kTY * kTX; i += kThreads) {
            const int r = i / kTX, cc = i - r * kTX;
            const int Y = y0 + r, X = x0 + cc;
            if (dst_ok(Y, X)) {
                const int ys = Y >> 1, ph = Y & 1;
                int32_t acc = 0;
                for (int k = 0; k < ks; ++k) acc += s_tmp[(ys - pad + ph + k - sy0) * kTX + cc] * A.kup[2 * k + ph];
                A.dst[(int64_t)(c + 1) * dplane + dst_at(Y, X)] = tshift(acc, kUpsPrec);
            }
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------ synthesis (integer)
constexpr int kRW = 64, kRH = 32, kRegion = kRW * kRH;
constexpr int kMaxSp = 3;

struct DecSynFused {
    const int32_t *in;
    int cin, H, W;
    int hid;                // fused head width (always ReLU), output linear (synfused semantics)
    const int32_t *w0, *b0, *w1, *b1;
    int n_sp;
    const int32_t *wsp[kMaxSp], *bsp[kMaxSp];
    int res[kMaxSp], relu[kMaxSp];
    int32_t *out;
    int tiles_x;
    int f24; // DecSynArgs::f24
};

// Window form (region decode): the input holds the window [iy0, iy1] x [ix0, ix1] of the
// frame's level-0 stack, compact at pitch `ipitch` (the region grown by the 3x3 layers' reach,
// clipped to the frame); the output is the region [ry, ry + rh) x [rx, rx + rw), compact
// [3][rh][rw].  Every replicate clamp still uses the frame's true H and W (DecSynFused): a
// window edge that is not a frame edge is never padded.  Input reads are clamped to the stored
// window on top (only the surplus lanes of a tile ever fall outside it).
struct DecSynFusedWin {
    DecSynFused F;
    int iy0, iy1, ix0, ix1, ipitch;
    int64_t iplane;
    int ry, rx, rh, rw;
};

template <int CIN, int CMID, bool F24, bool WIN>
__device__ __forceinline__ void syn_fused_body(const DecSynFused &A, const DecSynFusedWin *Wn, int gtx,
                                               int32_t (*s_buf)[CMID][kRegion]);

template <int CIN, int CMID>
__global__ __launch_bounds__(kThreads) void dec_syn_fused(DecSynFused A)
{
    __shared__ __attribute__((aligned(16))) int32_t s_buf[2][CMID][kRegion];
    if (A.f24) syn_fused_body<CIN, CMID, true, false>(A, nullptr, A.tiles_x, s_buf);
    else syn_fused_body<CIN, CMID, false, false>(A, nullptr, A.tiles_x, s_buf);
}

template <int CIN, int CMID>
__global__ __launch_bounds__(kThreads) void dec_syn_fused_batch(const DecSynFused *__restrict__ As)
{
    __shared__ __attribute__((aligned(16))) int32_t s_buf[2][CMID][kRegion];
    // by reference: the frame's argument record is read with scalar loads where it is used (a
    // by-value copy with runtime-indexed layer arrays lived in scratch, 160 bytes per lane)
    const DecSynFused &A = As[blockIdx.y];
    if (A.f24) syn_fused_body<CIN, CMID, true, false>(A, nullptr, A.tiles_x, s_buf);
    else syn_fused_body<CIN, CMID, false, false>(A, nullptr, A.tiles_x, s_buf);
}

// region decode: blockIdx.y = frame, gtx tiles across (the group shares one region size)
template <int CIN, int CMID>
__global__ __launch_bounds__(kThreads) void dec_syn_fused_win_batch(const DecSynFusedWin *__restrict__ As, int gtx)
{
    __shared__ __attribute__((aligned(16))) int32_t s_buf[2][CMID][kRegion];
    const DecSynFusedWin *Wn = As + blockIdx.y;
    const DecSynFused &A = Wn->F;
    if (A.f24) syn_fused_body<CIN, CMID, true, true>(A, Wn, gtx, s_buf);
    else syn_fused_body<CIN, CMID, false, true>(A, Wn, gtx, s_buf);
}

template <int CIN, int CMID, bool F24, bool WIN>
__device__ __forceinline__ void syn_fused_body(const DecSynFused &A, const DecSynFusedWin *Wn, int gtx,
                                               int32_t (*s_buf)[CMID][kRegion])
{
    const int halo = A.n_sp;
    const int TX = kRW - 2 * halo, TY = kRH - 2 * halo;
    // frame coordinates throughout; the window form's tiles start at the region's origin
    const int y0 = (blockIdx.x / gtx) * TY + (WIN ? Wn->ry : 0), x0 = (blockIdx.x % gtx) * TX + (WIN ? Wn->rx : 0);
    // the exclusive end of what is written, and where sample (gy, gx) of output plane 0 goes
    const int ye = WIN ? Wn->ry + Wn->rh : A.H, xe = WIN ? Wn->rx + Wn->rw : A.W;
    if (WIN && (y0 >= ye || x0 >= xe)) return;
    const int oy = y0 - halo, ox = x0 - halo;
    const int64_t plane = WIN ? (int64_t)Wn->rh * Wn->rw : (int64_t)A.H * A.W;   // of the output
    const int64_t iplane = WIN ? Wn->iplane : (int64_t)A.H * A.W;                // of the input
    const int c = threadIdx.x & (kRW - 1), r0 = threadIdx.x >> 6;
    const int gx = ox + c, cxg = clampi(gx, A.W - 1);
    auto out_at = [&](int gy) { return WIN ? (int64_t)(gy - Wn->ry) * Wn->rw + (gx - Wn->rx) : (int64_t)gy * A.W + gx; };
    auto in_pix = [&](int yy) { // input sample at row yy (any), this lane's column
        if (WIN)
            return (int64_t)(min(max(yy, Wn->iy0), Wn->iy1) - Wn->iy0) * Wn->ipitch + (min(max(gx, Wn->ix0), Wn->ix1) - Wn->ix0);
        return (int64_t)clampi(yy, A.H - 1) * A.W + cxg;
    };

    // the head's weight records (w0[j][0..CIN), b0[j], w1[0..CMID)[j]; 12 ints) in the second
    // ping-pong buffer, which the first 3x3 layer writes only after its barrier: read back as
    // three broadcast ds_read_b128 per hidden unit, issued ahead of use (scalar weight loads
    // per unit made every unit wait for its own s_load round trip)
    static_assert(CIN + 1 + CMID <= 12, "head record");
    int32_t *s_rec = &s_buf[1][0][0];
    const int hid = A.hid;
    const bool recs = hid * 12 <= CMID * kRegion;
    if (recs) {
        for (int i = threadIdx.x; i < hid * 12; i += kThreads) {
            const int j = i / 12, f = i - j * 12;
            int32_t v = 0;
            if (f < CIN) v = A.w0[j * CIN + f];
            else if (f == CIN) v = A.b0[j];
            else if (f < CIN + 1 + CMID) v = A.w1[(f - CIN - 1) * hid + j];
            s_rec[i] = v;
        }
        __syncthreads();
    }
    auto store_head = [&](int r, const int32_t (&o)[CMID]) {
        const int gy = oy + r;
#pragma unroll
        for (int m = 0; m < CMID; ++m) {
            const int32_t v = tshift(o[m], kSynPrec);
            if (halo == 0) {
                if (gy < ye && gx < xe) A.out[m * plane + out_at(gy)] = v;
            } else {
                s_buf[0][m][r * kRW + c] = v;
            }
        }
    };
    if (recs) {
        // two rows (r, r + 4) per pass over the records
        typedef int i4v __attribute__((ext_vector_type(4)));
        typedef const __attribute__((address_space(3))) i4v *lds_i4;
        lds_i4 rb = (lds_i4)s_rec;
        for (int r = r0; r < kRH; r += 8) {
            int32_t x[2][CIN], o[2][CMID];
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                const int64_t pix = in_pix(oy + r + 4 * p);
#pragma unroll
                for (int k = 0; k < CIN; ++k) x[p][k] = A.in[k * iplane + pix];
#pragma unroll
                for (int m = 0; m < CMID; ++m) o[p][m] = A.b1[m];
            }
#pragma unroll 2
            for (int j = 0; j < hid; ++j) {
                const i4v q0 = rb[3 * j], q1 = rb[3 * j + 1], q2 = rb[3 * j + 2];
                const int32_t w[12] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w};
#pragma unroll
                for (int p = 0; p < 2; ++p) {
                    int32_t acc = w[CIN];
#pragma unroll
                    for (int k = 0; k < CIN; ++k) acc += imul<F24>(x[p][k], w[k]);
                    acc = acc < 0 ? 0 : acc >> kSynPrec;
#pragma unroll
                    for (int m = 0; m < CMID; ++m) o[p][m] += imul<F24>(acc, w[CIN + 1 + m]);
                }
            }
            store_head(r, o[0]);
            store_head(r + 4, o[1]);
        }
    } else {
        for (int r = r0; r < kRH; r += 4) {
            const int64_t pix = in_pix(oy + r);
            int32_t x[CIN];
#pragma unroll
            for (int k = 0; k < CIN; ++k) x[k] = A.in[k * iplane + pix];
            int32_t o[CMID];
#pragma unroll
            for (int m = 0; m < CMID; ++m) o[m] = A.b1[m];
            for (int j = 0; j < hid; ++j) {
                int32_t acc = A.b0[j];
#pragma unroll
                for (int k = 0; k < CIN; ++k) acc += imul<F24>(x[k], A.w0[j * CIN + k]);
                acc = acc < 0 ? 0 : acc >> kSynPrec;
#pragma unroll
                for (int m = 0; m < CMID; ++m) o[m] += imul<F24>(acc, A.w1[m * hid + j]);
            }
            store_head(r, o);
        }
    }
    if (halo == 0) return;

    int cur = 0;
    for (int s = 0; s < A.n_sp; ++s) {
        __syncthreads();
        const int t = s + 1;
        const bool last = s == A.n_sp - 1;
        const int32_t *wt = A.wsp[s], *bs = A.bsp[s];
        const bool col_ok = c >= t && c < kRW - t;
        int lx[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) lx[d] = clampi(cxg + d - 1, A.W - 1) - ox;
        for (int r = r0 + t; r < kRH - t; r += 4) {
            const int gy = oy + r;
            if (!col_ok || (last && (gy >= ye || gx >= xe))) continue;
            const int cyg = clampi(gy, A.H - 1);
            int ly[3];
#pragma unroll
            for (int d = 0; d < 3; ++d) ly[d] = (clampi(cyg + d - 1, A.H - 1) - oy) * kRW;
            int32_t nb[CMID][3][3];
#pragma unroll
            for (int k = 0; k < CMID; ++k)
#pragma unroll
                for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                    for (int dx = 0; dx < 3; ++dx) nb[k][dy][dx] = s_buf[cur][k][ly[dy] + lx[dx]];
#pragma unroll
            for (int m = 0; m < CMID; ++m) {
                int32_t acc = bs[m];
                if (A.res[s]) acc += (int32_t)((uint32_t)nb[m][1][1] << kSynPrec);
#pragma unroll
                for (int k = 0; k < CMID; ++k)
#pragma unroll
                    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                        for (int dx = 0; dx < 3; ++dx) acc += imul<F24>(nb[k][dy][dx], wt[((m * CMID + k) * 3 + dy) * 3 + dx]);
                const int32_t v = acc < 0 ? (A.relu[s] ? 0 : -((-acc) >> kSynPrec)) : acc >> kSynPrec;
                if (last)
                    A.out[m * plane + out_at(gy)] = v;
                else
                    s_buf[cur ^ 1][m][r * kRW + c] = v;
            }
        }
        cur ^= 1;
    }
}

// generic integer conv layer (syn_cpu.hpp semantics, out-of-place, replicate padding).
// fused_hidden > 0: this launch is the fused 1x1 pair with that hidden width.
__global__ __launch_bounds__(kThreads) void dec_syn_layer(const int32_t *__restrict__ in, int cin, int H, int W,
                                                          const int32_t *__restrict__ wt,
                                                          const int32_t *__restrict__ bs, int nout, int ks,
                                                          int residual, int relu, int32_t *__restrict__ out)
{
    const int64_t plane = (int64_t)H * W;
    const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (p >= plane) return;
    const int y = (int)(p / W), x = (int)(p - (int64_t)y * W);
    const int pad = ks / 2;
    for (int m = 0; m < nout; ++m) {
        int32_t acc = bs[m];
        if (residual) acc += (int32_t)((uint32_t)in[m * plane + p] << kSynPrec);
        for (int k = 0; k < cin; ++k)
            for (int dy = 0; dy < ks; ++dy) {
                const int yy = clampi(y + dy - pad, H - 1);
                for (int dx = 0; dx < ks; ++dx)
                    acc += in[k * plane + (int64_t)yy * W + clampi(x + dx - pad, W - 1)] *
                           wt[((m * cin + k) * ks + dy) * ks + dx];
            }
        out[m * plane + p] = acc < 0 ? (relu ? 0 : -((-acc) >> kSynPrec)) : acc >> kSynPrec;
    }
}

__global__ __launch_bounds__(kThreads) void dec_syn_fused_generic(const int32_t *__restrict__ in, int cin, int64_t plane,
                                                                  const int32_t *__restrict__ w0,
                                                                  const int32_t *__restrict__ b0, int hid,
                                                                  const int32_t *__restrict__ w1,
                                                                  const int32_t *__restrict__ b1, int nout,
                                                                  int32_t *__restrict__ out)
{
    const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (p >= plane) return;
    for (int m = 0; m < nout; ++m) {
        int32_t o = b1[m];
        for (int j = 0; j < hid; ++j) {
            int32_t acc = b0[j];
            for (int k = 0; k < cin; ++k) acc += in[k * plane + p] * w0[j * cin + k];
            acc = acc < 0 ? 0 : acc >> kSynPrec;
            o += acc * w1[m * hid + j];
        }
        out[m * plane + p] = tshift(o, kSynPrec);
    }
}

__global__ __launch_bounds__(kThreads) void dec_blend_kernel(int32_t *acc, const int32_t *x, int64_t n, int32_t b_acc,
                                                             int32_t b_x, int first)
{
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    auto cl = [](int32_t v) { return v < 0 ? 0 : (v > (1 << kSynPrec) ? (1 << kSynPrec) : v); };
    const int32_t x0 = cl(x[i]);
    if (first) acc[i] = (cl(acc[i]) * b_acc + x0 * b_x) >> kSynPrec;
    else acc[i] = acc[i] + ((x0 * b_x) >> kSynPrec);
}

// ------------------------------------------------------------------ output bytes
struct DecOut {
    const int32_t *syn;
    int H, W, maxv, kind, bps;
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
    output_body(O.syn, O.H, O.W, O.maxv, O.kind, O.bps, O.dst);
}

__device__ __forceinline__ void output_body(const int32_t *__restrict__ syn, int H, int W, int maxv, int kind, int bps,
                                            uint8_t *__restrict__ dst)
{
    const int64_t plane = (int64_t)H * W;
    const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (p >= plane) return;
    auto smp = [maxv](int32_t v) {
        int32_t s = (v * maxv + (1 << (kSynPrec - 1))) >> kSynPrec;
        return s < 0 ? 0 : (s > maxv ? maxv : s);
    };
    auto put = [&](int64_t idx, int32_t s, bool big_endian) {
        if (bps == 1) dst[idx] = (uint8_t)s;
        else if (big_endian) { dst[2 * idx] = (uint8_t)(s >> 8); dst[2 * idx + 1] = (uint8_t)s; }
        else { dst[2 * idx] = (uint8_t)s; dst[2 * idx + 1] = (uint8_t)(s >> 8); }
    };
    const int y = (int)(p / W), x = (int)(p - (int64_t)y * W);
    if (kind == 2) { // PPM: interleaved RGB, 16-bit big endian
        for (int c = 0; c < 3; ++c) put(3 * p + c, smp(syn[c * plane + p]), true);
        return;
    }
    put(p, smp(syn[p]), false);
    if (kind == 1) {
        put(plane + p, smp(syn[plane + p]), false);
        put(2 * plane + p, smp(syn[2 * plane + p]), false);
    } else if (!(y & 1) && !(x & 1) && (y >> 1) < H / 2 && (x >> 1) < W / 2) {
        const int64_t cp = (int64_t)(H / 2) * (W / 2), ci = (int64_t)(y >> 1) * (W / 2) + (x >> 1);
        put(plane + ci, smp(syn[plane + p]), false);
        put(plane + cp + ci, smp(syn[2 * plane + p]), false);
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
// samples too, which the byte path writes one byte per thread.  DecOut::bps is unused here
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
    auto smp = [maxv](int32_t v) {
        int32_t s = (v * maxv + (1 << (kSynPrec - 1))) >> kSynPrec;
        return s < 0 ? 0 : (s > maxv ? maxv : s);
    };
    T v[4];
    if (j0 >= 0 && j0 + 4 <= direct) { // the common case: 4 samples of the flat prefix
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = out_sample<T>(smp(syn[direct_at(j0 + k)]), fmax);
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
                v[k] = out_sample<T>(smp(syn[direct_at(j)]), fmax);
                continue;
            }
            v[k] = out_sample<T>(smp(syn[CROP ? (1 + c) * splane + (int64_t)(oy + 2 * cy) * spitch + ox + 2 * cx
                                              : (1 + c) * plane + (int64_t)(2 * cy) * W + 2 * cx]),
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
//
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

// the float32 roundings of yuv2rgb's matrix (ccmi/io.py) and of its offsets / 255: R, G, B
__device__ constexpr float kFmtA[3] = {(float)-0.000007154783816076815, (float)-0.3441331386566162, (float)1.7720025777816772};
__device__ constexpr float kFmtB[3] = {(float)1.4019975662231445, (float)-0.7141380310058594, (float)0.00001542569043522235};
__device__ constexpr float kFmtO[3] = {(float)(-179.45477266423404 / 255.0), (float)(135.45870971679688 / 255.0),
                                       (float)(-226.8183044444304 / 255.0)};

struct DecFmtCall { // one value per launch
    float scale[3], bias[3];
    int64_t sc, sy, sx;
};
enum { kFmtMirror = 1, kFmtMatrix = 2 }; // per-frame flags (DecOut::bps of a formatted group)

// groups of 4 destination pixels that cover one row plus the up to 3 lead-in slots
__host__ __device__ inline int fmt_row_groups(int w) { return (w + 3 + 3) / 4; }

// steps 1-3 of the contract for one pixel: lrow / crow point at the pixel's luma row and at the
// row its chroma is taken from, x / xc are its luma and chroma columns
__device__ __forceinline__ void fmt_pixel(const int32_t *__restrict__ lrow, const int32_t *__restrict__ crow,
                                          int64_t splane, int x, int xc, int maxv, float fmax, bool matrix, float (&q)[3])
{
    auto smp = [maxv, fmax](int32_t v) {
        int32_t s = (v * maxv + (1 << (kSynPrec - 1))) >> kSynPrec;
        s = s < 0 ? 0 : (s > maxv ? maxv : s);
        return __fdiv_rn((float)s, fmax);
    };
    const float p0 = smp(lrow[x]), p1 = smp(crow[splane + xc]), p2 = smp(crow[2 * splane + xc]);
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

// the thread's row y and first destination pixel d0 of a w-wide row (see above); false: no work
template <typename T>
__device__ __forceinline__ bool fmt_group(const T *dst, const DecFmtCall &C, int h, int w, int &y, int &d0, int64_t &row,
                                          bool &nchw, bool &nhwc)
{
    const int gpr = fmt_row_groups(w);
    const int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    y = (int)(g / gpr);
    if (y >= h) return false;
    nchw = C.sx == 1, nhwc = !nchw && C.sc == 1 && C.sx == 3;
    row = (int64_t)y * C.sy;
    // elements from address 0 to (channel 0, y, x' = 0); group k starts mis slots before it, where
    // the address of its first pixel is a multiple of 4 elements (NHWC: 3 mis == a0 mod 4)
    const uint64_t a0 = (uint64_t)(reinterpret_cast<uintptr_t>(dst) / sizeof(T)) + (uint64_t)row;
    const int mis = nchw ? (int)(a0 & 3) : nhwc ? (int)((3 * a0) & 3) : 0;
    d0 = 4 * (int)(g - (int64_t)y * gpr) - mis;
    return d0 < w;
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

template <typename T>
__global__ __launch_bounds__(kThreads) void dec_output_fmt(const int32_t *__restrict__ syn, int H, int W, int oy, int ox,
                                                           int h, int w, int maxv, int kind, int flags,
                                                           T *__restrict__ dst, DecFmtCall C)
{
    output_fmt_body<T>(syn, (int64_t)H * W, W, oy, ox, h, w, maxv, kind, flags, dst, C);
}

// the colour forms (ccmi_colour): K = the frame's ops; the statistics pass of a frame with a contrast op
template <typename T>
__global__ __launch_bounds__(kThreads) void dec_output_fmt_col(const int32_t *__restrict__ syn, int H, int W, int oy, int ox,
                                                               int h, int w, int maxv, int kind, int flags,
                                                               T *__restrict__ dst, DecFmtCall C, DecCol K)
{
    output_fmt_body<T, kColWrite>(syn, (int64_t)H * W, W, oy, ox, h, w, maxv, kind, flags, dst, C, &K);
}

__global__ __launch_bounds__(kThreads) void dec_output_fmt_stat(const int32_t *__restrict__ syn, int H, int W, int oy, int ox,
                                                                int h, int w, int maxv, int kind, int flags, DecCol K)
{
    col_accumulate(K, output_fmt_body<float, kColStat>(syn, (int64_t)H * W, W, oy, ox, h, w, maxv, kind, flags, nullptr,
                                                       col_stat_call(), &K));
}

// a tail group: frame blockIdx.y's compact H x W synthesis output (DecOut::bps = its kFmt* flags)
template <typename T>
__global__ __launch_bounds__(kThreads) void dec_output_fmt_batch(const DecOut *__restrict__ Os, DecFmtCall C)
{
    const DecOut O = Os[blockIdx.y];
    output_fmt_body<T>(O.syn, (int64_t)O.H * O.W, O.W, 0, 0, O.H, O.W, O.maxv, O.kind, O.bps, reinterpret_cast<T *>(O.dst),
                       C);
}

// the colour forms of a tail group: Ks = the group's op tables, one per frame
template <typename T>
__global__ __launch_bounds__(kThreads) void dec_output_fmt_col_batch(const DecOut *__restrict__ Os, DecFmtCall C,
                                                                     const DecCol *__restrict__ Ks)
{
    const DecOut O = Os[blockIdx.y];
    output_fmt_body<T, kColWrite>(O.syn, (int64_t)O.H * O.W, O.W, 0, 0, O.H, O.W, O.maxv, O.kind, O.bps,
                                  reinterpret_cast<T *>(O.dst), C, Ks + blockIdx.y);
}

// only the frames with a contrast op take part
__global__ __launch_bounds__(kThreads) void dec_output_fmt_stat_batch(const DecOut *__restrict__ Os,
                                                                      const DecCol *__restrict__ Ks)
{
    const DecCol &K = Ks[blockIdx.y];
    if (K.contrast < 0) return;
    const DecOut O = Os[blockIdx.y];
    col_accumulate(K, output_fmt_body<float, kColStat>(O.syn, (int64_t)O.H * O.W, O.W, 0, 0, O.H, O.W, O.maxv, O.kind, O.bps,
                                                       nullptr, col_stat_call(), &K));
}

unsigned output_fmt_blocks(int h, int w)
{
    return (unsigned)(((int64_t)h * fmt_row_groups(w) + kThreads - 1) / kThreads);
}

DecFmtCall fmt_call(const DecFmt &f)
{
    DecFmtCall C;
    for (int c = 0; c < 3; ++c) C.scale[c] = f.scale[c], C.bias[c] = f.bias[c];
    C.sc = f.stride_c, C.sy = f.stride_y, C.sx = f.stride_x;
    return C;
}

int fmt_flags(const DecFmt &f) { return (f.mirror ? kFmtMirror : 0) | (f.matrix ? kFmtMatrix : 0); }

// ------------------------------------------------------------------ resampled formatted output
// The formatted sink with a ccmi_resample (steps 3a-3c of the contract in ccmi.h): the region,
// h x w, goes through an antialiased triangle filter to oh x ow between the colour step and
// scale / bias.  Two launches:
//   dec_resample_h     thread = (region row y, output column i), three channels: q per tap from
//                      the synthesis output, t[c][y][i] (float32, [3][h][ow]) to the workspace;
//   dec_resample_v<T>  thread = (output row, 4 destination pixels), as the formatted output stage:
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

// one frame of a resampling group: DecOut as for dec_output_fmt_batch (H x W = the region, compact)
struct DecOutRs {
    DecOut o;
    float *tmp;
};

// h x w = the region at (oy, ox) of the synthesis output, as for output_fmt_body
__device__ __forceinline__ void resample_h_body(const int32_t *__restrict__ syn, int64_t splane, int spitch, int oy, int ox,
                                                int h, int w, int ow, int maxv, int kind, int flags,
                                                float *__restrict__ tmp)
{
    const int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int y = (int)(g / ow);
    if (y >= h) return;
    const int i = (int)(g - (int64_t)y * ow);
    const RsTaps T = rs_taps(i, w, ow);
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
template <typename T, int COL = kColNone>
__device__ __forceinline__ uint32_t resample_v_body(const float *__restrict__ tmp, int h, int oh, int ow, int flags,
                                                    T *__restrict__ dst, const DecFmtCall &C, const DecCol *K = nullptr)
{
    int y, d0;
    int64_t row;
    bool nchw, nhwc;
    if (!fmt_group<T>(dst, C, oh, ow, y, d0, row, nchw, nhwc)) return 0;
    const RsTaps R = rs_taps(y, h, oh);
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

__global__ __launch_bounds__(kThreads) void dec_resample_h(const int32_t *__restrict__ syn, int H, int W, int oy, int ox,
                                                           int h, int w, int ow, int maxv, int kind, int flags,
                                                           float *__restrict__ tmp)
{
    resample_h_body(syn, (int64_t)H * W, W, oy, ox, h, w, ow, maxv, kind, flags, tmp);
}

template <typename T>
__global__ __launch_bounds__(kThreads) void dec_resample_v(const float *__restrict__ tmp, int h, int oh, int ow, int flags,
                                                           T *__restrict__ dst, DecFmtCall C)
{
    resample_v_body<T>(tmp, h, oh, ow, flags, dst, C);
}

template <typename T>
__global__ __launch_bounds__(kThreads) void dec_resample_v_col(const float *__restrict__ tmp, int h, int oh, int ow,
                                                               int flags, T *__restrict__ dst, DecFmtCall C, DecCol K)
{
    resample_v_body<T, kColWrite>(tmp, h, oh, ow, flags, dst, C, &K);
}

__global__ __launch_bounds__(kThreads) void dec_resample_v_stat(const float *__restrict__ tmp, int h, int oh, int ow,
                                                                int flags, DecCol K)
{
    col_accumulate(K, resample_v_body<float, kColStat>(tmp, h, oh, ow, flags, nullptr, col_stat_call(), &K));
}

// a tail group: frame blockIdx.y's compact region; the grid covers the group's largest region
__global__ __launch_bounds__(kThreads) void dec_resample_h_batch(const DecOutRs *__restrict__ Os, int ow)
{
    const DecOutRs R = Os[blockIdx.y];
    const DecOut &O = R.o;
    resample_h_body(O.syn, (int64_t)O.H * O.W, O.W, 0, 0, O.H, O.W, ow, O.maxv, O.kind, O.bps, R.tmp);
}

template <typename T>
__global__ __launch_bounds__(kThreads) void dec_resample_v_batch(const DecOutRs *__restrict__ Os, int oh, int ow,
                                                                 DecFmtCall C)
{
    const DecOutRs R = Os[blockIdx.y];
    resample_v_body<T>(R.tmp, R.o.H, oh, ow, R.o.bps, reinterpret_cast<T *>(R.o.dst), C);
}

template <typename T>
__global__ __launch_bounds__(kThreads) void dec_resample_v_col_batch(const DecOutRs *__restrict__ Os, int oh, int ow,
                                                                     DecFmtCall C, const DecCol *__restrict__ Ks)
{
    const DecOutRs R = Os[blockIdx.y];
    resample_v_body<T, kColWrite>(R.tmp, R.o.H, oh, ow, R.o.bps, reinterpret_cast<T *>(R.o.dst), C, Ks + blockIdx.y);
}

__global__ __launch_bounds__(kThreads) void dec_resample_v_stat_batch(const DecOutRs *__restrict__ Os, int oh, int ow,
                                                                      const DecCol *__restrict__ Ks)
{
    const DecCol &K = Ks[blockIdx.y];
    if (K.contrast < 0) return;
    const DecOutRs R = Os[blockIdx.y];
    col_accumulate(K, resample_v_body<float, kColStat>(R.tmp, R.o.H, oh, ow, R.o.bps, nullptr, col_stat_call(), &K));
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

// one frame of a warping group: DecOut as for dec_output_fmt_batch (H x W = the window, compact)
struct DecOutWarp {
    DecOut o;
    float m[6];
    int oy, ox, fh, fw; // the window's origin in the frame, and the frame
};

template <typename T, int COL = kColNone>
__device__ __forceinline__ uint32_t warp_body(const int32_t *__restrict__ syn, int h, int w, int oy, int ox, int fh, int fw,
                                              const float (&m)[6], int maxv, int kind, int flags, T *__restrict__ dst,
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
    T v[3][4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int d = d0 + k;
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c][k] = fmt_elem<T>(0.f);
        if (d < 0 || d >= Wc.ow) continue;
        const float cx = (float)(mirror ? Wc.ow - 1 - d : d) + 0.5f;
        const float xs = fmt_add(fmt_add(fmt_mul(m[0], cx), xr), m[2]);
        const float ys = fmt_add(fmt_add(fmt_mul(m[3], cx), yr), m[5]);
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

// one frame (DecOut::bps = its kFmt* flags): the per-frame tail's, A.o = the whole synthesis output
template <typename T>
__global__ __launch_bounds__(kThreads) void dec_warp(DecOutWarp A, DecFmtCall C, DecWarpCall Wc)
{
    warp_body<T>(A.o.syn, A.o.H, A.o.W, A.oy, A.ox, A.fh, A.fw, A.m, A.o.maxv, A.o.kind, A.o.bps,
                 reinterpret_cast<T *>(A.o.dst), C, Wc);
}

// a tail group: frame blockIdx.y's compact window
template <typename T>
__global__ __launch_bounds__(kThreads) void dec_warp_batch(const DecOutWarp *__restrict__ Os, DecFmtCall C, DecWarpCall Wc)
{
    const DecOutWarp A = Os[blockIdx.y];
    warp_body<T>(A.o.syn, A.o.H, A.o.W, A.oy, A.ox, A.fh, A.fw, A.m, A.o.maxv, A.o.kind, A.o.bps,
                 reinterpret_cast<T *>(A.o.dst), C, Wc);
}

template <typename T>
__global__ __launch_bounds__(kThreads) void dec_warp_col(DecOutWarp A, DecFmtCall C, DecWarpCall Wc, DecCol K)
{
    warp_body<T, kColWrite>(A.o.syn, A.o.H, A.o.W, A.oy, A.ox, A.fh, A.fw, A.m, A.o.maxv, A.o.kind, A.o.bps,
                            reinterpret_cast<T *>(A.o.dst), C, Wc, &K);
}

__global__ __launch_bounds__(kThreads) void dec_warp_stat(DecOutWarp A, DecWarpCall Wc, DecCol K)
{
    col_accumulate(K, warp_body<float, kColStat>(A.o.syn, A.o.H, A.o.W, A.oy, A.ox, A.fh, A.fw, A.m, A.o.maxv, A.o.kind,
                                                 A.o.bps, nullptr, col_stat_call(), Wc, &K));
}

template <typename T>
__global__ __launch_bounds__(kThreads) void dec_warp_col_batch(const DecOutWarp *__restrict__ Os, DecFmtCall C, DecWarpCall Wc,
                                                               const DecCol *__restrict__ Ks)
{
    const DecOutWarp A = Os[blockIdx.y];
    warp_body<T, kColWrite>(A.o.syn, A.o.H, A.o.W, A.oy, A.ox, A.fh, A.fw, A.m, A.o.maxv, A.o.kind, A.o.bps,
                            reinterpret_cast<T *>(A.o.dst), C, Wc, Ks + blockIdx.y);
}

__global__ __launch_bounds__(kThreads) void dec_warp_stat_batch(const DecOutWarp *__restrict__ Os, DecWarpCall Wc,
                                                                const DecCol *__restrict__ Ks)
{
    const DecCol &K = Ks[blockIdx.y];
    if (K.contrast < 0) return;
    const DecOutWarp A = Os[blockIdx.y];
    col_accumulate(K, warp_body<float, kColStat>(A.o.syn, A.o.H, A.o.W, A.oy, A.ox, A.fh, A.fw, A.m, A.o.maxv, A.o.kind,
                                                 A.o.bps, nullptr, col_stat_call(), Wc, &K));
}

DecWarpCall warp_call(const DecFmt &f)
{
    DecWarpCall Wc;
    Wc.oh = f.out_h, Wc.ow = f.out_w, Wc.pad = f.pad;
    for (int c = 0; c < 3; ++c) Wc.fill[c] = f.fill[c];
    return Wc;
}

} // namespace

size_t dec_ups_workspace_elems(const int *lh, const int *lw, int L)
{
    size_t n = 0;
    for (int k = 1; k <= L - 2; ++k) n += (size_t)(L - k) * lh[k] * lw[k];
    return n;
}

static bool ups_ks_ok(const DecUpsArgs &a)
{
    return a.ups_ks >= 2 && a.ups_ks <= kMaxKs && a.pre_ks >= 1 && a.pre_ks <= kMaxKs - 1;
}

// kernel arguments of every pyramid step of one frame (coarsest first); returns the step count.
// The stacks of levels 1..L-2 follow one another in the workspace: whole planes, or with
// `win` the windows win->lev[k], compact.
static int make_levels(const DecUpsArgs &a, DecLevel *lv, const DecRoi *win = nullptr)
{
    const int L = a.n_layers;
    int32_t *stack[CCMI_MAX_GRIDS] = {};
    int32_t *ws = a.workspace;
    for (int k = 1; k <= L - 2; ++k) {
        stack[k] = ws;
        ws += win ? (size_t)(L - k) * win->lev[k].h() * win->lev[k].w() : (size_t)(L - k) * a.lh[k] * a.lw[k];
    }
    for (int step = 0; step < L - 1; ++step) {
        const int k = L - 1 - step;
        DecLevel &A = lv[step];
        A = DecLevel{};
        A.src = k == L - 1 ? a.lat + a.off[k] : stack[k];
        A.C = L - k;
        A.hs = a.lh[k];
        A.ws = a.lw[k];
        A.src_prec = k == L - 1 ? kArmPrec : kUpsPrec;
        A.ref = a.lat + a.off[k - 1];
        A.dst = k - 1 == 0 ? a.out : stack[k - 1];
        A.hd = a.lh[k - 1];
        A.wd = a.lw[k - 1];
        // reference indices: ups layer (L-2-target)%n_ups, preconcat (L-2-layer)%n_pre; target = layer = k-1
        A.kup = a.kernels + ((L - 2 - (k - 1)) % a.n_ups) * a.ups_ks;
        A.ksx2 = a.ups_ks;
        A.kpre = a.kernels + a.n_ups * a.ups_ks + ((L - 2 - (k - 1)) % a.n_pre) * a.pre_ks;
        A.ks = a.pre_ks;
        A.tiles_x = ccmi_div_up(A.wd, kTX);
    }
    return L > 1 ? L - 1 : 0;
}

// The windows a region needs, finest level first, from the taps of ups_level_body and
// syn_fused_body.  A destination row Y of a pyramid step reads source rows
// (Y >> 1) - pad + (Y & 1) .. + ks - 1 (ks = ups_ks / 2 taps per phase, pad = ks / 2), clamped
// to the plane; the refined channel of a level reads its latent grid pre_ks / 2 rows either
// side, zero outside the plane.  Columns alike.
void dec_roi_plan(const int *lh, const int *lw, int L, int ups_ks, int pre_ks, int syn_halo, const DecWindow &rect,
                  DecRoi &r)
{
    r = DecRoi{};
    r.rect = rect;
    r.lev[0] = DecWindow{std::max(0, rect.y0 - syn_halo), std::min(lh[0], rect.y1 + syn_halo),
                         std::max(0, rect.x0 - syn_halo), std::min(lw[0], rect.x1 + syn_halo)};
    const int ks = ups_ks / 2, pad = ks / 2;
    auto lo = [&](int a) { return std::max(0, (a >> 1) - pad + (a & 1)); };
    auto hi = [&](int b, int n) { return std::min(n, ((b - 1) >> 1) + ((b - 1) & 1) - pad + ks); };
    for (int k = 1; k < L; ++k) {
        const DecWindow &d = r.lev[k - 1];
        r.lev[k] = DecWindow{lo(d.y0), hi(d.y1, lh[k]), lo(d.x0), hi(d.x1, lw[k])};
    }
    for (int l = 0; l < L; ++l) r.arm_rows[l] = l == L - 1 ? r.lev[l].y1 : std::min(lh[l], r.lev[l].y1 + pre_ks / 2);
    // What is read of each latent plane: the refine's taps around lev[l] (its tile loads reach
    // further, but those lanes' results are discarded); the coarsest plane is the raw source of
    // the first step, whose reads are clamped to lev[L-1].
    const int rp = pre_ks / 2;
    for (int l = 0; l < L; ++l) {
        const DecWindow &d = r.lev[l];
        r.lat[l] = l == L - 1 ? d
                              : DecWindow{std::max(0, d.y0 - rp), std::min(lh[l], d.y1 + rp), std::max(0, d.x0 - rp),
                                          std::min(lw[l], d.x1 + rp)};
    }
}

size_t dec_ups_workspace_elems_win(const DecRoi &r, int L)
{
    size_t n = 0;
    for (int k = 1; k <= L - 2; ++k) n += (size_t)(L - k) * r.lev[k].h() * r.lev[k].w();
    return n;
}

// window-form arguments of every pyramid step of one frame (coarsest first)
static int make_levels_win(const DecTailFrame &f, DecLevelWin *lv)
{
    const DecUpsArgs &a = f.ups;
    const DecRoi &R = f.roi;
    const int L = a.n_layers;
    DecLevel base[CCMI_MAX_GRIDS];
    const int steps = make_levels(a, base, &R); // src / dst: the window stacks
    for (int step = 0; step < steps; ++step) {
        const int k = L - 1 - step;
        DecLevelWin &Wn = lv[step];
        Wn = DecLevelWin{};
        Wn.L = base[step];
        const DecWindow &sw = R.lev[k], &dw = R.lev[k - 1];
        const bool raw = k == L - 1; // the coarsest latent plane itself: frame pitch, origin 0
        Wn.dy0 = dw.y0, Wn.dy1 = dw.y1, Wn.dx0 = dw.x0, Wn.dx1 = dw.x1;
        Wn.soy = raw ? 0 : sw.y0;
        Wn.sox = raw ? 0 : sw.x0;
        Wn.spitch = raw ? a.lw[k] : sw.w();
        Wn.splane = (int64_t)sw.h() * sw.w();
        Wn.sy0 = sw.y0, Wn.sy1 = sw.y1 - 1, Wn.sx0 = sw.x0, Wn.sx1 = sw.x1 - 1;
        Wn.ref_rows = R.arm_rows[k - 1];
    }
    return steps;
}

int launch_dec_ups(const DecUpsArgs &a, hipStream_t s)
{
    if (!ups_ks_ok(a))
        return ccmi_set_error(CCMI_ERR_UNSUPPORTED, "dec: upsampling kernel sizes %d/%d", a.ups_ks, a.pre_ks);
    DecLevel lv[CCMI_MAX_GRIDS];
    const int steps = make_levels(a, lv);
    for (int step = 0; step < steps; ++step) {
        const DecLevel &A = lv[step];
        hipLaunchKernelGGL(dec_ups_level, dim3(A.tiles_x * ccmi_div_up(A.hd, kTY)), dim3(kThreads), 0, s, A);
        CCMI_HIP_CHECK(hipGetLastError());
    }
    return CCMI_OK;
}

static int syn_maxc(const DecSynArgs &a)
{
    int m = a.c_in;
    for (int l = 0; l < a.n_layers; ++l) m = a.layers[l].n_out > m ? a.layers[l].n_out : m;
    return m;
}

static bool syn_fast(const DecSynArgs &a, int *cmid)
{
    if (a.n_layers < 2 || a.layers[0].ks != 1 || a.layers[1].ks != 1) return false;
    if (a.c_in < 1 || a.c_in > 8) return false;
    const int cm = a.layers[1].n_out;
    if (cm != 3) return false;
    if (a.n_layers - 2 > kMaxSp) return false;
    for (int l = 2; l < a.n_layers; ++l)
        if (a.layers[l].ks != 3 || a.layers[l].n_out != cm) return false;
    *cmid = cm;
    return true;
}

size_t dec_syn_workspace_elems(const DecSynArgs &a)
{
    int cm;
    if (syn_fast(a, &cm)) return 0;
    return 2 * (size_t)syn_maxc(a) * a.h * a.w;
}

// weight offsets of one branch (per layer W then b) and each layer's input width
static void syn_params(const DecSynArgs &a, const int32_t **wp, const int32_t **bp, int *cin_of)
{
    const int32_t *q = a.params;
    int c = a.c_in;
    for (int l = 0; l < a.n_layers; ++l) {
        cin_of[l] = c;
        wp[l] = q;
        q += (size_t)a.layers[l].n_out * c * a.layers[l].ks * a.layers[l].ks;
        bp[l] = q;
        q += a.layers[l].n_out;
        c = a.layers[l].n_out;
    }
}

// fused-synthesis kernel arguments of one frame (syn_fast architectures only)
static DecSynFused make_syn_fused(const DecSynArgs &a)
{
    const int32_t *wp[CCMI_MAX_SYN_LAYERS], *bp[CCMI_MAX_SYN_LAYERS];
    int cin_of[CCMI_MAX_SYN_LAYERS];
    syn_params(a, wp, bp, cin_of);
    DecSynFused F{};
    F.in = a.in;
    F.cin = a.c_in;
    F.H = a.h;
    F.W = a.w;
    F.hid = a.layers[0].n_out;
    F.w0 = wp[0];
    F.b0 = bp[0];
    F.w1 = wp[1];
    F.b1 = bp[1];
    F.n_sp = a.n_layers - 2;
    for (int i = 0; i < F.n_sp; ++i) {
        F.wsp[i] = wp[2 + i];
        F.bsp[i] = bp[2 + i];
        F.res[i] = a.layers[2 + i].residual;
        F.relu[i] = a.layers[2 + i].relu;
    }
    F.out = a.out;
    F.f24 = a.f24;
    F.tiles_x = ccmi_div_up(a.w, kRW - 2 * F.n_sp);
    return F;
}

// launch(std::integral_constant<int, CIN>) for the <CIN, 3> instantiation of a fused-synthesis
// kernel form (single, batch, window batch); syn_fast admits c_in 1..8
template <typename Launch>
static void with_syn_cin(int c_in, Launch &&launch)
{
    switch (c_in) {
    case 1: launch(std::integral_constant<int, 1>{}); break;
    case 2: launch(std::integral_constant<int, 2>{}); break;
    case 3: launch(std::integral_constant<int, 3>{}); break;
    case 4: launch(std::integral_constant<int, 4>{}); break;
    case 5: launch(std::integral_constant<int, 5>{}); break;
    case 6: launch(std::integral_constant<int, 6>{}); break;
    case 7: launch(std::integral_constant<int, 7>{}); break;
    default: launch(std::integral_constant<int, 8>{}); break;
    }
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

// launch(T{}) for the element type T of a formatted-output kernel
template <typename Launch>
static int with_elem_type(int elem, Launch &&launch)
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

int launch_dec_syn(const DecSynArgs &a, hipStream_t s)
{
    int cm;
    if (syn_fast(a, &cm)) {
        const DecSynFused F = make_syn_fused(a);
        const dim3 grid(F.tiles_x * ccmi_div_up(a.h, kRH - 2 * F.n_sp));
        with_syn_cin(a.c_in, [&](auto cin) {
            hipLaunchKernelGGL((dec_syn_fused<decltype(cin)::value, 3>), grid, dim3(kThreads), 0, s, F);
        });
        CCMI_HIP_CHECK(hipGetLastError());
        return CCMI_OK;
    }
    const int32_t *wp[CCMI_MAX_SYN_LAYERS], *bp[CCMI_MAX_SYN_LAYERS];
    int cin_of[CCMI_MAX_SYN_LAYERS];
    syn_params(a, wp, bp, cin_of);
    // generic: the reference fuses the first two layers whenever both are 1x1 (can_fuse)
    const int64_t plane = (int64_t)a.h * a.w;
    const int maxc = syn_maxc(a);
    int32_t *bufs[2] = {a.workspace, a.workspace + (size_t)maxc * plane};
    const int32_t *src = a.in;
    dim3 grid((unsigned)((plane + kThreads - 1) / kThreads));
    int l = 0, k = 0;
    while (l < a.n_layers) {
        const bool fused = l == 0 && a.n_layers >= 2 && a.layers[0].ks == 1 && a.layers[1].ks == 1;
        const int last_layer = fused ? 1 : l;
        int32_t *dst = last_layer == a.n_layers - 1 ? a.out : bufs[k & 1];
        if (fused) {
            hipLaunchKernelGGL(dec_syn_fused_generic, grid, dim3(kThreads), 0, s, src, cin_of[0], plane, wp[0], bp[0],
                               a.layers[0].n_out, wp[1], bp[1], a.layers[1].n_out, dst);
        } else {
            const SynLayerDesc &L = a.layers[l];
            hipLaunchKernelGGL(dec_syn_layer, grid, dim3(kThreads), 0, s, src, cin_of[l], a.h, a.w, wp[l], bp[l],
                               L.n_out, L.ks, L.residual, L.relu, dst);
        }
        CCMI_HIP_CHECK(hipGetLastError());
        src = dst;
        l = last_layer + 1;
        ++k;
    }
    return CCMI_OK;
}

int launch_dec_blend(int32_t *acc, const int32_t *x, int64_t n, int32_t b_acc, int32_t b_x, int first, hipStream_t s)
{
    hipLaunchKernelGGL(dec_blend_kernel, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, acc, x,
                       n, b_acc, b_x, first);
    CCMI_HIP_CHECK(hipGetLastError());
    return CCMI_OK;
}

int launch_dec_output(const int32_t *syn, int h, int w, int bitdepth, int kind, uint8_t *dst, hipStream_t s)
{
    const int64_t plane = (int64_t)h * w;
    hipLaunchKernelGGL(dec_output_kernel, dim3((unsigned)((plane + kThreads - 1) / kThreads)), dim3(kThreads), 0, s,
                       syn, h, w, (1 << bitdepth) - 1, kind, bitdepth <= 8 ? 1 : 2, dst);
    CCMI_HIP_CHECK(hipGetLastError());
    return CCMI_OK;
}

int launch_dec_output_tensor(const int32_t *syn, int h, int w, int bitdepth, int kind, int sample, void *dst,
                             hipStream_t s)
{
    if (kind != 0 && kind != 1) return ccmi_set_error(CCMI_ERR_ARG, "dec: tensor output kind %d", kind);
    const dim3 grid(output_tensor_blocks(h, w, kind));
    const int maxv = (1 << bitdepth) - 1;
    return with_sample_type(sample, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(dec_output_tensor<T>, grid, dim3(kThreads), 0, s, syn, h, w, maxv, kind, static_cast<T *>(dst));
    });
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

int launch_dec_output_tensor_roi(const int32_t *syn, int h, int w, const DecWindow &rect, int bitdepth, int kind,
                                 int sample, void *dst, hipStream_t s)
{
    if (int rc = check_region(rect, h, w, kind, false)) return rc;
    const dim3 grid(output_tensor_blocks(rect.h(), rect.w(), kind));
    const int maxv = (1 << bitdepth) - 1;
    return with_sample_type(sample, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(dec_output_tensor_crop<T>, grid, dim3(kThreads), 0, s, syn, h, w, rect.y0, rect.x0, rect.h(),
                           rect.w(), maxv, kind, static_cast<T *>(dst));
    });
}

// a per-frame tail's colour form needs the frame's op table (and a contrast op its accumulator)
static int col_frame(const DecFmt &fmt, const DecCol *col)
{
    if (fmt.col && (!col || (col->contrast >= 0 && !col->acc)))
        return ccmi_set_error(CCMI_ERR_ARG, "dec: colour without its op table");
    return CCMI_OK;
}

int launch_dec_output_fmt(const int32_t *syn, int h, int w, const DecWindow &rect, int bitdepth, int kind,
                          const DecFmt &fmt, void *dst, hipStream_t s, const DecCol *col)
{
    if (int rc = check_region(rect, h, w, kind, true)) return rc;
    if (int rc = col_frame(fmt, col)) return rc;
    const dim3 grid(output_fmt_blocks(rect.h(), rect.w()));
    const int maxv = (1 << bitdepth) - 1;
    if (fmt.col) {
        if (col->contrast >= 0) {
            hipLaunchKernelGGL(dec_output_fmt_stat, grid, dim3(kThreads), 0, s, syn, h, w, rect.y0, rect.x0, rect.h(), rect.w(),
                               maxv, kind, fmt_flags(fmt), *col);
            CCMI_HIP_CHECK(hipGetLastError());
        }
        return with_elem_type(fmt.elem, [&](auto t) {
            using T = decltype(t);
            hipLaunchKernelGGL(dec_output_fmt_col<T>, grid, dim3(kThreads), 0, s, syn, h, w, rect.y0, rect.x0, rect.h(),
                               rect.w(), maxv, kind, fmt_flags(fmt), static_cast<T *>(dst), fmt_call(fmt), *col);
        });
    }
    return with_elem_type(fmt.elem, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(dec_output_fmt<T>, grid, dim3(kThreads), 0, s, syn, h, w, rect.y0, rect.x0, rect.h(), rect.w(),
                           maxv, kind, fmt_flags(fmt), static_cast<T *>(dst), fmt_call(fmt));
    });
}

size_t dec_resample_tmp_elems(int region_h, int out_w) { return 3 * (size_t)region_h * out_w; }

int launch_dec_resample(const int32_t *syn, int h, int w, const DecWindow &rect, int bitdepth, int kind,
                        const DecFmt &fmt, float *tmp, void *dst, hipStream_t s, const DecCol *col)
{
    if (int rc = check_region(rect, h, w, kind, true)) return rc;
    if (!fmt.rs || fmt.out_h < 1 || fmt.out_w < 1 || !tmp) return ccmi_set_error(CCMI_ERR_ARG, "dec: resample without a size");
    if (int rc = col_frame(fmt, col)) return rc;
    const int maxv = (1 << bitdepth) - 1;
    hipLaunchKernelGGL(dec_resample_h, dim3(resample_h_blocks(rect.h(), fmt.out_w)), dim3(kThreads), 0, s, syn, h, w,
                       rect.y0, rect.x0, rect.h(), rect.w(), fmt.out_w, maxv, kind, fmt_flags(fmt), tmp);
    CCMI_HIP_CHECK(hipGetLastError());
    const dim3 grid(output_fmt_blocks(fmt.out_h, fmt.out_w));
    if (fmt.col) {
        if (col->contrast >= 0) {
            hipLaunchKernelGGL(dec_resample_v_stat, grid, dim3(kThreads), 0, s, tmp, rect.h(), fmt.out_h, fmt.out_w,
                               fmt_flags(fmt), *col);
            CCMI_HIP_CHECK(hipGetLastError());
        }
        return with_elem_type(fmt.elem, [&](auto t) {
            using T = decltype(t);
            hipLaunchKernelGGL(dec_resample_v_col<T>, grid, dim3(kThreads), 0, s, tmp, rect.h(), fmt.out_h, fmt.out_w,
                               fmt_flags(fmt), static_cast<T *>(dst), fmt_call(fmt), *col);
        });
    }
    return with_elem_type(fmt.elem, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(dec_resample_v<T>, grid, dim3(kThreads), 0, s, tmp, rect.h(), fmt.out_h, fmt.out_w,
                           fmt_flags(fmt), static_cast<T *>(dst), fmt_call(fmt));
    });
}

static DecOutWarp make_out_warp(const DecOut &o, const DecFmt &fmt, int oy, int ox, int fh, int fw)
{
    DecOutWarp A{o, {}, oy, ox, fh, fw};
    for (int k = 0; k < 6; ++k) A.m[k] = fmt.m[k];
    return A;
}

int launch_dec_warp(const int32_t *syn, int h, int w, int bitdepth, int kind, const DecFmt &fmt, void *dst, hipStream_t s,
                    const DecCol *col)
{
    if (int rc = check_region(DecWindow{0, h, 0, w}, h, w, kind, true)) return rc;
    if (!fmt.warp || fmt.out_h < 1 || fmt.out_w < 1) return ccmi_set_error(CCMI_ERR_ARG, "dec: warp without a size");
    if (kind == 0 && ((h | w) & 1)) return ccmi_set_error(CCMI_ERR_ARG, "dec: a 420 warp needs an even frame size");
    const DecOut o{syn, h, w, (1 << bitdepth) - 1, kind, fmt_flags(fmt), static_cast<uint8_t *>(dst)};
    const DecOutWarp A = make_out_warp(o, fmt, 0, 0, h, w);
    const dim3 grid(output_fmt_blocks(fmt.out_h, fmt.out_w));
    if (int rc = col_frame(fmt, col)) return rc;
    if (fmt.col) {
        if (col->contrast >= 0) {
            hipLaunchKernelGGL(dec_warp_stat, grid, dim3(kThreads), 0, s, A, warp_call(fmt), *col);
            CCMI_HIP_CHECK(hipGetLastError());
        }
        return with_elem_type(fmt.elem, [&](auto t) {
            hipLaunchKernelGGL(dec_warp_col<decltype(t)>, grid, dim3(kThreads), 0, s, A, fmt_call(fmt), warp_call(fmt), *col);
        });
    }
    return with_elem_type(fmt.elem, [&](auto t) {
        hipLaunchKernelGGL(dec_warp<decltype(t)>, grid, dim3(kThreads), 0, s, A, fmt_call(fmt), warp_call(fmt));
    });
}

// ------------------------------------------------------------------ batched decoder tail
bool dec_tail_batchable(const DecTailFrame &f)
{
    int cm;
    return f.ups.n_layers >= 2 && ups_ks_ok(f.ups) && f.syn.c_in == f.ups.n_layers && syn_fast(f.syn, &cm);
}

// launch geometry only: the grids depend on the plane sizes, the synthesis halo and the
// synthesis input width (template); everything else is per-frame table data
bool dec_tail_same_group(const DecTailFrame &a, const DecTailFrame &b)
{
    if (a.ups.n_layers != b.ups.n_layers || a.windowed != b.windowed) return false;
    // a formatted output is one kernel per element type; the format is one per call, so the
    // frames of a call group as they do without it
    if (a.fmt.on != b.fmt.on || a.fmt.elem != b.fmt.elem) return false;
    if (a.fmt.rs != b.fmt.rs || a.fmt.warp != b.fmt.warp || a.fmt.out_h != b.fmt.out_h || a.fmt.out_w != b.fmt.out_w)
        return false;
    if (a.fmt.col != b.fmt.col) return false; // one per call too: the frames' ops are table data
    if (a.windowed) {
        // region decode: the tables carry each frame's true plane sizes and its windows, the
        // grids cover the group's largest window; one region size (the output grid), any
        // frame size, any origin.  A resample's output grid is the output size (above): its
        // regions may differ, and the synthesis and horizontal-pass grids cover the largest; a
        // warp's likewise, its regions being the windows its matrices reach
        if (a.sample != b.sample || a.kind != b.kind) return false;
        if (a.syn.n_layers != b.syn.n_layers || a.syn.c_in != b.syn.c_in) return false;
        return a.fmt.rs || a.fmt.warp || (a.roi.rect.h() == b.roi.rect.h() && a.roi.rect.w() == b.roi.rect.w());
    }
    for (int l = 0; l < a.ups.n_layers; ++l)
        if (a.ups.lh[l] != b.ups.lh[l] || a.ups.lw[l] != b.ups.lw[l]) return false;
    // tensor outputs: the output grid is sized by the sample count, i.e. by the chroma format too
    if (a.sample != b.sample || (a.sample >= 0 && a.kind != b.kind)) return false;
    return a.syn.n_layers == b.syn.n_layers && a.syn.c_in == b.syn.c_in && a.syn.h == b.syn.h && a.syn.w == b.syn.w;
}

static size_t al16(size_t x) { return (x + 15) & ~(size_t)15; }

// Byte layout of the argument table of a group of n frames: [step][frame] pyramid levels, then
// [frame] synthesis arguments, then [frame] DecOut, each section 16-byte aligned.  A window-form
// group holds DecLevelWin / DecSynFusedWin, the others DecLevel / DecSynFused; a resampling
// group holds DecOutRs for DecOut, a warping group DecOutWarp (out_form: kOut*); a group of a
// call with colour ops ends with [frame] DecCol.
struct TailTable {
    size_t syn, out, col, bytes; // section offsets (the levels are at 0) and the total size
    TailTable(int steps, int n, bool windowed, int out_form, bool colour)
    {
        const size_t st = steps > 0 ? (size_t)steps : 0;
        syn = al16((windowed ? sizeof(DecLevelWin) : sizeof(DecLevel)) * st * n);
        out = syn + al16((windowed ? sizeof(DecSynFusedWin) : sizeof(DecSynFused)) * (size_t)n);
        const size_t entry = out_form == kOutRs     ? sizeof(DecOutRs)
                             : out_form == kOutWarp ? sizeof(DecOutWarp)
                                                    : sizeof(DecOut);
        col = out + al16(entry * (size_t)n);
        bytes = col + (colour ? al16(sizeof(DecCol) * (size_t)n) : 0);
    }
    // the group of `fr[0]`
    TailTable(const DecTailFrame &f0, int n)
        : TailTable(f0.ups.n_layers - 1, n, f0.windowed, dec_out_form(f0.fmt), f0.fmt.col != 0)
    {
    }
    template <typename T> T *at(void *tab, size_t off) const { return reinterpret_cast<T *>(static_cast<uint8_t *>(tab) + off); }
    template <typename T> const T *at(const void *tab, size_t off) const
    {
        return reinterpret_cast<const T *>(static_cast<const uint8_t *>(tab) + off);
    }
};

size_t dec_tail_table_bytes(int n_layers, int n, bool windowed, int out_form, bool col)
{
    return TailTable(n_layers - 1, n, windowed, out_form, col).bytes;
}

static DecOut make_out(const DecTailFrame &f, int h, int w)
{
    return DecOut{f.syn.out, h, w, (1 << f.bitdepth) - 1, f.kind, f.fmt.on ? fmt_flags(f.fmt) : f.bitdepth <= 8 ? 1 : 2,
                  f.dst};
}

// entry i of a group's output section: the h x w synthesis output sits at (oy, ox) of its frame
static void put_out(const TailTable &T, void *host_tab, int i, const DecTailFrame &f, int h, int w, int oy = 0, int ox = 0)
{
    if (f.fmt.warp)
        T.at<DecOutWarp>(host_tab, T.out)[i] = make_out_warp(make_out(f, h, w), f.fmt, oy, ox, f.syn.h, f.syn.w);
    else if (f.fmt.rs) T.at<DecOutRs>(host_tab, T.out)[i] = DecOutRs{make_out(f, h, w), f.rs_tmp};
    else T.at<DecOut>(host_tab, T.out)[i] = make_out(f, h, w);
    if (f.fmt.col) T.at<DecCol>(host_tab, T.col)[i] = *f.col;
}

// the window-form tables
static void dec_tail_fill_win(const DecTailFrame *const *fr, int n, void *host_tab)
{
    const int steps = fr[0]->ups.n_layers - 1;
    const TailTable T(*fr[0], n);
    DecLevelWin *lv = T.at<DecLevelWin>(host_tab, 0);
    DecSynFusedWin *sf = T.at<DecSynFusedWin>(host_tab, T.syn);
    for (int i = 0; i < n; ++i) {
        DecLevelWin tmp[CCMI_MAX_GRIDS];
        make_levels_win(*fr[i], tmp);
        for (int st = 0; st < steps; ++st) lv[(size_t)st * n + i] = tmp[st];
        const DecRoi &R = fr[i]->roi;
        DecSynFusedWin &S = sf[i];
        S = DecSynFusedWin{};
        S.F = make_syn_fused(fr[i]->syn);
        S.iy0 = R.lev[0].y0, S.iy1 = R.lev[0].y1 - 1, S.ix0 = R.lev[0].x0, S.ix1 = R.lev[0].x1 - 1;
        S.ipitch = R.lev[0].w();
        S.iplane = (int64_t)R.lev[0].h() * R.lev[0].w();
        S.ry = R.rect.y0, S.rx = R.rect.x0, S.rh = R.rect.h(), S.rw = R.rect.w();
        // the synthesis output is the region itself, compact: the whole-frame output kernel
        // converts it as a frame of the region's size (420: the origin is even, so its even
        // rows and columns are the frame's)
        put_out(T, host_tab, i, *fr[i], S.rh, S.rw, S.ry, S.rx);
    }
}

void dec_tail_fill(const DecTailFrame *const *fr, int n, void *host_tab)
{
    if (fr[0]->windowed) return dec_tail_fill_win(fr, n, host_tab);
    const int steps = fr[0]->ups.n_layers - 1;
    const TailTable T(*fr[0], n);
    DecLevel *lv = T.at<DecLevel>(host_tab, 0);
    DecSynFused *sf = T.at<DecSynFused>(host_tab, T.syn);
    for (int i = 0; i < n; ++i) {
        DecLevel tmp[CCMI_MAX_GRIDS];
        make_levels(fr[i]->ups, tmp);
        for (int st = 0; st < steps; ++st) lv[(size_t)st * n + i] = tmp[st];
        sf[i] = make_syn_fused(fr[i]->syn);
        put_out(T, host_tab, i, *fr[i], fr[i]->syn.h, fr[i]->syn.w);
    }
}

// the tensor output of a group: h x w samples of one kind and sample type per frame
static int launch_output_tensor_batch(const DecTailFrame &f0, int h, int w, int n, const DecOut *oo, hipStream_t s,
                                      const DecCol *kk = nullptr, bool stat = false)
{
    if (f0.fmt.col) { // kk = the group's op tables; stat: a frame has a contrast op
        const dim3 grid(output_fmt_blocks(f0.fmt.rs || f0.fmt.warp ? f0.fmt.out_h : h, f0.fmt.rs || f0.fmt.warp ? f0.fmt.out_w : w),
                        n);
        const DecFmtCall C = fmt_call(f0.fmt);
        if (f0.fmt.rs) {
            const DecOutRs *rr = reinterpret_cast<const DecOutRs *>(oo);
            const int oh = f0.fmt.out_h, ow = f0.fmt.out_w;
            hipLaunchKernelGGL(dec_resample_h_batch, dim3(resample_h_blocks(h, ow), n), dim3(kThreads), 0, s, rr, ow);
            CCMI_HIP_CHECK(hipGetLastError());
            if (stat) hipLaunchKernelGGL(dec_resample_v_stat_batch, grid, dim3(kThreads), 0, s, rr, oh, ow, kk);
            CCMI_HIP_CHECK(hipGetLastError());
            return with_elem_type(f0.fmt.elem, [&](auto t) {
                hipLaunchKernelGGL(dec_resample_v_col_batch<decltype(t)>, grid, dim3(kThreads), 0, s, rr, oh, ow, C, kk);
            });
        }
        if (f0.fmt.warp) {
            const DecOutWarp *ww = reinterpret_cast<const DecOutWarp *>(oo);
            if (stat) hipLaunchKernelGGL(dec_warp_stat_batch, grid, dim3(kThreads), 0, s, ww, warp_call(f0.fmt), kk);
            CCMI_HIP_CHECK(hipGetLastError());
            return with_elem_type(f0.fmt.elem, [&](auto t) {
                hipLaunchKernelGGL(dec_warp_col_batch<decltype(t)>, grid, dim3(kThreads), 0, s, ww, C, warp_call(f0.fmt), kk);
            });
        }
        if (stat) hipLaunchKernelGGL(dec_output_fmt_stat_batch, grid, dim3(kThreads), 0, s, oo, kk);
        CCMI_HIP_CHECK(hipGetLastError());
        return with_elem_type(f0.fmt.elem, [&](auto t) {
            hipLaunchKernelGGL(dec_output_fmt_col_batch<decltype(t)>, grid, dim3(kThreads), 0, s, oo, C, kk);
        });
    }
    if (f0.fmt.rs) { // the section holds DecOutRs; h = the group's tallest region
        const DecOutRs *rr = reinterpret_cast<const DecOutRs *>(oo);
        const int oh = f0.fmt.out_h, ow = f0.fmt.out_w;
        hipLaunchKernelGGL(dec_resample_h_batch, dim3(resample_h_blocks(h, ow), n), dim3(kThreads), 0, s, rr, ow);
        CCMI_HIP_CHECK(hipGetLastError());
        const dim3 grid(output_fmt_blocks(oh, ow), n);
        return with_elem_type(f0.fmt.elem, [&](auto t) {
            hipLaunchKernelGGL(dec_resample_v_batch<decltype(t)>, grid, dim3(kThreads), 0, s, rr, oh, ow, fmt_call(f0.fmt));
        });
    }
    if (f0.fmt.warp) { // the section holds DecOutWarp; the grid is the output size
        const dim3 grid(output_fmt_blocks(f0.fmt.out_h, f0.fmt.out_w), n);
        return with_elem_type(f0.fmt.elem, [&](auto t) {
            hipLaunchKernelGGL(dec_warp_batch<decltype(t)>, grid, dim3(kThreads), 0, s,
                               reinterpret_cast<const DecOutWarp *>(oo), fmt_call(f0.fmt), warp_call(f0.fmt));
        });
    }
    if (f0.fmt.on) { // the format but its per-frame flags (in the table) is the call's
        const dim3 grid(output_fmt_blocks(h, w), n);
        return with_elem_type(f0.fmt.elem, [&](auto t) {
            hipLaunchKernelGGL(dec_output_fmt_batch<decltype(t)>, grid, dim3(kThreads), 0, s, oo, fmt_call(f0.fmt));
        });
    }
    const dim3 grid(output_tensor_blocks(h, w, f0.kind), n); // one kind per group
    return with_sample_type(f0.sample, [&](auto t) {
        hipLaunchKernelGGL(dec_output_tensor_batch<decltype(t)>, grid, dim3(kThreads), 0, s, oo);
    });
}

// a frame of the group has a contrast op: the group runs its statistics pass
static bool col_group_stat(const DecTailFrame *const *fr, int n)
{
    for (int i = 0; i < n; ++i)
        if (fr[i]->fmt.col && fr[i]->col->contrast >= 0) return true;
    return false;
}

// region decode: one launch per stage for a window-form group (dec_tail_same_group); the
// grids cover the group's largest window of each level
static int launch_dec_tail_batch_win(const DecTailFrame *const *fr, int n, const void *dev_tab, hipStream_t s)
{
    const DecTailFrame &f0 = *fr[0];
    const int L = f0.ups.n_layers, steps = L - 1;
    if (f0.sample < 0) return ccmi_set_error(CCMI_ERR_ARG, "dec: a region decode writes tensors only");
    const TailTable T(f0, n);
    const DecLevelWin *lv = T.at<DecLevelWin>(dev_tab, 0);
    const DecSynFusedWin *sf = T.at<DecSynFusedWin>(dev_tab, T.syn);
    for (int st = 0; st < steps; ++st) {
        const int k = L - 1 - st;
        int gtx = 1, gty = 1; // tiles from each window's origin rounded down to even
        for (int i = 0; i < n; ++i) {
            const DecWindow &d = fr[i]->roi.lev[k - 1];
            gtx = std::max(gtx, ccmi_div_up(d.x1 - (d.x0 & ~1), kTX));
            gty = std::max(gty, ccmi_div_up(d.y1 - (d.y0 & ~1), kTY));
        }
        hipLaunchKernelGGL(dec_ups_level_win_batch, dim3(gtx * gty, n), dim3(kThreads), 0, s, lv + (size_t)st * n, gtx);
        CCMI_HIP_CHECK(hipGetLastError());
    }
    const int halo = f0.syn.n_layers - 2;
    int rh = 1, rw = 1; // one region size per group, but a resampling group's: the largest
    for (int i = 0; i < n; ++i) {
        rh = std::max(rh, fr[i]->roi.rect.h());
        rw = std::max(rw, fr[i]->roi.rect.w());
    }
    const int gtx = ccmi_div_up(rw, kRW - 2 * halo);
    const dim3 sg(gtx * ccmi_div_up(rh, kRH - 2 * halo), n);
    with_syn_cin(f0.syn.c_in, [&](auto cin) {
        hipLaunchKernelGGL((dec_syn_fused_win_batch<decltype(cin)::value, 3>), sg, dim3(kThreads), 0, s, sf, gtx);
    });
    CCMI_HIP_CHECK(hipGetLastError());
    return launch_output_tensor_batch(f0, rh, rw, n, T.at<DecOut>(dev_tab, T.out), s, T.at<DecCol>(dev_tab, T.col),
                                      col_group_stat(fr, n));
}

int launch_dec_tail_batch(const DecTailFrame *const *fr, int n, const void *dev_tab, hipStream_t s)
{
    if (n < 1 || n > 65535) return ccmi_set_error(CCMI_ERR_ARG, "dec: tail batch of %d frames", n);
    if (fr[0]->windowed) return launch_dec_tail_batch_win(fr, n, dev_tab, s);
    const DecTailFrame &f0 = *fr[0];
    const int L = f0.ups.n_layers, steps = L - 1;
    const TailTable T(f0, n);
    const DecLevel *lv = T.at<DecLevel>(dev_tab, 0);
    const DecSynFused *sf = T.at<DecSynFused>(dev_tab, T.syn);
    const DecOut *oo = T.at<DecOut>(dev_tab, T.out);
    for (int st = 0; st < steps; ++st) {
        const int k = L - 1 - st;
        const int hd = f0.ups.lh[k - 1], wd = f0.ups.lw[k - 1];
        const dim3 grid(ccmi_div_up(wd, kTX) * ccmi_div_up(hd, kTY), n);
        hipLaunchKernelGGL(dec_ups_level_batch, grid, dim3(kThreads), 0, s, lv + (size_t)st * n);
        CCMI_HIP_CHECK(hipGetLastError());
    }
    const int halo = f0.syn.n_layers - 2;
    const dim3 sg(ccmi_div_up(f0.syn.w, kRW - 2 * halo) * ccmi_div_up(f0.syn.h, kRH - 2 * halo), n);
    with_syn_cin(f0.syn.c_in, [&](auto cin) {
        hipLaunchKernelGGL((dec_syn_fused_batch<decltype(cin)::value, 3>), sg, dim3(kThreads), 0, s, sf);
    });
    CCMI_HIP_CHECK(hipGetLastError());
    if (f0.sample >= 0)
        return launch_output_tensor_batch(f0, f0.syn.h, f0.syn.w, n, oo, s, T.at<DecCol>(dev_tab, T.col), col_group_stat(fr, n));
    const int64_t plane = (int64_t)f0.syn.h * f0.syn.w;
    hipLaunchKernelGGL(dec_output_batch, dim3((unsigned)((plane + kThreads - 1) / kThreads), n), dim3(kThreads), 0, s, oo);
    CCMI_HIP_CHECK(hipGetLastError());
    return CCMI_OK;
}

} // namespace ccmi
