// dec_tail.hip -- path B: the decoder tail of the bit-exact fixed-point .cool decoder: pyramid,
// synthesis and blend kernels, their launchers and the batched tail (the ARM + CABAC kernels are
// dec_arm.hip, the output stage that ends the tail is dec_out.hip).
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
// [frame] synthesis arguments, then the [frame] output section, each section 16-byte aligned.  A
// window-form group holds DecLevelWin / DecSynFusedWin, the others DecLevel / DecSynFused; the
// output section's entries are the output stage's (dec_out_entry_bytes of out_form: kOut*); a group
// of a call with colour ops ends with [frame] DecCol.
struct TailTable {
    size_t syn, out, col, bytes; // section offsets (the levels are at 0) and the total size
    TailTable(int steps, int n, bool windowed, int out_form, bool colour)
    {
        const size_t st = steps > 0 ? (size_t)steps : 0;
        syn = al16((windowed ? sizeof(DecLevelWin) : sizeof(DecLevel)) * st * n);
        out = syn + al16((windowed ? sizeof(DecSynFusedWin) : sizeof(DecSynFused)) * (size_t)n);
        col = out + al16(dec_out_entry_bytes(out_form) * (size_t)n);
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

// the window-form tables
static void dec_tail_fill_win(const DecTailFrame *const *fr, int n, void *host_tab, int n_flt, void *host_flt_tab)
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
        dec_out_fill(T.at<void>(host_tab, T.out), T.at<void>(host_tab, T.col), i, *fr[i], S.rh, S.rw, S.ry, S.rx);
        if (i >= n - n_flt) dec_flt_fill(host_flt_tab, n_flt, i - (n - n_flt), *fr[i], S.rh, S.rw, S.ry, S.rx);
    }
}

void dec_tail_fill(const DecTailFrame *const *fr, int n, void *host_tab, int n_flt, void *host_flt_tab)
{
    if (fr[0]->windowed) return dec_tail_fill_win(fr, n, host_tab, n_flt, host_flt_tab);
    const int steps = fr[0]->ups.n_layers - 1;
    const TailTable T(*fr[0], n);
    DecLevel *lv = T.at<DecLevel>(host_tab, 0);
    DecSynFused *sf = T.at<DecSynFused>(host_tab, T.syn);
    for (int i = 0; i < n; ++i) {
        DecLevel tmp[CCMI_MAX_GRIDS];
        make_levels(fr[i]->ups, tmp);
        for (int st = 0; st < steps; ++st) lv[(size_t)st * n + i] = tmp[st];
        sf[i] = make_syn_fused(fr[i]->syn);
        dec_out_fill(T.at<void>(host_tab, T.out), T.at<void>(host_tab, T.col), i, *fr[i], fr[i]->syn.h, fr[i]->syn.w, 0, 0);
        if (i >= n - n_flt) dec_flt_fill(host_flt_tab, n_flt, i - (n - n_flt), *fr[i], fr[i]->syn.h, fr[i]->syn.w, 0, 0);
    }
}

// a frame of the group has a contrast op: the group runs its statistics pass
static bool col_group_stat(const DecTailFrame *const *fr, int n)
{
    for (int i = 0; i < n; ++i)
        if (fr[i]->fmt.col && fr[i]->col->contrast >= 0) return true;
    return false;
}

// The output stage of a group whose last n_flt frames take the filter stage: the others through the
// group's output kernels as ever (their entries lead the output and colour sections), the staged
// ones as launches of their own (launch_dec_out_group_flt).
static int launch_out_stage(const DecTailFrame *const *fr, int n, int n_flt, int h, int w, const TailTable &T,
                            const void *dev_tab, const void *dev_flt_tab, hipStream_t s)
{
    const int n0 = n - n_flt;
    const DecCol *kk = T.at<DecCol>(dev_tab, T.col);
    if (n0 > 0)
        if (int rc = launch_dec_out_group(*fr[0], h, w, n0, T.at<void>(dev_tab, T.out), kk, col_group_stat(fr, n0), s))
            return rc;
    if (n_flt > 0) return launch_dec_out_group_flt(fr + n0, n_flt, h, w, dev_flt_tab, kk + n0, s);
    return CCMI_OK;
}

// region decode: one launch per stage for a window-form group (dec_tail_same_group); the
// grids cover the group's largest window of each level
static int launch_dec_tail_batch_win(const DecTailFrame *const *fr, int n, const void *dev_tab, hipStream_t s, int n_flt,
                                     const void *dev_flt_tab)
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
    return launch_out_stage(fr, n, n_flt, rh, rw, T, dev_tab, dev_flt_tab, s);
}

int launch_dec_tail_batch(const DecTailFrame *const *fr, int n, const void *dev_tab, hipStream_t s, int n_flt,
                          const void *dev_flt_tab)
{
    if (n < 1 || n > 65535 || n_flt < 0 || n_flt > n) return ccmi_set_error(CCMI_ERR_ARG, "dec: tail batch of %d frames", n);
    if (fr[0]->windowed) return launch_dec_tail_batch_win(fr, n, dev_tab, s, n_flt, dev_flt_tab);
    const DecTailFrame &f0 = *fr[0];
    const int L = f0.ups.n_layers, steps = L - 1;
    const TailTable T(f0, n);
    const DecLevel *lv = T.at<DecLevel>(dev_tab, 0);
    const DecSynFused *sf = T.at<DecSynFused>(dev_tab, T.syn);
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
    return launch_out_stage(fr, n, n_flt, f0.syn.h, f0.syn.w, T, dev_tab, dev_flt_tab, s);
}

} // namespace ccmi
