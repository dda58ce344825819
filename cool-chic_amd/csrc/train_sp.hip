// train_sp.hip -- the overfit step's 3x3 synthesis layers and its MSE: t_sp_fwd<LOSS> (the last
// layer of a training step with the loss fused in), t_loss (the loss on its own: forward-only
// calls, steps without a 3x3 layer) and t_sp_bwd<MODE>.  launch_sp_bwd owns the MODE choice
// (CCMI_SP_BWD_PF, the previous layer's ReLU mask).
#include <stdlib.h>

#include "fwd_common.h"
#include "train_internal.h"

using namespace ccmi_train;
using ccmi_fwd::cfloat_ptr;

namespace {

// 3x3, 3 -> 3, replicate padding (synthesis.py:69-84), optional residual / ReLU.  A thread
// computes kSpRows vertically consecutive pixels of one column: the rows it reads overlap, so
// it loads (kSpRows + 2) x 3 neighbours per channel instead of 9 per pixel (one pixel per
// thread issued 27 loads per pixel); same FMA order per pixel.
// LOSS (the last layer of a training step): t_loss's MSE fused in -- the layer's output is
// consumed where it is produced (its gradient graw, the squared errors into the frame's mse
// slots) and stored only when store_out (a ReLU's mask for the backward, or the caller's raw
// output).  1: 444 target; 2: 420 target (chroma at even rows / columns, frame.py:175-183).
constexpr int kSpRows = 4;
template <int LOSS>
__global__ __launch_bounds__(kT) void t_sp_fwd(const float *__restrict__ in, Geo g, const float *__restrict__ th, int64_t ps,
                                               int wo, int bo, int res, int relu, float *__restrict__ out,
                                               const float *__restrict__ tgt, int64_t tstride, float k2,
                                               float *__restrict__ graw, float *__restrict__ mslots, int store_out)
{
    // 1-D grid of (blocks per frame) x frames in XCD-aware order: the row groups above and below,
    // which load 2 of the same rows, run on one L2
    const int per = (((g.H + kSpRows - 1) / kSpRows) * g.W + kT - 1) / kT; // blocks per frame
    const int wt = ccmi_fwd::xcd_order(blockIdx.x, gridDim.x);
    const int b = wt / per;
    const int64_t npx = (int64_t)g.H * g.W;
    const int q = (wt - b * per) * kT + threadIdx.x; // (row group, column); a frame fits 31 bits
    const int gy = q / g.W, px = q - gy * g.W, y0 = gy * kSpRows;
    float se = 0.f;
    if (y0 < g.H) { // (no early return: the fused loss's block reduction needs every thread)
        const cfloat_ptr P = (cfloat_ptr)(size_t)(th + (int64_t)b * ps);
        const float *x = in + (int64_t)b * 3 * npx;
        int xo[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) xo[d] = clampi(px + d - 1, g.W - 1);
        float v[3][kSpRows + 2][3];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int r = 0; r < kSpRows + 2; ++r) {
                const float *row = x + i * npx + (int64_t)clampi(y0 + r - 1, g.H - 1) * g.W;
#pragma unroll
                for (int d = 0; d < 3; ++d) v[i][r][d] = row[xo[d]];
            }
        const int64_t pix = (int64_t)y0 * g.W + px;
        float *o = out + (int64_t)b * 3 * npx + pix;
        const int h2 = g.H / 2, w2 = g.W / 2;
        // the fused loss's target values, loaded with the inputs (loaded where used, each was a
        // dependent memory latency per output: 62 % of the wave cycles in WAIT_ANY,
        // profiles/r5zk_train_pmc.txt)
        float tv[LOSS > 0 ? kSpRows : 1][3];
        bool tu[LOSS > 0 ? kSpRows : 1][3];
        if constexpr (LOSS > 0) {
#pragma unroll
            for (int t = 0; t < kSpRows; ++t)
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int y = y0 + t;
                    bool used = y < g.H;
                    int64_t ti = c * npx + (int64_t)y * g.W + px;
                    if (LOSS == 2 && c > 0) {
                        used = used && (y % 2 == 0) && (px % 2 == 0) && (y / 2) < h2 && (px / 2) < w2;
                        ti = npx + (int64_t)(c - 1) * h2 * w2 + (int64_t)(y / 2) * w2 + px / 2;
                    }
                    tu[t][c] = used;
                    tv[t][c] = used ? tgt[(int64_t)b * tstride + ti] : 0.f;
                }
        }
#pragma unroll
        for (int t = 0; t < kSpRows; ++t) {
            if (y0 + t >= g.H) break;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float a = P[bo + c];
#pragma unroll
                for (int i = 0; i < 3; ++i)
#pragma unroll
                    for (int k = 0; k < 9; ++k) a = fmaf(P[wo + (c * 3 + i) * 9 + k], v[i][t + k / 3][k % 3], a);
                if (res) a += v[c][t + 1][1];
                if (relu) a = fmaxf(a, 0.f);
                const int64_t e = c * npx + (int64_t)t * g.W;
                if (LOSS == 0 || store_out) o[e] = a;
                if constexpr (LOSS > 0) { // t_loss on this pixel, same arithmetic
                    float gv = 0.f;
                    if (tu[t][c]) {
                        const float vc = fminf(fmaxf(a, 0.f), 1.f), d = vc - tv[t][c];
                        se += d * d;
                        gv = (a >= 0.f && a <= 1.f) ? k2 * d : 0.f;
                    }
                    graw[(int64_t)b * 3 * npx + e + pix] = gv;
                }
            }
        }
    }
    if constexpr (LOSS > 0) {
        __shared__ float s_red[8];
        const float sum = block_sum(se, s_red);
        if (threadIdx.x == 0) atomicAdd(&mslots[b * kDwSlots + blockIdx.x % kDwSlots], sum);
    }
}

// Train-mode frame output + MSE (frame.py:175-183, loss.py _compute_mse): gradient of the
// MSE w.r.t. the raw synthesis output; sum of squared errors into acc4[b][0].
// 444: kLossPx pixels per thread and iteration with every load issued first (one pixel per
// iteration left the kernel waiting on memory latency: 82 % of its wave cycles in WAIT_ANY at
// 2 waves / SIMD, profiles/r5l_train_pmc.txt); 420: the chroma planes at even rows / columns.
constexpr int kLossPx = 4;
__global__ __launch_bounds__(kT) void t_loss(const float *__restrict__ raw, Geo g, const float *__restrict__ tgt,
                                             int64_t tstride, int yuv420, float *__restrict__ graw, float *__restrict__ acc4)
{
    __shared__ float s_red[8];
    const int b = blockIdx.y;
    const int64_t npx = (int64_t)g.H * g.W;
    const int h2 = g.H / 2, w2 = g.W / 2;
    const float total = yuv420 ? (float)(npx + 2 * (int64_t)h2 * w2) : (float)(3 * npx);
    const float k2 = 2.f / total;
    float se = 0.f;
    const float *o = raw + (int64_t)b * 3 * npx;
    const float *T = tgt + (int64_t)b * tstride;
    float *go = graw + (int64_t)b * 3 * npx;
    // grid-stride: a few hundred workgroups per frame, so the per-workgroup atomic on the
    // frame's one loss slot stays cheap (one workgroup per 256 pixels serialised ~1,500
    // same-address atomics per frame: 124 us per 8-frame 512x768 iteration)
    if (!yuv420) {
        for (int64_t p0 = (int64_t)blockIdx.x * kT * kLossPx + threadIdx.x; p0 < npx; p0 += (int64_t)gridDim.x * kT * kLossPx) {
            float v[kLossPx][3], t[kLossPx][3];
#pragma unroll
            for (int u = 0; u < kLossPx; ++u) {
                const int64_t p = p0 + u * kT;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    v[u][c] = p < npx ? o[c * npx + p] : 0.f;
                    t[u][c] = p < npx ? T[c * npx + p] : 0.f;
                }
            }
#pragma unroll
            for (int u = 0; u < kLossPx; ++u) {
                const int64_t p = p0 + u * kT;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float vc = fminf(fmaxf(v[u][c], 0.f), 1.f), d = vc - t[u][c];
                    se += d * d; // 0 past the frame
                    if (p < npx) go[c * npx + p] = (v[u][c] >= 0.f && v[u][c] <= 1.f) ? k2 * d : 0.f;
                }
            }
        }
    } else {
        for (int64_t p = (int64_t)blockIdx.x * kT + threadIdx.x; p < npx; p += (int64_t)gridDim.x * kT) {
            const int py = (int)p / g.W, px = (int)p - py * g.W; // a frame's pixels fit 31 bits
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                bool used = true;
                int64_t ti = c * npx + p;
                if (c > 0) {
                    used = (py % 2 == 0) && (px % 2 == 0) && (py / 2) < h2 && (px / 2) < w2;
                    ti = npx + (int64_t)(c - 1) * h2 * w2 + (int64_t)(py / 2) * w2 + px / 2;
                }
                float gv = 0.f;
                if (used) {
                    const float vv = o[c * npx + p], vc = fminf(fmaxf(vv, 0.f), 1.f), d = vc - T[ti];
                    se += d * d;
                    gv = (vv >= 0.f && vv <= 1.f) ? k2 * d : 0.f;
                }
                go[c * npx + p] = gv;
            }
        }
    }
    const float s = block_sum(se, s_red);
    if (threadIdx.x == 0) atomicAdd(&acc4[b * 4 + 0], s);
}

// 3x3 layer backward on 16 x 64 pixel tiles staged in LDS (grid-stride over the tiles).
//  * X (the layer input) at replicate-clamped coordinates over the tile + 1-pixel ring:
//    dW[c][i][ky][kx] += G[c][q] X[i][clamp(q + (ky-1, kx-1))], accumulated per thread in
//    registers over every tile the workgroup visits, reduced once at the end;
//  * G (the output gradient, times relu'(out) when the layer has a ReLU) over the same ring,
//    zero outside the image: the input gradient of
//    an interior pixel p is the plain correlation sum_{c,k} W[c][i][k] G[c][p - d_k]; a
//    pixel on the image border also collects the taps that the replicate padding clamps
//    onto it (one kernel row / column / corner tap per image side it lies on), all within the ring.
// MODE 3: input gradient and weight / bias gradients in one launch that reads every tile once, the
// weight gradients in the 4 accumulator registers of v_mfma_f32_4x4x1_16b_f32 (+ 3 bias sums).
// (An earlier pair of launches, input gradient / weight gradients as 84 per-thread VALU sums, sat
// 71 % of its wave cycles in s_waitcnt / barrier waits, SQ_WAIT_ANY.  Measured and dropped too:
// the input gradient one channel per iteration with 27 scalar weights each instead of all 81 at
// once -- 74 vs 40 us, the scalar-load waits per channel.)
// MODE 7 = MODE 3 over a persistent grid (one resident round of workgroups per frame): the next
// tile's ring (X, and G with the ReLU mask already applied) is loaded into registers while the
// current tile computes, and a workgroup flushes its weight gradients once for all its tiles.
// MODE 11 / 15 = MODE 3 / 7 + bit 8 (mask_in, below).
constexpr int kSY = 16, kSX = 64;
template <int MODE>
__global__ __launch_bounds__(kT) __attribute__((amdgpu_waves_per_eu((MODE & 4) ? 4 : 5))) void t_sp_bwd(const float *__restrict__ gout, const float *__restrict__ outp,
                                               const float *__restrict__ in, Geo g, const float *__restrict__ th,
                                               int64_t ps, int wo, int bo, int res, float *__restrict__ gin,
                                               float *__restrict__ gth, int64_t gstride)
{
    static_assert((MODE & 3) == 3 && MODE < 16, "modes 3, 7, 11, 15");
    constexpr bool PF = (MODE & 4) != 0;
    // MODE bit 8: the previous layer's ReLU applied to the input gradient written here, where its
    // output (this layer's input X) is staged -- that layer's backward then loads no output planes
    // (a compile-time bit: as a run-time flag the border pass's select spilled ~50 VGPRs)
    constexpr bool mask_in = (MODE & 8) != 0;
    constexpr int RH = kSY + 2, RW = kSX + 2;
    // ring images at row pitch kRP = 67 and plane pitch kPP = 1225 (== 3 and 9 mod 32 banks): the 27
    // taps (i, ky, kx) of one pixel sit on 27 distinct banks (9 i + 3 ky + kx), so the weight-
    // gradient MFMA loop's operand reads are conflict-free (pitches 66 / 1188: ~3-way)
    constexpr int kRP = 67, kPP = 1225;
    static_assert(kRP >= RW && kPP >= RH * kRP, "ring fits its pitches");
    __shared__ float sXf[3 * kPP];
    __shared__ float sGf[3 * kPP];
#define SX(ch, r, q) sXf[(ch) * kPP + (r) * kRP + (q)]
#define SG(ch, r, q) sGf[(ch) * kPP + (r) * kRP + (q)]
    __shared__ float s_red[4][84];
    __shared__ float s_wt[81]; // the layer's weights for the border-tap fold
    const int b = blockIdx.y;
    const int H = g.H, W = g.W;
    const int64_t npx = (int64_t)H * W;
    const cfloat_ptr P = (cfloat_ptr)(size_t)(th + (int64_t)b * ps);
    const float *Gb = gout + (int64_t)b * 3 * npx;
    const float *Ob = outp ? outp + (int64_t)b * 3 * npx : nullptr;
    const float *Xb = in + (int64_t)b * 3 * npx;
    float *Ib = gin + (int64_t)b * 3 * npx;
    const int tx = (W + kSX - 1) / kSX, ntile = tx * ((H + kSY - 1) / kSY);
    const int c = threadIdx.x & 63, rb = (threadIdx.x >> 6) * 4;
    for (int e = threadIdx.x; e < 81; e += kT) s_wt[e] = P[wo + e]; // visible after the tile loop's first barrier
    v4f dacc = {0.f, 0.f, 0.f, 0.f}; // the weight gradients' MFMA blocks
    float bacc[3] = {0.f, 0.f, 0.f};  // bias sums
    // PF: the ring of tile tt in registers: X and the masked G of NU elements per thread
    constexpr int kPU = (RH * RW + kT - 1) / kT;
    float px_[PF ? kPU : 1][3], pg_[PF ? kPU : 1][3], po_[PF ? kPU : 1][3]; // raw: the mask is applied at the LDS store (a select here would wait for the loads)
    auto prefetch = [&](int tt) __attribute__((always_inline)) {
        const int py0 = (tt / tx) * kSY, px0 = (tt % tx) * kSX;
#pragma unroll
        for (int u = 0; u < kPU; ++u) {
            const int i = threadIdx.x + u * kT;
            const int r = i / RW, q = i - r * RW;
            const int y = py0 - 1 + r, x = px0 - 1 + q;
            const int64_t cl = (int64_t)clampi(y, H - 1) * W + clampi(x, W - 1);
            const bool inb = y >= 0 && y < H && x >= 0 && x < W, live = i < RH * RW;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                px_[u][ch] = live ? Xb[ch * npx + cl] : 0.f;
                pg_[u][ch] = (live && inb) ? Gb[ch * npx + cl] : 0.f;
                po_[u][ch] = (Ob && live && inb) ? Ob[ch * npx + cl] : 1.f;
            }
        }
    };
    if constexpr (PF)
        if ((int)blockIdx.x < ntile) prefetch(blockIdx.x);
    for (int t = blockIdx.x; t < ntile; t += gridDim.x) {
        const int y0 = (t / tx) * kSY, x0 = (t % tx) * kSX;
        __syncthreads();
        if constexpr (PF) {
#pragma unroll
            for (int u = 0; u < kPU; ++u) {
                const int i = threadIdx.x + u * kT;
                if (i >= RH * RW) continue;
                const int r = i / RW, q = i - r * RW;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    SX(ch, r, q) = px_[u][ch];
                    SG(ch, r, q) = po_[u][ch] <= 0.f ? 0.f : pg_[u][ch];
                }
            }
            if (t + (int)gridDim.x < ntile) prefetch(t + gridDim.x); // in flight behind this tile's work
        } else {
            // the whole ring in one batch: every load of a thread is in flight before its LDS stores
            constexpr int NU = (RH * RW + kT - 1) / kT;
            float xs[NU][3], gs[NU][3], os[NU][3];
            bool inb[NU];
#pragma unroll
            for (int uu = 0; uu < NU; ++uu) {
                const int i = threadIdx.x + uu * kT;
                const int r = i / RW, q = i - r * RW;
                const int y = y0 - 1 + r, x = x0 - 1 + q;
                const int64_t cl = (int64_t)clampi(y, H - 1) * W + clampi(x, W - 1);
                inb[uu] = y >= 0 && y < H && x >= 0 && x < W;
                const bool live = i < RH * RW;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
#if defined(CCMI_DIAG_SPB_NOLOAD) // diagnostic builds only (tools/spb_diag.sh): wrong results
                    xs[uu][ch] = 0.001f * (float)(cl + ch);
                    gs[uu][ch] = inb[uu] ? 0.002f * (float)(cl - ch) : 0.f;
                    os[uu][ch] = 1.f;
#else
                    xs[uu][ch] = live ? Xb[ch * npx + cl] : 0.f;
                    gs[uu][ch] = (live && inb[uu]) ? Gb[ch * npx + cl] : 0.f;
                    os[uu][ch] = (Ob && live && inb[uu]) ? Ob[ch * npx + cl] : 1.f;
#endif
                }
            }
#pragma unroll
            for (int uu = 0; uu < NU; ++uu) {
                const int i = threadIdx.x + uu * kT;
                if (i >= RH * RW) continue;
                const int r = i / RW, q = i - r * RW;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    SX(ch, r, q) = xs[uu][ch];
                    SG(ch, r, q) = os[uu][ch] <= 0.f ? 0.f : gs[uu][ch];
                }
            }
        }
        __syncthreads();
#if !defined(CCMI_DIAG_SPB_NODW)
        {
            // dW[oc][n = (i, ky, kx)] += sum_q G[oc][q] X[i][q + (ky - 1, kx - 1)] over the wave's 4 x 64
            // pixels: block bk = lane >> 2 < 14 is (column quad nq = bk % 7, pixel stream bk / 7;
            // stream s takes rows rb + 2 s, rb + 2 s + 1), A = G[oc = lane & 3], B = X at tap column
            // n = 4 nq + (lane & 3), one pixel per MFMA.  Row oc = 3, column n = 27 and blocks 14, 15
            // read valid (clamped) LDS and are never flushed.  Every operand address is a lane base +
            // a compile-time offset.
            const int ln4 = threadIdx.x & 3, bk = (threadIdx.x & 63) >> 2;
            const int st = bk >= 7 ? 1 : 0, n = min(4 * (bk - 7 * st) + ln4, 26);
            const int i = n / 9, k = n - 9 * i, ky = k / 3, kx = k - 3 * ky;
            const float *pa = &SG(ln4 < 3 ? ln4 : 0, rb + 2 * st + 1, 1);
            const float *pb = &SX(i, rb + 2 * st + ky, kx);
#pragma unroll 1
            for (int j = 0; j < 2 * kSX; j += 16) { // 16 pixels per iteration (operand reads in flight)
                const int o = (j >= kSX ? kRP - kSX : 0) + j;
#pragma unroll
                for (int cc = 0; cc < 16; ++cc) dacc = mfma4x4(pa[o + cc], pb[o + cc], dacc);
            }
        }
#endif
        const int px = x0 + c;
#pragma unroll 1
        for (int pr = 0; pr < 4; ++pr) {
            const int ry = rb + pr, py = y0 + ry;
            if (py >= H || px >= W) continue;
            // weight / bias gradients at output q = (py, px)
            float gp[3];
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) gp[ch] = SG(ch, ry + 1, c + 1);
#pragma unroll
            for (int oc = 0; oc < 3; ++oc) bacc[oc] += gp[oc];
            // input gradient at p = (py, px): the correlation sum_{oc,k} W[oc][i][k] G[oc][p - d_k]
            // (G is zero outside the image); border pixels get the rest after the row loop
            float gi[3] = {0.f, 0.f, 0.f};
#if !defined(CCMI_DIAG_SPB_NODX)
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                const int ky = k / 3, kx = k % 3;
#pragma unroll
                for (int oc = 0; oc < 3; ++oc) {
                    const float gq = SG(oc, ry + 2 - ky, c + 2 - kx);
#pragma unroll
                    for (int i = 0; i < 3; ++i) gi[i] = fmaf(P[wo + (oc * 3 + i) * 9 + k], gq, gi[i]);
                }
            }
#endif
            const int64_t pi = (int64_t)py * W + px;
            // mask_in (MODE bit 8): the previous layer's ReLU
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const float v = gi[i] + (res ? gp[i] : 0.f);
                Ib[i * npx + pi] = (mask_in && SX(i, ry + 1, c + 1) <= 0.f) ? 0.f : v;
            }
        }
#if !defined(CCMI_DIAG_SPB_NODX) && !defined(CCMI_DIAG_SPB_NOBORDER)
        // What the replicate padding clamps onto a border pixel -- the padded-domain adjoint at the
        // ring positions r with clamp(r) = p: above the top row the kernel's row 0 against G's row
        // py, below the bottom row its row 2, left / right of the image its column 0 / 2 against G's
        // column px, at a corner the one corner tap against G(p); a 1-pixel image side takes both of
        // its edges' terms.  (The qrange enumeration's sums in another order.)  Added after the
        // barrier by one thread per border pixel of a tile that touches the image border -- inside
        // the row loop, a border lane held up its whole wave (profiles/r5ze_*, r5zf_*).  Slots:
        // threads [0, 64) the top row, [64, 128) the bottom row, [128, 144) / [144, 160) the left /
        // right column without those rows; the barrier orders the rows' global writes before these.
        {
            const int rbot = H - 1 - y0, crt = W - 1 - x0; // the image's last row / column in tile coordinates
            const bool etop = y0 == 0, ebot = rbot < kSY, elft = x0 == 0, ergt = crt < kSX;
            if (etop || ebot || elft || ergt) { // workgroup-uniform
                __syncthreads();
                const int t = threadIdx.x;
                int ry = -1, cx = -1;
                if (t < kSX) {
                    if (etop) ry = 0, cx = t;
                } else if (t < 2 * kSX) {
                    if (ebot && !(etop && rbot == 0)) ry = rbot, cx = t - kSX;
                } else if (t < 2 * kSX + kSY) {
                    const int r = t - 2 * kSX;
                    if (elft && y0 + r != 0 && r != rbot) ry = r, cx = 0;
                } else if (t < 2 * kSX + 2 * kSY) {
                    const int r = t - 2 * kSX - kSY;
                    if (ergt && !(elft && crt == 0) && y0 + r != 0 && r != rbot) ry = r, cx = crt;
                }
                const int by = y0 + ry, bx = x0 + cx;
                if (ry >= 0 && by < H && bx < W) {
                    const bool top = by == 0, bot = by == H - 1, lft = bx == 0, rgt = bx == W - 1;
                    float e[3] = {0.f, 0.f, 0.f};
#pragma unroll
                    for (int oc = 0; oc < 3; ++oc) {
                        const float *Wk = s_wt + oc * 27;
                        const float gq = SG(oc, ry + 1, cx + 1);
#pragma unroll
                        for (int i = 0; i < 3; ++i) {
                            const float *Wi = Wk + i * 9; // Wi[3 ky + kx]
#pragma unroll
                            for (int u = 0; u < 3; ++u) {
                                const float wr = (top ? Wi[u] : 0.f) + (bot ? Wi[6 + u] : 0.f);
                                const float wc = (lft ? Wi[3 * u] : 0.f) + (rgt ? Wi[3 * u + 2] : 0.f);
                                e[i] = fmaf(wr, SG(oc, ry + 1, cx + 2 - u), e[i]);
                                e[i] = fmaf(wc, SG(oc, ry + 2 - u, cx + 1), e[i]);
                            }
                            const float wy0 = top ? 1.f : 0.f, wy2 = bot ? 1.f : 0.f;
                            const float wcn = (lft ? wy0 * Wi[0] + wy2 * Wi[6] : 0.f) + (rgt ? wy0 * Wi[2] + wy2 * Wi[8] : 0.f);
                            e[i] = fmaf(wcn, gq, e[i]);
                        }
                    }
                    const int64_t pi = (int64_t)by * W + bx;
#pragma unroll
                    for (int i = 0; i < 3; ++i) // a masked pixel was written 0 and stays 0
                        Ib[i * npx + pi] += (mask_in && SX(i, ry + 1, cx + 1) <= 0.f) ? 0.f : e[i];
                }
            }
        }
#endif
    }
    // block reduction of the 84 weight / bias gradients
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    // lane l < 27 and lane l + 28 (the same column quad, the other stream) hold column n = l;
    // register r is row oc = r
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const float v = dacc[r] + __shfl(dacc[r], (lane + 28) & 63);
        if (lane < 27) s_red[wid][r * 27 + lane] = v;
    }
#pragma unroll
    for (int oc = 0; oc < 3; ++oc) {
        const float v = wave_sum(bacc[oc]);
        if (lane == 0) s_red[wid][81 + oc] = v;
    }
    __syncthreads();
    if (threadIdx.x < 84) {
        const int e = threadIdx.x;
        const float v = s_red[0][e] + s_red[1][e] + s_red[2][e] + s_red[3][e];
        float *dst = gth + ((int64_t)b * kDwSlots + blockIdx.x % kDwSlots) * gstride; // this workgroup's slot row
        atomicAdd(&dst[e < 81 ? wo + e : bo + (e - 81)], v);
    }
}
#undef SX
#undef SG

// the 3x3 backward as a persistent prefetching grid (t_sp_bwd<7>) or one tile per workgroup
// (t_sp_bwd<3>); CCMI_SP_BWD_PF=0 selects the latter (A/B)
bool sp_bwd_persistent()
{
    const char *e = getenv("CCMI_SP_BWD_PF");
    return !(e && *e == '0');
}

} // namespace

// fused_loss (the last layer of a training step): the MSE in the same pass -- no separate t_loss
// over the synthesis output, which is stored only when something reads it
void ccmi_train::launch_sp_fwd(const Geo &g, const ccmi_train_args &a, const Work &w, int i, bool fused_loss, hipStream_t s)
{
    const int store = !fused_loss || a.raw_out || g.sp_relu[i];
    const dim3 grid(grid1((int64_t)ccmi_div_up(g.H, kSpRows) * g.W, 1).x * a.batch);
    auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, dim3(kT), 0, s, w.z[i], g, a.params, a.param_stride, g.sp_w[i], g.sp_b[i], g.sp_res[i],
                           g.sp_relu[i], w.z[i + 1], a.target, a.target_stride, 2.f / loss_samples(g, a.yuv420), w.graw, w.mslots,
                           store);
    };
    if (!fused_loss) go(t_sp_fwd<0>);
    else if (a.yuv420) go(t_sp_fwd<2>);
    else go(t_sp_fwd<1>);
}

void ccmi_train::launch_loss(const Geo &g, const ccmi_train_args &a, const Work &w, hipStream_t s)
{
    hipLaunchKernelGGL(t_loss, dim3(sum_blocks((int64_t)g.H * g.W, kLossPx), a.batch), dim3(kT), 0, s, w.z[g.n_sp], g, a.target,
                       a.target_stride, a.yuv420, w.graw, w.acc4);
}

// Both halves in one launch: each tile's X / G / out read once
void ccmi_train::launch_sp_bwd(const Geo &g, const ccmi_train_args &a, const Work &w, int i, const float *gout, float *gin,
                               hipStream_t s)
{
    const int ntile = ccmi_div_up(g.W, kSX) * ccmi_div_up(g.H, kSY), B = a.batch;
    // a ReLU layer's mask comes from its output planes only for the last layer (its output
    // gradient is the loss's); for the others the next layer's backward applied it (mask_in)
    const float *outp = g.sp_relu[i] && i == g.n_sp - 1 ? w.z[i + 1] : nullptr;
    const bool mask_in = i >= 1 && g.sp_relu[i - 1];
    const bool persistent = sp_bwd_persistent();
    const auto k = persistent ? (mask_in ? t_sp_bwd<15> : t_sp_bwd<7>) : (mask_in ? t_sp_bwd<11> : t_sp_bwd<3>);
    const dim3 grid = persistent ? resident_grid((const void *)k, kT, 0, ntile, B) : dim3((unsigned)ntile, B);
    hipLaunchKernelGGL(k, grid, dim3(kT), 0, s, gout, outp, w.z[i], g, a.params, a.param_stride, g.sp_w[i], g.sp_b[i], g.sp_res[i],
                       gin, w.slots, (int64_t)g.P);
}
