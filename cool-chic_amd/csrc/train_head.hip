// train_head.hip -- the overfit step's 1x1 synthesis head (C -> hid -> 3, synthesis.py:264-277):
// t_head_fwd, and the backward in three forms -- t_head_bwd_t (LDS-tiled, the default for a
// linear output layer), t_head_bwd_m (register form, CCMI_HEAD_BWD_REGS=1) and t_head_bwd
// (full width, output-ReLU architectures).  launch_head_fwd / launch_head_bwd own the
// CIN x hidden-tile ladder, the choice of form and the dynamic-LDS sizes.
#include <stdlib.h>

#include <cmath>

#include "fwd_common.h"
#include "train_internal.h"

using namespace ccmi_train;
using ccmi_fwd::cfloat_ptr;

namespace {

// Four pixels per thread (p + u kT of the workgroup's 4 kT, u = 0..3, as two packed pairs):
// each broadcast weight record serves four pixels, a quarter of the one-pixel form's LDS record
// traffic per pixel (that form sat 56 % of its wave cycles in SQ_WAIT_INST_LDS, the two-pixel
// form still 55 %, profiles/r5d_train_pmc.txt).  The records and the packed FMAs that take
// their weights in place are the path-A fused kernel's (fwd_common.h, "head weight records"):
// fields dense from slot 0, read as whole ds_read_b128, a unit of two pixel pairs as one
// hidden-chain statement and one statement per output channel.
constexpr int kHeadFwdPx = 4 * kT; // pixels per workgroup
template <int CIN>
__global__ __launch_bounds__(kT) void t_head_fwd(const float *__restrict__ dense, Geo g, const float *__restrict__ th,
                                                 int64_t ps, float *__restrict__ z0)
{
    using ccmi_fwd::f2;
    using ccmi_fwd::f4v;
    using ccmi_fwd::head_hidden2;
    using ccmi_fwd::head_out2;
    using ccmi_fwd::rec_pair;
    using ccmi_fwd::rec_w0_pairs;
    constexpr int kRecVecs = (CIN + 4 + 3) / 4;
    __shared__ __attribute__((aligned(16))) float s_rec[64][16];
    static_assert(CIN + 4 <= 16, "hidden-unit record");
    const int b = blockIdx.y, hid = g.hid;
    const cfloat_ptr P = (cfloat_ptr)(size_t)(th + (int64_t)b * ps);
    for (int e = threadIdx.x; e < 64 * 16; e += kT) {
        const int j = e >> 4, f = e & 15;
        float v = 0.f;
        if (j < hid) {
            if (f < CIN) v = P[g.w0 + j * CIN + f];
            else if (f == CIN) v = P[g.b0 + j];
            else if (f <= CIN + 3) v = P[g.w1 + (f - CIN - 1) * hid + j];
        }
        if (f <= CIN + 3) s_rec[j][f] = v; // other slots are never operands
    }
    const int64_t npx = (int64_t)g.H * g.W, p0 = (int64_t)blockIdx.x * kHeadFwdPx + threadIdx.x;
    const float *x = dense + (int64_t)b * CIN * npx;
    // pair q = pixels p0 + 2q kT, p0 + (2q + 1) kT (zeros past the frame)
    f2 xv[2][CIN];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int64_t pa = p0 + 2 * q * kT, pb = pa + kT;
#pragma unroll
        for (int i = 0; i < CIN; ++i) xv[q][i] = f2{pa < npx ? x[i * npx + pa] : 0.f, pb < npx ? x[i * npx + pb] : 0.f};
    }
    __syncthreads();
    const f2 lo0 = f2(g.r0 ? 0.f : -INFINITY);
    f2 o[2][3];
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int m = 0; m < 3; ++m) o[q][m] = f2(P[g.b1 + m]);
    struct Rec { f4v v[kRecVecs]; };
    // (through an LDS pointer the compiler cannot fold to a constant: base + immediate offsets)
    typedef const __attribute__((address_space(3))) f4v *lds_f4;
    lds_f4 hb = (lds_f4)(&s_rec[0][0]);
    asm volatile("" : "+v"(hb));
    auto load = [&](int j) {
        const lds_f4 p = hb + 4 * (j < 63 ? j : 63);
        Rec r;
#pragma unroll
        for (int i = 0; i < kRecVecs; ++i) r.v[i] = p[i];
        return r;
    };
    auto unit = [&](const Rec &r) __attribute__((always_inline)) {
        f2 w[4], h[2];
        rec_w0_pairs<CIN>(r.v, w);
        head_hidden2<CIN, false>(w, rec_pair<CIN>(r.v), xv[0], xv[1], h[0], h[1]);
        h[0] = __builtin_elementwise_max(h[0], lo0);
        h[1] = __builtin_elementwise_max(h[1], lo0);
        head_out2<(CIN + 1) & 1>(rec_pair<CIN + 1>(r.v), h[0], h[1], o[0][0], o[1][0]);
        head_out2<(CIN + 2) & 1>(rec_pair<CIN + 2>(r.v), h[0], h[1], o[0][1], o[1][1]);
        head_out2<(CIN + 3) & 1>(rec_pair<CIN + 3>(r.v), h[0], h[1], o[0][2], o[1][2]);
    };
    // software pipelined: the records of units j + 2 and j + 3 are read while units j and j + 1
    // compute (an LDS read does not move across the units' statements)
    Rec ra = load(0), rb = load(1);
    for (int j = 0; j < hid; j += 2) {
        unit(ra);
        ra = load(j + 2);
        if (j + 1 < hid) unit(rb);
        rb = load(j + 3);
    }
    float *z = z0 + (int64_t)b * 3 * npx;
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int m = 0; m < 3; ++m) {
            f2 v = o[q][m];
            if (g.r1) v = __builtin_elementwise_max(v, f2(0.f));
            const int64_t pa = p0 + 2 * q * kT, pb = pa + kT;
            if (pa < npx) z[m * npx + pa] = v.x;
            if (pb < npx) z[m * npx + pb] = v.y;
        }
}

// 1x1 head backward.  Per pixel (lane = pixel, VALU): the hidden layer recomputed, g_h and
// g_dense.  The weight gradients are sums over pixels -- GEMMs with K = pixels -- and run on
// the matrix cores (v_mfma_f32_16x16x4_f32, f32 in / f32 accumulate: the same products as
// an fmaf chain, only the summation order differs):
//   dW1[k][j] = sum_px gp[px][k] h[px][j]          (M = k < 3, N = j, one MFMA per 16 j)
//   dW0[j][i] = sum_px gh[px][j] [x[px][i] | 1]    (M = j, N = i <= CIN, column CIN = db0)
// A wave stages its 64 pixels' rows in LDS (pixel-major, pitch kHP: conflict-free writes)
// and feeds 4 pixels per MFMA (K = lane >> 4).  Accumulators live in registers across
// every pixel chunk the workgroup visits (grid-stride) and are flushed once, with one
// atomic per weight per wave.
// diagnostic build (tools/arm_diag.sh; wrong results, timing only): NOHMFMA drops the
// weight-gradient MFMAs
#if defined(CCMI_DIAG_ARM_NOHMFMA)
#define HEAD_MFMA(a, b, c) (c)
#else
#define HEAD_MFMA(a, b, c) mfma4(a, b, c)
#endif
// The per-pixel work runs over PAIRS of hidden units with packed FMAs -- records interleave the
// two units' weights ({w0[j][i], w0[j+1][i]}, {b0[j], b0[j+1]}, {w1[k][j], w1[k][j+1]}), so every
// packed operand is an aligned register pair -- and the output / g_x sums keep one partial
// per unit parity, added at the end: 26 VALU per unit pair instead of the 46 of a unit at a time
// (397 vs 350-383 us per 8-frame iteration).
template <int CIN, int NT>
__global__ __launch_bounds__(kHeadT) void t_head_bwd(const float *__restrict__ dense, const float *__restrict__ gz0, Geo g,
                                                     const float *__restrict__ th, int64_t ps, float *__restrict__ gdense,
                                                     float *__restrict__ gth, int64_t gstride)
{
    // dynamic LDS, per wave: [64][hp] h, then g_h (pixel-major, hp = 16 NT + 1: conflict-free
    // row writes, columns [hid, 16 NT) zero); [64][kXP] gp | 0, then x | 1 | 0.  The zero
    // columns let every lane read its MFMA operand unconditionally (no exec-mask branches
    // between the LDS reads and the MFMAs).
    extern __shared__ float s_dyn[];
    // odd row pitch: conflict-free row writes (lane * kXP covers the 32 banks once per half),
    // and rows s and s + 16 of the MFMA operand reads land 16 banks apart
    constexpr int kXP = (CIN + 2 > 5 ? CIN + 2 : 5) | 1;
    // hidden unit j: w0[j][0..CIN), b0[j], w1[0..3)[j] -- read back as broadcast ds_read_b128
    // (sized for the 16 NT units of the instantiation: 2.3 KB at NT = 3, where 64 units' worth
    // put the workgroup at exactly 32 KB and five per CU did not fit)
    __shared__ __attribute__((aligned(16))) float s_rec[16 * NT][12];
    static_assert(CIN + 4 <= 12, "hidden-unit record");
    const int b = blockIdx.y, t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int hid = g.hid; // NT = ceil(hid / 16), a template argument: the accumulator tiles
                           // must be compile-time registers
    constexpr int hp = 16 * NT + 1;
    const int64_t npx = (int64_t)g.H * g.W;
    const float *P = th + (int64_t)b * ps;
    using ccmi_fwd::f2;
    // pair records: unit pair jp = units 2jp, 2jp + 1, field f interleaved as [2f + parity]
    constexpr int kPR = 2 * (CIN + 4) <= 24 ? 24 : 32;
    float(*s_rec2)[kPR] = reinterpret_cast<float(*)[kPR]>(&s_rec[0][0]);
    static_assert(8 * NT * kPR <= 16 * NT * 12, "pair records fit in the record area");
    for (int e = t; e < 8 * NT * kPR; e += kHeadT) {
        const int jp = e / kPR, r = e - jp * kPR, f = r >> 1, j = 2 * jp + (r & 1);
        float v = 0.f;
        if (j < hid) {
            if (f < CIN) v = P[g.w0 + j * CIN + f];
            else if (f == CIN) v = P[g.b0 + j];
            else if (f <= CIN + 3) v = P[g.w1 + (f - CIN - 1) * hid + j];
        }
        s_rec2[jp][r] = v;
    }
    const float bo0 = P[g.b1], bo1 = P[g.b1 + 1], bo2 = P[g.b1 + 2];
    float *sv = s_dyn + w * 64 * (hp + kXP), *sw = sv + 64 * hp;
    const int ln = lane & 15, lk = lane >> 4;
    for (int j = hid; j < 16 * NT; ++j) sv[lane * hp + j] = 0.f; // pad columns of this lane's row
    const int ia = ln < 3 ? ln : 3, ib = ln <= CIN ? ln : CIN + 1; // operand columns (pads read 0)
    v4f a1[NT], a0[NT];
#pragma unroll
    for (int q = 0; q < NT; ++q) a1[q] = a0[q] = v4f{0.f, 0.f, 0.f, 0.f};
    float db1[3] = {0.f, 0.f, 0.f};
    __syncthreads(); // s_rec staged
    const int64_t nchunk = (npx + kHeadT - 1) / kHeadT;
    // the next chunk's pixel inputs (x, g_out) are loaded into registers while this one is
    // processed: at 2 waves / SIMD (LDS-bound) the loads' latency was left exposed per chunk
    float nx[CIN], ng[3];
    auto load_chunk = [&](int64_t ch) {
        const int64_t p = ch * kHeadT + t;
        const bool valid = p < npx;
        const float *x = dense + (int64_t)b * CIN * npx + p;
        const float *G = gz0 + (int64_t)b * 3 * npx + p;
#pragma unroll
        for (int i = 0; i < CIN; ++i) nx[i] = valid ? x[i * npx] : 0.f;
#pragma unroll
        for (int k = 0; k < 3; ++k) ng[k] = valid ? G[k * npx] : 0.f;
    };
    if ((int64_t)blockIdx.x < nchunk) load_chunk(blockIdx.x);
    for (int64_t ch = blockIdx.x; ch < nchunk; ch += gridDim.x) {
        const int64_t p = ch * kHeadT + t;
        const bool valid = p < npx;
        float xv[CIN], gp1[3];
#pragma unroll
        for (int i = 0; i < CIN; ++i) xv[i] = nx[i];
#pragma unroll
        for (int k = 0; k < 3; ++k) gp1[k] = ng[k];
        if (ch + gridDim.x < nchunk) load_chunk(ch + gridDim.x);
        // ---- hidden layer (kept in this lane's LDS row) and the output pre-activations
        float o0 = bo0, o1 = bo1, o2 = bo2;
        {
            const f2 lo0 = f2(g.r0 ? 0.f : -INFINITY);
            f2 op[3] = {f2(0.f), f2(0.f), f2(0.f)};
#pragma unroll 2
            for (int jp = 0; jp < (hid + 1) / 2; ++jp) {
                const f2 *r = reinterpret_cast<const f2 *>(s_rec2[jp]);
                f2 a = r[CIN];
#pragma unroll
                for (int i = 0; i < CIN; ++i) a = __builtin_elementwise_fma(r[i], f2(xv[i]), a);
                a = __builtin_elementwise_max(a, lo0);
                sv[lane * hp + 2 * jp] = a.x;
                sv[lane * hp + 2 * jp + 1] = a.y;
#pragma unroll
                for (int k = 0; k < 3; ++k) op[k] = __builtin_elementwise_fma(r[CIN + 1 + k], a, op[k]);
            }
            o0 += op[0].x + op[0].y;
            o1 += op[1].x + op[1].y;
            o2 += op[2].x + op[2].y;
        }
        if (g.r1) {
            if (o0 <= 0.f) gp1[0] = 0.f;
            if (o1 <= 0.f) gp1[1] = 0.f;
            if (o2 <= 0.f) gp1[2] = 0.f;
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) db1[k] += gp1[k];
        // ---- dW1 += gp^T h (invalid pixels have gp = 0)
#pragma unroll
        for (int k = 0; k < 3; ++k) sw[lane * kXP + k] = gp1[k];
        sw[lane * kXP + 3] = 0.f;
        wave_lds_sync();
        // K = pixels in the order px = s + 16 (lane >> 4): the two 16-lane groups of each
        // 32-lane half read rows 16 apart, i.e. 16 banks apart (pitches hp, kXP odd)
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            const int px = s + 16 * lk;
            const float a = sw[px * kXP + ia];
#pragma unroll
            for (int q = 0; q < NT; ++q) a1[q] = HEAD_MFMA(a, sv[px * hp + 16 * q + ln], a1[q]);
        }
        wave_lds_sync();
        // ---- g_h (replaces h in this lane's row), g_x
        float gxv[CIN];
#pragma unroll
        for (int i = 0; i < CIN; ++i) gxv[i] = 0.f;
        {
            f2 gxp[CIN];
#pragma unroll
            for (int i = 0; i < CIN; ++i) gxp[i] = f2(0.f);
#pragma unroll 2
            for (int jp = 0; jp < (hid + 1) / 2; ++jp) {
                const f2 *r = reinterpret_cast<const f2 *>(s_rec2[jp]);
                f2 gh = r[CIN + 1] * f2(gp1[0]);
                gh = __builtin_elementwise_fma(r[CIN + 2], f2(gp1[1]), gh);
                gh = __builtin_elementwise_fma(r[CIN + 3], f2(gp1[2]), gh);
                float *row = sv + lane * hp + 2 * jp;
                if (g.r0) {
                    if (row[0] <= 0.f) gh.x = 0.f;
                    if (row[1] <= 0.f) gh.y = 0.f;
                }
                row[0] = gh.x;
                row[1] = gh.y;
#pragma unroll
                for (int i = 0; i < CIN; ++i) gxp[i] = __builtin_elementwise_fma(r[i], gh, gxp[i]);
            }
#pragma unroll
            for (int i = 0; i < CIN; ++i) gxv[i] = gxp[i].x + gxp[i].y;
        }
        if (valid) {
            float *gd = gdense + (int64_t)b * CIN * npx + p;
#pragma unroll
            for (int i = 0; i < CIN; ++i) gd[i * npx] = gxv[i];
        }
        // ---- dW0 | db0 += g_h^T [x | 1]
#pragma unroll
        for (int i = 0; i < CIN; ++i) sw[lane * kXP + i] = xv[i];
        sw[lane * kXP + CIN] = 1.f;
        sw[lane * kXP + CIN + 1] = 0.f;
        wave_lds_sync();
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            const int px = s + 16 * lk;
            const float bb = sw[px * kXP + ib];
#pragma unroll
            for (int q = 0; q < NT; ++q) a0[q] = HEAD_MFMA(sv[px * hp + 16 * q + ln], bb, a0[q]);
        }
        wave_lds_sync();
    }
    // ---- flush: accumulator register r of lane l holds D[m = 4 (l >> 4) + r][n = l & 15].
    // The waves' partial sums meet in LDS (each wave's own rows, free after the chunk loop),
    // then ONE atomic per value per workgroup (one per wave put every workgroup of a frame on
    // the same few hundred addresses -- the t_arm16 flush lesson, profiles/r4l_*)
    // partial row: w0 [hid][CIN] | b0 [hid] | w1 [3][hid] | b1 [3]
    const int nred = hid * (CIN + 4) + 3;
    float *red = s_dyn + w * 64 * (hp + kXP);
    static_assert(64 * (hp + kXP) >= 16 * NT * (CIN + 4) + 3, "a wave's partial row fits its LDS rows");
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NT; ++q) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = 4 * lk + r;
            if (m < 3) { // dW1[k = m][j]
                const int j = 16 * q + ln;
                if (j < hid) red[hid * (CIN + 1) + m * hid + j] = a1[q][r];
            }
            const int j = 16 * q + m; // dW0[j][i = ln]
            if (j < hid) {
                if (ln < CIN) red[j * CIN + ln] = a0[q][r];
                else if (ln == CIN) red[hid * CIN + j] = a0[q][r];
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float v = db1[k];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if (lane == 0) red[hid * (CIN + 4) + k] = v;
    }
    __syncthreads();
    float *Gp = gth + ((int64_t)b * kDwSlots + blockIdx.x % kDwSlots) * gstride; // this workgroup's slot row
    constexpr int kW = kHeadT / 64;
    for (int e = t; e < nred; e += kHeadT) {
        float v = 0.f;
#pragma unroll
        for (int ww = 0; ww < kW; ++ww) v += s_dyn[ww * 64 * (hp + kXP) + e];
        const int dst = e < hid * CIN ? g.w0 + e
                        : e < hid * (CIN + 1) ? g.b0 + (e - hid * CIN)
                        : e < hid * (CIN + 4) ? g.w1 + (e - hid * (CIN + 1))
                                              : g.b1 + (e - hid * (CIN + 4));
        atomicAdd(&Gp[dst], v);
    }
}

// Register form (the one launched for a linear output layer): no LDS round trip between the
// hidden layer and the matrix cores.  Per 16-pixel block a wave evaluates the hidden layer TWICE
// on v_mfma_f32_16x16x4_f32 (K = the CIN inputs + the constant 1 of the bias, two K-steps), with
// the same operand registers in swapped roles:
//   layout B: Z^T = W0 X, accumulator register r of lane l = unit 16 t + 4 (l >> 4) + r of pixel
//     l & 15 -- g_h in this layout is exactly the A operand of g_x = g_h W0 with the K order
//     permuted (K-step r takes units 16 t + 4 g + r from lane group g), so g_x comes out of the
//     matrix cores with no data movement;
//   layout A: Z = X^T W0^T, register r of lane l = pixel 4 (l >> 4) + r of unit 16 t + (l & 15) --
//     g_h here is the A operand of dW0 = g_h^T [x | 1] with K = the pixels (K-step r takes
//     pixel 4 g + r from lane group g), and dW1 = g_out h^T is 12 VALU FMAs into per-lane
//     partial sums (3 outputs: a matrix core would be 13/16 padding).
// Two hidden-layer evaluations cost 4 MFMA per 16-unit tile; what they replace is the LDS staging
// of every tile (WAIT_INST_LDS 17 % of the tiled form's wave cycles, profiles/r5zk_train_pmc.txt).
template <int CIN, int NT>
__global__ __launch_bounds__(256) void t_head_bwd_m(const float *__restrict__ dense, const float *__restrict__ gz0, Geo g,
                                                    const float *__restrict__ th, int64_t ps, float *__restrict__ gdense,
                                                    float *__restrict__ gth, int64_t gstride)
{
    static_assert(CIN + 1 <= 8, "inputs + bias in two K-steps of 4");
    constexpr int kU = 16 * NT, kRedN = kU * (CIN + 4) + 3;
    __shared__ __attribute__((aligned(16))) float s_w1[3][kU];
    __shared__ float s_red[4][kRedN];
    const int b = blockIdx.y, t = threadIdx.x, lane = t & 63, w = t >> 6, i = lane & 15, gq = lane >> 4;
    const int hid = g.hid;
    const int64_t npx = (int64_t)g.H * g.W;
    const cfloat_ptr P = (cfloat_ptr)(size_t)(th + (int64_t)b * ps);
    for (int e = t; e < 3 * kU; e += 256) {
        const int k = e / kU, u = e - k * kU;
        s_w1[k][u] = u < hid ? P[g.w1 + k * hid + u] : 0.f;
    }
    // per-lane constants: aB[tt][s] = W0|b0 [unit 16 tt + i][input 4 s + gq] (A of layout B, B of
    // layout A); bG[tt][r] = W0[unit 16 tt + 4 gq + r][input i] (B of g_x); w1A[tt][k] = W1[k][16 tt + i]
    float aB[NT][2], bG[NT][4], w1A[NT][3];
#pragma unroll
    for (int tt = 0; tt < NT; ++tt) {
        const int u = 16 * tt + i;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int c = 4 * s + gq;
            aB[tt][s] = u < hid ? (c < CIN ? P[g.w0 + u * CIN + c] : c == CIN ? P[g.b0 + u] : 0.f) : 0.f;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int ur = 16 * tt + 4 * gq + r;
            bG[tt][r] = (ur < hid && i < CIN) ? P[g.w0 + ur * CIN + i] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) w1A[tt][k] = u < hid ? P[g.w1 + k * hid + u] : 0.f;
    }
    const bool relu = g.r0 != 0;
    v4f dw0[NT];
    float acc1[NT][3], db1[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int tt = 0; tt < NT; ++tt) {
        dw0[tt] = v4f{0.f, 0.f, 0.f, 0.f};
        acc1[tt][0] = acc1[tt][1] = acc1[tt][2] = 0.f;
    }
    __syncthreads(); // s_w1 staged
    const float *xg = dense + (int64_t)b * CIN * npx;
    const float *gpg = gz0 + (int64_t)b * 3 * npx;
    float *gdb = gdense + (int64_t)b * CIN * npx;
    const int64_t nblk = (npx + 15) >> 4, wstride = (int64_t)gridDim.x * 4;
    for (int64_t blk = (int64_t)blockIdx.x * 4 + w; blk < nblk; blk += wstride) {
        const int64_t p0 = blk << 4, pi = p0 + i, pa = p0 + 4 * gq;
        // X[input 4 s + gq][pixel p0 + i] (0 past the frame, bias input included)
        float xb[2];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int c = 4 * s + gq;
            xb[s] = pi >= npx ? 0.f : c < CIN ? xg[c * npx + pi] : c == CIN ? 1.f : 0.f;
        }
        float gpT[3], gpA[3][4], xA[4];
#pragma unroll
        for (int k = 0; k < 3; ++k) gpT[k] = pi < npx ? gpg[k * npx + pi] : 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const bool v = pa + r < npx;
#pragma unroll
            for (int k = 0; k < 3; ++k) gpA[k][r] = v ? gpg[k * npx + pa + r] : 0.f;
            xA[r] = !v ? 0.f : i < CIN ? xg[i * npx + pa + r] : i == CIN ? 1.f : 0.f;
        }
        if (gq == 0) {
#pragma unroll
            for (int k = 0; k < 3; ++k) db1[k] += gpT[k];
        }
        v4f gx = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int tt = 0; tt < NT; ++tt) {
            v4f zT = mfma4(aB[tt][0], xb[0], v4f{0.f, 0.f, 0.f, 0.f});
            zT = mfma4(aB[tt][1], xb[1], zT);
            v4f zA = mfma4(xb[0], aB[tt][0], v4f{0.f, 0.f, 0.f, 0.f});
            zA = mfma4(xb[1], aB[tt][1], zA);
            // layout B: g_h of units 16 tt + 4 gq + r at pixel i, then g_x += g_h W0
            const v4f wk0 = *reinterpret_cast<const v4f *>(&s_w1[0][16 * tt + 4 * gq]);
            const v4f wk1 = *reinterpret_cast<const v4f *>(&s_w1[1][16 * tt + 4 * gq]);
            const v4f wk2 = *reinterpret_cast<const v4f *>(&s_w1[2][16 * tt + 4 * gq]);
            float ghT[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float sgh = fmaf(wk2[r], gpT[2], fmaf(wk1[r], gpT[1], wk0[r] * gpT[0]));
                ghT[r] = (!relu || zT[r] > 0.f) ? sgh : 0.f;
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) gx = mfma4(ghT[r], bG[tt][r], gx);
            // layout A: h and g_h of unit 16 tt + i at pixels 4 gq + r; dW1 partials, dW0 += g_h^T [x | 1]
            float ghA[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float h = relu ? fmaxf(zA[r], 0.f) : zA[r];
#pragma unroll
                for (int k = 0; k < 3; ++k) acc1[tt][k] = fmaf(gpA[k][r], h, acc1[tt][k]);
                const float sgh = fmaf(w1A[tt][2], gpA[2][r], fmaf(w1A[tt][1], gpA[1][r], w1A[tt][0] * gpA[0][r]));
                ghA[r] = (!relu || zA[r] > 0.f) ? sgh : 0.f;
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) dw0[tt] = mfma4(ghA[r], xA[r], dw0[tt]);
        }
        // g_x: register r of lane l = pixel 4 gq + r, input i
        if (i < CIN) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (pa + r < npx) gdb[i * npx + pa + r] = gx[r];
        }
    }
    // ---- flush: this wave's partial row (w0 [hid][CIN] | b0 [hid] | w1 [3][hid] | b1 [3]), the
    // four waves summed in LDS, one atomic per value per workgroup into its slot row
    float *red = s_red[w];
    const int nred = hid * (CIN + 4) + 3;
    for (int e = lane; e < nred; e += 64) red[e] = 0.f;
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int tt = 0; tt < NT; ++tt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int u = 16 * tt + 4 * gq + r; // dW0[u][c = i]
            if (u < hid) {
                if (i < CIN) red[u * CIN + i] = dw0[tt][r];
                else if (i == CIN) red[hid * CIN + u] = dw0[tt][r];
            }
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            float v = acc1[tt][k];
            v += __shfl_xor(v, 16);
            v += __shfl_xor(v, 32);
            const int u = 16 * tt + i;
            if (gq == 0 && u < hid) red[hid * (CIN + 1) + k * hid + u] = v;
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float v = wave_sum(db1[k]);
        if (lane == 0) red[hid * (CIN + 4) + k] = v;
    }
    __syncthreads();
    float *Gp = gth + ((int64_t)b * kDwSlots + blockIdx.x % kDwSlots) * gstride; // this workgroup's slot row
    for (int e = t; e < nred; e += 256) {
        const float v = (s_red[0][e] + s_red[1][e]) + (s_red[2][e] + s_red[3][e]);
        const int dst = e < hid * CIN ? g.w0 + e
                        : e < hid * (CIN + 1) ? g.b0 + (e - hid * CIN)
                        : e < hid * (CIN + 4) ? g.w1 + (e - hid * (CIN + 1))
                                              : g.b1 + (e - hid * (CIN + 4));
        atomicAdd(&Gp[dst], v);
    }
}

// Tiled form (the one launched): the hidden layer stays in registers (pairs of units, packed
// FMAs, as the PAIR form), and the LDS that feeds the weight-gradient MFMAs holds ONE 16-unit
// tile at a time next to the pixel fields gp | 0 | x | 1 shared by both MFMA loops: 8.2 KB of
// LDS per wave instead of 14.8 KB (LDS had capped the full-width form at 2.5 waves / SIMD with
// 55 % of its wave cycles in WAIT_ANY; profiles/r4w_train_pmc.txt).  Both are stored
// pixel-minor -- one row of the wave's 64 pixels per unit / field, pitch 68 -- so a lane's
// writes are consecutive across the wave and an MFMA loop reads its operands for four K-steps
// (4 pixels) with one 128-bit read each (the 16 lanes of a read start 4 banks apart).
// Per tile q: h -> dW1 tile (M = k < 3, N = the tile's units) -> g_h (the ReLU mask from the
// registers) -> dW0 tile (M = the tile's units, N = i <= CIN) and this pixel's g_x.
// Both products run on the 4x4x1 sixteen-block MFMA (blocks = pixel streams x unit / column
// quads, the streams summed once at the flush): on 16x16x4 the dW1 tile used 3 of 16 rows and
// the dW0 tile 8 of 16 columns, 1,024 MFMA cycles per tile and wave; now 128 + 256.
// The output layer must be linear (g.r1 == 0, every reference architecture's "X-1-linear-none"):
// then g_out needs no pass over all units first, and a tile's units are computed just in time.
constexpr int kHbXP = 68;
constexpr int head_bwd_t_wave_floats(int cin) { return (16 + 4 + cin + 1) * kHbXP; }

template <int CIN, int NT>
__global__ __launch_bounds__(kHeadT, 4) void t_head_bwd_t(const float *__restrict__ dense, const float *__restrict__ gz0,
                                                       Geo g, const float *__restrict__ th, int64_t ps,
                                                       float *__restrict__ gdense, float *__restrict__ gth, int64_t gstride)
{
    extern __shared__ float s_dyn[];
    constexpr int kXP = kHbXP;         // row pitch (64 pixels + 4)
    constexpr int kGX = 4;             // first x row
    constexpr int kWF = head_bwd_t_wave_floats(CIN);
    __shared__ __attribute__((aligned(16))) float s_rec[16 * NT][12];
    static_assert(CIN + 4 <= 12, "hidden-unit record");
    constexpr int kPR = 2 * (CIN + 4) <= 24 ? 24 : 32;
    static_assert(8 * NT * kPR <= 16 * NT * 12, "pair records fit in the record area");
    float(*s_rec2)[kPR] = reinterpret_cast<float(*)[kPR]>(&s_rec[0][0]);
    const int b = blockIdx.y, t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int hid = g.hid;
    const int64_t npx = (int64_t)g.H * g.W;
    const float *P = th + (int64_t)b * ps;
    // pair records: unit pair jp = units 2jp, 2jp + 1, field f interleaved as [2f + parity];
    // units >= hid are zero records (h = 0: no contribution anywhere)
    for (int e = t; e < 8 * NT * kPR; e += kHeadT) {
        const int jp = e / kPR, r = e - jp * kPR, f = r >> 1, j = 2 * jp + (r & 1);
        float v = 0.f;
        if (j < hid) {
            if (f < CIN) v = P[g.w0 + j * CIN + f];
            else if (f == CIN) v = P[g.b0 + j];
            else if (f <= CIN + 3) v = P[g.w1 + (f - CIN - 1) * hid + j];
        }
        s_rec2[jp][r] = v;
    }
    // sv: [16 units][64 px] (the tile's h, then its g_h); sw: [field][64 px]
    float *sv = s_dyn + w * kWF, *sw = sv + 16 * kXP;
    const int ln = lane & 15, lk = lane >> 4;
    // weight gradients on v_mfma_f32_4x4x1_16b (mfma4x4), 4x4 blocks bk = lane >> 2:
    //  dW1: block (pixel stream lk, unit quad), A = gp k = lane & 3 (3: the zero row 3),
    //       B = h of unit ln; stream lk covers pixels 16 lk .. 16 lk + 15
    //  dW0: block (pixel stream s0, column quad iq, unit quad), A = g_h of unit ln, B = x | 1
    //       column 4 iq + (lane & 3) (> CIN: the zero row 3); kNQ column quads, 4 / kNQ
    //       streams of kPS pixels each
    constexpr int kNQ = CIN + 1 <= 4 ? 1 : CIN + 1 <= 8 ? 2 : 4, kPS = 16 * kNQ;
    const int iq = lk % kNQ, s0 = lk / kNQ, ic = 4 * iq + (lane & 3);
    const int ia = (lane & 3) < 3 ? (lane & 3) : 3, ib = ic <= CIN ? kGX + ic : 3;
    // constant rows: 0 (row 3), 1 (row kGX + CIN), written once
    sw[3 * kXP + lane] = 0.f;
    sw[(kGX + CIN) * kXP + lane] = 1.f;
    typedef float v4 __attribute__((ext_vector_type(4)));
    v4f a1[NT], a0[NT];
#pragma unroll
    for (int q = 0; q < NT; ++q) a1[q] = a0[q] = v4f{0.f, 0.f, 0.f, 0.f};
    float db1[3] = {0.f, 0.f, 0.f};
    __syncthreads(); // records staged
    const int64_t nchunk = (npx + kHeadT - 1) / kHeadT;
    float nx[CIN], ng[3];
    auto load_chunk = [&](int64_t ch) {
        const int64_t p = ch * kHeadT + t;
        const bool valid = p < npx;
        const float *x = dense + (int64_t)b * CIN * npx + p;
        const float *G = gz0 + (int64_t)b * 3 * npx + p;
#pragma unroll
        for (int i = 0; i < CIN; ++i) nx[i] = valid ? x[i * npx] : 0.f;
#pragma unroll
        for (int k = 0; k < 3; ++k) ng[k] = valid ? G[k * npx] : 0.f;
    };
    using ccmi_fwd::f2;
    const f2 lo0 = f2(g.r0 ? 0.f : -INFINITY);
    if ((int64_t)blockIdx.x < nchunk) load_chunk(blockIdx.x);
    for (int64_t ch = blockIdx.x; ch < nchunk; ch += gridDim.x) {
        const int64_t p = ch * kHeadT + t;
        const bool valid = p < npx;
        float xv[CIN], gp1[3];
#pragma unroll
        for (int i = 0; i < CIN; ++i) xv[i] = nx[i];
#pragma unroll
        for (int k = 0; k < 3; ++k) gp1[k] = ng[k];
        if (ch + gridDim.x < nchunk) load_chunk(ch + gridDim.x);
#pragma unroll
        for (int k = 0; k < 3; ++k) db1[k] += gp1[k];
        // ---- this pixel's column: gp, x (invalid pixels: gp = 0, x = 0)
#pragma unroll
        for (int k = 0; k < 3; ++k) sw[k * kXP + lane] = gp1[k];
#pragma unroll
        for (int i = 0; i < CIN; ++i) sw[(kGX + i) * kXP + lane] = xv[i];
        f2 gxp[CIN];
#pragma unroll
        for (int i = 0; i < CIN; ++i) gxp[i] = f2(0.f);
#pragma unroll
        for (int q = 0; q < NT; ++q) {
            // the tile's records through an opaque base: the compiler must not keep them (or the
            // other tiles') loaded across the chunk
            int roff = 0;
            asm volatile("" : "+s"(roff));
            const float(*rec)[kPR] = s_rec2 + 8 * q + roff;
            float *col = sv + lane; // unit u of this pixel at col[u * kXP]
            // ---- the tile's hidden units h (pairs, packed FMAs) -> this lane's row; only the
            // ReLU mask stays in a register (bit 2u + parity)
            uint32_t hmask = 0;
#pragma unroll 2
            for (int u = 0; u < 8; ++u) {
                const f2 *r = reinterpret_cast<const f2 *>(rec[u]);
                f2 a = r[CIN];
#pragma unroll
                for (int i = 0; i < CIN; ++i) a = __builtin_elementwise_fma(r[i], f2(xv[i]), a);
                a = __builtin_elementwise_max(a, lo0);
                col[(2 * u) * kXP] = a.x;
                col[(2 * u + 1) * kXP] = a.y;
                hmask |= ((a.x > 0.f ? 1u : 0u) | (a.y > 0.f ? 2u : 0u)) << (2 * u);
            }
            wave_lds_sync();
            // ---- dW1 tile q += gp^T h, per pixel stream; four MFMAs per pair of 128-bit reads
#pragma unroll
            for (int s = 0; s < 16; s += 4) {
                const v4 av = *reinterpret_cast<const v4 *>(sw + ia * kXP + 16 * lk + s);
                const v4 bv = *reinterpret_cast<const v4 *>(sv + ln * kXP + 16 * lk + s);
#pragma unroll
                for (int e = 0; e < 4; ++e) a1[q] = mfma4x4(av[e], bv[e], a1[q]);
            }
            wave_lds_sync(); // every lane has read the h rows before g_h replaces them
            // ---- g_h of the tile (replaces h in this lane's row) and g_x
            const uint32_t keep = g.r0 ? hmask : 0xFFFFu;
#pragma unroll 2
            for (int u = 0; u < 8; ++u) {
                const f2 *r = reinterpret_cast<const f2 *>(rec[u]);
                f2 gh = r[CIN + 1] * f2(gp1[0]);
                gh = __builtin_elementwise_fma(r[CIN + 2], f2(gp1[1]), gh);
                gh = __builtin_elementwise_fma(r[CIN + 3], f2(gp1[2]), gh);
                gh.x = (keep >> (2 * u)) & 1u ? gh.x : 0.f; // selects, not exec-mask branches
                gh.y = (keep >> (2 * u + 1)) & 1u ? gh.y : 0.f;
                col[(2 * u) * kXP] = gh.x;
                col[(2 * u + 1) * kXP] = gh.y;
#pragma unroll
                for (int i = 0; i < CIN; ++i) gxp[i] = __builtin_elementwise_fma(r[i], gh, gxp[i]);
            }
            wave_lds_sync();
            // ---- dW0 | db0 tile q += g_h^T [x | 1]
#pragma unroll
            for (int s = 0; s < kPS; s += 4) {
                const v4 av = *reinterpret_cast<const v4 *>(sv + ln * kXP + kPS * s0 + s);
                const v4 bv = *reinterpret_cast<const v4 *>(sw + ib * kXP + kPS * s0 + s);
#pragma unroll
                for (int e = 0; e < 4; ++e) a0[q] = mfma4x4(av[e], bv[e], a0[q]);
            }
            wave_lds_sync(); // before the next tile's h (or the next chunk's rows) overwrite these
        }
        if (valid) {
            float *gd = gdense + (int64_t)b * CIN * npx + p;
#pragma unroll
            for (int i = 0; i < CIN; ++i) gd[i * npx] = gxp[i].x + gxp[i].y;
        }
    }
    // ---- flush (t_head_bwd's): the waves' partial rows meet in LDS, one atomic per value
#if defined(CCMI_DIAG_NOFLUSH) // diagnostic build only (make diag): wrong results -- and with the
    return;                       // accumulators dead, the compiler drops the weight-gradient work too
#endif
    const int nred = hid * (CIN + 4) + 3;
    float *red = s_dyn + w * kWF;
    static_assert(kWF >= 16 * NT * (CIN + 4) + 3, "a wave's partial row fits its LDS rows");
    __syncthreads();
    // the pixel streams' partial blocks summed across lanes (16 lanes apart), then register r of
    // lane l holds dW1[k = r][unit 16 q + ln] (l < 16) and dW0[unit 16 q + 4 ((l >> 2) & 3) + r][ic]
    // (l < 16 kNQ)
#pragma unroll
    for (int q = 0; q < NT; ++q) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float v1 = a1[q][r], v0 = a0[q][r];
            v1 += __shfl_xor(v1, 16);
            v1 += __shfl_xor(v1, 32);
#pragma unroll
            for (int o = 16 * kNQ; o < 64; o <<= 1) v0 += __shfl_xor(v0, o);
            if (r < 3 && lane < 16) { // dW1[k = r][j]
                const int j = 16 * q + ln;
                if (j < hid) red[hid * (CIN + 1) + r * hid + j] = v1;
            }
            const int j = 16 * q + 4 * ((lane >> 2) & 3) + r; // dW0[j][i = ic]
            if (lane < 16 * kNQ && j < hid) {
                if (ic < CIN) red[j * CIN + ic] = v0;
                else if (ic == CIN) red[hid * CIN + j] = v0;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float v = wave_sum(db1[k]);
        if (lane == 0) red[hid * (CIN + 4) + k] = v;
    }
    __syncthreads();
    float *Gp = gth + ((int64_t)b * kDwSlots + blockIdx.x % kDwSlots) * gstride; // this workgroup's slot row
    constexpr int kW = kHeadT / 64;
    for (int e = t; e < nred; e += kHeadT) {
        float v = 0.f;
#pragma unroll
        for (int ww = 0; ww < kW; ++ww) v += s_dyn[ww * kWF + e];
        const int dst = e < hid * CIN ? g.w0 + e
                        : e < hid * (CIN + 1) ? g.b0 + (e - hid * CIN)
                        : e < hid * (CIN + 4) ? g.w1 + (e - hid * (CIN + 1))
                                              : g.b1 + (e - hid * (CIN + 4));
        atomicAdd(&Gp[dst], v);
    }
}

// the 1x1 head backward in the register form (t_head_bwd_m, opt-in: CCMI_HEAD_BWD_REGS=1) or the
// LDS-tiled form (t_head_bwd_t, the default).  The register form is bit-for-bit a different
// summation but passes every gradient test; it measured 273 us per launch against the tiled
// form's 190 us (step 0.842 -> 0.910 ms, profiles/r6h_head_bwd_regs_ab.txt): its 36 16x16x4
// MFMAs per 16 pixels are half padding (N = 8 of 16 inputs for g_x and dW0), and at 180 VGPRs it
// runs 2 waves / SIMD with no prefetch of the next block's 25 small loads.
// (read per call, like CCMI_SP_BWD_PF of the 3x3 backward, so a test can select either form
// within one process: a getenv per launch against a ~1 ms step)
bool head_bwd_regs()
{
    const char *e = getenv("CCMI_HEAD_BWD_REGS");
    return e && *e == '1';
}

// The three backward forms take the same arguments: dense, gz0, g, th, ps, gdense, gth, gstride
using HeadBwdKernel = void (*)(const float *, const float *, Geo, const float *, int64_t, float *, float *, int64_t);
enum HeadBwdForm { kHeadTiled, kHeadRegs, kHeadFull };

template <int CIN, int NT>
HeadBwdKernel head_bwd_kernel(HeadBwdForm form)
{
    if (form == kHeadRegs) return t_head_bwd_m<(CIN + 1 <= 8 ? CIN : 7), NT>; // (never chosen for CIN = 8)
    if (form == kHeadTiled) return t_head_bwd_t<CIN, NT>;
    return t_head_bwd<CIN, NT>;
}
template <int CIN>
HeadBwdKernel head_bwd_kernel(int nt, HeadBwdForm form)
{
    switch (nt) {
    case 1: return head_bwd_kernel<CIN, 1>(form);
    case 2: return head_bwd_kernel<CIN, 2>(form);
    case 3: return head_bwd_kernel<CIN, 3>(form);
    default: return head_bwd_kernel<CIN, 4>(form);
    }
}

} // namespace

void ccmi_train::launch_head_fwd(const Geo &g, const ccmi_train_args &a, const Work &w, hipStream_t s)
{
    const dim3 grid((unsigned)(((int64_t)g.H * g.W + kHeadFwdPx - 1) / kHeadFwdPx), (unsigned)a.batch);
    auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, dim3(kT), 0, s, w.dense, g, a.params, a.param_stride, w.z[0]); };
    switch (g.L) {
    case 2: go(t_head_fwd<2>); break;
    case 3: go(t_head_fwd<3>); break;
    case 4: go(t_head_fwd<4>); break;
    case 5: go(t_head_fwd<5>); break;
    case 6: go(t_head_fwd<6>); break;
    case 7: go(t_head_fwd<7>); break;
    default: go(t_head_fwd<8>); break;
    }
}

void ccmi_train::launch_head_bwd(const Geo &g, const ccmi_train_args &a, const Work &w, const float *gz0, hipStream_t s)
{
    const int cin = g.L, nt = (g.hid + 15) / 16, B = a.batch;
    const int64_t npx = (int64_t)g.H * g.W;
    // the tiled form for a linear output layer (every reference architecture), or the register
    // form when asked for; the full-width form otherwise
    const bool tiled = !g.r1;
    const HeadBwdForm form = !tiled ? kHeadFull : head_bwd_regs() && cin + 1 <= 8 ? kHeadRegs : kHeadTiled;
    HeadBwdKernel k;
    switch (cin) {
    case 2: k = head_bwd_kernel<2>(nt, form); break;
    case 3: k = head_bwd_kernel<3>(nt, form); break;
    case 4: k = head_bwd_kernel<4>(nt, form); break;
    case 5: k = head_bwd_kernel<5>(nt, form); break;
    case 6: k = head_bwd_kernel<6>(nt, form); break;
    case 7: k = head_bwd_kernel<7>(nt, form); break;
    default: k = head_bwd_kernel<8>(nt, form); break;
    }
    if (form == kHeadRegs) {
        hipLaunchKernelGGL(k, resident_grid((const void *)k, 256, 0, (npx + 63) / 64, B), dim3(256), 0, s, w.dense, gz0, g, a.params,
                           a.param_stride, w.gdense, w.slots, (int64_t)g.P);
        return;
    }
    const int kXP = (cin + 2 > 5 ? cin + 2 : 5) | 1; // t_head_bwd's per-wave LDS rows
    const size_t lds = tiled ? sizeof(float) * (kHeadT / 64) * head_bwd_t_wave_floats(cin)
                             : sizeof(float) * (kHeadT / 64) * 64 * (16 * nt + 1 + kXP);
    // one resident round over the pixel chunks (full-width form LDS-bound: 5 workgroups per CU
    // at 32,000 B each, 276 us; at exactly 32 KB the query also allowed 5, but they did not all
    // fit: 399 us against 286 us capped at 4; profiles/r4n_*, r4o_*, r4y_*)
    const int64_t nchunk = (npx + kHeadT - 1) / kHeadT;
    hipLaunchKernelGGL(k, resident_grid((const void *)k, kHeadT, lds, nchunk, B), dim3(kHeadT), lds, s, w.dense, gz0, g, a.params,
                       a.param_stride, w.gdense, w.slots, (int64_t)g.P);
}

#undef HEAD_MFMA
