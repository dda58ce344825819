// train_ups.hip -- the backward of the overfit step's upsampling pyramid (upsampling.py:195-202,
// 322-335, 476-506; the forward is fwd_ups.hip's, keeping every stack): per pyramid step the
// refine backward of the destination level (t_ref_bwd) and the transposed-conv backward of the
// source stack, for K = 8 both in one launch (t_lvl_bwd), for K = 4 / 6 as t_ref_bwd, t_up_u,
// t_up_gu, t_up_dw and t_up_gs through the HBM temporaries.  launch_ups_bwd_step performs one
// step: the stack offsets, the fused-or-separate choice and the K / Kp ladders.
#include <type_traits>

#include "fwd_common.h"
#include "train_internal.h"

using namespace ccmi_train;

namespace {

// Polyphase taps of the 2x transposed conv: destination 2j + a reads source clamp(j + d)
// with tap a + K/2 - 1 - 2d (fwd_ups.hip).
struct UpLevel {
    int C, hs, ws, hd, wd, K, d_lo, d_hi, sidx; // sidx: kernel slot (step % n_ups)
};

// Sum of per-thread tap gradients over the workgroup, folded onto the symmetric half
// kernel (upsampling.py:46-68): one atomic per half tap per workgroup.
// (The slot rows: see kDwSlots.)
template <int K>
__device__ __forceinline__ void reduce_taps(float (&dw)[K], float *__restrict__ dst)
{
    __shared__ float s_r[kT / 64][K];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const float v = wave_sum(dw[k]);
        if (lane == 0) s_r[wid][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < K) {
        float v = 0.f;
#pragma unroll
        for (int i = 0; i < kT / 64; ++i) v += s_r[i][threadIdx.x];
        atomicAdd(&dst[min((int)threadIdx.x, K - 1 - (int)threadIdx.x)], v);
    }
}

// Refine backward of one pyramid level in ONE launch (formerly four
// passes over the level through HBM temporaries): a 16 x 64 tile of the level
// with its KP / 2 halo of X and GY staged in LDS; the horizontal pass U = X * w and the
// vertical adjoint GU = GY (*) w of the tile are formed in LDS, then the latent gradient
// GX += GY + horizontal adjoint of GU and the tap gradients (GY x U, GU x X) of the tile's
// positions.  Per element the same fmaf chains in the same order as the former separate passes
// (a zero-padded tap adds an exact 0).
struct RefBwd {
    const float *GY;
    int64_t gys;
    const float *X;
    int64_t xs;
    int h, w;
    const float *kf;
    int kstride, koff;
    float *GX;
    int64_t gxs;
    float *slots;
    int64_t gstride;
    int hoff, tiles_x;
};
template <int KP>
constexpr int ref_bwd_lds()
{
    return 2 * (16 + KP / 2 * 2) * (64 + KP / 2 * 2) + (16 + KP / 2 * 2) * 64 + 16 * (64 + KP / 2 * 2);
}
// tile bx of the level (blockIdx.x of its own launch, or of the combined t_lvl_bwd)
template <int KP>
__device__ __forceinline__ void ref_bwd_tile(float *pool, int bx, int b, const RefBwd &R)
{
    constexpr int P = KP / 2, TY = 16, TX = 64, SY = TY + 2 * P, SX = TX + 2 * P;
    float(*sx)[SX] = reinterpret_cast<float(*)[SX]>(pool);
    float(*sg)[SX] = reinterpret_cast<float(*)[SX]>(pool + SY * SX);
    float(*su)[TX] = reinterpret_cast<float(*)[TX]>(pool + 2 * SY * SX);
    float(*sgu)[SX] = reinterpret_cast<float(*)[SX]>(pool + 2 * SY * SX + SY * TX);
    const float *GY = R.GY, *X = R.X, *kf = R.kf;
    const int64_t gys = R.gys, xs = R.xs, gxs = R.gxs, gstride = R.gstride;
    const int h = R.h, w = R.w, kstride = R.kstride, koff = R.koff, hoff = R.hoff, tiles_x = R.tiles_x;
    float *GX = R.GX, *slots = R.slots;
    const int tid = threadIdx.x;
    const int ty0 = (bx / tiles_x) * TY, tx0 = (bx % tiles_x) * TX;
    const float *wk = kf + (int64_t)b * kstride + koff;
    float wv[KP];
#pragma unroll
    for (int k = 0; k < KP; ++k) wv[k] = wk[k];
    const float *xb = X + (int64_t)b * xs, *gb = GY + (int64_t)b * gys;
    {
        // every load of a thread in flight before its LDS stores
        constexpr int NL = (SY * SX + kT - 1) / kT;
        float vx[NL], vg[NL];
#pragma unroll
        for (int k = 0; k < NL; ++k) {
            const int i = tid + k * kT, r = i / SX, c = i - r * SX, y = ty0 - P + r, x = tx0 - P + c;
            const bool in = i < SY * SX && y >= 0 && y < h && x >= 0 && x < w;
            vx[k] = in ? xb[(int64_t)y * w + x] : 0.f;
            vg[k] = in ? gb[(int64_t)y * w + x] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < NL; ++k) {
            const int i = tid + k * kT;
            if (i < SY * SX) {
                (&sx[0][0])[i] = vx[k];
                (&sg[0][0])[i] = vg[k];
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < SY * TX; i += kT) { // U rows ty0 - P .. ty0 + TY + P - 1
        const int r = i / TX, c = i - r * TX;
        float a = 0.f;
#pragma unroll
        for (int k = 0; k < KP; ++k) a = fmaf(wv[k], sx[r][c + k], a);
        su[r][c] = a;
    }
    for (int i = tid; i < TY * SX; i += kT) { // GU cols tx0 - P .. tx0 + TX + P - 1
        const int t = i / SX, c = i - t * SX;
        float a = 0.f;
#pragma unroll
        for (int k = 0; k < KP; ++k) a = fmaf(wv[k], sg[t + 2 * P - k][c], a);
        sgu[t][c] = a;
    }
    __syncthreads();
    float dw[KP];
#pragma unroll
    for (int k = 0; k < KP; ++k) dw[k] = 0.f;
    float *gxb = GX + (int64_t)b * gxs;
    for (int i = tid; i < TY * TX; i += kT) {
        const int t = i / TX, c = i - t * TX, y = ty0 + t, x = tx0 + c;
        if (y >= h || x >= w) continue;
        const float gv = sg[t + P][c + P], guv = sgu[t][c + P];
        float a = gv;
#pragma unroll
        for (int k = 0; k < KP; ++k) a = fmaf(wv[k], sgu[t][c - k + 2 * P], a);
        gxb[(int64_t)y * w + x] += a;
#pragma unroll
        for (int k = 0; k < KP; ++k) {
            dw[k] = fmaf(gv, su[t + k][c], dw[k]);
            dw[k] = fmaf(guv, sx[t + P][c + k], dw[k]);
        }
    }
    reduce_taps<KP>(dw, slots + ((int64_t)b * kDwSlots + bx % kDwSlots) * gstride + hoff);
}

template <int KP>
__global__ __launch_bounds__(kT) void t_ref_bwd(RefBwd R)
{
    __shared__ __attribute__((aligned(16))) float pool[ref_bwd_lds<KP>()];
    ref_bwd_tile<KP>(pool, blockIdx.x, blockIdx.y, R);
}

__device__ __forceinline__ int up_tap(int a, int d, int K) { return a + K / 2 - 1 - 2 * d; }

// upsample, horizontal pass: U[c][r][xd] = sum_d w[tap] S[c][r][clamp(xd/2 + d)]
__global__ void t_up_u(const float *__restrict__ S, int64_t ss, UpLevel A, const float *__restrict__ kf, int kstride,
                       int koff, float *__restrict__ U, int64_t us)
{
    const int b = blockIdx.y;
    const int n = A.C * A.hs * A.wd, i = blockIdx.x * kT + threadIdx.x;
    if (i >= n) return;
    const int cr = i / A.wd, xd = i - cr * A.wd; // cr = c * hs + r
    const float *wk = kf + (int64_t)b * kstride + koff, *src = S + (int64_t)b * ss + cr * A.ws;
    const int j = xd >> 1, a = xd & 1;
    float acc = 0.f;
    for (int d = A.d_lo; d <= A.d_hi; ++d) {
        const int t = up_tap(a, d, A.K);
        if (t >= 0 && t < A.K) acc = fmaf(wk[t], src[clampi(j + d, A.ws - 1)], acc);
    }
    U[(int64_t)b * us + i] = acc;
}

// upsample, vertical adjoint: GU[c][r][xd] = sum over (yd = 2j + a, d) with clamp(j + d) == r
__global__ void t_up_gu(const float *__restrict__ GY, int64_t gys, UpLevel A, const float *__restrict__ kf, int kstride,
                        int koff, float *__restrict__ GU, int64_t us)
{
    const int b = blockIdx.y;
    const int n = A.C * A.hs * A.wd, i = blockIdx.x * kT + threadIdx.x;
    if (i >= n) return;
    const int cr = i / A.wd, xd = i - cr * A.wd;
    const int c = cr / A.hs, r = cr - c * A.hs;
    const float *wk = kf + (int64_t)b * kstride + koff;
    const float *gy = GY + (int64_t)b * gys + (int64_t)(c + 1) * A.hd * A.wd + xd; // channel c+1 of the dest stack
    const int nj = (A.hd + 1) >> 1;
    float acc = 0.f;
    for (int d = A.d_lo; d <= A.d_hi; ++d) {
        int jlo = r == 0 ? 0 : r - d, jhi = r == A.hs - 1 ? nj - 1 : r - d;
        jlo = max(jlo, 0);
        jhi = min(jhi, nj - 1);
        for (int j = jlo; j <= jhi; ++j) {
            if (clampi(j + d, A.hs - 1) != r) continue;
            for (int a = 0; a < 2; ++a) {
                const int yd = 2 * j + a, t = up_tap(a, d, A.K);
                if (yd < A.hd && t >= 0 && t < A.K) acc = fmaf(wk[t], gy[(int64_t)yd * A.wd], acc);
            }
        }
    }
    GU[(int64_t)b * us + i] = acc;
}

// upsample, horizontal adjoint: GS[c][r][m] (+= into the source gradient)
__global__ void t_up_gs(const float *__restrict__ GU, int64_t us, UpLevel A, const float *__restrict__ kf, int kstride,
                        int koff, float *__restrict__ GS, int64_t gss, int accumulate)
{
    const int b = blockIdx.y;
    const int n = A.C * A.hs * A.ws, i = blockIdx.x * kT + threadIdx.x;
    if (i >= n) return;
    const int cr = i / A.ws, m = i - cr * A.ws;
    const float *wk = kf + (int64_t)b * kstride + koff;
    const float *gu = GU + (int64_t)b * us + cr * A.wd;
    const int nj = (A.wd + 1) >> 1;
    float acc = 0.f;
    for (int d = A.d_lo; d <= A.d_hi; ++d) {
        int jlo = m == 0 ? 0 : m - d, jhi = m == A.ws - 1 ? nj - 1 : m - d;
        jlo = max(jlo, 0);
        jhi = min(jhi, nj - 1);
        for (int j = jlo; j <= jhi; ++j) {
            if (clampi(j + d, A.ws - 1) != m) continue;
            for (int a = 0; a < 2; ++a) {
                const int xd = 2 * j + a, t = up_tap(a, d, A.K);
                if (xd < A.wd && t >= 0 && t < A.K) acc = fmaf(wk[t], gu[xd], acc);
            }
        }
    }
    float *o = GS + (int64_t)b * gss + i;
    *o = accumulate ? *o + acc : acc;
}

// upsample kernel gradient: vertical taps over destination row pairs (c, j, xd),
// horizontal taps over destination column pairs (c, r, j); taps are compile-time per
// parity: destination 2j + a, source offset d -> tap a + K/2 - 1 - 2d.
template <int K>
__global__ __launch_bounds__(kT) void t_up_dw(const float *__restrict__ GY, int64_t gys, const float *__restrict__ U,
                                              const float *__restrict__ GU, int64_t us, const float *__restrict__ S,
                                              int64_t ss, UpLevel A, float *__restrict__ gth, int64_t gstride, int hoff)
{
    constexpr int K2 = K / 2, DLO = -((K2 + 1) / 2), DHI = K2 / 2;
    const int b = blockIdx.y;
    float dw[K];
#pragma unroll
    for (int k = 0; k < K; ++k) dw[k] = 0.f;
    const int njy = (A.hd + 1) >> 1, njx = (A.wd + 1) >> 1;
    const float *gyb = GY + (int64_t)b * gys, *ub = U + (int64_t)b * us, *gub = GU + (int64_t)b * us;
    const float *sb = S + (int64_t)b * ss;
    const int64_t nv = (int64_t)A.C * njy * A.wd;
    for (int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x; i < nv; i += (int64_t)gridDim.x * kT) {
        const int cj = (int)i / A.wd, xd = (int)i - cj * A.wd;
        const int c = cj / njy, j = cj - c * njy;
        const float *gy = gyb + (int64_t)(c + 1) * A.hd * A.wd + xd;
        const float ge = gy[(int64_t)(2 * j) * A.wd];
        const float go = 2 * j + 1 < A.hd ? gy[(int64_t)(2 * j + 1) * A.wd] : 0.f;
        const float *u = ub + (int64_t)c * A.hs * A.wd + xd;
#pragma unroll
        for (int d = DLO; d <= DHI; ++d) {
            const float uv = u[(int64_t)clampi(j + d, A.hs - 1) * A.wd];
            const int te = K2 - 1 - 2 * d, to = K2 - 2 * d;
            if (te >= 0 && te < K) dw[te] = fmaf(ge, uv, dw[te]);
            if (to >= 0 && to < K) dw[to] = fmaf(go, uv, dw[to]);
        }
    }
    const int64_t nh = (int64_t)A.C * A.hs * njx;
    for (int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x; i < nh; i += (int64_t)gridDim.x * kT) {
        const int cr = (int)i / njx, j = (int)i - cr * njx;
        const float *gu = gub + cr * A.wd;
        const float ge = gu[2 * j];
        const float go = 2 * j + 1 < A.wd ? gu[2 * j + 1] : 0.f;
        const float *src = sb + cr * A.ws;
#pragma unroll
        for (int d = DLO; d <= DHI; ++d) {
            const float sv = src[clampi(j + d, A.ws - 1)];
            const int te = K2 - 1 - 2 * d, to = K2 - 2 * d;
            if (te >= 0 && te < K) dw[te] = fmaf(ge, sv, dw[te]);
            if (to >= 0 && to < K) dw[to] = fmaf(go, sv, dw[to]);
        }
    }
    reduce_taps<K>(dw, gth + ((int64_t)b * kDwSlots + blockIdx.x % kDwSlots) * gstride + hoff);
}

// Upsampling backward of one pyramid step in ONE launch (formerly t_up_u, t_up_gu, t_up_dw
// and t_up_gs with compile-time taps, with the [C][hs][wd] temporaries U and GU through HBM).  A workgroup owns
// source rows [r0, r0 + TR) x destination columns [x0, x0 + TX) of one channel.  It stages
// in LDS the clamped source rows r0 + DLO .. r0 + TR - 1 + DHI (columns m0 + DLO .. m0 + TM - 1
// + DHI, m0 = x0 / 2) and the destination-gradient rows 2 (r0 - DHI) .. 2 (r0 + TR - 1 - DLO) + 1
// with 2 DHI halo columns on each side (zero outside the level), forms
//   U  = horizontal pass of S        rows r0 + DLO .. r0 + TR - 1 + DHI, the tile's columns;
//   GU = vertical adjoint of GY      rows r0 .. r0 + TR - 1, the tile's columns + halo;
// and emits GS (horizontal adjoint of GU) for its TM source columns and the tap-gradient
// partial sums (GY x U, GU x S) of its destination positions.  Border rows / columns take
// the generic clamped-gather loops of t_up_gu / t_up_gs over the staged tiles.
struct UpBwd {
    const float *GY;
    int64_t gys;
    const float *S;
    int64_t ss;
    UpLevel A;
    const float *kf;
    int kstride, koff;
    float *GS;
    int64_t gss;
    int accumulate;
    float *slots;
    int64_t gstride;
    int hoff, tiles_x, tiles_y;
    int batch; // frames (t_lvl_bwd's 1-D grid)
};
template <int K>
constexpr int up_bwd_lds()
{
    constexpr int K2 = K / 2, DW = K2 / 2 + (K2 + 1) / 2, TR = 16, TX = 64, TM = TX / 2;
    return (TR + DW) * (TM + DW) + (TR + DW) * TX + 2 * (TR + DW) * (TX + 2 * DW) + TR * (TX + 2 * DW);
}
template <int K>
__device__ __forceinline__ void up_bwd_tile(float *pool, int bx, int b, const UpBwd &Q)
{
    constexpr int K2 = K / 2, DLO = -((K2 + 1) / 2), DHI = K2 / 2, DW = DHI - DLO;
    constexpr int TR = 16, TX = 64, TM = TX / 2;
    constexpr int SR = TR + DW, SC = TM + DW; // staged source tile
    constexpr int GR = 2 * (TR + DW), GC = TX + 2 * DW; // staged GY tile (GU has GC columns too)
    float(*s_s)[SC] = reinterpret_cast<float(*)[SC]>(pool);
    float(*s_u)[TX] = reinterpret_cast<float(*)[TX]>(pool + SR * SC);
    float(*s_gy)[GC] = reinterpret_cast<float(*)[GC]>(pool + SR * SC + SR * TX);
    float(*s_gu)[GC] = reinterpret_cast<float(*)[GC]>(pool + SR * SC + SR * TX + GR * GC);
    const float *GY = Q.GY, *S = Q.S, *kf = Q.kf;
    const int64_t gys = Q.gys, ss = Q.ss, gss = Q.gss, gstride = Q.gstride;
    const UpLevel A = Q.A;
    const int kstride = Q.kstride, koff = Q.koff, accumulate = Q.accumulate, hoff = Q.hoff;
    const int tiles_x = Q.tiles_x, tiles_y = Q.tiles_y;
    float *GS = Q.GS, *slots = Q.slots;
    const int tid = threadIdx.x;
    const int tile = bx % (tiles_x * tiles_y), c = bx / (tiles_x * tiles_y);
    const int r0 = (tile / tiles_x) * TR, x0 = (tile % tiles_x) * TX, m0 = x0 / 2;
    const int gy0 = 2 * (r0 - DHI), gx0 = x0 - 2 * DHI; // GY / GU tile origin
    const int hs = A.hs, ws = A.ws, hd = A.hd, wd = A.wd;
    const int njy = (hd + 1) >> 1, njx = (wd + 1) >> 1;
    float w[K];
    {
        const float *wk = kf + (int64_t)b * kstride + koff;
#pragma unroll
        for (int t = 0; t < K; ++t) w[t] = wk[t];
    }
    const float *sb = S + (int64_t)b * ss + (int64_t)c * hs * ws;
    const float *gb = GY + (int64_t)b * gys + (int64_t)(c + 1) * hd * wd; // channel c + 1 of the dest stack
    // staging: every load of a thread issued before its LDS stores (a load-store pair per
    // loop iteration paid one memory latency per element)
    {
        constexpr int NS = (SR * SC + kT - 1) / kT, NG = (GR * GC + kT - 1) / kT;
        float vs[NS], vg[NG];
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            const int i = tid + k * kT, r = i / SC, q = i - r * SC;
            vs[k] = i < SR * SC ? sb[(int64_t)clampi(r0 + DLO + r, hs - 1) * ws + clampi(m0 + DLO + q, ws - 1)] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < NG; ++k) {
            const int i = tid + k * kT, r = i / GC, q = i - r * GC, y = gy0 + r, x = gx0 + q;
            vg[k] = (i < GR * GC && y >= 0 && y < hd && x >= 0 && x < wd) ? gb[(int64_t)y * wd + x] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            const int i = tid + k * kT;
            if (i < SR * SC) (&s_s[0][0])[i] = vs[k];
        }
#pragma unroll
        for (int k = 0; k < NG; ++k) {
            const int i = tid + k * kT;
            if (i < GR * GC) (&s_gy[0][0])[i] = vg[k];
        }
    }
    __syncthreads();
    // U: destination column x0 + q reads source columns m0 + (q >> 1) + d.  A thread takes the
    // column pair (2 j, 2 j + 1), so the tap index of each parity is a compile-time constant (a
    // per-lane parity made every w[t] a select chain over the K registers)
    for (int i = tid; i < SR * TM; i += kT) {
        const int r = i / TM, j = i - r * TM;
        float acc[2] = {0.f, 0.f};
#pragma unroll
        for (int d = DLO; d <= DHI; ++d) {
            const float sv = s_s[r][j + d - DLO];
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                const int t = a + K2 - 1 - 2 * d;
                if (t >= 0 && t < K) acc[a] = fmaf(w[t], sv, acc[a]);
            }
        }
        s_u[r][2 * j] = acc[0];
        s_u[r][2 * j + 1] = acc[1];
    }
    // GU at source row r0 + tr, destination column gx0 + q
    for (int i = tid; i < TR * GC; i += kT) {
        const int tr = i / GC, q = i - tr * GC, r = r0 + tr, x = gx0 + q;
        float acc = 0.f;
        if (r < hs && x >= 0 && x < wd) {
            if (r >= 1 && r <= hs - 2 && r - DHI >= 0 && r - DLO <= njy - 1 && 2 * (r - DLO) + 1 < hd) {
#pragma unroll
                for (int d = DLO; d <= DHI; ++d)
#pragma unroll
                    for (int a = 0; a < 2; ++a) {
                        const int t = a + K2 - 1 - 2 * d;
                        if (t >= 0 && t < K) acc = fmaf(w[t], s_gy[2 * (tr - d + DHI) + a][q], acc);
                    }
            } else {
                for (int d = DLO; d <= DHI; ++d) {
                    int jlo = r == 0 ? 0 : r - d, jhi = r == hs - 1 ? njy - 1 : r - d;
                    jlo = max(jlo, 0);
                    jhi = min(jhi, njy - 1);
                    for (int j = jlo; j <= jhi; ++j) {
                        if (clampi(j + d, hs - 1) != r) continue;
                        for (int a = 0; a < 2; ++a) {
                            const int yd = 2 * j + a, t = up_tap(a, d, K);
                            if (yd < hd && t >= 0 && t < K) acc = fmaf(w[t], s_gy[yd - gy0][q], acc);
                        }
                    }
                }
            }
        }
        s_gu[tr][q] = acc;
    }
    __syncthreads();
    // GS at source row r0 + tr, column m0 + mm
    float *gsb = GS + (int64_t)b * gss + (int64_t)c * hs * ws;
    for (int i = tid; i < TR * TM; i += kT) {
        const int tr = i / TM, mm = i - tr * TM, r = r0 + tr, m = m0 + mm;
        if (r >= hs || m >= ws) continue;
        float acc = 0.f;
        if (m >= 1 && m <= ws - 2 && m - DHI >= 0 && m - DLO <= njx - 1 && 2 * (m - DLO) + 1 < wd) {
#pragma unroll
            for (int d = DLO; d <= DHI; ++d)
#pragma unroll
                for (int a = 0; a < 2; ++a) {
                    const int t = a + K2 - 1 - 2 * d;
                    if (t >= 0 && t < K) acc = fmaf(w[t], s_gu[tr][2 * (mm - d + DHI) + a], acc);
                }
        } else {
            for (int d = DLO; d <= DHI; ++d) {
                int jlo = m == 0 ? 0 : m - d, jhi = m == ws - 1 ? njx - 1 : m - d;
                jlo = max(jlo, 0);
                jhi = min(jhi, njx - 1);
                for (int j = jlo; j <= jhi; ++j) {
                    if (clampi(j + d, ws - 1) != m) continue;
                    for (int a = 0; a < 2; ++a) {
                        const int xd = 2 * j + a, t = up_tap(a, d, K);
                        if (xd < wd && t >= 0 && t < K) acc = fmaf(w[t], s_gu[tr][xd - gx0], acc);
                    }
                }
            }
        }
        float *o = gsb + (int64_t)r * ws + m;
        *o = accumulate ? *o + acc : acc;
    }
#if defined(CCMI_DIAG_LVL_NODW)
    return;
#endif
    // tap gradients: vertical use (GY x U at the tile's destination rows), horizontal use
    // (GU x S at the tile's source rows)
    float dw[K];
#pragma unroll
    for (int k = 0; k < K; ++k) dw[k] = 0.f;
    // vertical use: destination row ty has parity a = ty & 1 -- with kT a multiple of 2 TX, the
    // parity of a wave's rows (tid >> 6) never changes: a wave-uniform branch into a loop whose
    // tap indices are compile-time constants
    static_assert(kT % (2 * TX) == 0 && TX == 64, "row parity is wave-uniform");
    auto vertical = [&](auto par) {
        constexpr int a = decltype(par)::value;
        for (int i = tid; i < 2 * TR * TX; i += kT) {
            const int ty = i / TX, q = i - ty * TX;
            if (2 * r0 + ty >= hd || x0 + q >= wd) continue;
            const float g = s_gy[ty + 2 * DHI][q + 2 * DHI];
#pragma unroll
            for (int d = DLO; d <= DHI; ++d) {
                const int t = a + K2 - 1 - 2 * d;
                if (t >= 0 && t < K) dw[t] = fmaf(g, s_u[(ty >> 1) + d - DLO][q], dw[t]);
            }
        }
    };
    if (((tid >> 6) & 1) == 0) vertical(std::integral_constant<int, 0>{});
    else vertical(std::integral_constant<int, 1>{});
    // horizontal use: a thread takes the column pair (2 j, 2 j + 1), one per parity
    for (int i = tid; i < TR * TM; i += kT) {
        const int tr = i / TM, j = i - tr * TM;
        if (r0 + tr >= hs) continue;
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const int q = 2 * j + a;
            if (x0 + q >= wd) continue;
            const float g = s_gu[tr][q + 2 * DHI];
#pragma unroll
            for (int d = DLO; d <= DHI; ++d) {
                const int t = a + K2 - 1 - 2 * d;
                if (t >= 0 && t < K) dw[t] = fmaf(g, s_s[tr - DLO][j + d - DLO], dw[t]);
            }
        }
    }
    reduce_taps<K>(dw, slots + ((int64_t)b * kDwSlots + bx % kDwSlots) * gstride + hoff);
}

// One pyramid step of the upsampling backward in ONE launch: workgroups [0, nref) are tiles
// of the refine backward (latent k-1, channel 0 of the destination gradient), the rest tiles of
// the transposed-conv backward (channels 1..C): the two read disjoint inputs and write
// disjoint outputs, so they run side by side (the coarse levels are a few workgroups each and
// were latency-bound as two launches)
template <int KP, int K>
__global__ __launch_bounds__(kT) void t_lvl_bwd(RefBwd R, UpBwd Q, int nref)
{
    constexpr int n = ref_bwd_lds<KP>() > up_bwd_lds<K>() ? ref_bwd_lds<KP>() : up_bwd_lds<K>();
    __shared__ __attribute__((aligned(16))) float pool[n];
    // 1-D grid of (nref + up tiles) x frames in XCD-aware order (neighbouring tiles share their
    // halos through one L2)
    const int per = gridDim.x / Q.batch, wt = ccmi_fwd::xcd_order(blockIdx.x, gridDim.x);
    const int b = wt / per, bx = wt - b * per;
#if defined(CCMI_DIAG_LVL_NOREF) // diagnostic builds only (tools/arm_diag.sh): wrong results
    if (bx < nref) return;
#endif
#if defined(CCMI_DIAG_LVL_NOUP)
    if (bx >= nref) return;
#endif
    if (bx < nref) ref_bwd_tile<KP>(pool, bx, b, R);
    else up_bwd_tile<K>(pool, bx - nref, b, Q);
}

} // namespace

// Pyramid step `step` (L - 2 first): source level k = L - 1 - step, destination level k - 1.
// The destination's gradient GY is the dense gradient (level 0) or its gradient stack; the
// source's gradient goes to its gradient stack, or -- the coarsest level, a bare latent --
// into the latent gradients.
void ccmi_train::launch_ups_bwd_step(const Geo &g, const Work &w, int B, int step, hipStream_t s)
{
    const int k = g.L - 1 - step;
    const int hd = g.h[k - 1], wd = g.w[k - 1], C = g.L - k, K2 = g.K / 2;
    const bool finest = k - 1 == 0, coarsest = k == g.L - 1;
    float *uslots = w.slots + g.up_off; // the upsampling kernels' columns (their offsets are relative to up_off)
    const float *GY = finest ? w.gdense : w.gstack + w.gstack_off[k - 1];
    const int64_t gys = finest ? (int64_t)g.L * g.H * g.W : w.gstack_per;
    // refine of y_hat(k-1): channel 0 of the destination stack (tiles 16 x 64)
    const int rtx = ccmi_div_up(wd, 64), nref = rtx * ccmi_div_up(hd, 16);
    const RefBwd R{GY, gys, w.yq + g.off[k - 1], (int64_t)g.N, hd, wd, w.kf, g.kfull,
                   g.n_ups * g.K + (step % g.n_pre) * g.Kp, w.gq + g.off[k - 1], (int64_t)g.N, uslots, (int64_t)g.P,
                   g.pre_off + (step % g.n_pre) * g.hp - g.up_off, rtx};
    // transposed-conv upsampling of the source stack: channels 1..C
    const UpLevel A{C, g.h[k], g.w[k], hd, wd, g.K, -((K2 + 1) / 2), K2 / 2, step % g.n_ups};
    const float *S = w.yq + g.off[k];
    int64_t ss = g.N;
    if (!coarsest) {
        // stacks laid out by ccmi_launch_ups_f32: level k at sum_{k'<k} (L-k') h w, [batch][...]
        int64_t so = 0;
        for (int kk = 1; kk < k; ++kk) so += (int64_t)(g.L - kk) * g.h[kk] * g.w[kk] * B;
        S = w.stacks + so;
        ss = (int64_t)(g.L - k) * g.h[k] * g.w[k];
    }
    const int koff = A.sidx * g.K, hoff = A.sidx * g.hu;
    float *GSd = coarsest ? w.gq + g.off[k] : w.gstack + w.gstack_off[k];
    const int64_t gss = coarsest ? (int64_t)g.N : w.gstack_per;
    const int accumulate = coarsest ? 1 : 0;
    if (g.K == 8) {
        // the whole step, refine and transposed conv, in one launch (t_lvl_bwd)
        const int tx = ccmi_div_up(wd, 64), ty = ccmi_div_up(A.hs, 16);
        const UpBwd Q{GY, gys, S, ss, A, w.kf, g.kfull, koff, GSd, gss, accumulate, uslots, (int64_t)g.P, hoff, tx, ty, B};
        const dim3 grid((unsigned)((nref + tx * ty * C) * B));
        auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, dim3(kT), 0, s, R, Q, nref); };
        switch (g.Kp) {
        case 1: go(t_lvl_bwd<1, 8>); break;
        case 3: go(t_lvl_bwd<3, 8>); break;
        case 5: go(t_lvl_bwd<5, 8>); break;
        case 7: go(t_lvl_bwd<7, 8>); break;
        default: go(t_lvl_bwd<9, 8>); break;
        }
        return;
    }
    auto ref = [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3((unsigned)nref, B), dim3(kT), 0, s, R); };
    switch (g.Kp) {
    case 1: ref(t_ref_bwd<1>); break;
    case 3: ref(t_ref_bwd<3>); break;
    case 5: ref(t_ref_bwd<5>); break;
    case 7: ref(t_ref_bwd<7>); break;
    default: ref(t_ref_bwd<9>); break;
    }
    float *U = w.tmpU, *GU = w.tmpG;
    const int64_t nu = (int64_t)C * A.hs * wd;
    hipLaunchKernelGGL(t_up_u, grid1(nu, B), dim3(kT), 0, s, S, ss, A, w.kf, g.kfull, koff, U, w.tmp_per);
    hipLaunchKernelGGL(t_up_gu, grid1(nu, B), dim3(kT), 0, s, GY, gys, A, w.kf, g.kfull, koff, GU, w.tmp_per);
    auto dw = [&](auto kernel) {
        const dim3 gr(dw_blocks((int64_t)C * hd * wd, 8), B); // measured: 8 items per thread beat 1 here
        hipLaunchKernelGGL(kernel, gr, dim3(kT), 0, s, GY, gys, U, GU, w.tmp_per, S, ss, A, uslots, (int64_t)g.P, hoff);
    };
    switch (g.K) {
    case 4: dw(t_up_dw<4>); break;
    case 6: dw(t_up_dw<6>); break;
    default: dw(t_up_dw<8>); break;
    }
    hipLaunchKernelGGL(t_up_gs, grid1((int64_t)C * A.hs * A.ws, B), dim3(kT), 0, s, GU, w.tmp_per, A, w.kf, g.kfull, koff, GSd,
                       gss, accumulate);
}
