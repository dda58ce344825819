// train_arm.hip -- the overfit step's ARM: forward, Laplace rate and the full backward in one pass
// over 4 x 64 latent tiles (arm.py:227-370, coolchic.py:395-424).  t_arm<D, NH> is the VALU form
// (dim_arm 8 / 24 / 32), t_arm16<NH> the matrix-core form (dim_arm 16); launch_arm owns the
// D x NH ladder.  The CCMI_DIAG_ARM_* / CCMI_DIAG_A16_* switches build timing-only variants
// (tools/arm_diag.sh).
#include "fwd_common.h"
#include "train_internal.h"

using namespace ccmi_train;
using ccmi_fwd::cfloat_ptr;

namespace {

constexpr float kLn2 = 0.6931471805599453f;

template <int D>
__device__ __forceinline__ void ctx_off(int i, int &dy, int &dx)
{
    constexpr signed char k8[8] = {13, 22, 30, 31, 32, 37, 38, 39};
    constexpr signed char k16[16] = {13, 14, 20, 21, 22, 23, 24, 28, 29, 30, 31, 32, 33, 37, 38, 39};
    constexpr signed char k24[24] = {4, 11, 12, 13, 14, 15, 19, 20, 21, 22, 23, 24, 25, 28, 29, 30, 31, 32, 33, 34,
                                     36, 37, 38, 39};
    constexpr signed char k32[32] = {2, 3, 4, 5, 10, 11, 12, 13, 14, 15, 16, 19, 20, 21, 22, 23, 24, 25, 26, 27,
                                     28, 29, 30, 31, 32, 33, 34, 35, 36, 37, 38, 39};
    const int k = D == 8 ? k8[i] : D == 16 ? k16[i] : D == 24 ? k24[i] : k32[i];
    dy = k / 9 - 4;
    dx = k % 9 - 4;
}

// The context gradients a position (r, c) of the tile + causal halo receives: the gradient of
// every latent of the tile whose context holds it (context input k of the latent at
// (r - kAH - dy_k, c - kAH - dx_k)), plus the latent's own gradient (column D of its s_g row)
// when (r, c) is a latent of the tile.  s_g: [kATY * kATX][D + 1].  Every term's LDS read is
// issued unconditionally -- a term outside the tile reads s_zero -- so a position's D + 1
// reads are in flight together (as `if (inside) v += s_g[..]` they compiled to D + 1
// exec-mask branches with one LDS round trip each).
// Summation order as before (own value, then k = 0 .. D - 1).
template <int D>
__device__ __forceinline__ float gather_ctx(const float *s_g, const float *s_zero, int r, int c)
{
    const int ly0 = r - kAH, lx0 = c - kAH;
    const int base = (ly0 * kATX + lx0) * (D + 1);
    auto inside = [](int ly, int lx) { return (unsigned)ly < (unsigned)kATY && (unsigned)lx < (unsigned)kATX; };
    float t[D + 1];
    t[D] = *(inside(ly0, lx0) ? s_g + base + D : s_zero);
#pragma unroll
    for (int k = 0; k < D; ++k) {
        int dy, dx;
        ctx_off<D>(k, dy, dx);
        t[k] = *(inside(ly0 - dy, lx0 - dx) ? s_g + base + (-dy * kATX - dx) * (D + 1) + k : s_zero);
    }
    // all reads issued before the first add (the scheduler otherwise sinks each read to its
    // add: one LDS round trip per term again)
    __builtin_amdgcn_sched_barrier(0);
    float v = t[D];
#pragma unroll
    for (int k = 0; k < D; ++k) v += t[k];
    return v;
}

// Lane exchanges between the four 16-lane rows of a wave on gfx950's permlane swaps (VALU ops,
// no LDS round trip as ds_bpermute / __shfl): v_permlane16_swap exchanges rows 1 <-> 0 and
// 3 <-> 2 of its two operands, v_permlane32_swap lanes 32..63 <-> 0..31.
struct f2 {
    float a, b;
};
__device__ __forceinline__ f2 swap16(float x)
{
    const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return {__uint_as_float(r[0]), __uint_as_float(r[1])}; // {rows 0, 0, 2, 2}, {rows 1, 1, 3, 3}
}
__device__ __forceinline__ f2 swap32(float x)
{
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return {__uint_as_float(r[0]), __uint_as_float(r[1])}; // {rows 0, 1, 0, 1}, {rows 2, 3, 2, 3}
}
// x + x[lane ^ 16], then + the same at lane ^ 32: the sum over the four rows, in every lane
// (the values and their order are those of two __shfl_xor steps)
__device__ __forceinline__ float sum_rows(float x)
{
    const f2 h = swap16(x);
    const f2 q = swap32(h.a + h.b);
    return q.a + q.b;
}
// bc[g] = row g of x, in every row (as __shfl(x, 16 g + (lane & 15)))
__device__ __forceinline__ void bcast_rows(float x, float (&bc)[4])
{
    const f2 h = swap32(x), lo = swap16(h.a), hi = swap16(h.b);
    bc[0] = lo.a;
    bc[1] = lo.b;
    bc[2] = hi.a;
    bc[3] = hi.b;
}

// One layer's weight gradient over a wave's 64 rows, on the matrix cores:
// acc[mt][nt] += G^T A, G = [64][R] (pitch R + 1, column R zero), A = [64][D] (pitch D + 1,
// column D zero): a GEMM
// whose K is the latent index, 4 latents per MFMA.
// With B = 1 the same A operand also accumulates the bias gradient sum_k A[m][k] (accb).
template <int R, int D, bool BIAS = true>
__device__ __forceinline__ void mfma_outer(const float *s_g, const float *s_a, v4f (&acc)[(R + 15) / 16][(D + 15) / 16],
                                           v4f (&accb)[(R + 15) / 16])
{
    constexpr int MT = (R + 15) / 16, NT = (D + 15) / 16;
    const int lane = threadIdx.x & 63, ln = lane & 15, lk = lane >> 4;
    // operand columns past R / D read the rows' zero pad column (R, D): no exec-mask branch
    // between the LDS reads and the MFMAs
    int ca[MT], cb[NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) ca[mt] = 16 * mt + ln < R ? 16 * mt + ln : R;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) cb[nt] = 16 * nt + ln < D ? 16 * nt + ln : D;
    // K = rows in the order r = s + 16 lk: the two 16-lane groups of a 32-lane half read rows 16
    // apart, 16 banks apart for the odd pitches D + 1 / R + 1 (4 s + lk put rows 1 apart:
    // a 2-way conflict per read)
#pragma unroll 4
    for (int s = 0; s < 16; ++s) {
        const int r = s + 16 * lk;
        float bv[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) bv[nt] = s_a[r * (D + 1) + cb[nt]];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const float av = s_g[r * (R + 1) + ca[mt]];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = mfma4(av, bv[nt], acc[mt][nt]);
#if !defined(CCMI_DIAG_ARM_NOBIAS) // diagnostic builds only (tools/arm_diag.sh): wrong results
            if constexpr (BIAS) accb[mt] = mfma4(av, 1.f, accb[mt]);
#endif
        }
    }
}

// mfma_outer's accumulators stored into a wave's partial [R][D] weight-gradient block and its
// [R] bias in LDS (every element is written), for the workgroup-level reduction of the flush
template <int R, int D>
__device__ __forceinline__ void stage_outer(const v4f (&acc)[(R + 15) / 16][(D + 15) / 16], const v4f (&accb)[(R + 15) / 16],
                                            float *dst, float *dstb)
{
    constexpr int MT = (R + 15) / 16, NT = (D + 15) / 16;
    const int lane = threadIdx.x & 63, ln = lane & 15, lk = lane >> 4;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = 16 * mt + 4 * lk + r, n = 16 * nt + ln;
                if (m < R && n < D) dst[m * D + n] = acc[mt][nt][r];
                if (nt == 0 && m < R && ln == 0) dstb[m] = accb[mt][r];
            }
}

// Sum over the wave of v, added to *dst by lane 0.
__device__ __forceinline__ void wave_add(float v, float *dst)
{
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) atomicAdd(dst, v);
}

// weights of the ARM MLP: wave-uniform scalar loads (the diagnostic build replaces them by
// constants to bound their cost -- wrong results, tools/arm_diag.sh)
#if defined(CCMI_DIAG_ARM_NOWLOAD)
#define ARMW(ptr, idx) (0.001f * (float)((idx) & 7))
#else
#define ARMW(ptr, idx) ((ptr)[idx])
#endif
// Laplace rate of one latent and its gradients (coolchic.py:419-424, arm.py:262-266):
// scale = exp(clamp(ls - 4, -4.6, 5)); P = F(q + 1/2) - F(q - 1/2); bits = -log2(max(P, 2^-16)).
// Returns (through refs) the rate in bits (valid latents) and dL/dq, dL/dmu, dL/dls for the
// per-latent rate weight lam (0 when P < 2^-16: clamp_min blocks the gradient).
__device__ __forceinline__ void arm_rate(float q, float mu, float ls, bool valid, float lam, float &rbits, float &g_q,
                                         float &g_mu, float &g_ls)
// One IEEE division (1 / sig) shared by the four |s| / sig terms and the two gradient terms
// (torch divides each time; the products differ from those quotients by at most an ulp of
// the argument, far inside the gradient tolerances -- the exp / expm1 evaluations themselves
// keep their accurate forms, which the tail cancellation of P = F1 - F2 needs).
{
    const float l4 = ls - 4.f, sig = expf(fminf(fmaxf(l4, -4.6f), 5.0f));
    const float inv = 1.f / sig;
    const float s1 = q + 0.5f - mu, s2 = q - 0.5f - mu;
    const float a1 = fabsf(s1) * inv, a2 = fabsf(s2) * inv;
    const float sg1 = s1 > 0.f ? 1.f : (s1 < 0.f ? -1.f : 0.f), sg2 = s2 > 0.f ? 1.f : (s2 < 0.f ? -1.f : 0.f);
    const float F1 = 0.5f - 0.5f * sg1 * expm1f(-a1), F2 = 0.5f - 0.5f * sg2 * expm1f(-a2);
    const float Pr = F1 - F2;
    g_q = 0.f, g_mu = 0.f, g_ls = 0.f, rbits = 0.f;
    if (valid) {
        rbits = -log2f(fmaxf(Pr, 1.52587890625e-05f));
        if (Pr >= 1.52587890625e-05f) { // clamp_min passes the gradient where P >= 2^-16
            const float dLdP = -lam / (Pr * kLn2);
            // torch autograd of 0.5 - 0.5 sign(s) expm1(-|s|/sig): d/ds = 0.5 sign(s)^2 e / sig,
            // d/dsig = -0.5 sign(s) e |s| / sig^2 = -sign(s) (0.5 e / sig) (|s| / sig)
            const float h1 = 0.5f * expf(-a1) * inv, h2 = 0.5f * expf(-a2) * inv;
            const float Fs1 = sg1 * sg1 * h1, Fs2 = sg2 * sg2 * h2;
            const float Fg1 = -sg1 * h1 * a1, Fg2 = -sg2 * h2 * a2;
            g_q = dLdP * (Fs1 - Fs2);
            g_mu = -g_q;
            const float g_sig = dLdP * (Fg1 - Fg2);
            g_ls = (l4 >= -4.6f && l4 <= 5.0f) ? g_sig * sig : 0.f;
        }
    }
}

// waves / SIMD the VALU ARM's registers are budgeted for (3: <= 168 VGPRs); the dim-24 / 32
// ARMs with 2+ hidden layers hold more per-latent state than that (-DCCMI_TARM_WPE24=2 builds
// the A/B variant with their 256-VGPR budget)
#ifndef CCMI_TARM_WPE24
#define CCMI_TARM_WPE24 3
#endif
constexpr int t_arm_wpe(int d, int nh) { return d >= 24 && nh >= 2 ? CCMI_TARM_WPE24 : 3; }

template <int D, int NH>
__global__ __launch_bounds__(kT) __attribute__((amdgpu_waves_per_eu(t_arm_wpe(D, NH)))) void t_arm(const float *__restrict__ yq, Geo g, ArmTiles at, const float *__restrict__ th,
                                            int64_t ps, float lam_px, float *__restrict__ gq,
                                            float *__restrict__ gth, int64_t gstride, float *__restrict__ acc4,
                                            const float *__restrict__ grad_rate, float *__restrict__ rate_out)
{
    constexpr int NT = (D + 15) / 16, MT = (D + 15) / 16;
    __shared__ float s_y[kALH][kALW];
    // MFMA staging rows (per wave: gradients s_g, activations s_a), one array so the
    // context-gradient planes can span both once the MFMA stage is over
    __shared__ float s_ga[2 * kT * (D + 1)];
    float *const s_g = s_ga, *const s_a = s_ga + kT * (D + 1);
    __shared__ float s_zero[1]; // what the context gather reads for terms outside the tile
    if (threadIdx.x == 0) s_zero[0] = 0.f; // visible after the tile loop's first barrier

    const int b = blockIdx.y;
    const int w = threadIdx.x >> 6;
    const cfloat_ptr P = (cfloat_ptr)(size_t)(th + (int64_t)b * ps);
    float *sg = s_g + 64 * w * (D + 1), *sa = s_a + 64 * w * (D + 1); // this wave's rows
    const int cx = threadIdx.x % kATX, cy = threadIdx.x / kATX;
    // weight-gradient accumulators (matrix cores) and bias-gradient sums (VALU), kept over
    // every tile this workgroup visits
    v4f acc_o[1][NT], acc_h[NH > 0 ? NH : 1][MT][NT], accb_o[1], accb_h[NH > 0 ? NH : 1][MT];
    const v4f z4 = {0.f, 0.f, 0.f, 0.f};
    accb_o[0] = z4;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc_o[0][nt] = z4;
#pragma unroll
    for (int L = 0; L < (NH > 0 ? NH : 1); ++L)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            accb_h[L][mt] = z4;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc_h[L][mt][nt] = z4;
        }
    float rsum = 0.f;

    // the latent tile (+ causal halo) of the NEXT tile is loaded into registers while this
    // one is processed, so a tile starts without waiting on HBM
    constexpr int kSU = (kALH * kALW + kT - 1) / kT;
    float pre[kSU];
    auto tile_geo = [&](int t, int &l, int &y0, int &x0) {
        l = 0;
#pragma unroll
        for (int k = 1; k < CCMI_MAX_GRIDS; ++k)
            if (k < at.n && t >= at.start[k]) l = k;
        const int lt = t - at.start[l];
        y0 = (lt / at.tiles_x[l]) * kATY;
        x0 = (lt % at.tiles_x[l]) * kATX;
    };
    auto load_tile = [&](int t) {
        int l, y0, x0;
        tile_geo(t, l, y0, x0);
        const int H = g.h[l], W = g.w[l];
        const float *src = yq + (int64_t)b * g.N + g.off[l];
        int tid = threadIdx.x; // opaque: its tile-invariant indices are not hoisted and kept live
        asm volatile("" : "+v"(tid));
#pragma unroll
        for (int u = 0; u < kSU; ++u) {
            const int i = tid + u * kT;
            const int r = i / kALW, c = i - r * kALW;
            const int y = y0 - kAH + r, x = x0 - kAH + c;
            pre[u] = (i < kALH * kALW && y >= 0 && y < H && x >= 0 && x < W) ? src[y * W + x] : 0.f;
        }
    };
    const int n_tiles = at.start[at.n];
    if ((int)blockIdx.x < n_tiles) load_tile(blockIdx.x);

    for (int t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        int l, y0, x0;
        tile_geo(t, l, y0, x0);
        const int H = g.h[l], W = g.w[l];
        float *gdst = gq + (int64_t)b * g.N + g.off[l];
        __syncthreads(); // previous tile's LDS readers are done
#pragma unroll
        for (int u = 0; u < kSU; ++u) {
            const int i = threadIdx.x + u * kT;
            if (i < kALH * kALW) (&s_y[0][0])[i] = pre[u];
        }
        if (t + (int)gridDim.x < n_tiles) load_tile(t + gridDim.x);
        __syncthreads();
        const bool valid = (y0 + cy) < H && (x0 + cx) < W;

        float xs[NH + 1][D];
#pragma unroll
        for (int i = 0; i < D; ++i) {
            int dy, dx;
            ctx_off<D>(i, dy, dx);
            xs[0][i] = s_y[cy + kAH + dy][cx + kAH + dx];
        }
#pragma unroll
        for (int L = 0; L < NH; ++L) {
            const cfloat_ptr Wl = P + L * (D * D + D);
#pragma unroll
            for (int j = 0; j < D; ++j) {
                float z = ARMW(Wl, D * D + j);
#pragma unroll
                for (int i = 0; i < D; ++i) z = fmaf(ARMW(Wl, j * D + i), xs[L][i], z);
                z += xs[L][j];
                xs[L + 1][j] = fmaxf(z, 0.f);
            }
        }
        const cfloat_ptr Wo = P + NH * (D * D + D);
        float mu = ARMW(Wo, 2 * D), ls = ARMW(Wo, 2 * D + 1);
#pragma unroll
        for (int i = 0; i < D; ++i) {
            mu = fmaf(ARMW(Wo, i), xs[NH][i], mu);
            ls = fmaf(ARMW(Wo, D + i), xs[NH][i], ls);
        }
        const float q = s_y[cy + kAH][cx + kAH];
        float g_q, g_mu, g_ls, rbits;
        {
            const int64_t li = (int64_t)b * g.N + g.off[l] + (int64_t)(y0 + cy) * W + (x0 + cx);
            float lam = lam_px;
            if (valid && grad_rate) {
                lam = grad_rate[li];
                // waited for here: at the use below, past the branch, the compiler's wait is a
                // vmcnt(0) on every path -- also behind the next tile's prefetch loads and the
                // gather atomics when there is no grad_rate (training)
                __builtin_amdgcn_s_waitcnt(0x0f70); // vmcnt(0)
            }
            arm_rate(q, mu, ls, valid, lam, rbits, g_q, g_mu, g_ls);
            if (valid) {
                rsum += rbits;
                if (rate_out) rate_out[li] = rbits;
            }
        }
        // ---- backward through the MLP; weight gradients on the matrix cores
        float gx[D];
        {
#pragma unroll
            for (int i = 0; i < D; ++i) gx[i] = ARMW(Wo, i) * g_mu + ARMW(Wo, D + i) * g_ls;
            sg[(threadIdx.x & 63) * 3 + 0] = g_mu; // [64][2], pitch 3, column 2 zero
            sg[(threadIdx.x & 63) * 3 + 1] = g_ls;
            sg[(threadIdx.x & 63) * 3 + 2] = 0.f;
#pragma unroll
            for (int i = 0; i < D; ++i) sa[(threadIdx.x & 63) * (D + 1) + i] = xs[NH][i];
            sa[(threadIdx.x & 63) * (D + 1) + D] = 0.f;
            wave_lds_sync(); // each wave stages and reads only its own 64 rows
#if !defined(CCMI_DIAG_ARM_NOOUTER)
            mfma_outer<2, D>(sg, sa, acc_o, accb_o);
#endif
            wave_lds_sync();
        }
#pragma unroll
        for (int L = NH - 1; L >= 0; --L) {
            const cfloat_ptr Wl = P + L * (D * D + D);
            float gz[D];
#pragma unroll
            for (int j = 0; j < D; ++j) {
                gz[j] = xs[L + 1][j] > 0.f ? gx[j] : 0.f;
                sg[(threadIdx.x & 63) * (D + 1) + j] = gz[j];
            }
            sg[(threadIdx.x & 63) * (D + 1) + D] = 0.f;
#pragma unroll
            for (int i = 0; i < D; ++i) sa[(threadIdx.x & 63) * (D + 1) + i] = xs[L][i];
            sa[(threadIdx.x & 63) * (D + 1) + D] = 0.f;
            wave_lds_sync();
#if !defined(CCMI_DIAG_ARM_NOOUTER)
            mfma_outer<D, D>(sg, sa, acc_h[L], accb_h[L]);
#endif
            wave_lds_sync();
#pragma unroll
            for (int i = 0; i < D; ++i) {
                float a = gz[i]; // residual
#pragma unroll
                for (int j = 0; j < D; ++j) a = fmaf(ARMW(Wl, j * D + i), gz[j], a);
                gx[i] = a;
            }
        }
        // ---- context gradients: each latent's D + 1 gradients (contexts, then its own value)
        // go to LDS rows (this wave's own rows of s_g, free after its MFMA stage); every
        // position of the tile + causal halo then GATHERS what the latents whose context holds
        // it send, and adds the sum to HBM with one atomic.  (Scattering with LDS float atomics
        // instead runs at about half a lane per clock on gfx950: 35 % of this kernel; a
        // row-per-wave gather over zero-padded planes measured slower than this form.)
        {
            float *row = sg + (threadIdx.x & 63) * (D + 1);
#pragma unroll
            for (int i = 0; i < D; ++i) row[i] = valid ? gx[i] : 0.f;
            row[D] = valid ? g_q : 0.f;
        }
        __syncthreads();
        // the context of dims 8 / 16 reaches 3 rows up (halo row 0 receives nothing); that of
        // dims 24 / 32 reaches 4 (offsets 4 and 2..5 of ctx_off: dy = -4)
        constexpr int kR0 = D >= 24 ? 0 : 1;
        // a fixed number of atomics per thread (positions past the halo or outside the grid add
        // 0 at a clamped in-grid address): the next tile's staging then waits for its prefetch
        // loads only, not for these atomics; indices from an opaque thread index (not hoisted)
        constexpr int kGN = (kALH - kR0) * kALW, kGI = (kGN + kT - 1) / kT;
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));
#pragma unroll
        for (int u = 0; u < kGI; ++u) {
            const int i = tid + u * kT;
            const int r = kR0 + i / kALW, c = i - (r - kR0) * kALW;
            const int y = y0 - kAH + r, x = x0 - kAH + c;
            const float v = gather_ctx<D>(s_g, s_zero, r, c);
            const bool in = i < kGN && y >= 0 && y < H && x >= 0 && x < W;
            atomicAdd(&gdst[min(max(y, 0), H - 1) * W + min(max(x, 0), W - 1)], in ? v : 0.f);
        }
    }
    // ---- flush: the four waves' weight / bias gradients meet in LDS, then one atomic per value
    // per workgroup (see t_arm16's flush)
    static_assert(kT == 4 * 64, "four waves per workgroup");
    constexpr int LS = D * D + D, kRed = NH * LS + 2 * D + 2;
    static_assert(4 * kRed <= 2 * kT * (D + 1), "the partial rows fit s_ga");
    float *red = s_ga + w * kRed;
    __syncthreads(); // last tile's gather reads of s_g are done
    stage_outer<2, D>(acc_o, accb_o, red + NH * LS, red + NH * LS + 2 * D);
#pragma unroll
    for (int L = 0; L < NH; ++L) stage_outer<D, D>(acc_h[L], accb_h[L], red + L * LS, red + L * LS + D * D);
    __syncthreads();
    float *G = gth + ((int64_t)b * kDwSlots + blockIdx.x % kDwSlots) * gstride; // this workgroup's slot row
    for (int e = threadIdx.x; e < kRed; e += kT)
        atomicAdd(&G[e], (s_ga[e] + s_ga[kRed + e]) + (s_ga[2 * kRed + e] + s_ga[3 * kRed + e]));
    wave_add(rsum, &acc4[b * kDwSlots + blockIdx.x % kDwSlots]); // the frame's rate slots
}

// ARM forward + rate + backward for dim_arm = 16 with the MLP on the matrix cores.
// A wave owns one 64-latent row of the 4 x 64 tile, as 4 groups of 16 latents.  Each
// 16 x 16 layer is Z^T = W X^T on v_mfma_f32_16x16x4_f32 (A = W, B = X^T, K = the layer's
// inputs), with the K order permuted so that input k = 4 (lane >> 4) + s: the accumulator
// register r of lane l then holds unit 4 (l >> 4) + r of latent l & 15 -- exactly the B
// operand of the next layer, so activations never leave the registers, and residual, bias
// and ReLU are elementwise on the accumulators.  The weights (W for the forward, W^T for
// the input gradients, the output layer) are loaded from HBM ONCE per workgroup (one frame)
// into LDS and read from there per tile: no per-tile global weight loads (their scalar-load
// waits were 37 % of the VALU kernel, tools/arm_diag.sh NOWLOAD).  The 2-wide output layer and the rate are VALU
// (an M = 2 MFMA would be 8x padding); the rate runs one latent per lane (lane = tile
// column: group g's values sit in the lanes with lane >> 4 == g).  Weight gradients of the
// hidden layers: LDS-staged rows on the matrix cores (mfma_outer, K = latents); biases and
// the output layer's weight gradients: per-lane partial sums over every tile the workgroup
// visits, reduced once at the end.
// waves / SIMD the register allocation targets: 4 (<= 128 VGPRs) for up to two hidden layers --
// the few values it spills are the epilogue's, outside the tile loop -- 3 for three
#ifndef CCMI_ARM16_WAVES
#define CCMI_ARM16_WAVES 4
#endif
constexpr int t_arm16_wpe(int nh) { return nh <= 2 ? CCMI_ARM16_WAVES : 3; }
template <int NH>
__global__ __launch_bounds__(kT) __attribute__((amdgpu_waves_per_eu(t_arm16_wpe(NH)))) void t_arm16(
    const float *__restrict__ yq, Geo g, ArmTiles at, const float *__restrict__ th, int64_t ps, float lam_px,
    float *__restrict__ gq, float *__restrict__ gth, int64_t gstride, float *__restrict__ acc4,
    const float *__restrict__ grad_rate, float *__restrict__ rate_out)
{
    constexpr int D = 16, LS = D * D + D, NL = NH > 0 ? NH : 1;
    __shared__ float s_y[kALH][kALW];
    __shared__ float s_ga[2 * kT * (D + 1)];
    float *const s_g = s_ga, *const s_a = s_ga + kT * (D + 1);
    __shared__ float s_zero[1]; // what the context gather reads for terms outside the tile
    if (threadIdx.x == 0) s_zero[0] = 0.f; // visible after the tile loop's first barrier
    const int b = blockIdx.y, w = threadIdx.x >> 6, lane = threadIdx.x & 63, ln = lane & 15, lk = lane >> 4;
    const int cy = w, cx = lane; // per-latent phase: this lane's latent in the tile
    const cfloat_ptr P = (cfloat_ptr)(size_t)(th + (int64_t)b * ps);
    float *sg = s_g + 64 * w * (D + 1), *sa = s_a + 64 * w * (D + 1);

    // the hidden layers' weights and biases in LDS (2.2 KB for two layers: the workgroup's LDS
    // stays <= 40 KB, 4 workgroups per CU), read per tile as the MFMA A operands: held in
    // registers (24 VGPRs) they pushed the kernel past 128 VGPRs into scratch
    __shared__ __attribute__((aligned(16))) float s_w[NL][LS];
    for (int i = threadIdx.x; i < NH * LS; i += kT) s_w[i / LS][i % LS] = P[i];
    const cfloat_ptr Wo = P + NH * LS;
    // the output layer's weights in LDS too, read where used (8 fewer persistent VGPRs)
    __shared__ __attribute__((aligned(16))) float s_wo[2 * D];
    for (int i = threadIdx.x; i < 2 * D; i += kT) s_wo[i] = Wo[i];
    const float bo0 = Wo[2 * D], bo1 = Wo[2 * D + 1];
    // s_y offsets of the context inputs k = 4 lk + s, derived per tile from an opaque lane
    // index (kept across the tile loop they were 4 more persistent VGPRs)
    auto ctx_offsets = [&](int (&coff)[4]) {
        int lko = lk;
        asm volatile("" : "+v"(lko));
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            int o[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                int dy, dx;
                ctx_off<D>(4 * q + s, dy, dx);
                o[q] = dy * kALW + dx;
            }
            coff[s] = lko == 0 ? o[0] : lko == 1 ? o[1] : lko == 2 ? o[2] : o[3];
        }
    };

    const v4f z4 = {0.f, 0.f, 0.f, 0.f};
    v4f acc_h[NL][1][1], accb_dummy[1];
    float accb[NL][4], accwo0[4], accwo1[4];
#pragma unroll
    for (int L = 0; L < NL; ++L) {
        acc_h[L][0][0] = z4;
#pragma unroll
        for (int r = 0; r < 4; ++r) accb[L][r] = 0.f;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) accwo0[r] = accwo1[r] = 0.f;
    float accbo0 = 0.f, accbo1 = 0.f, rsum = 0.f;

    constexpr int kSU = (kALH * kALW + kT - 1) / kT;
    float pre[kSU];
    auto tile_geo = [&](int t, int &l, int &y0, int &x0) {
        l = 0;
#pragma unroll
        for (int k = 1; k < CCMI_MAX_GRIDS; ++k)
            if (k < at.n && t >= at.start[k]) l = k;
        const int lt = t - at.start[l];
        y0 = (lt / at.tiles_x[l]) * kATY;
        x0 = (lt % at.tiles_x[l]) * kATX;
    };
    auto load_tile = [&](int t) {
        int l, y0, x0;
        tile_geo(t, l, y0, x0);
        const int H = g.h[l], W = g.w[l];
        const float *src = yq + (int64_t)b * g.N + g.off[l];
        // the staging indices from an opaque thread index, re-derived per tile: hoisted, two
        // of them were spilled and their reloads' vmcnt(0) inside this prefetch waited for the
        // previous tile's gather atomics (measured neutral, 232 us either way: r6k)
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));
#pragma unroll
        for (int u = 0; u < kSU; ++u) {
            const int i = tid + u * kT;
            const int r = i / kALW, c = i - r * kALW;
            const int y = y0 - kAH + r, x = x0 - kAH + c;
            pre[u] = (i < kALH * kALW && y >= 0 && y < H && x >= 0 && x < W) ? src[y * W + x] : 0.f;
        }
    };
    const int n_tiles = at.start[at.n];
    if ((int)blockIdx.x < n_tiles) load_tile(blockIdx.x);

    for (int t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        int l, y0, x0;
        tile_geo(t, l, y0, x0);
        const int H = g.h[l], W = g.w[l];
        float *gdst = gq + (int64_t)b * g.N + g.off[l];
        __syncthreads(); // previous tile's LDS readers are done
#pragma unroll
        for (int u = 0; u < kSU; ++u) {
            const int i = threadIdx.x + u * kT;
            if (i < kALH * kALW) (&s_y[0][0])[i] = pre[u];
        }
        if (t + (int)gridDim.x < n_tiles) load_tile(t + gridDim.x);
        __syncthreads();
        const bool valid = (y0 + cy) < H && (x0 + cx) < W;

        // ---- forward: X[L][g][r] = input / activation unit 4 lk + r of latent 16 g + ln.
        // What the backward needs of the hidden activations is kept small: their ReLU masks (as
        // lane masks, SGPRs), and the input of the last hidden
        // layer (X[NH - 1], NH >= 2) staged in this wave's rows of s_a right away, where that
        // layer's weight-gradient MFMAs read it -- 32 fewer live VGPRs across the backward, so
        // the kernel fits 4 waves / SIMD without spills (round 3: 168 VGPRs + 13 spilled, and
        // the spill reloads' vmcnt(0) waited for the previous tile's gradient atomics)
        const float *yrow = &s_y[cy + kAH][kAH + ln];
        int coff[4];
        ctx_offsets(coff);
        float X[NH + 1][4][4];
        bool pos[NL][4][4]; // ReLU masks: lane masks in SGPR pairs, one v_cndmask each in the backward
#pragma unroll
        for (int gg = 0; gg < 4; ++gg)
#pragma unroll
            for (int s = 0; s < 4; ++s) X[0][gg][s] = yrow[16 * gg + coff[s]];
#pragma unroll
        for (int L = 0; L < NH; ++L) {
            // A = W[j = ln][i = 4 lk + s]; bias of unit 4 lk + r
            const v4f WA = *reinterpret_cast<const v4f *>(&s_w[L][ln * D + 4 * lk]);
            const v4f BI = *reinterpret_cast<const v4f *>(&s_w[L][D * D + 4 * lk]);
#pragma unroll
            for (int gg = 0; gg < 4; ++gg) {
                v4f acc = BI;
#pragma unroll
                for (int s = 0; s < 4; ++s) acc = mfma4(WA[s], X[L][gg][s], acc);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    X[L + 1][gg][r] = fmaxf(acc[r] + X[L][gg][r], 0.f);
                    pos[L][gg][r] = X[L + 1][gg][r] > 0.f;
                    if (NH >= 2 && L + 1 == NH - 1) sa[(16 * gg + ln) * (D + 1) + 4 * lk + r] = X[L + 1][gg][r];
                }
            }
        }
        // output layer: partial dot products over this lane's 4 units, summed over the 4
        // lanes of the latent; group g's (mu, ls) kept by the lanes with lk == g
        float mu = 0.f, ls = 0.f;
        v4f WO0 = *reinterpret_cast<const v4f *>(&s_wo[4 * lk]), WO1 = *reinterpret_cast<const v4f *>(&s_wo[D + 4 * lk]);
#pragma unroll
        for (int gg = 0; gg < 4; ++gg) {
            float pm = 0.f, pl = 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                pm = fmaf(WO0[r], X[NH][gg][r], pm);
                pl = fmaf(WO1[r], X[NH][gg][r], pl);
            }
            pm = sum_rows(pm);
            pl = sum_rows(pl);
            if (gg == lk) {
                mu = pm + bo0;
                ls = pl + bo1;
            }
        }
        // ---- rate, one latent per lane
        const float q = s_y[cy + kAH][cx + kAH];
        float g_q, g_mu, g_ls, rbits;
        {
            const int64_t li = (int64_t)b * g.N + g.off[l] + (int64_t)(y0 + cy) * W + (x0 + cx);
            float lam = lam_px;
            if (valid && grad_rate) {
                lam = grad_rate[li];
                // waited for here: at the use below, past the branch, the compiler's wait is a
                // vmcnt(0) on every path -- also behind the next tile's prefetch loads and the
                // gather atomics when there is no grad_rate (training)
                __builtin_amdgcn_s_waitcnt(0x0f70); // vmcnt(0)
            }
#if defined(CCMI_DIAG_A16_NORATE) // diagnostic builds only (tools/arm_diag.sh): wrong results
            rbits = mu; g_q = ls * lam; g_mu = q * ls; g_ls = mu * q;
#else
            arm_rate(q, mu, ls, valid, lam, rbits, g_q, g_mu, g_ls);
#endif
            if (valid) {
                rsum += rbits;
                if (rate_out) rate_out[li] = rbits;
            }
        }
        accbo0 += g_mu;
        accbo1 += g_ls;
        // ---- backward: output layer (VALU), its weight gradients as per-lane partial sums
        WO0 = *reinterpret_cast<const v4f *>(&s_wo[4 * lk]);
        WO1 = *reinterpret_cast<const v4f *>(&s_wo[D + 4 * lk]);
        float G[4][4], gmb[4], glb[4];
        bcast_rows(g_mu, gmb);
        bcast_rows(g_ls, glb);
#pragma unroll
        for (int gg = 0; gg < 4; ++gg) {
            const float gm = gmb[gg], gl = glb[gg];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                G[gg][r] = WO0[r] * gm + WO1[r] * gl;
                accwo0[r] = fmaf(gm, X[NH][gg][r], accwo0[r]);
                accwo1[r] = fmaf(gl, X[NH][gg][r], accwo1[r]);
            }
        }
        // hidden layers
#pragma unroll
        for (int L = NH - 1; L >= 0; --L) {
            float gz[4][4];
#pragma unroll
            for (int gg = 0; gg < 4; ++gg)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    gz[gg][r] = pos[L][gg][r] ? G[gg][r] : 0.f;
                    sg[(16 * gg + ln) * (D + 1) + 4 * lk + r] = gz[gg][r];
                    // layer 0's input is the context, re-read from the tile (not kept live);
                    // the last hidden layer's input was staged by the forward
                    if (L == 0) sa[(16 * gg + ln) * (D + 1) + 4 * lk + r] = yrow[16 * gg + coff[r]];
                    else if (L != NH - 1) sa[(16 * gg + ln) * (D + 1) + 4 * lk + r] = X[L][gg][r];
                }
#pragma unroll
            for (int r = 0; r < 4; ++r) accb[L][r] += (gz[0][r] + gz[1][r]) + (gz[2][r] + gz[3][r]);
            wave_lds_sync(); // each wave stages and reads only its own 64 rows
#if !defined(CCMI_DIAG_A16_NOOUTER)
            mfma_outer<D, D, false>(sg, sa, acc_h[L], accb_dummy);
#endif
            wave_lds_sync();
            // input gradient: W^T gz + gz (residual), K permuted like the forward;
            // A = W^T[i = ln][j = 4 lk + s]
            float WT[4];
#pragma unroll
            for (int s = 0; s < 4; ++s) WT[s] = s_w[L][(4 * lk + s) * D + ln];
#pragma unroll
            for (int gg = 0; gg < 4; ++gg) {
                v4f acc = {gz[gg][0], gz[gg][1], gz[gg][2], gz[gg][3]};
#pragma unroll
                for (int s = 0; s < 4; ++s) acc = mfma4(WT[s], gz[gg][s], acc);
#pragma unroll
                for (int r = 0; r < 4; ++r) G[gg][r] = acc[r];
            }
        }
        // ---- context gradients (input k = 4 lk + r of latent 16 g + ln) and the latent's own
        // gradient to this wave's rows of s_g, then the gather of t_arm
#pragma unroll
        for (int gg = 0; gg < 4; ++gg)
#pragma unroll
            for (int r = 0; r < 4; ++r) sg[(16 * gg + ln) * (D + 1) + 4 * lk + r] = G[gg][r];
        sg[lane * (D + 1) + D] = g_q;
        __syncthreads();
        // exactly two atomics per thread (positions past the halo, or outside the grid, add 0 at
        // a clamped in-grid address): with a fixed count after the next tile's prefetch loads,
        // the next tile's staging waits for those loads only (vmcnt(2)), not for these atomics
        static_assert((kALH - 1) * kALW <= 2 * kT, "two gather positions per thread");
        // the positions' tile-invariant indices are re-derived from an opaque copy of the
        // thread index per tile: hoisted out of the tile loop they held ~60 VGPRs
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));
#if defined(CCMI_DIAG_A16_NOGATHER)
        if (tid < 0)
#endif
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int i = tid + u * kT;
            const int r = 1 + i / kALW, c = i - (r - 1) * kALW;
            const int y = y0 - kAH + r, x = x0 - kAH + c;
            const float v = gather_ctx<D>(s_g, s_zero, r, c);
            const bool in = i < (kALH - 1) * kALW && y >= 0 && y < H && x >= 0 && x < W;
            atomicAdd(&gdst[min(max(y, 0), H - 1) * W + min(max(x, 0), W - 1)], in ? v : 0.f);
        }
    }
#if defined(CCMI_DIAG_NOFLUSH) // diagnostic build only (make diag): wrong results -- and with the
    return;                       // accumulators dead, the compiler drops the weight-gradient work too
#endif
    // ---- flush: the four waves' partial sums meet in LDS (s_ga is free after the tile loop) and
    // each value goes out with ONE atomic per workgroup.  (One atomic per value per wave, every
    // workgroup of a frame on the same ~600 addresses, serialised in L2: the kernel's time grew
    // linearly with its grid -- 293 / 460 / 572 / 745 us for 1024 / 2048 / 3072 / 4096
    // workgroups, profiles/r4l_*.)
    static_assert(kT == 4 * 64, "four waves per workgroup");
    constexpr int kRed = NH * LS + 2 * D + 2; // the gradient row's ARM part, Gp layout
    float *red = s_ga + w * kRed;             // this wave's partial row
    __syncthreads();                          // last tile's gather reads of s_g are done
#pragma unroll
    for (int L = 0; L < NH; ++L) {
#pragma unroll
        for (int r = 0; r < 4; ++r) { // dW_L[m = 4 lk + r][n = ln]
            red[L * LS + (4 * lk + r) * D + ln] = acc_h[L][0][0][r];
            float v = accb[L][r];
            for (int o = 1; o < 16; o <<= 1) v += __shfl_xor(v, o);
            if (ln == 0) red[L * LS + D * D + 4 * lk + r] = v;
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        float v0 = accwo0[r], v1 = accwo1[r];
        for (int o = 1; o < 16; o <<= 1) {
            v0 += __shfl_xor(v0, o);
            v1 += __shfl_xor(v1, o);
        }
        if (ln == 0) {
            red[NH * LS + 4 * lk + r] = v0;
            red[NH * LS + D + 4 * lk + r] = v1;
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        accbo0 += __shfl_xor(accbo0, o);
        accbo1 += __shfl_xor(accbo1, o);
    }
    if (lane == 0) {
        red[NH * LS + 2 * D] = accbo0;
        red[NH * LS + 2 * D + 1] = accbo1;
    }
    __syncthreads();
    float *Gp = gth + ((int64_t)b * kDwSlots + blockIdx.x % kDwSlots) * gstride; // this workgroup's slot row
    for (int e = threadIdx.x; e < kRed; e += kT)
        atomicAdd(&Gp[e], (s_ga[e] + s_ga[kRed + e]) + (s_ga[2 * kRed + e] + s_ga[3 * kRed + e]));
    wave_add(rsum, &acc4[b * kDwSlots + blockIdx.x % kDwSlots]); // the frame's rate slots
}

#undef ARMW

// Both ARM kernels take the same arguments: yq, g, at, th, ps, lam_px, gq, gth, gstride, acc4,
// grad_rate, rate_out
using ArmKernel = void (*)(const float *, Geo, ArmTiles, const float *, int64_t, float, float *, float *, int64_t, float *,
                           const float *, float *);

// dim_arm D: the matrix-core ARM (t_arm16) for 16 -- its MFMA chains replace the scalar weight
// loads of the VALU kernel's tile loop (606 -> 499 us per 8-frame iteration) --
// and the VALU ARM (t_arm) otherwise
template <int D>
ArmKernel arm_kernel(int nh)
{
    if constexpr (D == 16) {
        switch (nh) {
        case 0: return t_arm16<0>;
        case 1: return t_arm16<1>;
        case 2: return t_arm16<2>;
        default: return t_arm16<3>;
        }
    }
    switch (nh) {
    case 0: return t_arm<D, 0>;
    case 1: return t_arm<D, 1>;
    case 2: return t_arm<D, 2>;
    default: return t_arm<D, 3>;
    }
}

} // namespace

// Persistent over the latent tiles of every level: one resident round of workgroups for the
// batch, at most cap per CU
void ccmi_train::launch_arm(const Geo &g, const ArmTiles &at, const ccmi_train_args &a, const Work &w, float lam_px, float *gq,
                            int cap, hipStream_t s)
{
    const ArmKernel k = g.d == 8 ? arm_kernel<8>(g.nh) : g.d == 16 ? arm_kernel<16>(g.nh) : g.d == 24 ? arm_kernel<24>(g.nh) : arm_kernel<32>(g.nh);
    hipLaunchKernelGGL(k, resident_grid((const void *)k, kT, 0, at.start[at.n], a.batch, cap), dim3(kT), 0, s, w.yq, g, at, a.params,
                       a.param_stride, lam_px, gq, w.slots, (int64_t)g.P, w.rslots, a.grad_rate, a.rate_out);
}
