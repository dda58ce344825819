// train.hip -- the encoder overfit step on the GPU: training forward, backward, gradient
// clipping and Adam for a batch of independent frames (one network + latents each).
//
// Reference, enc/training/train.py:238-262 (one iteration):
//   frame_encoder.forward (train mode)  coolchic.py:291-479, frame.py:175-183
//     quantize            quantizer.py:16-232   (softround / noise / STE variants)
//     ARM + Laplace rate  arm.py:227-370, coolchic.py:395-424
//     Upsampling          upsampling.py:195-202, 322-335, 476-506 (train = kron-2D form,
//                         mathematically the separable eval form computed here)
//     Synthesis           synthesis.py:69-84, 264-277
//     420 nearest + clamp yuv.py:275-299
//   loss_function          loss.py (MSE + lmbda * rate_bpp)
//   loss.backward(); clip_grad_norm_(params, 0.1); torch.optim.Adam.step()
//
// This unit holds the driver (ccmi_train_step_dist), the workspace plan, the quantiser, the
// gradient fold, the norm and Adam; the other stages live in a unit each behind a launcher
// (train_internal.h).  Launch order (all frames of the batch in every launch), unit in brackets:
//   t_prologue            per-step zeroing + trainable half kernels -> full symmetric kernels
//                         (upsampling.py:46-68)                                       [train.hip]
//   t_quant               y_hat = Q(gain * y) and dQ/dy; noise from a counter-based RNG (or
//                         given)                                                      [train.hip]
//   t_arm / t_arm16       ARM forward + rate + full backward in one pass, on a side stream
//                         (CCMI_ARM_OVERLAP) that joins before t_dw_fold           [train_arm.hip]
//   (upsampling forward: the path-A level kernels, keeping every pyramid stack)     [fwd_ups.hip]
//   t_head_fwd            1x1 head forward                                        [train_head.hip]
//   t_sp_fwd<LOSS>        3x3 layers forward, intermediate 3-channel maps kept; the last one
//                         of a training step with the MSE and its gradient fused in [train_sp.hip]
//   t_loss                the MSE on its own (forward-only calls, no 3x3 layer);
//                         with a ccmi_train_dist the MS-SSIM stage instead [train_sp.hip, dist_msssim.hip]
//   t_sp_bwd<MODE>        3x3 layers backward (replicate-padding adjoint as a gather) [train_sp.hip]
//   t_head_bwd_t / _m / t_head_bwd   1x1 head backward, weight gradients on the matrix
//                         cores                                                   [train_head.hip]
//   t_lvl_bwd             upsampling backward, one launch per pyramid step (refine + transposed
//                         conv); K = 4 / 6: t_ref_bwd, t_up_u, t_up_gu, t_up_dw, t_up_gs [train_ups.hip]
//   t_dw_fold             the parameter gradients' slot rows summed into the gradient row [train.hip]
//   t_latgrad_sumsq, t_adam_bc, t_adam / t_finish   dL/dy + global grad norm, clipped Adam
//                         update, the loss row                                        [train.hip]
#include <stdlib.h>

#include <cmath>
#include <map>
#include <mutex>
#include <tuple>

#include "ccmi_noise.h"
#include "train_internal.h"

using namespace ccmi_train;

namespace {

// ------------------------------------------------------------------ parameters
// Per-step prologue in one launch (three launches before: a memset, t_zero_rows, t_expand --
// each a dependent dispatch of ~6 us on the step's critical path, profiles/r5l_train_timeline.txt):
// zero nz floats from z (acc4, the rate and parameter-gradient slots, the ARM's side gradient),
// expand the symmetric upsampling kernels, and count the step in the caller's step counters.
__global__ void t_prologue(float *__restrict__ z, int64_t nz, const float *__restrict__ th, int64_t ps, Geo g,
                           float *__restrict__ kf, int B, int32_t *__restrict__ counters)
{
    if (counters && blockIdx.x == 0)
        for (int i = threadIdx.x; i < B; i += kT) counters[i] += 1; // the caller's per-frame step counts
    const int64_t n = nz + (int64_t)B * g.kfull;
    for (int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x; i < n; i += (int64_t)gridDim.x * kT) {
        if (i < nz) {
            z[i] = 0.f;
        } else {
            const int j = (int)(i - nz), b = j / g.kfull, e = j - b * g.kfull;
            const float *p = th + (int64_t)b * ps;
            float v;
            if (e < g.n_ups * g.K) {
                const int u = e / g.K, t = e - u * g.K;
                v = p[g.up_off + u * g.hu + min(t, g.K - 1 - t)];
            } else {
                const int r = e - g.n_ups * g.K, u = r / g.Kp, t = r - u * g.Kp;
                v = p[g.pre_off + u * g.hp + min(t, g.Kp - 1 - t)];
            }
            kf[(int64_t)b * g.kfull + e] = v;
        }
    }
}

// ------------------------------------------------------------------ quantizer
using ccmi::mix64; // the generator of ccmi.h (ccmi_noise.h)
using ccmi::unif;

struct SoftRound {
    float t, inv; // inv = 1 / tanh(1 / (2t))
    __device__ float f(float x) const
    {
        const float fx = floorf(x), d = x - fx - 0.5f;
        return fx + 0.5f * tanhf(d / t) * inv + 0.5f;
    }
    __device__ float df(float x) const
    {
        const float fx = floorf(x), th = tanhf((x - fx - 0.5f) / t);
        return 0.5f * (1.f - th * th) / t * inv;
    }
    // f(x) and df(x) from one tanh (the same expressions as f / df)
    __device__ void fdf(float x, float &y, float &d) const
    {
        const float fx = floorf(x), th = tanhf((x - fx - 0.5f) / t);
        y = fx + 0.5f * th * inv + 0.5f;
        d = 0.5f * (1.f - th * th) / t * inv;
    }
};

// Quantiser constants, uniform over the launch (computed once on the host): softround
// temperature and 1 / tanh(1 / 2t); kumaraswamy a, 1 / a and 1 / b (quantizer.py:60-102)
struct QuantArgs {
    float temp, inv, ka_inv, kb_inv, nprm;
};

QuantArgs quant_args(float temp, float nprm)
{
    QuantArgs q{temp, 0.f, 0.f, 0.f, nprm};
    if (temp > 0.f) q.inv = 1.f / std::tanh(1.f / (2.f * temp));
    if (nprm > 0.f) {
        const float a = nprm, b = (std::exp2(a) * (a - 1.f) + 1.f) / a;
        q.ka_inv = 1.f / a;
        q.kb_inv = 1.f / b;
    }
    return q;
}

__global__ void t_quant(const float *__restrict__ lat, int64_t ls, int N, float gain, int qt, int nz, QuantArgs Q,
                        uint64_t seed, int step, const float *__restrict__ noise_in, float *__restrict__ yq,
                        float *__restrict__ dq, float *__restrict__ gq)
{
    const int b = blockIdx.y, i = blockIdx.x * kT + threadIdx.x;
    if (i >= N) return;
    const int64_t li = (int64_t)b * ls + i, wi = (int64_t)b * N + i;
    const float x = gain * lat[li];
    float n = 0.f;
    if (noise_in) {
        n = noise_in[li];
    } else if (nz != CCMI_NOISE_NONE) {
        const uint64_t r = mix64(seed ^ mix64(((uint64_t)step << 40) ^ ((uint64_t)b << 32) ^ (uint64_t)i));
        const float u1 = unif(r);
        if (nz == CCMI_NOISE_KUMARASWAMY) { // generate_kumaraswamy_noise: (1 - (1 - u)^(1/b))^(1/a) - 1/2
            // powers through v_log_f32 / v_exp_f32 (u1 in (0, 1]: both bases in [0, 1], the ends
            // giving -inf -> 0); every draw is held to the generator of ccmi.h by
            // tests/test_train_noise_gpu.py: |CDF(n) - u1| <= K(a) 2^-24 (tests/noise_ref.py)
            const float p = exp2f(__log2f(1.f - u1) * Q.kb_inv);
            n = exp2f(__log2f(1.f - p) * Q.ka_inv) - 0.5f;
        } else { // gaussian: Box-Muller
            const float u2 = unif(mix64(r + 0x632BE59BD9B4E019ull));
            n = sqrtf(-2.f * logf(u1)) * cospif(2.f * u2) * Q.nprm;
        }
    }
    const SoftRound s{Q.temp, Q.inv};
    float y, d;
    switch (qt) {
    case CCMI_Q_NONE: y = x + n; d = 1.f; break;
    case CCMI_Q_SOFTROUND_ALONE: s.fdf(x, y, d); break;
    case CCMI_Q_SOFTROUND: {
        float fx, dx, du;
        s.fdf(x, fx, dx);
        s.fdf(fx + n, y, du);
        d = du * dx;
        break;
    }
    case CCMI_Q_STE: y = rintf(x); d = s.df(x); break;
    case CCMI_Q_TRUE_STE: y = rintf(x); d = 1.f; break;
    default: y = rintf(x); d = 0.f; break; // hardround: torch.round has a zero gradient
    }
    yq[wi] = y;
    if (dq) dq[wi] = gain * d;
    if (gq) gq[wi] = 0.f;
}

__global__ void t_dw_fold(const float *__restrict__ slots, int nreg, float *__restrict__ gth, int64_t gstride, int off)
{
    const int b = blockIdx.y, e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nreg) return;
    const float *sl = slots + (int64_t)b * kDwSlots * nreg + e;
    float v = 0.f;
#pragma unroll 8
    for (int k = 0; k < kDwSlots; ++k) v += sl[(int64_t)k * nreg];
    gth[(int64_t)b * gstride + off + e] = v; // the only writer of the parameter gradients
}

// ------------------------------------------------------------------ latents, norm, Adam

// dL/dy of the latents (G[0, N) = dL/dyhat * dyhat/dy) and the squared norm of the whole
// gradient row (latents + parameters, clip_grad_norm_) in one pass
__global__ __launch_bounds__(kT) void t_latgrad_sumsq(const float *__restrict__ gq, const float *__restrict__ gq2,
                                                      const float *__restrict__ dq, int N, float *__restrict__ G,
                                                      int64_t n, int64_t gstride, float *__restrict__ acc4)
{
    __shared__ float s_red[8];
    const int b = blockIdx.y;
    float *g = G + (int64_t)b * gstride;
    const float *gqb = gq + (int64_t)b * N, *dqb = dq + (int64_t)b * N;
    const float *gq2b = gq2 ? gq2 + (int64_t)b * N : nullptr; // the ARM's part (side-stream form)
    float s = 0.f;
    // four elements per thread and iteration, every load issued first (one per iteration waited
    // on memory latency, as t_loss did)
    constexpr int U = 4;
    for (int64_t i0 = (int64_t)blockIdx.x * kT * U + threadIdx.x; i0 < n; i0 += (int64_t)gridDim.x * kT * U) {
        float a[U], a2[U], d[U], r[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t i = i0 + u * kT, il = i < N ? i : 0;
            a[u] = gqb[il];
            a2[u] = gq2b ? gq2b[il] : 0.f;
            d[u] = dqb[il];
            r[u] = (i >= N && i < n) ? g[i] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t i = i0 + u * kT;
            float v = r[u];
            if (i < N) {
                v = (gq2b ? a2[u] + a[u] : a[u]) * d[u];
                g[i] = v;
            }
            s = fmaf(v, v, s); // 0 past the row
        }
    }
    s = block_sum(s, s_red);
    if (threadIdx.x == 0) atomicAdd(&acc4[b * 4 + 2], s);
}

struct AdamArgs {
    float lr_bc1, inv_sqrt_bc2, beta1, beta2, eps, clip;
    int N, latents_only;
    int64_t n, gstride, ls, ps, ms;
    const float *bc; // optional [B][2] per-frame (lr / bc1, 1 / sqrt(bc2)) (per-frame Adam steps)
    float *loss_out; // optional [B][4]: t_finish's row, written by workgroup (0, b)
    const float *rslots, *mslots;
    float inv_total, lam_px;
    const float *dist4; // optional [B][4]: finish_row
};

// per-frame bias corrections when frames carry their own Adam step (a frame whose optimizer
// state was reloaded from its best record, train.py:226-236): computed in double like the
// host path (torch.optim.Adam's bias_correction1/2 are Python floats); step <= 0 freezes
// the frame: its parameters AND its Adam moments stay as they are (marked by a negative
// second entry, which t_adam checks first)
__global__ void t_adam_bc(const int32_t *__restrict__ steps, double lr, double beta1, double beta2, int B,
                          float *__restrict__ bc)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int t = steps[b];
    if (t <= 0) {
        bc[2 * b] = 0.f;
        bc[2 * b + 1] = -1.f;
        return;
    }
    bc[2 * b] = (float)(lr / (1.0 - pow(beta1, (double)t)));
    bc[2 * b + 1] = (float)(1.0 / sqrt(1.0 - pow(beta2, (double)t)));
}

// torch.optim.Adam (_single_tensor_adam, no weight decay / amsgrad) after clip_grad_norm_
// rslots: [B][kDwSlots] rate sums; mslots: [B][kDwSlots] squared-error sums of the loss fused
// into the last t_sp_fwd (zero when t_loss ran: it adds into acc4[b][0])
__device__ __forceinline__ void finish_row(const float *__restrict__ acc4, const float *__restrict__ rslots,
                                           const float *__restrict__ mslots, float inv_total, float lam_px,
                                           float *__restrict__ out, int b, const float *__restrict__ dist4)
{
    float rate = 0.f, sq = acc4[b * 4 + 0];
#pragma unroll 8
    for (int k = 0; k < kDwSlots; ++k) {
        rate += rslots[b * kDwSlots + k];
        sq += mslots[b * kDwSlots + k];
    }
    // dist4: [B][4] of the MS-SSIM stage (ccmi_train_step_dist): D and MSE come from there
    const float mse = dist4 ? dist4[b * 4 + 2] : sq * inv_total;
    out[b * 4 + 0] = (dist4 ? dist4[b * 4 + 0] : mse) + lam_px * rate;
    out[b * 4 + 1] = mse;
    out[b * 4 + 2] = rate;
    out[b * 4 + 3] = sqrtf(acc4[b * 4 + 2]);
}
__global__ void t_adam(const float *__restrict__ G, float *__restrict__ lat, float *__restrict__ th, float *__restrict__ m,
                       float *__restrict__ v, const float *__restrict__ acc4, AdamArgs A)
{
    const int b = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (A.loss_out && i == 0) finish_row(acc4, A.rslots, A.mslots, A.inv_total, A.lam_px, A.loss_out, b, A.dist4); // (t_finish folded in)
    if (i >= A.n || (A.latents_only && i >= A.N)) return;
    if (A.bc && A.bc[2 * b + 1] < 0.f) return; // frozen frame (adam_steps <= 0)
    float coef = 1.f;
    if (A.clip > 0.f) coef = fminf(A.clip / (sqrtf(acc4[b * 4 + 2]) + 1e-6f), 1.f);
    const float g = G[(int64_t)b * A.gstride + i] * coef;
    const int64_t mi = (int64_t)b * A.ms + i;
    const float mm = A.beta1 * m[mi] + (1.f - A.beta1) * g;
    const float vv = A.beta2 * v[mi] + (1.f - A.beta2) * g * g;
    m[mi] = mm;
    v[mi] = vv;
    const float lr_bc1 = A.bc ? A.bc[2 * b] : A.lr_bc1, inv_sqrt_bc2 = A.bc ? A.bc[2 * b + 1] : A.inv_sqrt_bc2;
    const float denom = sqrtf(vv) * inv_sqrt_bc2 + A.eps;
    float *p = i < A.N ? lat + (int64_t)b * A.ls + i : th + (int64_t)b * A.ps + (i - A.N);
    *p -= lr_bc1 * mm / denom;
}

// one thread per frame, ceil(B / 64) blocks of 64 (one block of B threads is no valid launch
// past B = 1024)
__global__ void t_finish(const float *__restrict__ acc4, const float *__restrict__ rslots, const float *__restrict__ mslots,
                         float inv_total, float lam_px, float *__restrict__ out, int B, const float *__restrict__ dist4)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) finish_row(acc4, rslots, mslots, inv_total, lam_px, out, b, dist4);
}

// ------------------------------------------------------------------ host planning
// CCMI_ARM_OVERLAP = k > 0: the ARM forward + backward runs on a side stream, concurrently with
// the synthesis / upsampling forward and backward, with at most k workgroups per CU (its latent
// gradients in their own buffer, summed by t_latgrad_sumsq).  k = 1: the latency-bound ARM
// fills what the chain's kernels leave of each CU (8-frame 512x768 step 1.112 / 1.117 ->
// 1.049 / 1.050 ms; k = 2: 1.067 / 1.072, k = 3: 1.084 / 1.076; profiles/r4ah_*).  With the
// full resident grid (round 4, earlier) it took every CU's LDS and the chain queued behind it.
#ifndef CCMI_ARM_OVERLAP
#define CCMI_ARM_OVERLAP 1
#endif
// the compile-time default, or the environment's CCMI_ARM_OVERLAP (0 .. 3) read once per process
// (0 runs the ARM in line: kernel traces where every kernel runs alone)
static int arm_overlap()
{
    static const int v = [] {
        const char *e = getenv("CCMI_ARM_OVERLAP");
        if (e && e[0] >= '0' && e[0] <= '3' && !e[1]) return e[0] - '0';
        return (int)CCMI_ARM_OVERLAP;
    }();
    return v;
}
struct Plan {
    Geo g;
    ArmTiles at;
    int B, nblk_arm;
    // workspace offsets (bytes)
    size_t gq_arm = 0; // the ARM's latent gradients when it runs on the side stream (CCMI_ARM_OVERLAP)
    size_t yq, dq, gq, kf, stacks, stacks_bytes, dense, z[kMaxSp + 1], graw, gbuf[2], gdense, gstack, tmpU, tmpG, G,
        acc4, bc, rslots, mslots, slots, total;
    int64_t gstack_off[CCMI_MAX_GRIDS]; // per level k (1..L-2) inside gstack, elements per frame
    int64_t gstack_per, stack_per, tmp_per;
};

int make_plan(const ccmi_train_args *a, Plan &pl)
{
    Geo &g = pl.g;
    g = Geo{};
    const int L = a->n_grids;
    if (a->batch < 1) return ccmi_set_error(CCMI_ERR_ARG, "train: batch must be >= 1");
    if (L < 2 || L > CCMI_MAX_GRIDS) return ccmi_set_error(CCMI_ERR_ARG, "train: n_grids %d", L);
    g.L = L;
    int off = 0;
    for (int l = 0; l < L; ++l) {
        g.h[l] = a->h[l];
        g.w[l] = a->w[l];
        if (g.h[l] < 1 || g.w[l] < 1) return ccmi_set_error(CCMI_ERR_ARG, "train: grid %d is %dx%d", l, g.h[l], g.w[l]);
        if (l > 0 && (g.h[l] != (g.h[l - 1] + 1) / 2 || g.w[l] != (g.w[l - 1] + 1) / 2))
            return ccmi_set_error(CCMI_ERR_ARG, "train: grid %d is not ceil(half) of grid %d", l, l - 1);
        g.off[l] = off;
        off += g.h[l] * g.w[l];
    }
    g.N = off;
    g.H = g.h[0];
    g.W = g.w[0];
    if (a->latent_stride < g.N) return ccmi_set_error(CCMI_ERR_ARG, "train: latent_stride < %d", g.N);
    g.d = a->dim_arm;
    g.nh = a->n_hidden;
    if ((g.d != 8 && g.d != 16 && g.d != 24 && g.d != 32) || g.nh < 0 || g.nh > 3)
        return ccmi_set_error(CCMI_ERR_UNSUPPORTED, "train: ARM dim %d with %d hidden layers", g.d, g.nh);
    g.P_arm = g.nh * (g.d * g.d + g.d) + 2 * g.d + 2;
    g.K = a->ups_k;
    g.n_ups = a->n_ups;
    g.Kp = a->pre_k;
    g.n_pre = a->n_pre;
    if ((g.K != 4 && g.K != 6 && g.K != 8) || (g.Kp != 1 && g.Kp != 3 && g.Kp != 5 && g.Kp != 7 && g.Kp != 9) ||
        g.n_ups < 1 || g.n_pre < 1)
        return ccmi_set_error(CCMI_ERR_UNSUPPORTED, "train: upsampling kernels %d / %d", g.K, g.Kp);
    g.hu = (g.K + 1) / 2;
    g.hp = (g.Kp + 1) / 2;
    g.up_off = g.P_arm;
    g.pre_off = g.up_off + g.n_ups * g.hu;
    g.syn_off = g.pre_off + g.n_pre * g.hp;
    g.kfull = g.n_ups * g.K + g.n_pre * g.Kp;
    // synthesis: 1x1 (C -> hid) + 1x1 (hid -> 3), then <= 3 3x3 layers 3 -> 3
    const int ns = a->n_syn_layers;
    if (ns < 2 || ns > 2 + kMaxSp) return ccmi_set_error(CCMI_ERR_UNSUPPORTED, "train: %d synthesis layers", ns);
    const ccmi_syn_layer *S = a->syn;
    if (S[0].ks != 1 || S[1].ks != 1 || S[0].residual || S[1].residual || S[1].n_out != 3 || S[0].n_out < 1 ||
        S[0].n_out > 64)
        return ccmi_set_error(CCMI_ERR_UNSUPPORTED, "train: synthesis head must be 1x1 (C -> <=64) then 1x1 (-> 3)");
    g.hid = S[0].n_out;
    g.r0 = S[0].relu;
    g.r1 = S[1].relu;
    int p = g.syn_off;
    g.w0 = p;
    p += g.hid * L;
    g.b0 = p;
    p += g.hid;
    g.w1 = p;
    p += 3 * g.hid;
    g.b1 = p;
    p += 3;
    g.P_head = p - g.syn_off;
    g.n_sp = ns - 2;
    for (int i = 0; i < g.n_sp; ++i) {
        const ccmi_syn_layer &l = S[2 + i];
        if (l.ks != 3 || l.n_out != 3) return ccmi_set_error(CCMI_ERR_UNSUPPORTED, "train: layer %d must be 3x3, 3 -> 3", 2 + i);
        g.sp_w[i] = p;
        p += 81;
        g.sp_b[i] = p;
        p += 3;
        g.sp_res[i] = l.residual;
        g.sp_relu[i] = l.relu;
    }
    g.P = p;
    if (a->param_stride < g.P) return ccmi_set_error(CCMI_ERR_ARG, "train: param_stride < %d", g.P);

    pl.B = a->batch;
    ArmTiles &at = pl.at;
    at = ArmTiles{};
    at.n = L;
    int tiles = 0;
    for (int l = 0; l < L; ++l) {
        at.tiles_x[l] = ccmi_div_up(g.w[l], kATX);
        at.start[l] = tiles;
        tiles += at.tiles_x[l] * ccmi_div_up(g.h[l], kATY);
    }
    at.start[L] = tiles;
    pl.nblk_arm = tiles;
    const int64_t npx = (int64_t)g.H * g.W;

    // buffers
    const size_t B = (size_t)pl.B;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t r = o; o += align256(bytes); return r; };
    pl.yq = take(4 * B * g.N);
    pl.dq = take(4 * B * g.N);
    pl.gq = take(4 * B * g.N);
    pl.kf = take(4 * B * g.kfull);
    pl.stack_per = 0;
    for (int k = 1; k <= L - 2; ++k) pl.stack_per += (int64_t)(L - k) * g.h[k] * g.w[k];
    pl.stacks_bytes = 4 * B * (size_t)pl.stack_per;
    pl.stacks = take(pl.stacks_bytes + 4);
    pl.dense = take(4 * B * L * npx);
    for (int i = 0; i <= g.n_sp; ++i) pl.z[i] = take(4 * B * 3 * npx);
    pl.graw = take(4 * B * 3 * npx);
    pl.gbuf[0] = take(4 * B * 3 * npx);
    pl.gbuf[1] = take(4 * B * 3 * npx);
    pl.gdense = take(4 * B * L * npx);
    pl.gstack_per = pl.stack_per;
    {
        int64_t so = 0;
        for (int k = 1; k <= L - 2; ++k) {
            pl.gstack_off[k] = so;
            so += (int64_t)(L - k) * g.h[k] * g.w[k];
        }
    }
    pl.gstack = take(4 * B * pl.gstack_per + 4);
    int64_t tmax = 0;
    for (int k = 1; k <= L - 1; ++k) {
        tmax = std::max(tmax, (int64_t)(L - k) * g.h[k] * g.w[k - 1]); // upsample temps: C x hs x wd
        tmax = std::max(tmax, (int64_t)g.h[k - 1] * g.w[k - 1]);       // refine temps: hd x wd
    }
    pl.tmp_per = tmax;
    pl.tmpU = take(4 * B * tmax);
    pl.tmpG = take(4 * B * tmax);
    pl.G = take(4 * B * ((size_t)g.N + g.P));
    pl.acc4 = take(4 * B * 4);
    pl.bc = take(4 * B * 2);
    pl.rslots = take(4 * B * kDwSlots);
    pl.mslots = take(4 * B * kDwSlots); // the fused loss's squared-error sums
    // every parameter's gradient through kDwSlots slot rows per frame (one row per workgroup
    // residue), folded into the gradient row by t_dw_fold (kDwSlots)
    pl.slots = take(4 * B * kDwSlots * (size_t)g.P);
    if (arm_overlap()) pl.gq_arm = take(4 * B * g.N); // after acc4: zeroed with it
    pl.total = o;
    return CCMI_OK;
}

// The plan's buffers as pointers into the caller's workspace
Work resolve(const Plan &pl, void *workspace)
{
    auto F = [&](size_t off) { return reinterpret_cast<float *>(static_cast<uint8_t *>(workspace) + off); };
    Work w{};
    w.yq = F(pl.yq), w.dq = F(pl.dq), w.gq = F(pl.gq), w.kf = F(pl.kf), w.stacks = F(pl.stacks), w.dense = F(pl.dense);
    for (int i = 0; i <= pl.g.n_sp; ++i) w.z[i] = F(pl.z[i]);
    w.graw = F(pl.graw), w.gbuf[0] = F(pl.gbuf[0]), w.gbuf[1] = F(pl.gbuf[1]), w.gdense = F(pl.gdense);
    w.gstack = F(pl.gstack), w.tmpU = F(pl.tmpU), w.tmpG = F(pl.tmpG), w.acc4 = F(pl.acc4);
    w.rslots = F(pl.rslots), w.mslots = F(pl.mslots), w.slots = F(pl.slots);
    w.G = F(pl.G), w.bc = F(pl.bc), w.gq_arm = F(pl.gq_arm);
    for (int k = 1; k <= pl.g.L - 2; ++k) w.gstack_off[k] = pl.gstack_off[k];
    w.gstack_per = pl.gstack_per, w.tmp_per = pl.tmp_per;
    return w;
}

// The upsampling forward on the quantised latents: fwd_ups.hip's level kernels with the expanded
// kernels kf as parameters, keeping every pyramid stack for the backward
int ups_forward(const Plan &pl, const Work &w, hipStream_t s)
{
    const Geo &g = pl.g;
    ccmi_ups_args u{};
    u.latent = w.yq;
    u.latent_stride = g.N;
    u.n_grids = g.L;
    for (int l = 0; l < g.L; ++l) {
        u.h[l] = g.h[l];
        u.w[l] = g.w[l];
    }
    u.gain = 1.f;
    u.quantize = 0;
    u.ups_k = g.K;
    u.n_ups = g.n_ups;
    u.pre_k = g.Kp;
    u.n_pre = g.n_pre;
    u.params = w.kf;
    u.param_stride = g.kfull;
    u.out = w.dense;
    u.out_stride = (int64_t)g.L * g.H * g.W;
    u.workspace = w.stacks;
    u.workspace_bytes = pl.stacks_bytes + 4;
    u.batch = pl.B;
    return ccmi_launch_ups_f32(&u, s);
}

// Workgroups of `fn` that fit on the device at once (occupancy x CUs): the grid of the
// persistent (grid-stride) training kernels is ONE resident round.  A second round only adds
// workgroups, and each workgroup's flush costs one atomic per value on addresses every
// workgroup of the frame shares (t_arm16: 227 us with one round of 1024 workgroups, 232 us
// with 2048, after the flush reduction; before it 293 vs 460 us, profiles/r4l_*, r4m_*).
static int resident_wgs(const void *fn, int threads, size_t lds, int max_per_cu)
{
    static std::mutex mu;
    static std::map<std::tuple<const void *, size_t, int, int>, int> cache;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    std::lock_guard<std::mutex> lk(mu);
    const auto key = std::make_tuple(fn, lds, dev, max_per_cu);
    auto it = cache.find(key);
    if (it != cache.end()) return it->second;
    int cus = 0, per = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) cus = 256;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, fn, threads, lds) != hipSuccess || per < 1) per = 1;
    return cache[key] = std::min(per, max_per_cu) * cus;
}

} // namespace

dim3 ccmi_train::resident_grid(const void *fn, int threads, size_t lds, int64_t units, int B, int max_per_cu)
{
    const int64_t per_frame = std::max<int64_t>(1, resident_wgs(fn, threads, lds, max_per_cu) / B);
    return dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>(units, per_frame)), (unsigned)B);
}

extern "C" int ccmi_quantize_f32(const float *x, int64_t n, int quantizer, float temperature, const float *noise,
                                 float *y, float *dy, void *stream)
{
    if (!x || !y || n < 0) return ccmi_set_error(CCMI_ERR_ARG, "quantize: null argument");
    if (n > INT32_MAX - kT) return ccmi_set_error(CCMI_ERR_ARG, "quantize: n > 2^31 - %d", kT); // int thread indices
    if (quantizer < CCMI_Q_NONE || quantizer > CCMI_Q_TRUE_STE) return ccmi_set_error(CCMI_ERR_ARG, "quantize: type %d", quantizer);
    if ((quantizer == CCMI_Q_SOFTROUND || quantizer == CCMI_Q_SOFTROUND_ALONE || quantizer == CCMI_Q_STE) &&
        !(temperature > 0.f))
        return ccmi_set_error(CCMI_ERR_ARG, "quantize: soft-round temperature must be > 0");
    if (n == 0) return CCMI_OK;
    // noise comes as a tensor (or none): the counter-based generator is not used here
    hipLaunchKernelGGL(t_quant, grid1(n, 1), dim3(kT), 0, static_cast<hipStream_t>(stream), x, (int64_t)n, (int)n, 1.f,
                       quantizer, (int)CCMI_NOISE_NONE, quant_args(temperature, 1.f), (uint64_t)0, 0, noise, y, dy,
                       (float *)nullptr);
    CCMI_HIP_CHECK(hipGetLastError());
    return CCMI_OK;
}

extern "C" size_t ccmi_train_param_count(const ccmi_train_args *a)
{
    if (!a) return 0;
    ccmi_train_args t = *a;
    t.latent_stride = 1 << 30;
    t.param_stride = 1 << 30;
    t.batch = 1;
    Plan pl;
    if (make_plan(&t, pl)) return 0;
    return (size_t)pl.g.P;
}

// The MS-SSIM stage of ccmi_train_step_dist: the step's raw output [B][3][H][W] as the planes of
// ccmi_msssim_args (4:2:0: chroma at even rows and columns, as t_loss), the target as Y.  x, grad, out
// and the workspace are left to the caller; grad is set to a non-null placeholder so that the
// workspace counts the gradient's part.
static ccmi_msssim_args dist_args(const ccmi_train_args *a, const ccmi_train_dist *d, int H, int W)
{
    ccmi_msssim_args m{};
    const int64_t npx = (int64_t)H * W;
    m.batch = a->batch;
    m.n_planes = 3;
    m.n_scales = d->n_scales;
    m.clamp = 1;
    for (int p = 0; p < 3; ++p) {
        const int sub = a->yuv420 && p > 0 ? 2 : 1;
        m.h[p] = H / sub;
        m.w[p] = W / sub;
        m.x_off[p] = p * npx;
        m.x_pitch[p] = W;
        m.x_sub[p] = sub;
        m.channel_weights[p] = d->channel_weights[p];
    }
    m.x_stride = 3 * npx;
    m.y = a->target;
    m.y_stride = a->target_stride;
    for (int s = 0; s < 5; ++s) m.weights[s] = d->weights[s];
    m.alpha_mse = d->alpha_mse;
    m.beta_ms = d->beta_ms;
    return m;
}

extern "C" size_t ccmi_train_workspace_bytes_dist(const ccmi_train_args *a, const ccmi_train_dist *d)
{
    if (!a) return 0;
    Plan pl;
    if (make_plan(a, pl)) return 0;
    if (!d) return pl.total;
    ccmi_msssim_args m = dist_args(a, d, pl.g.H, pl.g.W);
    float one;
    m.grad = &one; // counted, never written
    const size_t n = ccmi_msssim_workspace_bytes(&m);
    if (!n) return 0;
    // after the step's own plan: the stage's [B][4] row, then its workspace
    return align256(pl.total) + align256(sizeof(float) * 4 * (size_t)a->batch) + n;
}

extern "C" size_t ccmi_train_workspace_bytes(const ccmi_train_args *a) { return ccmi_train_workspace_bytes_dist(a, nullptr); }

// The ARM's side stream (CCMI_ARM_OVERLAP): leased from the process-wide pool for one call
// (ccmi_api.cpp; st[0], events ev[0] fork and ev[1] join).  SideJoin orders the side stream
// back into the caller's stream on EVERY exit after the fork: the explicit waits (forward-only
// return, before t_latgrad_sumsq) and, through its destructor, every error return in between,
// so no ARM kernel can still be writing gq_arm / acc4 / Gth / rate_out once the call returned.
struct SideJoin {
    hipStream_t s = nullptr, side = nullptr;
    hipEvent_t ev = nullptr;
    bool recorded = false, pending = false;
    void record()
    {
        if (pending && !recorded) recorded = hipEventRecord(ev, side) == hipSuccess;
    }
    hipError_t wait()
    {
        if (!pending) return hipSuccess;
        record();
        pending = false;
        return recorded ? hipStreamWaitEvent(s, ev, 0) : hipStreamSynchronize(side);
    }
    ~SideJoin() { (void)wait(); }
};

#if defined(CCMI_DIAG_SIDE_SPIN)
// Diagnostic build only (make spin): ~5 ms of spinning queued on the side stream before the
// ARM, so a consumer that reads the ARM's outputs without the join sees stale data every time.
__global__ void t_diag_spin(uint64_t ticks)
{
    const uint64_t t0 = __builtin_amdgcn_s_memrealtime(); // 100 MHz constant clock
    while (__builtin_amdgcn_s_memrealtime() - t0 < ticks) __builtin_amdgcn_s_sleep(8);
}
#endif

extern "C" int ccmi_train_step(const ccmi_train_args *a, void *stream) { return ccmi_train_step_dist(a, nullptr, stream); }

extern "C" int ccmi_train_step_dist(const ccmi_train_args *a, const ccmi_train_dist *d, void *stream)
{
    if (!a || !a->latent || !a->params || !a->target) return ccmi_set_error(CCMI_ERR_ARG, "train: null argument");
    Plan pl;
    if (int rc = make_plan(a, pl)) return rc;
    size_t need = pl.total;
    ccmi_msssim_args ms{};
    float *dist4 = nullptr; // the MS-SSIM stage's [B][4] row (finish_row reads D and MSE from it)
    if (d) {
        if (a->grad_raw) return ccmi_set_error(CCMI_ERR_ARG, "train: a distortion and grad_raw are exclusive");
        if (a->target_stride <= 0) return ccmi_set_error(CCMI_ERR_ARG, "train: a distortion needs a target per frame");
        need = ccmi_train_workspace_bytes_dist(a, d);
        if (!need) return CCMI_ERR_ARG; // the message is ccmi_msssim's
    }
    if (!a->workspace || a->workspace_bytes < need)
        return ccmi_set_error(CCMI_ERR_ARG, "train: workspace of %zu bytes needed", need);
    if (d) {
        uint8_t *w8 = static_cast<uint8_t *>(a->workspace) + align256(pl.total);
        ms = dist_args(a, d, pl.g.H, pl.g.W);
        dist4 = d->dist_out ? d->dist_out : reinterpret_cast<float *>(w8);
        ms.out = dist4;
        ms.x = reinterpret_cast<float *>(static_cast<uint8_t *>(a->workspace) + pl.z[pl.g.n_sp]);
        ms.workspace = w8 + align256(sizeof(float) * 4 * (size_t)a->batch);
        ms.workspace_bytes = need - (size_t)(static_cast<uint8_t *>(ms.workspace) - static_cast<uint8_t *>(a->workspace));
        ms.grad = a->forward_only ? nullptr : reinterpret_cast<float *>(static_cast<uint8_t *>(a->workspace) + pl.graw);
        if (int rc = ccmi_msssim_check(&ms)) return rc;
    }
    if (a->update && (!a->adam_m || !a->adam_v || (a->step < 1 && !a->adam_steps)))
        return ccmi_set_error(CCMI_ERR_ARG, "train: Adam state and step >= 1 needed to update");
    if ((a->quantizer == CCMI_Q_SOFTROUND || a->quantizer == CCMI_Q_SOFTROUND_ALONE || a->quantizer == CCMI_Q_STE) &&
        !(a->temperature > 0.f))
        return ccmi_set_error(CCMI_ERR_ARG, "train: soft-round temperature must be > 0");
    if (a->noise == CCMI_NOISE_KUMARASWAMY && !(a->noise_param > 0.f))
        return ccmi_set_error(CCMI_ERR_ARG, "train: kumaraswamy parameter must be > 0");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const Geo &g = pl.g;
    const int B = pl.B;
    const Work w = resolve(pl, a->workspace);
    const int64_t GS = (int64_t)g.N + g.P; // gradient row per frame: latents then parameters
    float *G = a->grad_out ? a->grad_out : w.G;
    const int64_t npx = (int64_t)g.H * g.W;
    const float lam_px = a->lmbda / (float)npx, inv_total = 1.f / loss_samples(g, a->yuv420);
    const dim3 per_frame((unsigned)ccmi_div_up(B, 64)); // t_finish, t_adam_bc: one thread per frame, blocks of 64

    {
        // acc4 .. the end of the workspace plan (rate and parameter-gradient slots, the ARM's side
        // gradient) zeroed and the symmetric kernels expanded, in one launch; the gradient rows
        // need no zeroing: t_latgrad_sumsq writes their latent part and t_dw_fold their parameters
        const int64_t nz = (int64_t)(pl.total - pl.acc4) / (int64_t)sizeof(float);
        const int64_t n = nz + (int64_t)B * g.kfull;
        const unsigned nb = (unsigned)std::max<int64_t>(1, std::min<int64_t>(ccmi_div_up(n, 4 * kT), 2048));
        hipLaunchKernelGGL(t_prologue, dim3(nb), dim3(kT), 0, s, w.acc4, nz, a->params, a->param_stride, g, w.kf, B,
                           a->update ? a->step_counters : nullptr);
    }

    // ---- forward
    hipLaunchKernelGGL(t_quant, grid1(g.N, B), dim3(kT), 0, s, a->latent, a->latent_stride, g.N, a->gain, a->quantizer,
                       a->noise, quant_args(a->temperature, a->noise_param), (uint64_t)a->seed, a->step, a->noise_in, w.yq,
                       w.dq, w.gq);
    StreamSetLease lease; // declared before the join: released after it
    SideJoin join;
    bool side = false;
    {
        // the ARM in line or, with CCMI_ARM_OVERLAP, on the side stream with at most that many
        // workgroups per CU and its latent gradients in a buffer of their own
        hipStream_t sa = s;
        float *gqa = w.gq;
        int cap = 1 << 20;
        if (arm_overlap() > 0) {
            lease.set = ccmi_streamset_acquire(1, 2, false);
            if (!lease.set) return CCMI_ERR_HIP;
            CCMI_HIP_CHECK(hipEventRecord(lease.set->ev[0], s));
            CCMI_HIP_CHECK(hipStreamWaitEvent(lease.set->st[0], lease.set->ev[0], 0));
            side = true;
            sa = lease.set->st[0];
            join.s = s;
            join.side = sa;
            join.ev = lease.set->ev[1];
            join.pending = true; // from here on every return joins
            gqa = w.gq_arm;
            cap = arm_overlap();
#if defined(CCMI_DIAG_SIDE_SPIN)
            hipLaunchKernelGGL(t_diag_spin, dim3(1), dim3(64), 0, sa, (uint64_t)500000);
#endif
        }
        launch_arm(g, pl.at, *a, w, lam_px, gqa, cap, sa);
        CCMI_HIP_CHECK(hipGetLastError());
        join.record();
    }
    if (int rc = ups_forward(pl, w, s)) return rc; // joined by ~SideJoin
    launch_head_fwd(g, *a, w, s);
    // the training step's MSE fused into the last 3x3 layer
    const bool fuse_loss = !d && !a->forward_only && !a->grad_raw && g.n_sp > 0;
    for (int i = 0; i < g.n_sp; ++i) launch_sp_fwd(g, *a, w, i, fuse_loss && i == g.n_sp - 1, s);
    if (a->raw_out)
        CCMI_HIP_CHECK(hipMemcpyAsync(a->raw_out, w.z[g.n_sp], sizeof(float) * 3 * npx * B, hipMemcpyDeviceToDevice, s));
    if (a->forward_only) {
        // the ARM's rate (rate_out, the rate sums in acc4) comes from the side stream
        CCMI_HIP_CHECK(join.wait());
        if (a->loss_out) {
            // with a real target (target_stride > 0) the loss row holds the built-in MSE too;
            // otherwise (autograd: the loss lives in torch) MSE reads 0 and loss = lmbda-rate
            if (d) {
                if (int rc = ccmi_launch_msssim(&ms, s)) return rc;
            } else if (a->target && a->target_stride > 0)
                launch_loss(g, *a, w, s);
            hipLaunchKernelGGL(t_finish, per_frame, dim3(64), 0, s, w.acc4, w.rslots, w.mslots, inv_total, lam_px, a->loss_out, B, dist4);
        }
        CCMI_HIP_CHECK(hipGetLastError());
        return CCMI_OK;
    }

    // ---- the loss's gradient w.r.t. the raw output
    if (a->grad_raw) // the caller's d loss / d raw output (autograd); no built-in MSE term
        CCMI_HIP_CHECK(hipMemcpyAsync(w.graw, a->grad_raw, sizeof(float) * 3 * npx * B, hipMemcpyDeviceToDevice, s));
    else if (d) {
        // the MS-SSIM stage in t_loss's place: it writes d loss / d raw at the sampled positions; the
        // chroma planes' unsampled ones (4:2:0) are cleared first, every frame's pair in one memset
        if (a->yuv420)
            CCMI_HIP_CHECK(hipMemset2DAsync(w.graw + npx, sizeof(float) * 3 * npx, 0, sizeof(float) * 2 * npx, (size_t)B, s));
        if (int rc = ccmi_launch_msssim(&ms, s)) return rc;
    } else if (!fuse_loss)
        launch_loss(g, *a, w, s);

    // ---- backward: 3x3 layers, head, pyramid (finest level first)
    const float *gcur = w.graw;
    for (int i = g.n_sp - 1; i >= 0; --i) {
        launch_sp_bwd(g, *a, w, i, gcur, w.gbuf[i & 1], s);
        gcur = w.gbuf[i & 1];
    }
    launch_head_bwd(g, *a, w, gcur, s);
    for (int step = g.L - 2; step >= 0; --step) launch_ups_bwd_step(g, w, B, step, s);
    CCMI_HIP_CHECK(hipGetLastError());

    // ---- join, fold, latent gradients, norm, Adam
    CCMI_HIP_CHECK(join.wait());
    // every parameter gradient (the ARM's from the side stream too) from its slot rows
    hipLaunchKernelGGL(t_dw_fold, dim3((unsigned)ccmi_div_up(g.P, 64), B), dim3(64), 0, s, w.slots, g.P, G + g.N, GS, 0);
    hipLaunchKernelGGL(t_latgrad_sumsq, dim3(sum_blocks(GS, 4), B), dim3(kT), 0, s, w.gq, side ? w.gq_arm : nullptr, w.dq, g.N,
                       G, GS, GS, w.acc4);
    if (a->loss_out && !a->update)
        hipLaunchKernelGGL(t_finish, per_frame, dim3(64), 0, s, w.acc4, w.rslots, w.mslots, inv_total, lam_px, a->loss_out, B, dist4);
    if (a->update) {
        const double bc1 = 1.0 - std::pow((double)a->beta1, a->step), bc2 = 1.0 - std::pow((double)a->beta2, a->step);
        AdamArgs A{(float)(a->lr / bc1), (float)(1.0 / std::sqrt(bc2)), a->beta1, a->beta2, a->eps, a->clip, g.N,
                   a->update == 2 ? 1 : 0, GS, GS,
                   a->latent_stride, a->param_stride, (int64_t)a->latent_stride + a->param_stride, nullptr,
                   a->loss_out, w.rslots, w.mslots, inv_total, lam_px, dist4};
        if (a->adam_steps) {
            A.bc = w.bc;
            hipLaunchKernelGGL(t_adam_bc, per_frame, dim3(64), 0, s, a->adam_steps, (double)a->lr, (double)a->beta1,
                               (double)a->beta2, B, w.bc);
        }
        hipLaunchKernelGGL(t_adam, grid1(GS, B), dim3(kT), 0, s, G, a->latent, a->params, a->adam_m, a->adam_v, w.acc4, A);
    }
    CCMI_HIP_CHECK(hipGetLastError());
    return CCMI_OK;
}
