// train_internal.h -- what the units of the encoder overfit step share (train.hip: the driver, the
// plan, the quantiser and Adam; train_arm.hip, train_head.hip, train_sp.hip, train_ups.hip: one
// stage each): the frame geometry, the workspace pointers, the launch constants, the device
// helpers with more than one user, and the stage launchers the driver calls.  Each unit keeps
// its kernels in an anonymous namespace of its own.
#pragma once

#include <algorithm>

#include "ccmi_internal.h"

namespace ccmi_train {

constexpr int kT = 256;
constexpr int kMaxSp = 3;
constexpr int kHeadT = 128;
// Parameter gradients: every workgroup that reduces weight / bias gradients (the ARM, the head,
// the 3x3 layers, the upsampling kernels) adds its partial sums into one of kDwSlots copies of
// the frame's parameter-gradient row (slot = workgroup % kDwSlots), and t_dw_fold sums the
// slots into the gradient row once per step: same-address atomics serialise (≈80 ns each), and
// the persistent kernels' workgroups all flush at once at their end.  The ARM's rate sums take
// the same form (kDwSlots per frame).
constexpr int kDwSlots = 32;

// Per-frame geometry and parameter offsets (same for every frame of a batch).
struct Geo {
    int L, N, H, W;
    int h[CCMI_MAX_GRIDS], w[CCMI_MAX_GRIDS], off[CCMI_MAX_GRIDS];
    int d, nh, P_arm;
    int K, n_ups, hu, up_off;
    int Kp, n_pre, hp, pre_off;
    int syn_off, hid, r0, r1, w0, b0, w1, b1, P_head;
    int n_sp, sp_w[kMaxSp], sp_b[kMaxSp], sp_res[kMaxSp], sp_relu[kMaxSp];
    int P, kfull;
};

// The ARM's latent tile (kATX x kATY, causal halo kAH) and the tiles of every level in one list
constexpr int kATX = 64, kATY = 4, kAH = 4;
constexpr int kALW = kATX + 2 * kAH, kALH = kATY + kAH;

struct ArmTiles {
    int n, tiles_x[CCMI_MAX_GRIDS], start[CCMI_MAX_GRIDS + 1];
};

typedef float v4f __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// Sum over the wave, in every lane, without an LDS round trip: DPP within the 16-lane rows
// (xor 1, xor 2, half-row mirror, row mirror), then gfx950's permlane16 / permlane32 swaps
// across them.  (The __shfl_xor butterfly is six ds_bpermute_b32 in a dependent chain.)
template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}
__device__ __forceinline__ float wave_sum(float v)
{
    v += dpp_mov<0xb1>(v);  // quad_perm [1, 0, 3, 2]: lane ^ 1
    v += dpp_mov<0x4e>(v);  // quad_perm [2, 3, 0, 1]: lane ^ 2
    v += dpp_mov<0x141>(v); // row_half_mirror: the other quad of the half-row
    v += dpp_mov<0x140>(v); // row_mirror: the other half of the row
    const auto h = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    v = __uint_as_float(h[0]) + __uint_as_float(h[1]);
    const auto q = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return __uint_as_float(q[0]) + __uint_as_float(q[1]);
}

__device__ __forceinline__ float block_sum(float v, float *red)
{
    v = wave_sum(v);
    const int wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[wid] = v;
    __syncthreads();
    float s = 0.f;
    for (int i = 0; i < nw; ++i) s += red[i];
    return s;
}

// v_mfma_f32_16x16x4_f32 (f32 in, f32 accumulate: an fmaf chain in another order).
// Lane l supplies A[m = l & 15][k = l >> 4] and B[k = l >> 4][n = l & 15]; accumulator
// register r of lane l is D[m = 4 (l >> 4) + r][n = l & 15].
__device__ __forceinline__ v4f mfma4(float a, float b, v4f c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
// v_mfma_f32_4x4x1_16b_f32: sixteen independent 4x4 outer products, block bk = l >> 2.  Lane l
// supplies A[bk][m = l & 3] and B[bk][n = l & 3]; accumulator register r of lane l is
// D[bk][m = r][n = l & 3].  2 passes (8 cycles) against 16x16x4's 8 (32 cycles) at a quarter
// of the MACs -- the same MAC rate, so a product whose M or N is 3-8 wide wastes less of it.
__device__ __forceinline__ v4f mfma4x4(float a, float b, v4f c) { return __builtin_amdgcn_mfma_f32_4x4x1f32(a, b, c, 0, 0, 0); }

// Orders a wave's LDS stores before its own later LDS loads of other lanes' rows: a wave's
// LDS instructions execute in order, so only the compiler must not move them across.
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ------------------------------------------------------------------ host side
// The step's workspace buffers, resolved once per call from the plan's byte offsets (make_plan)
struct Work {
    float *yq, *dq, *gq, *kf, *stacks, *dense, *z[kMaxSp + 1], *graw, *gbuf[2], *gdense, *gstack, *tmpU, *tmpG, *G, *acc4, *bc;
    float *gq_arm; // the ARM's latent gradients when it runs on the side stream
    // the rate and squared-error slots ([B][kDwSlots]) and the parameter gradients' slot rows
    // ([B][kDwSlots][P], see kDwSlots)
    float *rslots, *mslots, *slots;
    int64_t gstack_off[CCMI_MAX_GRIDS]; // per level k (1..L-2) inside gstack, elements per frame
    int64_t gstack_per, tmp_per;
};

inline size_t align256(size_t v) { return (v + 255) / 256 * 256; }
inline dim3 grid1(int64_t n, int B) { return dim3((unsigned)((n + kT - 1) / kT), (unsigned)B); }
// kernel-gradient reductions spread over kDwSlots addresses: one item per thread (the
// loops are latency-bound -- their inputs were just written by other XCDs, so every load
// goes past the local L2 -- and a thread's items run one after another)
inline unsigned dw_blocks(int64_t n, int per_thread = 1)
{
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + per_thread * kT - 1) / (per_thread * kT), 4096));
}

// workgroups per frame of the per-frame sum reductions (t_loss, t_latgrad_sumsq): each
// workgroup ends in ONE atomic on the frame's accumulator, and same-address atomics serialise
// at ≈80 ns each (256 -> 384 workgroups per frame took t_loss from 29 to 35 us and 256 -> 512
// t_latgrad_sumsq from 29 to 53 us, profiles/r5m_*), so a frame gets at most kSumWGs
// workgroups, each with several batched iterations
constexpr int kSumWGs = 128;
inline unsigned sum_blocks(int64_t n, int per_iter)
{
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>(kSumWGs, (n + (int64_t)kT * per_iter - 1) / ((int64_t)kT * per_iter)));
}

// samples the frame's MSE averages over: three planes, or luma and two half-size chroma planes
inline float loss_samples(const Geo &g, int yuv420)
{
    const int64_t npx = (int64_t)g.H * g.W;
    return yuv420 ? (float)(npx + 2 * (int64_t)(g.H / 2) * (g.W / 2)) : (float)(3 * npx);
}

// grid of a persistent kernel over `units` work units per frame, B frames: one resident round of
// workgroups (train.hip, which keeps the occupancy cache).  The launcher that sizes a grid with
// it lives in the unit that defines the kernel.
dim3 resident_grid(const void *fn, int threads, size_t lds, int64_t units, int B, int max_per_cu = 1 << 20);

// The stage launchers, in the step's order; each owns its ladders from run-time values to
// template arguments.  They enqueue on s and report nothing: the driver checks hipGetLastError.
// train_arm.hip: forward + rate + backward, latent gradients into gq, at most cap workgroups per CU
void launch_arm(const Geo &g, const ArmTiles &at, const ccmi_train_args &a, const Work &w, float lam_px, float *gq, int cap,
                hipStream_t s);
// train_head.hip: w.dense -> w.z[0]; gz0 (the gradient of z[0]) -> w.gdense
void launch_head_fwd(const Geo &g, const ccmi_train_args &a, const Work &w, hipStream_t s);
void launch_head_bwd(const Geo &g, const ccmi_train_args &a, const Work &w, const float *gz0, hipStream_t s);
// train_sp.hip: 3x3 layer i, w.z[i] -> w.z[i + 1] (fused_loss: the MSE and w.graw with it); the
// MSE of w.z[n_sp] on its own; layer i's backward, gout -> gin
void launch_sp_fwd(const Geo &g, const ccmi_train_args &a, const Work &w, int i, bool fused_loss, hipStream_t s);
void launch_loss(const Geo &g, const ccmi_train_args &a, const Work &w, hipStream_t s);
void launch_sp_bwd(const Geo &g, const ccmi_train_args &a, const Work &w, int i, const float *gout, float *gin, hipStream_t s);
// train_ups.hip: pyramid step `step` (source level L - 1 - step) of the upsampling backward
void launch_ups_bwd_step(const Geo &g, const Work &w, int B, int step, hipStream_t s);

} // namespace ccmi_train
