// fwd_common.h -- path A pieces shared by the per-stage kernels (fwd_ups.hip,
// fwd_syn.hip) and the fused decode kernel (fwd_fused.hip).  Internal.
#pragma once

#include <type_traits>

#include "ccmi_internal.h"

namespace ccmi_fwd {

typedef float f2 __attribute__((ext_vector_type(2)));
// Weights are read through a constant-address-space pointer: the loads are wave-uniform
// and the buffer is never written by the kernel, so they become scalar (SMEM) loads even
// after the kernel's own global stores (which would otherwise force vector loads).
typedef const __attribute__((address_space(4))) float *cfloat_ptr;

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// XCD-aware workgroup order for a 1-D grid of n workgroups: the dispatcher deals workgroups
// round-robin over the 8 XCDs (block i and i + 8 share one, MI355X_MICROARCH.md "Workgroup
// dispatch"), so block i is given work item xcd_order(i, n), which hands each XCD a contiguous
// run of items: neighbouring tiles, which re-read each other's halos, then meet in one L2.
// A bijection of [0, n) for any n.
__device__ __forceinline__ int xcd_order(int i, int n)
{
    const int per = (n + 7) >> 3, rem = n & 7, xcd = i & 7;
    return (rem == 0 ? xcd * per : xcd * per - max(0, xcd - rem)) + (i >> 3);
}

// ---------------------------------------------------------------- packed ARM weights
// The pairs form of the path-A ARM (fwd_arm.hip, arm_fwd_pairs_kernel) reads a transposed
// copy of a frame's ARM parameters, so that the weights of two neighbouring output units for
// one input are an aligned pair of one scalar row load.  Per frame, in floats:
//   hidden layer l at l * arm_pack_layer(d): rows i = 0 .. d-1 of arm_pack_row(d) floats,
//     row i = Wt[i][j] = W_l[j][i] for j < d (the d weights that multiply input i), then one
//     row b_l[j];
//   at n_hidden * arm_pack_layer(d): WoT[i][2] = (W_out[0][i], W_out[1][i]), 2 d floats, then
//     b_out[2].
// Every row and the output block start on a 64-byte boundary (a row is padded to 16 floats)
// and the frame stride arm_pack_stride() is a multiple of 16 floats; padding is written as 0.
constexpr int arm_pack_row(int d) { return (d + 15) & ~15; }
constexpr int arm_pack_layer(int d) { return (d + 1) * arm_pack_row(d); }
constexpr int arm_pack_stride(int d, int nh) { return (nh * arm_pack_layer(d) + 2 * d + 2 + 15) & ~15; }
// Index in the public parameter block (ccmi_arm_args.params order) of the value stored at
// position t < arm_pack_stride(d, nh) of the packed block; -1 for padding.
__host__ __device__ constexpr int arm_pack_src(int d, int nh, int t)
{
    const int rs = arm_pack_row(d), ls = arm_pack_layer(d), lp = d * d + d;
    if (t < nh * ls) {
        const int l = t / ls, r = t - l * ls, i = r / rs, j = r - i * rs;
        if (j >= d) return -1;
        return l * lp + (i < d ? j * d + i : d * d + j);
    }
    const int u = t - nh * ls;
    if (u < 2 * d) return nh * lp + (u & 1) * d + (u >> 1);
    return u < 2 * d + 2 ? nh * lp + u : -1;
}

// ---------------------------------------------------------------- head weight records
// The packed FMAs of a 1x1 head that reads its weights from LDS records (the fused kernel's VALU
// head in fwd_syn.hip, the training forward's t_head_fwd in train_head.hip).  A hidden unit's record
// is 16 floats, its fields dense from slot 0: w0[0..CIN), b0, w1[0..CMID), read back as whole
// 128-bit vectors.  Both halves of an FMA are d = fma(w, x, c) with the weight w one half of an
// aligned register pair, selected by op_sel / op_sel_hi, so a weight is used where its
// ds_read_b128 left it (a plain f2(w) splat of the dword in slot 3 or 7 of a dense record is
// copied into a fresh pair first: one v_mov_b32 in ten of the head's vector instructions).
// They are written as few, long statements: the compiler cannot see into a statement, and
// wherever one reads a register that an earlier one wrote with no instruction of its own in
// between, it pads a wait state (s_nop) that the hardware does not need.  Inside a statement
// nothing is padded, and between the statements of a unit stand the next record's reads.
typedef float f4v __attribute__((ext_vector_type(4)));
// the aligned register pair that holds slot S of a record read as N vectors; the slot is its
// half S & 1 (S past the record: pair 0, for operands that are never named)
template <int S, int N>
__device__ __forceinline__ f2 rec_pair(const f4v (&v)[N])
{
    constexpr int s = S < 4 * N ? S : 0;
    return __builtin_shufflevector(v[s / 4], v[s / 4], s & 2, (s & 2) + 1);
}
// the four pairs that hold w0[0..8) of a record, as head_hidden2 takes them
template <int CIN, int N>
__device__ __forceinline__ void rec_w0_pairs(const f4v (&v)[N], f2 (&w)[4])
{
    w[0] = rec_pair<0>(v);
    w[1] = rec_pair<(CIN >= 3 ? 2 : 0)>(v);
    w[2] = rec_pair<(CIN >= 5 ? 4 : 0)>(v);
    w[3] = rec_pair<(CIN >= 7 ? 6 : 0)>(v);
}
// head_hidden2: the hidden chain of one unit on two pixel pairs, per pair as it always was:
// the bias (half CIN & 1 of the pair b), then the CIN products in order, w0[k] being half
// k & 1 of the pair w[k / 2], the last one clamped to [0, 1] with RELU (the scaled ReLU).
// The two pairs' chains alternate.
#define CCMI_HS0(CL)                                                                                      \
    "v_pk_fma_f32 %[a0], %[w0], %[x00], %[b] op_sel:[0,0,%[bh]] op_sel_hi:[0,1,%[bh]]" CL "\n\t"          \
    "v_pk_fma_f32 %[a1], %[w0], %[x10], %[b] op_sel:[0,0,%[bh]] op_sel_hi:[0,1,%[bh]]" CL "\n\t"
#define CCMI_HS(K, P, H, CL)                                                                              \
    "v_pk_fma_f32 %[a0], %[w" #P "], %[x0" #K "], %[a0] op_sel:[" #H ",0,0] op_sel_hi:[" #H ",1,1]" CL "\n\t" \
    "v_pk_fma_f32 %[a1], %[w" #P "], %[x1" #K "], %[a1] op_sel:[" #H ",0,0] op_sel_hi:[" #H ",1,1]" CL "\n\t"
#define CCMI_HPRE1 CCMI_HS0("")
#define CCMI_HPRE2 CCMI_HPRE1 CCMI_HS(1, 0, 1, "")
#define CCMI_HPRE3 CCMI_HPRE2 CCMI_HS(2, 1, 0, "")
#define CCMI_HPRE4 CCMI_HPRE3 CCMI_HS(3, 1, 1, "")
#define CCMI_HPRE5 CCMI_HPRE4 CCMI_HS(4, 2, 0, "")
#define CCMI_HPRE6 CCMI_HPRE5 CCMI_HS(5, 2, 1, "")
#define CCMI_HPRE7 CCMI_HPRE6 CCMI_HS(6, 3, 0, "")
#define CCMI_HCHAIN1(CL) CCMI_HS0(CL)
#define CCMI_HCHAIN2(CL) CCMI_HPRE1 CCMI_HS(1, 0, 1, CL)
#define CCMI_HCHAIN3(CL) CCMI_HPRE2 CCMI_HS(2, 1, 0, CL)
#define CCMI_HCHAIN4(CL) CCMI_HPRE3 CCMI_HS(3, 1, 1, CL)
#define CCMI_HCHAIN5(CL) CCMI_HPRE4 CCMI_HS(4, 2, 0, CL)
#define CCMI_HCHAIN6(CL) CCMI_HPRE5 CCMI_HS(5, 2, 1, CL)
#define CCMI_HCHAIN7(CL) CCMI_HPRE6 CCMI_HS(6, 3, 0, CL)
#define CCMI_HCHAIN8(CL) CCMI_HPRE7 CCMI_HS(7, 3, 1, CL)
template <int CIN, bool RELU>
__device__ __forceinline__ void head_hidden2(const f2 (&w)[4], f2 b, const f2 (&x0)[CIN], const f2 (&x1)[CIN], f2 &a0, f2 &a1)
{
    static_assert(CIN >= 1 && CIN <= 8, "hidden chain length");
    constexpr int L = CIN - 1;
    auto X = [](int k) constexpr { return k < L ? k : L; }; // (operands past the chain's end are not named in its string)
    // the results are early-clobber: the chain writes them while it still has operands to read
#define CCMI_HOPS                                                                                         \
    : [a0] "=&v"(a0), [a1] "=&v"(a1)                                                                      \
    : [w0] "v"(w[0]), [w1] "v"(w[1]), [w2] "v"(w[2]), [w3] "v"(w[3]), [b] "v"(b), [bh] "n"(CIN & 1),      \
      [x00] "v"(x0[0]), [x01] "v"(x0[X(1)]), [x02] "v"(x0[X(2)]), [x03] "v"(x0[X(3)]), [x04] "v"(x0[X(4)]), \
      [x05] "v"(x0[X(5)]), [x06] "v"(x0[X(6)]), [x07] "v"(x0[X(7)]),                                      \
      [x10] "v"(x1[0]), [x11] "v"(x1[X(1)]), [x12] "v"(x1[X(2)]), [x13] "v"(x1[X(3)]), [x14] "v"(x1[X(4)]), \
      [x15] "v"(x1[X(5)]), [x16] "v"(x1[X(6)]), [x17] "v"(x1[X(7)])
#define CCMI_HCASE(N)                                                                                     \
    if constexpr (CIN == N) {                                                                             \
        if constexpr (RELU) asm volatile(CCMI_HCHAIN##N(" clamp") CCMI_HOPS);                             \
        else asm volatile(CCMI_HCHAIN##N("") CCMI_HOPS);                                                  \
    }
    CCMI_HCASE(1) CCMI_HCASE(2) CCMI_HCASE(3) CCMI_HCASE(4) CCMI_HCASE(5) CCMI_HCASE(6) CCMI_HCASE(7) CCMI_HCASE(8)
#undef CCMI_HCASE
#undef CCMI_HOPS
}
#undef CCMI_HCHAIN1
#undef CCMI_HCHAIN2
#undef CCMI_HCHAIN3
#undef CCMI_HCHAIN4
#undef CCMI_HCHAIN5
#undef CCMI_HCHAIN6
#undef CCMI_HCHAIN7
#undef CCMI_HCHAIN8
#undef CCMI_HPRE1
#undef CCMI_HPRE2
#undef CCMI_HPRE3
#undef CCMI_HPRE4
#undef CCMI_HPRE5
#undef CCMI_HPRE6
#undef CCMI_HPRE7
#undef CCMI_HS
#undef CCMI_HS0
// head_out2: one output channel's FMAs of a unit on two pixel pairs, o += w1 h with w1 = half H
// of the pair w
template <int H>
__device__ __forceinline__ void head_out2(f2 w, f2 h0, f2 h1, f2 &o0, f2 &o1)
{
    asm volatile("v_pk_fma_f32 %[o0], %[w], %[h0], %[o0] op_sel:[%[h],0,0] op_sel_hi:[%[h],1,1]\n\t"
                 "v_pk_fma_f32 %[o1], %[w], %[h1], %[o1] op_sel:[%[h],0,0] op_sel_hi:[%[h],1,1]"
                 : [o0] "+v"(o0), [o1] "+v"(o1)
                 : [w] "v"(w), [h0] "v"(h0), [h1] "v"(h1), [h] "n"(H));
}

// f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>), in order
template <int N, class F>
__device__ __forceinline__ void static_for(F &&f)
{
    if constexpr (N > 0) {
        static_for<N - 1>(f);
        f(std::integral_constant<int, N - 1>{});
    }
}

// ---------------------------------------------------------------- synthesis plan
constexpr int kMaxIn = 8;    // fused path: max synthesis input channels
constexpr int kMaxMid = 4;   // fused path: max channels through the 3x3 layers
constexpr int kMaxSp = 3;    // fused path: max number of 3x3 layers
constexpr int kMaxHid = 64;  // fused path: max hidden width of the 1x1 head (presets: <= 48)

struct SpLayer {
    int w_off, b_off; // offsets in the frame's parameter block
    int residual, relu;
};

struct FusedArgs {
    const float *in;
    int64_t in_stride;
    int cin, H, W;
    int n_head;          // 1 or 2 1x1 layers
    int hid;             // hidden width of a 2-layer head
    int head_mfma;       // 2-layer head on the f32 MFMA form (fwd_syn.hip, CCMI_HEAD_MFMA)
    int head_generic;    // never the unrolled 48-wide head (CCMI_HEAD_GENERIC, a test form)
    int ntiles;          // runs per frame (the fused kernel's 1-D grid is ntiles x batch)
    int run_base, run_extra; // a strip's run i walks run_base + (i < run_extra) windows (RunPlan)
    int w0_off, b0_off, relu0;
    int w1_off, b1_off, relu1;
    int n_sp;            // 3x3 layers after the head
    SpLayer sp[kMaxSp];
    const float *params;
    int64_t pstride;
    float *out;
    int64_t out_stride;
    int tiles_x;
    float qmax;          // > 0: write the post-processed frame (2^bitdepth - 1)
    int yuv420;
};

struct Plan {
    bool fused;
    int hid, cmid;
    FusedArgs fa;
};

// Run plan of the fused kernel: a workgroup walks a run of consecutive windows (rh head rows
// each) down one column strip.  With h 3x3 layers a run of n windows emits rh n - 2 h rows
// (only its first window pays the vertical halo), run i starts at the row where run i - 1
// ended and the last run is clipped at H.  R caps the windows of one run (h = 0: 1, there is
// no halo to save).  The windows are dealt as evenly as possible, longer runs first: run i
// holds base + (i < extra) of them.
#ifndef CCMI_FUSED_RUN
#define CCMI_FUSED_RUN 6
#endif
struct RunPlan {
    int n_runs, base, extra;
};
inline RunPlan fused_run_plan(int H, int h, int R, int rh)
{
    if (h == 0 || R < 1) R = 1;
    const int per = rh * R - 2 * h; // rows a full-length run emits
    const int n_runs = (H + per - 1) / per;
    const int windows = (H + 2 * h * n_runs + rh - 1) / rh;
    return RunPlan{n_runs, windows / n_runs, windows % n_runs};
}
inline int run_windows(const RunPlan &p, int i) { return p.base + (i < p.extra ? 1 : 0); }
// first output row of run i
inline int run_start(const RunPlan &p, int i, int h, int rh)
{
    return rh * (i * p.base + (i < p.extra ? i : p.extra)) - 2 * h * i;
}

// Offsets of each layer's weights / biases in a frame's parameter block.
void layer_offsets(const ccmi_syn_args *a, int *w_off, int *b_off, int *cin_of, int64_t *total);
// Fills P for architectures the fused synthesis kernel handles (1x1 head of <= 2 layers,
// then <= 3 same-width 3x3 layers of 3 or 4 channels); false otherwise.
bool make_plan(const ccmi_syn_args *a, Plan *P);

// ---------------------------------------------------------------- upsampling level
struct LevelArgs {
    // source stack (level k): C channels of hs x ws; channel c at src + c * hs * ws
    const float *src;
    int64_t src_stride;
    int src_quant; // source is the raw coarsest latent grid -> round(gain * x)
    int C, hs, ws;
    // refine input: raw latent grid of level k-1 (flat latent vector + offset)
    const float *ref_src;
    int64_t ref_stride;
    int ref_quant;
    // destination stack (level k-1): C + 1 channels of hd x wd
    float *dst;
    int64_t dst_stride;
    int hd, wd;
    float gain;
    // kernels, per frame: up taps at params + up_off, refine taps at params + pre_off
    const float *params;
    int64_t pstride;
    int up_off, K;
    int pre_off, Kp;
    int tiles_x;
};

// Polyphase geometry of a K-tap 2x transposed conv with a KP-tap refine, for a
// destination tile of TY x TX.
template <int K, int KP, int TY, int TX>
struct UpsTile {
    static constexpr int K2 = K / 2;
    static constexpr int D0 = -((K2 + 1) / 2);      // min source offset over both parities
    static constexpr int NS = K2 + 1;               // source samples shared by an (even, odd) pair
    static constexpr int SH = TY / 2 + NS - 1;      // source tile rows
    static constexpr int SW = TX / 2 + NS - 1;      // source tile cols
    static constexpr int PAD = KP / 2;
    static constexpr int RH = TY + KP - 1, RW = TX + KP - 1;
    // tap used by parity a at source offset d (or -1)
    static constexpr int tap(int a, int d) { return (a + K2 - 1 - 2 * d >= 0 && a + K2 - 1 - 2 * d < K) ? a + K2 - 1 - 2 * d : -1; }
};

// Validates the ups arguments and (launch = true) runs pyramid steps 0 .. L-3 (every step
// but the last, which produces the full-resolution stack); fills *last with the arguments
// of the final step (source level 1 -> level 0).  prev (fold): step L-3 (level 2 -> 1) is not
// launched either, its arguments go to *prev for a kernel that evaluates it in place.
// form (CCMI_UPS_FORM_*): the level kernel the launched steps use.  Returns CCMI_OK or an error code.
int ups_pyramid(const ccmi_ups_args *a, hipStream_t s, LevelArgs *last, bool launch = true, LevelArgs *prev = nullptr,
                int form = CCMI_UPS_FORM_DEFAULT);

} // namespace ccmi_fwd
