// fwd_syn.hip -- path A synthesis (Synthesis.forward), float32, plus frame post-processing.
//
// Reference: coolchic/enc/component/core/synthesis.py
//   SynthesisConv2d.forward :69-84  -- replicate pad (ks-1)/2, conv2d + bias, (+ x if residual)
//   Synthesis.forward      :264-277 -- layers in sequence, ReLU / identity after each.
// Post-processing: FrameEncoder.forward eval branch, coolchic/enc/component/frame.py:175-183,
//   convert_444_to_420 coolchic/enc/io/format/yuv.py:275-299 (nearest = even rows / cols).
//
// Fast path (every architecture made of a 1x1 "MLP" head followed by 3x3 layers with
// <= 4 channels -- all the reference presets: hop, mop, lop, ...): ONE fused kernel per
// launch.  A workgroup walks a run of consecutive 32 x 64 pixel windows down one column strip
// (fwd_common.h fused_run_plan: at most CCMI_FUSED_RUN windows).  Per window, pass 0 evaluates
// the per-pixel MLP (c_in -> hid -> c_mid, weights from LDS records) on the whole window and
// keeps its c_mid outputs in registers; each 3x3 layer then works in registers (the horizontal
// taps across lanes by DPP, the vertical ones from the thread's own rows and the last two rows
// of the thread above through LDS) and writes its output one row up, so that a window needs
// nothing from below: the two rows above its first come from the run's previous window (a
// small carry area in LDS).  Only a run's first window pays the vertical halo (its top two
// rows per 3x3 layer are not stored); columns lose one pixel per 3x3 layer on either side in
// every window.  The last layer writes to HBM.  Replicate padding is reproduced by evaluating
// pixels outside the image at the clamped image coordinate.  HBM traffic: c_in planes read
// once (+ halo), c_out planes written once.
//
// Any other architecture runs the generic per-layer kernel (one launch per layer,
// ping-pong through the caller's workspace).
#include <stdlib.h>
#include <type_traits>

#include "fwd_common.h"

using namespace ccmi_fwd;

namespace {

constexpr int kThreads = 256;


// Fused head + 3x3 tail.  The workgroup's working region is a fixed 32 x 64 window
// (2048 pixels, 512 threads, 4 per thread), moved down by 32 rows per iteration of the run.
// Thread (c = tid & 63, g = tid >> 6) owns column c and the register rows 4g .. 4g+3; with the
// window's head rows at image rows oy .. oy+31, register row r of stage t (the output of t
// 3x3 layers) holds image row oy + r - t.  Stage t is valid on columns [t, 64-t); on rows it
// is valid everywhere except above row oy + t in a run's first window (no carry yet).  So
// after n_sp layers a run's first window stores 32 - 2 n_sp rows and every later one 32.
//  * head: packed fp32 (v_pk_fma_f32) over pixel pairs, weight records broadcast from LDS,
//    hidden activations consumed as they are produced (never stored);
//  * 3x3 layers: in registers (see "3x3 layers, replicate padding" below).  Pixels outside
//    the image or outside the stage's valid band are computed but never stored, which keeps
//    control flow uniform.
// window height (and threads per workgroup) overridable at build time for the window-size
// A/B of DESIGN.md 7 (profiles/r4c_fused_window_ab.txt); the product build uses 32 rows, 512 threads
#ifndef CCMI_FUSED_RH
#define CCMI_FUSED_RH 32
#endif
#ifndef CCMI_FUSED_THREADS
#define CCMI_FUSED_THREADS 512
#endif
constexpr int kFThreads = CCMI_FUSED_THREADS;
constexpr int kRW = 64, kRH = CCMI_FUSED_RH;
constexpr int kRowsPerThread = kRH / (kFThreads / kRW); // 4
constexpr int kNW = kFThreads / 64;                     // waves per workgroup (8)

// Fused-upsampling input (UPS = true): the window's CIN input channels are not read from
// a [CIN][H][W] tensor but evaluated in the kernel from the level-1 stack and the
// full-resolution latent (the last Upsampling step, same operation order as
// ups_level_fixed<8, 7>): the horizontal passes of the 2x transposed conv (C = CIN-1
// channels, kHsRows half-resolution rows) and of the refine (kHrRows rows) are staged in
// LDS for the window's clamped image rectangle, and each head pixel finishes the vertical
// passes from there.  The staging area aliases the second 3x3 ping-pong buffer, which is
// first written after the head has finished reading it.
// Output of channel m at (gy, gx): the synthesis value, or with A.qmax > 0 the
// post-processed frame of FrameEncoder.forward (eval): round to the 2^bd - 1 grid, clamp
// to [0, 1], and for yuv420 the chroma planes sampled at even rows / columns.
// lut8 (8-bit output): the 256 quotients k / 255 in LDS, so the rounded value costs a
// lookup instead of an IEEE division; clamping k to [0, 255] first gives the same value
// as clamping the quotient (NaN -> 0 both ways).
// 32-bit byte offsets from a wave-uniform base (a frame's planes stay below 4 GB, checked at
// launch): the address is SGPR base + zero-extended VGPR offset, no 64-bit VALU arithmetic
__device__ __forceinline__ float *at(float *base, uint32_t i) { return (float *)((char *)base + i * 4u); }
__device__ __forceinline__ float ldu(const float *base, uint64_t byte) { return *(const float *)((const char *)base + byte); }
// A 32-bit byte offset as the 64-bit register pair ldu() adds to its base, made in this window
// and opaque: z is a zero the compiler cannot fold (a thread index >> 31).  From a plain zero
// extension the compiler keeps one loop-invariant zero register for the upper halves, holds it
// across the whole window loop and spills it there.
__device__ __forceinline__ uint64_t off64(uint32_t byte, uint32_t z)
{
    uint64_t o = ((uint64_t)z << 32) | byte;
    asm volatile("" : "+v"(o));
    return o;
}

__device__ __forceinline__ void store_out(const FusedArgs &A, float *out, int64_t plane, int m, int gy, int gx, float v,
                                          const float *lut8)
{
    const uint32_t pl = (uint32_t)plane, px = (uint32_t)(gy * A.W + gx);
    if (A.qmax <= 0.f) {
        *at(out, m * pl + px) = v;
        return;
    }
    const float q = lut8 ? lut8[(int)fminf(fmaxf(rintf(v * 255.f), 0.f), 255.f)]
                         : fminf(fmaxf(rintf(v * A.qmax) / A.qmax, 0.f), 1.f);
    if (!A.yuv420 || m == 0) {
        *at(out, m * pl + px) = q;
    } else if (!(gy & 1) && !(gx & 1) && (gy >> 1) < (A.H >> 1) && (gx >> 1) < (A.W >> 1)) {
        const uint32_t cp = (uint32_t)((A.H >> 1) * (A.W >> 1));
        *at(out, pl + (m - 1) * cp + (uint32_t)((gy >> 1) * (A.W >> 1) + (gx >> 1))) = q;
    }
}

// ---- exact-f32 MFMA head (both 1x1 layers' products of the first, the hidden layer) -------
// v_mfma_f32_16x16x4_f32: D[16 x 16] += A[16 x 4] B[4 x 16], each product an exact f32 fma
// (the instruction is an fmaf chain over its K = 4, MI355X_MICROARCH.md "Matrix cores").
// Lane l = (g = l >> 4, r = l & 15) supplies A[m = r][k = g] and B[k = g][n = r] and holds
// D[m = 4 g + i][n = r] in accumulator register i.  The head's first layer is
// H[unit][px] = W0[unit][ch] X[ch][px] with M = 16 hidden units per tile, N = 16 pixels,
// K = 8 = the c_in channels, a constant 1 (its weight is the bias) and zeros, in two
// K-steps; the MFMA pipe then carries 7/10 of the head's multiply-adds while the VALU does
// the ReLU and the 48 -> 3 layer from the accumulators.
typedef float v4f __attribute__((ext_vector_type(4)));
__device__ __forceinline__ v4f mfma16(float a, float b, v4f c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// 4 x 4 transpose of 16-lane rows over four registers: on return, row j of t[g] is row g of
// the input v[j] (two permlane16 swaps, then two permlane32 swaps)
__device__ __forceinline__ void rows_transpose4(const float (&v)[4], float (&t)[4])
{
    const auto p = __builtin_amdgcn_permlane16_swap(__float_as_uint(v[0]), __float_as_uint(v[1]), false, false);
    const auto q = __builtin_amdgcn_permlane16_swap(__float_as_uint(v[2]), __float_as_uint(v[3]), false, false);
    const auto a = __builtin_amdgcn_permlane32_swap(p[0], q[0], false, false);
    const auto b = __builtin_amdgcn_permlane32_swap(p[1], q[1], false, false);
    t[0] = __uint_as_float(a[0]);
    t[1] = __uint_as_float(b[0]);
    t[2] = __uint_as_float(a[1]);
    t[3] = __uint_as_float(b[1]);
}

// The kernarg segment through a pointer the compiler cannot see through: arguments read
// through it are loaded after this point (scalar loads), not held in SGPRs from further up.
// Only for code inlined into a kernel.
typedef const __attribute__((address_space(4))) char *kernarg_ptr;
__device__ __forceinline__ kernarg_ptr fresh_kernargs()
{
    kernarg_ptr p = (kernarg_ptr)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return p;
}

#if defined(CCMI_ARM_STAMPS)
// diagnostic build (make stamps): per-phase cycle totals of the fused kernel, wave 0 of
// every workgroup; read with ccmi_debug_fused_stamps()
__device__ unsigned long long g_fstamp[8];
#define FSTAMP(k)                                                                  \
    do {                                                                           \
        __syncthreads();                                                           \
        const unsigned long long _t = __builtin_amdgcn_s_memtime();                \
        if (threadIdx.x == 0) atomicAdd(&g_fstamp[k], _t - t_prev);                \
        t_prev = _t;                                                               \
    } while (0)
#else
#define FSTAMP(k)
#endif

using FT = UpsTile<8, 7, kRH, kRW>;
constexpr int kHsRows = kRH / 2 + 1 + FT::NS - 1; // half-res rows under <= kRH clamped rows
constexpr int kHrRows = kRH + 7 - 1;              // refine rows incl. the 7-tap halo
constexpr int kSW = kRW / 2 + 1 + FT::NS - 1 + 2; // raw source tile pitch (37 used; odd: the rows of
                                                  // phase B's pair 32, 8 apart, fall in distinct banks)
constexpr int kTW = kRW + 7 - 1 + 2;              // raw latent tile pitch (70 used, 72 read)

// Fused upsampling stages the level-1 channels in NG groups of GC (one group's raw tile and
// horizontal passes in LDS at a time), and the head's weight records live in region 1 once the
// gathers are done (or behind the pool, staged once per run: fused_run_recs, an opt-in build):
// 51 KB of LDS for the 7-grid hop decoder, three resident workgroups per CU (measured: one
// workgroup per CU instead of two costs +41 %, tools/occ_probe.sh).
constexpr int fused_groups(int cin, bool ups) { return ups && cin - 1 >= 4 ? 2 : 1; }
// carry rows of a run: per 3x3 layer, the last two rows of the window's bottom wave, kept for
// the top wave of the run's next window ([layer][2 rows][CMID][column])
constexpr int fused_carry_floats(int cmid) { return kMaxSp * 2 * cmid * kRW; }
// a channel group's raw tiles (region 0 under fused upsampling), rounded to whole 128-bit words so
// that everything behind region 0 stays 16-byte aligned
constexpr int fused_raw_floats(int gc) { return (gc * kHsRows * kSW + kHrRows * kTW + 3) / 4 * 4; }
// the pool without per-run head records (fused_run_recs below)
constexpr int fused_lds_floats(int cin, int cmid, bool ups)
{
    const int C = ups ? cin - 1 : 0, GC = (C + fused_groups(cin, ups) - 1) / fused_groups(cin, ups);
    const int raw = ups ? fused_raw_floats(GC) : 0;
    const int stage = ups ? GC * kHsRows * kRW + kHrRows * kRW : 0;
    const int xr = 2 * cmid * kFThreads; // a 3x3 layer's halo-row exchange buffer
    const int b0 = xr > raw ? xr : raw;
    int b1 = xr > stage ? xr : stage;
    b1 = b1 > kMaxHid * 16 + 256 ? b1 : kMaxHid * 16 + 256; // head records (+ the MFMA head's weight table)
    return b0 + b1 + fused_carry_floats(cmid) + 256; // + the runs' carry rows + the 8-bit quotient table
}
// waves per SIMD the register allocation must allow: 3 workgroups of 8 waves on 4 SIMDs when
// the LDS fits three (<= 160 KB / 3), else 2
constexpr int fused_wpe(int cin, int cmid, bool ups, bool mh = false)
{
#ifdef CCMI_FUSED_WPE
    if (!mh) return CCMI_FUSED_WPE; // window-size A/B builds only
#endif
    return !mh && 4 * fused_lds_floats(cin, cmid, ups) <= 160 * 1024 / 3 ? 6 : 4;
}
// Head records staged once per run, in LDS of their own behind the pool (kRunRecPitch floats per
// hidden unit: three 128-bit words, the fields of a 7-grid record with up to 4 outputs): the
// unrolled VALU head with two channel groups, where the records fit under 160 KB / 3.  That is
// the 7-grid 48-wide head with a 3-channel tail (hop, plain and folded: 54,576 B); with a
// 4-channel tail they do not fit (53,808 B without them) and, like every other instantiation,
// it stages its records in region 1 in every window.
// Off in the product build (-DCCMI_FUSED_RUN_RECS=1 builds it): it saves two barriers and the
// staging per window, and measured 1.5 % slower on the headline than per-window staging at
// 52,272 B (profiles/fused_rows_ab.txt; DESIGN.md 5 "Stride-2 row pairs").
#ifndef CCMI_FUSED_RUN_RECS
#define CCMI_FUSED_RUN_RECS 0
#endif
constexpr int kRunRecPitch = 12;
constexpr bool fused_run_recs(int cin, int cmid, bool ups, bool mh, int hid)
{
    return CCMI_FUSED_RUN_RECS && ups && !mh && hid > 0 && fused_groups(cin, ups) == 2 && cin + 1 + cmid <= kRunRecPitch &&
           4 * (fused_lds_floats(cin, cmid, ups) + kRunRecPitch * hid) <= 160 * 1024 / 3;
}

// MH: split-f16 MFMA first head layer (a separate instantiation: compiled into the default
// kernel as a runtime branch, its registers pushed the VALU variant from 108 to 133 VGPRs,
// i.e. from 4 to 3 waves per SIMD, and decode_fused from 0.97 to 1.40 ms per 32 frames)
// HID > 0: the 2-layer head's hidden width fixed at compile time (fully unrolled unit loop:
// weight records at immediate LDS offsets, no loop counter or record rotation)
// FOLD (UPS only): the pyramid's level-2 -> 1 step is evaluated in the kernel too (U2 holds its
// arguments): the level-1 values phase A needs are computed from the level-2 stack and the
// level-1 latent instead of read from a level-1 stack in HBM (see "fold" below)
template <int CIN, int CMID, bool UPS, bool MH = false, int HID = 0, bool FOLD = false>
__global__ __launch_bounds__(kFThreads) __attribute__((amdgpu_waves_per_eu(fused_wpe(CIN, CMID, UPS, MH)))) void syn_fused_kernel(FusedArgs Ak, LevelArgs Uk, LevelArgs U2k)
{
    static_assert(!FOLD || (UPS && CIN >= 3), "the fold needs the fused level-1 -> 0 step and a level-2 stack");
    constexpr int NR = kRowsPerThread;
    constexpr int C = UPS ? CIN - 1 : 0, NG = fused_groups(CIN, UPS), GC = (C + NG - 1) / NG;
    // region 0: raw input tiles of a channel group (UPS, phases A-B), then the 3x3 layers'
    // halo-row buffer 0; region 1: the group's horizontal-pass results (UPS), then the head's
    // weight records (unless kRunRecs), then the halo-row buffer 1
    constexpr int kRaw = UPS ? fused_raw_floats(GC) : 0;
    constexpr int kBuf0 = 2 * CMID * kFThreads > kRaw ? 2 * CMID * kFThreads : kRaw;
    constexpr int kTot = fused_lds_floats(CIN, CMID, UPS);
    // kRunRecs: the head's weight records behind the pool, staged once per run (fused_run_recs)
    constexpr bool kRunRecs = fused_run_recs(CIN, CMID, UPS, MH, HID);
    constexpr int kRecPitch = kRunRecs ? kRunRecPitch : 16;
    static_assert(kBuf0 % 4 == 0 && kTot % 4 == 0, "the records are read as 128-bit words");
    __shared__ __attribute__((aligned(16))) float s_pool[kTot + (kRunRecs ? kRunRecPitch * HID : 0)];
    float *s_st = s_pool;                      // [GC][kHsRows][kSW] raw source tile (UPS only)
    float *s_yt = s_st + GC * kHsRows * kSW;   // [kHrRows][kTW] raw latent tile (UPS only)
    float *s_hs = s_pool + kBuf0;              // [GC][kHsRows][kRW]   (UPS only)
    float *s_hr = s_hs + GC * kHsRows * kRW;   // [kHrRows][kRW]       (UPS only)
    float *s_lut8 = s_pool + kTot - 256;
    float *s_carry = s_lut8 - fused_carry_floats(CMID); // [kMaxSp][2][CMID][kRW]
#if defined(CCMI_ARM_STAMPS)
    unsigned long long t_prev = __builtin_amdgcn_s_memtime();
#endif
    // head hidden unit j as a record of kRecPitch floats, its fields dense from slot 0: w0[j][0..CIN),
    // b0[j], w1[0..CMID)[j].  The VALU head reads a record back as kRecVecs broadcast
    // ds_read_b128 (all lanes, one address; three for up to 12 fields: hop has 11), issued a
    // unit ahead of use, unlike the SGPR path whose scalar loads the compiler waits on at once.
    // The slots behind the fields are read with the last vector but are never operands.
    // An LDS read is serviced in lane groups whatever its addresses (identical addresses
    // only remove bank conflicts inside a group): a ds_read_b128 takes 4 LDS-array cycles per
    // wave, a ds_read_b96 or a ds_read2_b64 takes 8, and the four SIMDs of a CU share the
    // array.  So the reads must stay whole 128-bit ones: from a record that skipped every
    // fourth slot (to spare the compiler's copy of a broadcast operand out of an odd dword)
    // the compiler read three ds_read_b96 and half a ds_read2_b64 per unit, 28 array cycles
    // against 12 here, more than the unit's 80 VALU cycles on each of four SIMDs leave room
    // for.  The operands are taken in place by op_sel instead (head_hidden2 / head_out2,
    // fwd_common.h).
    float *s_head = s_pool + (kRunRecs ? kTot : kBuf0); // [unit][kRecPitch]
    float *s_w1p = s_pool + kBuf0 + kMaxHid * 16; // MH: the second layer's weights by lane row
    static_assert(CIN + 1 + CMID <= kRecPitch, "hidden-unit record");
    constexpr int kRecVecs = (CIN + 1 + CMID + 3) / 4;

    // XCD-aware order of the runs (raster order, frame after frame, a contiguous stretch per
    // XCD): neighbouring strips re-read each other's halo columns from one L2
    const int wt = xcd_order(blockIdx.x, gridDim.x);
    const int b0 = wt / Ak.ntiles, tile = wt - b0 * Ak.ntiles;
    // the work item is a run: nwin consecutive windows of one column strip, the first one's
    // head rows starting halo rows above the run's first output row (fused_run_plan)
    const int ri = tile / Ak.tiles_x;
    const int nwin = Ak.run_base + (ri < Ak.run_extra ? 1 : 0);
    const int y0 = kRH * (ri * Ak.run_base + min(ri, Ak.run_extra)) - 2 * Ak.n_sp * ri;
    const int x0 = (tile - ri * Ak.tiles_x) * (kRW - 2 * Ak.n_sp);
    const int oy0 = y0 - Ak.n_sp, ox0 = x0 - Ak.n_sp; // global coords of the first window's (0,0)
    // per-run table in LDS: the 8-bit output quotients (own area)
    if (Ak.qmax == 255.f) s_lut8[threadIdx.x & 255] = (float)(threadIdx.x & 255) / 255.f;
    // the thread index as an opaque copy per use (see the top of the loop)
    auto tixf = []() __attribute__((always_inline)) {
        int t = threadIdx.x;
        asm volatile("" : "+v"(t));
        return t;
    };
    // The head's weight records (L2-resident: every workgroup of a frame reads the same ones) are
    // fetched into two registers per thread (fetch_recs) and stored into LDS from there
    // (store_recs): once per run where they have LDS of their own (kRunRecs), else in every
    // window, where they share region 1 with the horizontal passes.
    constexpr int kHeadRegs = (kMaxHid * 16 + kFThreads - 1) / kFThreads;
    // scaled ReLU for the unrolled VALU head (HID > 0, !MH; launched only with a first-layer ReLU)
    constexpr bool kScaledRelu = HID > 0 && !MH;
    constexpr float kW0Scale = kScaledRelu ? 0x1p-32f : 1.f, kW1Scale = kScaledRelu ? 0x1p32f : 1.f;
    auto fetch_recs = [&](const FusedArgs &A, cfloat_ptr prm, float(&hv)[kHeadRegs]) __attribute__((always_inline)) {
        const int tid = tixf();
#pragma unroll
        for (int k = 0; k < kHeadRegs; ++k) {
            const int i = tid + k * kFThreads, j = i >> 4, f = i & 15;
            float v = 0.f;
            if (i < kMaxHid * 16 && A.n_head == 2 && j < A.hid) {
                // the unrolled VALU head's records carry the scaled-ReLU exponents ("Scaled ReLU" below):
                // hidden weights / bias x 2^-32, output weights x 2^32 -- exact power-of-two scalings
                if (f < CIN) v = prm[A.w0_off + j * CIN + f] * kW0Scale;
                else if (f == CIN) v = prm[A.b0_off + j] * kW0Scale;
                else if (f <= CIN + CMID) v = prm[A.w1_off + (f - CIN - 1) * A.hid + j] * kW1Scale;
            }
            hv[k] = v;
        }
    };
    auto store_recs = [&](const float(&hv)[kHeadRegs]) __attribute__((always_inline)) {
        const int tid = tixf();
        constexpr int kUnits = kRunRecs ? HID : kMaxHid;
#pragma unroll
        for (int k = 0; k < kHeadRegs; ++k) {
            const int i = tid + k * kFThreads, j = i >> 4, f = i & 15;
            if (j < kUnits && f <= CIN + CMID) s_head[j * kRecPitch + f] = hv[k]; // other slots are never operands
        }
    };
    if constexpr (kRunRecs) {
        // This run's records (one frame, one workgroup).  Their first reader is the first
        // window's head, behind that window's barriers; nothing else ever writes the area.
        const FusedArgs &A = *(const FusedArgs *)fresh_kernargs();
        float hv[kHeadRegs];
        fetch_recs(A, (cfloat_ptr)(size_t)(A.params + (int64_t)b0 * A.pstride), hv);
        store_recs(hv);
    }
    // The walk.  The trip count is a function of the work item alone (scalar), every barrier
    // below is reached by all waves in every iteration, and nothing leaves the loop early.
#pragma clang loop unroll(disable)
    for (int win = 0; win < nwin; ++win) {
    // Loop-invariant values must not be hoisted out of this loop: held across a whole window
    // they cost the kernel its 6 waves per SIMD.  So the thread index is an opaque copy per
    // use, tixf above (values derived from it, lane masks and LDS addresses, were hoisted and
    // spilled),
    // and the kernel's arguments are re-read from the kernarg segment in every window, through
    // a pointer the compiler cannot see through (hoisted, they filled the SGPRs and the spilled
    // ones took vector registers).
    const auto kargs = fresh_kernargs();
    constexpr size_t kOffU = (sizeof(FusedArgs) + alignof(LevelArgs) - 1) / alignof(LevelArgs) * alignof(LevelArgs);
    constexpr size_t kOffU2 = (kOffU + sizeof(LevelArgs) + alignof(LevelArgs) - 1) / alignof(LevelArgs) * alignof(LevelArgs);
    const FusedArgs &A = *(const FusedArgs *)kargs;
    const LevelArgs &U = *(const LevelArgs *)(kargs + kOffU);
    const LevelArgs &U2 = *(const LevelArgs *)(kargs + kOffU2);
    const int halo = A.n_sp;
    // (the frame and the strip's column likewise: what the compiler derives from them is a few
    // scalar instructions per window, hoisted it occupies SGPRs across the loop)
    int b = b0, ox = ox0;
    asm volatile("" : "+s"(b), "+s"(ox));
    const int oy = oy0 + kRH * win; // image row of this window's head row 0
    const cfloat_ptr prm = (cfloat_ptr)(size_t)(A.params + (int64_t)b * A.pstride);
    const float *in = A.in + (int64_t)b * A.in_stride;
    float *out = A.out + (int64_t)b * A.out_stride;
    const int64_t plane = (int64_t)A.H * A.W;
    // lane-derived indices; re-derived at the top of every window and after the head (below) so
    // that they are not live across the head or the loop's back edge: held across the head
    // they were the kernel's 5 spilled VGPRs (scratch traffic in every wave)
    int c, rb, gx, cxg; // column, first window row of this thread, image column, clamped
    auto reidx = [&]() {
        int t = threadIdx.x;
        asm volatile("" : "+v"(t)); // an opaque copy: the compiler cannot reuse the old values
        c = t & (kRW - 1);
        rb = (t >> 6) * NR;
        gx = ox + c;
        cxg = clampi(gx, A.W - 1);
    };

    const float *lut8 = A.qmax == 255.f ? s_lut8 : nullptr;
    // per-window staging of the head's weight records (!kRunRecs), in region 1: before anything
    // else without fused upsampling, after the gathers with it.  They are fetched before the
    // last upsampling group, so their latency hides behind its passes, and staged once region 1
    // is free
    float hv[kHeadRegs];
    auto load_head = [&]() {
        if constexpr (!kRunRecs) fetch_recs(A, prm, hv);
    };
    auto stage_head = [&]() {
        if constexpr (!kRunRecs) store_recs(hv);
        if constexpr (MH) {
            const int tid = tixf();
            // [tile][lane row][m][4 units]: the second layer's weights of the 4 hidden units a
            // lane's accumulator registers hold (one ds_read_b128 per output channel)
            constexpr int n = (HID / 16) * 4 * CMID * 4;
            static_assert(n <= kFThreads, "one entry per thread");
            const int i = tid;
            if (i < n) {
                const int u4 = i & 3, m = (i >> 2) % CMID, lgi = (i / (4 * CMID)) & 3, mt = i / (16 * CMID);
                s_w1p[i] = prm[A.w1_off + m * A.hid + 16 * mt + 4 * lgi + u4];
            }
        }
    };
    reidx();
    if constexpr (!UPS) {
        load_head();
        stage_head();
        __syncthreads();
    }

    float x[NR][CIN];
    // window's clamped image origin (fused upsampling only)
    const int Ya = clampi(oy, A.H - 1), Xa = clampi(ox, A.W - 1);
    // interior windows (no row clamping): the thread's 4 rows are consecutive, so the
    // vertical passes share their LDS rows -- 10 refine rows and 6 or 7 half-res rows per
    // channel for 4 pixels, offsets fixed by the parity of the window's first row
    const bool interior = oy >= 0 && oy + kRH <= A.H;
    if constexpr (UPS) {
        // the level's taps, re-read per window through the constant address space (scalar loads
        // even behind the previous window's stores): held in SGPRs across the head and the 3x3
        // layers they cost the kernel its 6 waves per SIMD
        float wu[8], wr[7];
        const cfloat_ptr uprm = (cfloat_ptr)(size_t)(U.params + (int64_t)b * U.pstride);
#pragma unroll
        for (int k = 0; k < 8; ++k) wu[k] = uprm[U.up_off + k];
#pragma unroll
        for (int k = 0; k < 7; ++k) wr[k] = uprm[U.pre_off + k];
        const int jbase = Ya / 2 + FT::D0, ibase = Xa / 2 + FT::D0;
        // Phases A + B are row-parallel and wave-private: wave wv owns the rows r = wv + kNW u of
        // a group's [GC][kHsRows] raw tile and the raw latent rows yr = wv + kNW u; lane = column.
        // Row addresses are wave-uniform (scalar), so a load costs no VALU index math, and a
        // wave's horizontal passes read back only rows it wrote itself -- a wave-level fence
        // instead of a workgroup barrier between the raw tiles and the horizontal passes.
        const int wv = __builtin_amdgcn_readfirstlane((int)(tixf() >> 6));
        const int lane = tixf() & 63;
        constexpr int kSR = GC * kHsRows, kSU = (kSR + kNW - 1) / kNW; // a group's source rows, per wave
        constexpr int kLU = (kHrRows + kNW - 1) / kNW;         // latent rows per wave
        static_assert(kSW <= 64 && kTW <= 128 && kTW > 64 && kHsRows >= kNW, "lane = raw column, one row wrap per step");
        const float *src = U.src + (int64_t)b * U.src_stride;
        const float *rs = U.ref_src + (int64_t)b * U.ref_stride;
        float sv[NG][kSU], tv[kLU][2];
        bool tin[2];
        // phase A: every group's raw rows and the latent tile, all loads in flight at once;
        // clamped source coordinates are always inside the stack.  (channel, row) of
        // r = wv + kNW u in 32-bit scalar registers (a frame's stack stays below 2 GB; checked
        // at launch)
        {
            const int splane = U.hs * U.ws;
            // lanes past the tile re-read the last column (same cache lines, no extra fetch)
            const uint32_t zhi = (uint32_t)tixf() >> 31; // 0
            const uint64_t scol = off64(4u * (uint32_t)clampi(ibase + (lane < kSW ? lane : kSW - 1), U.ws - 1), zhi);
#pragma unroll
            for (int G = 0; G < NG; ++G)
#pragma unroll
                for (int u = 0; u < kSU; ++u) {
                    if constexpr (FOLD) break; // computed below from the level-2 stack
                    const int r = wv + kNW * u;
                    // ch = r / kHsRows without a division: wv < kNW moves r past at most one boundary
                    const int c0 = (kNW * u) / kHsRows, tb = kHsRows * (c0 + 1) - kNW * u; // folded (u unrolled)
                    const int lc = c0 + (wv >= tb ? 1 : 0), jj = r - lc * kHsRows;
                    sv[G][u] = 0.f;
                    if ((u < kSU - 1 || r < kSR) && G * GC + lc < C) {
                        const int row = (G * GC + lc) * splane + clampi(jbase + jj, U.hs - 1) * U.ws;
#if defined(CCMI_DIAG_NOLOAD) // diagnostic build only: phase A without its global loads
                        sv[G][u] = 0.001f * (float)(jj + scol);
#else
                        sv[G][u] = ldu(src + row, scol);
#endif
                    }
                }
            // latent tile: zero outside the image (the refine's zero padding)
            uint64_t tx[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int X = Xa - 3 + (lane + 64 * h < kTW ? lane + 64 * h : kTW - 1);
                tin[h] = X >= 0 && X < U.wd;
                tx[h] = off64(4u * (uint32_t)clampi(X, U.wd - 1), zhi);
            }
#pragma unroll
            for (int u = 0; u < kLU; ++u) {
                const int yr = wv + kNW * u;
                const int Y = Ya - 3 + yr;
                const int row = clampi(Y, U.hd - 1) * U.wd;
#pragma unroll
                for (int h = 0; h < 2; ++h) {
#if defined(CCMI_DIAG_NOLOAD)
                    tv[u][h] = 0.001f * (float)(yr + tx[h]);
#else
                    tv[u][h] = ldu(rs + row, tx[h]);
#endif
                }
            }
        }
        if constexpr (FOLD) {
            // ---- fold: the level-1 stack values of this window's phase A, computed here from
            // the level-2 stack (C2 channels) and the level-1 latent with ups_level_fixed<8, 7>'s
            // operation order (bitwise the values the pyramid's level-2 -> 1 launch writes):
            // F1 the raw tiles into LDS, F2 the horizontal passes, F3 each wave's rows of the
            // [channel][kHsRows] tile (lane = column) by the vertical passes, into sv.  The
            // window reads level-1 rows clamp(jbase + jj) and columns clamp(ibase + lane): the
            // rectangle [R0, R1] x [C0, C1] (<= 21 x 37) of the level-1 image.
            constexpr int C2 = CIN - 2;
            constexpr int kFLR = kHsRows + 6, kFLW = kSW + 6, kFLP = kFLW + 1; // latent-1 tile (refine halo 3)
            constexpr int kFP = 40;                                          // pitch of the horizontal passes
            constexpr int kF2R = (kHsRows - 1) / 2 + 1 + FT::NS - 1;         // level-2 rows under <= 21 level-1 rows
            constexpr int kF2W = (kSW - 1) / 2 + 1 + FT::NS - 1, kF2P = kF2W + 1;
            static_assert(kFP >= kSW, "pass pitch");
            float *f_lat = s_pool;                       // [kFLR][kFLP]
            float *f_ref = f_lat + kFLR * kFLP;          // [kFLR][kFP]   refine, horizontal
            float *f_src = f_ref + kFLR * kFP;           // [C2][kF2R][kF2P]
            float *f_h2 = f_src + C2 * kF2R * kF2P;      // [C2][kF2R][kFP] transposed conv, horizontal
            static_assert(kFLR * kFLP + kFLR * kFP + C2 * kF2R * (kF2P + kFP) <= kTot - 256 - fused_carry_floats(CMID), "fold tiles fit before the carry rows");
            const int hs1 = U.hs, ws1 = U.ws, hs2 = U2.hs, ws2 = U2.ws;
            const int R0 = clampi(jbase, hs1 - 1), R1 = clampi(jbase + kHsRows - 1, hs1 - 1);
            const int C0 = clampi(ibase, ws1 - 1);
            const int r2 = (R0 >> 1) + FT::D0, c2 = (C0 >> 1) + FT::D0; // level-2 origin of the tile
            const cfloat_ptr uprm2 = (cfloat_ptr)(size_t)(U2.params + (int64_t)b * U2.pstride);
            float wu2[8], wr2[7];
#pragma unroll
            for (int k = 0; k < 8; ++k) wu2[k] = uprm2[U2.up_off + k];
#pragma unroll
            for (int k = 0; k < 7; ++k) wr2[k] = uprm2[U2.pre_off + k];
            const int tid = tixf();
            // F1: every load in flight before the first LDS store
            {
                const float *l1 = U2.ref_src + (int64_t)b * U2.ref_stride;
                const float *s2 = U2.src + (int64_t)b * U2.src_stride;
                constexpr int NL = (kFLR * kFLW + kFThreads - 1) / kFThreads;
                constexpr int NS2 = (C2 * kF2R * kF2W + kFThreads - 1) / kFThreads;
                float lv[NL], sv2[NS2];
#pragma unroll
                for (int u = 0; u < NL; ++u) {
                    const int i = tid + u * kFThreads, r = i / kFLW, c = i - r * kFLW;
                    const int Y = R0 - 3 + r, X = C0 - 3 + c;
                    lv[u] = (i < kFLR * kFLW && Y >= 0 && Y < hs1 && X >= 0 && X < ws1) ? l1[Y * ws1 + X] : 0.f;
                }
#pragma unroll
                for (int u = 0; u < NS2; ++u) {
                    const int i = tid + u * kFThreads, ch = i / (kF2R * kF2W), rem = i - ch * (kF2R * kF2W);
                    const int r = rem / kF2W, c = rem - r * kF2W;
                    sv2[u] = i < C2 * kF2R * kF2W
                                 ? s2[(ch * hs2 + clampi(r2 + r, hs2 - 1)) * ws2 + clampi(c2 + c, ws2 - 1)]
                                 : 0.f;
                }
#pragma unroll
                for (int u = 0; u < NL; ++u) {
                    const int i = tid + u * kFThreads, r = i / kFLW, c = i - r * kFLW;
                    if (i < kFLR * kFLW) f_lat[r * kFLP + c] = U2.ref_quant ? rintf(U2.gain * lv[u]) : lv[u];
                }
#pragma unroll
                for (int u = 0; u < NS2; ++u) {
                    const int i = tid + u * kFThreads, ch = i / (kF2R * kF2W), rem = i - ch * (kF2R * kF2W);
                    const int r = rem / kF2W, c = rem - r * kF2W;
                    if (i < C2 * kF2R * kF2W) f_src[(ch * kF2R + r) * kF2P + c] = U2.src_quant ? rintf(U2.gain * sv2[u]) : sv2[u];
                }
            }
            __syncthreads();
            // F2: horizontal passes.  Refine: 7 taps over the zero-padded latent row.  Transposed
            // conv: level-1 columns (2 q, 2 q + 1) from level-2 columns q + D0 .. q + D0 + NS - 1,
            // for the pairs q covering columns C0 .. C0 + kSW - 1.
            for (int i = tid; i < kFLR * kSW; i += kFThreads) {
                const int r = i / kSW, c = i - r * kSW;
                const float *p = f_lat + r * kFLP + c;
                float acc = 0.f;
#pragma unroll
                for (int k = 0; k < 7; ++k) acc = fmaf(wr2[k], p[k], acc);
                f_ref[r * kFP + c] = acc;
            }
            {
                constexpr int NQ = kSW / 2 + 1; // pairs touching C0 .. C0 + kSW - 1
                const int q0 = C0 >> 1;
                for (int i = tid; i < C2 * kF2R * NQ; i += kFThreads) {
                    const int ch = i / (kF2R * NQ), rem = i - ch * (kF2R * NQ), r = rem / NQ, q = rem - r * NQ;
                    const float *p = f_src + (ch * kF2R + r) * kF2P + q; // level-2 column q0 + q + D0
                    float e = 0.f, o = 0.f;
#pragma unroll
                    for (int m = 0; m < FT::NS; ++m) {
                        const float v = p[m];
                        const int te = FT::tap(0, FT::D0 + m), to = FT::tap(1, FT::D0 + m);
                        if (te >= 0) e = fmaf(wu2[te], v, e);
                        if (to >= 0) o = fmaf(wu2[to], v, o);
                    }
                    const int ce = 2 * (q0 + q) - C0; // tile column of the even output
                    float *h = f_h2 + (ch * kF2R + r) * kFP;
                    if (ce >= 0 && ce < kSW) h[ce] = e;
                    if (ce + 1 < kSW) h[ce + 1] = o;
                }
            }
            __syncthreads();
            // F3: this wave's rows r = wv + kNW u of each group's [GC][kHsRows] tile, lane = column
            {
                const int cx = clampi(ibase + (lane < kSW ? lane : kSW - 1), ws1 - 1) - C0;
#pragma unroll
                for (int G = 0; G < NG; ++G)
#pragma unroll
                    for (int u = 0; u < kSU; ++u) {
                        const int r = wv + kNW * u;
                        const int c0 = (kNW * u) / kHsRows, tb = kHsRows * (c0 + 1) - kNW * u;
                        const int lc = c0 + (wv >= tb ? 1 : 0), jj = r - lc * kHsRows;
                        const int ch = G * GC + lc; // level-1 channel: 0 the refined latent, 1.. upsampled
                        float v = 0.f;
                        if ((u < kSU - 1 || r < kSR) && ch < C) {
                            const int Y1 = clampi(jbase + jj, hs1 - 1), ry = Y1 - R0; // wave-uniform
                            if (ch == 0) {
                                const float *p = f_ref + ry * kFP + cx;
                                float acc = 0.f;
#pragma unroll
                                for (int k = 0; k < 7; ++k) acc = fmaf(wr2[k], p[k * kFP], acc);
                                v = acc + f_lat[(ry + 3) * kFLP + cx + 3];
                            } else {
                                const float *p = f_h2 + ((ch - 1) * kF2R + (Y1 >> 1) - (R0 >> 1)) * kFP + cx;
                                float acc = 0.f;
                                if (Y1 & 1) {
#pragma unroll
                                    for (int m = 0; m < FT::NS; ++m) {
                                        const int t = FT::tap(1, FT::D0 + m);
                                        if (t >= 0) acc = fmaf(wu2[t], p[m * kFP], acc);
                                    }
                                } else {
#pragma unroll
                                    for (int m = 0; m < FT::NS; ++m) {
                                        const int t = FT::tap(0, FT::D0 + m);
                                        if (t >= 0) acc = fmaf(wu2[t], p[m * kFP], acc);
                                    }
                                }
                                v = acc;
                            }
                        }
                        sv[G][u] = v;
                    }
            }
            (void)R1;
            __syncthreads(); // the fold's tiles are overwritten by phase A's stores below
        }
        f2 wp[FT::NS];
#pragma unroll
        for (int m = 0; m < FT::NS; ++m) {
            const int te = FT::tap(0, FT::D0 + m), to = FT::tap(1, FT::D0 + m);
            wp[m] = f2{te >= 0 ? wu[te] : 0.f, to >= 0 ? wu[to] : 0.f};
        }
        auto group = [&](auto GI) {
            constexpr int G = decltype(GI)::value;
            if constexpr (G > 0) __syncthreads(); // every wave done with the previous group
#pragma unroll
            for (int u = 0; u < kSU; ++u) {
                const int r = wv + kNW * u;
                if ((u < kSU - 1 || r < kSR) && lane < kSW)
                    s_st[r * kSW + lane] = U.src_quant ? rintf(U.gain * sv[G][u]) : sv[G][u];
            }
            if constexpr (G == 0) {
#pragma unroll
                for (int u = 0; u < kLU; ++u) {
                    const int yr = wv + kNW * u;
                    if (yr >= kHrRows) continue;
                    const int Y = Ya - 3 + yr;
                    const bool yin = Y >= 0 && Y < U.hd;
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const float v = U.ref_quant ? rintf(U.gain * tv[u][h]) : tv[u][h];
                        if (lane + 64 * h < kTW) s_yt[yr * kTW + lane + 64 * h] = (yin && tin[h]) ? v : 0.f;
                    }
                }
            }
            // the wave reads back rows it wrote (other lanes' columns): order its LDS accesses
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            if constexpr (G == 0) FSTAMP(0);
            // phase B: horizontal passes, in ups_level_fixed's operation order.  Transposed
            // conv: lane = (row half, pair k = lane & 31); the (even, odd) outputs of pair k read
            // source columns k .. k + NS - 1 and land in window columns 2k - (Xa & 1), +1.
            {
                const int odd = Xa & 1;
                const int k = lane & 31, hsel = lane >> 5;
                const int xe = 2 * k - odd;
                static_assert(32 + FT::NS - 1 < kSW, "pair 32 reads stay inside the source row");
                auto pair = [&](int r, int kk, int xw) {
                    const float *sr = s_st + r * kSW + kk;
                    f2 eo = f2(0.f);
#pragma unroll
                    for (int m = 0; m < FT::NS; ++m) eo = __builtin_elementwise_fma(wp[m], f2(sr[m]), eo);
                    float *hrow = s_hs + r * kRW;
                    if (xw >= 0) hrow[xw] = eo.x;
                    if (xw + 1 < kRW) hrow[xw + 1] = eo.y;
                };
#pragma unroll
                for (int u = 0; u < kSU; u += 2) {
                    const int r = wv + kNW * (u + hsel);
                    if (u + 1 < kSU - 1 || r < kSR) pair(r, k, xe);
                }
                if (odd) { // pair 32 of every row (window columns 63, 64)
                    const int r = wv + kNW * lane;
                    if (lane < kSU && r < kSR) pair(r, 32, 63);
                }
                if constexpr (G == 0) {
                    // refine: lane = window column, 7-tap sliding window over the wave's latent rows
#pragma unroll
                    for (int u = 0; u < kLU; ++u) {
                        const int yr = wv + kNW * u;
                        if (yr >= kHrRows) continue;
                        const float *tr = s_yt + yr * kTW + lane;
                        float acc = 0.f;
#pragma unroll
                        for (int q = 0; q < 7; ++q) acc = fmaf(wr[q], tr[q], acc);
                        s_hr[yr * kRW + lane] = acc;
                    }
                }
            }
            __syncthreads();
            if constexpr (G == 0) FSTAMP(1);
            // gather: the vertical passes of this group's channels (+ the refine for G = 0)
            const int xi = cxg - Xa;
            if (interior) {
                auto gather = [&](auto par) {
                    constexpr int P = decltype(par)::value; // parity of oy (and of row rb)
                    if constexpr (G == 0) {
                        float h[NR + 6];
#pragma unroll
                        for (int k = 0; k < NR + 6; ++k) h[k] = s_hr[(rb + k) * kRW + xi];
#pragma unroll
                        for (int p = 0; p < NR; ++p) {
                            float acc = 0.f;
#pragma unroll
                            for (int k = 0; k < 7; ++k) acc = fmaf(wr[k], h[p + k], acc);
                            x[p][0] = acc + s_yt[(rb + p + 3) * kTW + xi + 3];
                        }
                    }
                    constexpr int NH = FT::NS + (NR / 2) - 1 + P; // half-res rows for 4 pixels
                    const int j0 = rb / 2;
#pragma unroll
                    for (int lc = 0; lc < GC; ++lc) {
                        constexpr int dummy = 0;
                        (void)dummy;
                        const int k = 1 + G * GC + lc;
                        if (k >= CIN) break;
                        float h[NH];
#pragma unroll
                        for (int m = 0; m < NH; ++m) h[m] = s_hs[(lc * kHsRows + j0 + m) * kRW + xi];
#pragma unroll
                        for (int p = 0; p < NR; ++p) {
                            const int a = (P + p) & 1, off = (P + p) >> 1;
                            float acc = 0.f;
#pragma unroll
                            for (int m = 0; m < FT::NS; ++m) {
                                const int te = FT::tap(0, FT::D0 + m), to = FT::tap(1, FT::D0 + m);
                                if ((a ? to : te) >= 0) acc = fmaf(wu[a ? to : te], h[off + m], acc);
                            }
                            x[p][k] = acc;
                        }
                    }
                };
                if (oy & 1) gather(std::integral_constant<int, 1>{});
                else gather(std::integral_constant<int, 0>{});
            } else {
#pragma unroll
                for (int p = 0; p < NR; ++p) {
                    // vertical passes at the clamped row, in ups_level_fixed's operation order
                    const int Y = clampi(oy + rb + p, A.H - 1);
                    const int yi = Y - Ya;
                    if constexpr (G == 0) {
                        float acc = 0.f;
#pragma unroll
                        for (int k = 0; k < 7; ++k) acc = fmaf(wr[k], s_hr[(yi + k) * kRW + xi], acc);
                        // residual: the (quantised) latent, from the raw tile still in LDS
                        x[p][0] = acc + s_yt[(yi + 3) * kTW + xi + 3];
                    }
                    const int jj0 = Y / 2 - Ya / 2, a = Y & 1;
#pragma unroll
                    for (int lc = 0; lc < GC; ++lc) {
                        const int k = 1 + G * GC + lc;
                        if (k >= CIN) break;
                        const float *h = s_hs + (lc * kHsRows + jj0) * kRW + xi;
                        // both parities' chains (compile-time taps), then a select: a per-lane
                        // parity had made every wu[t] a compare / select chain over the taps
                        float acc_e = 0.f, acc_o = 0.f;
#pragma unroll
                        for (int m = 0; m < FT::NS; ++m) {
                            const int te = FT::tap(0, FT::D0 + m), to = FT::tap(1, FT::D0 + m);
                            const float hv = h[m * kRW];
                            if (te >= 0) acc_e = fmaf(wu[te], hv, acc_e);
                            if (to >= 0) acc_o = fmaf(wu[to], hv, acc_o);
                        }
                        x[p][k] = a ? acc_o : acc_e;
                    }
                }
            }
        };
        if constexpr (NG > 1) {
            group(std::integral_constant<int, 0>{});
            load_head(); // in flight behind the last group's passes
            group(std::integral_constant<int, 1>{});
        } else {
            load_head();
            group(std::integral_constant<int, 0>{});
        }
    } else {
#pragma unroll
        for (int p = 0; p < NR; ++p) {
            const int64_t pix = (int64_t)clampi(oy + rb + p, A.H - 1) * A.W + cxg;
#pragma unroll
            for (int k = 0; k < CIN; ++k) x[p][k] = in[k * plane + pix];
        }
    }

    // the current stage's image at this thread's 4 rows, as stride-2 row pairs: img[q] = {row
    // rb + q, row rb + q + 2}.  A 3x3 layer's five input pairs are then two pairs made of a row
    // from above and the pairs as they stand (no pair straddles two others), and a pair holds
    // rows of one parity: pair 0 the even image rows, which is all the 4:2:0 chroma stores.
    constexpr int NP = NR / 2; // pairs: NP = 2 in what follows
    static_assert(NR % 4 == 0, "a pair's rows have one parity");
    f2 img[NP][CMID];
    auto row_of = [&](int p, int m) __attribute__((always_inline)) { return p < NP ? img[p][m].x : img[p - NP][m].y; };
    // ------------------------ pass 0: per-pixel 1x1 head ------------------------
    {
        const FusedArgs &A = *(const FusedArgs *)fresh_kernargs(); // (re-read: see the top of the loop)
        const cfloat_ptr w0 = prm + A.w0_off, b0 = prm + A.b0_off;
        const cfloat_ptr b1 = prm + A.b1_off;
        float o[NR][CMID];
        // region 1 (the last group's horizontal passes) is free once every wave has gathered:
        // the head's weight records go there.
        // With kRunRecs nothing is staged here and the head needs no barrier of its own.  What
        // the two barriers of the per-window staging ordered besides the records:
        //  * region 0 is next written by publish(xb0) below.  Its raw tiles were last read by the
        //    last group's phase B (the source rows) and by group 0's gather (the latent tile's
        //    residual); with two groups both lie before the barrier that closes the last group's
        //    phase B, which every wave has passed before it publishes.
        //  * region 1 (the last group's horizontal passes, read by the gather) is next written by
        //    the first non-last 3x3 layer's publish(xout), behind that layer's barrier, which a
        //    wave reaches only after its gather; with a single 3x3 layer, by the next window's
        //    phase B, behind the barrier that closes this window.
        if constexpr (UPS && !kRunRecs) {
            __syncthreads();
            stage_head();
        }
        FSTAMP(2);
        if constexpr (MH) {
            // ---- exact-f32 MFMA first layer (+ bias), ReLU and the second layer on the VALU
            // from the accumulators; per window row, four 16-pixel groups per wave
            static_assert(HID % 16 == 0 && HID <= kMaxHid && CIN + 1 <= 8 && CMID <= 4, "f32-MFMA head shape");
            constexpr int NT = HID / 16;
            const int lane = tixf() & 63, lr = lane & 15, lg = lane >> 4;
            __syncthreads(); // s_head / s_w1p staged
            float a1[NT][2]; // A[m = lr][k = lg] of K-step s: W0[16 mt + lr][4 s + lg] (channel c_in: the bias)
#pragma unroll
            for (int mt = 0; mt < NT; ++mt)
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    const int ch = 4 * k + lg;
                    a1[mt][k] = ch <= CIN ? s_head[(16 * mt + lr) * kRecPitch + ch] : 0.f; // slot CIN: the bias
                }
            const f2 lo0 = f2(A.relu0 ? 0.f : -INFINITY);
            const float lo1 = A.relu1 ? 0.f : -INFINITY;
            typedef const __attribute__((address_space(3))) v4f *lds_v4;
            lds_v4 wb = (lds_v4)s_w1p;
            asm volatile("" : "+v"(wb));
#pragma unroll
            for (int p = 0; p < NR; ++p) {
                // the weight table re-read per row (an opaque base: held across rows it costs 36
                // registers)
                asm volatile("" : "+v"(wb));
                // B operands: channel 4 s + lg of pixel 16 g + lr, by two 16-lane-row transposes
                float T[2][4];
                {
                    float v0[4], v1[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        v0[k] = k < CIN ? x[p][k] : (k == CIN ? 1.f : 0.f);
                        v1[k] = 4 + k < CIN ? x[p][4 + k] : (4 + k == CIN ? 1.f : 0.f);
                    }
                    rows_transpose4(v0, T[0]);
                    rows_transpose4(v1, T[1]);
                }
                float P[4][CMID]; // partial outputs of this lane's 4 units per tile, pixel 16 g + lr
#pragma unroll
                for (int gh = 0; gh < 2; ++gh) {
                    f2 P2[2][CMID];
#pragma unroll
                    for (int gi = 0; gi < 2; ++gi)
#pragma unroll
                        for (int m = 0; m < CMID; ++m) P2[gi][m] = f2(0.f);
#pragma unroll
                    for (int mt = 0; mt < NT; ++mt) {
                        v4f w[CMID]; // w1[m][16 mt + 4 lg + i], i = 0..3
#pragma unroll
                        for (int m = 0; m < CMID; ++m) w[m] = wb[(mt * 4 + lg) * CMID + m];
#pragma unroll
                        for (int gi = 0; gi < 2; ++gi) {
                            const int g = 2 * gh + gi;
                            v4f acc = mfma16(a1[mt][0], T[0][g], v4f{0.f, 0.f, 0.f, 0.f});
                            acc = mfma16(a1[mt][1], T[1][g], acc);
                            const f2 h01 = __builtin_elementwise_max(f2{acc[0], acc[1]}, lo0);
                            const f2 h23 = __builtin_elementwise_max(f2{acc[2], acc[3]}, lo0);
#pragma unroll
                            for (int m = 0; m < CMID; ++m) {
                                P2[gi][m] = __builtin_elementwise_fma(f2{w[m][0], w[m][1]}, h01, P2[gi][m]);
                                P2[gi][m] = __builtin_elementwise_fma(f2{w[m][2], w[m][3]}, h23, P2[gi][m]);
                            }
                        }
                    }
#pragma unroll
                    for (int gi = 0; gi < 2; ++gi)
#pragma unroll
                        for (int m = 0; m < CMID; ++m) P[2 * gh + gi][m] = P2[gi][m].x + P2[gi][m].y;
                }
                // sum over the 4 lane rows (unit groups) and return to lane = column
#pragma unroll
                for (int m = 0; m < CMID; ++m) {
                    const float v[4] = {P[0][m], P[1][m], P[2][m], P[3][m]};
                    float t[4];
                    rows_transpose4(v, t);
                    o[p][m] = fmaxf(((t[0] + t[1]) + (t[2] + t[3])) + b1[m], lo1);
                }
            }
        } else if (A.n_head == 2) {
            const int hid = HID > 0 ? HID : A.hid;
            f2 xp[NR / 2][CIN], op[NR / 2][CMID];
#pragma unroll
            for (int q = 0; q < NR / 2; ++q) {
#pragma unroll
                for (int k = 0; k < CIN; ++k) xp[q][k] = f2{x[q][k], x[q + NR / 2][k]}; // stride-2 row pairs
#pragma unroll
                for (int m = 0; m < CMID; ++m) op[q][m] = f2(0.f);
            }
            if constexpr (!kRunRecs) __syncthreads(); // s_head staged
            // software pipelined: the record of unit j+1 is loaded while unit j computes
            struct Rec { f4v v[kRecVecs]; };
            // records through an LDS pointer the compiler cannot fold to a constant, so the
            // unrolled reads are base + immediate offset (not one v_mov of an address each)
            typedef const __attribute__((address_space(3))) f4v *lds_f4;
            constexpr int kRecStep = kRecPitch / 4; // a record's pitch in 128-bit words
            lds_f4 hb = (lds_f4)s_head;
            asm volatile("" : "+v"(hb));
            auto load = [&](int j) {
                const lds_f4 p = hb + kRecStep * (j < hid ? j : hid - 1);
                Rec r;
#pragma unroll
                for (int i = 0; i < kRecVecs; ++i) r.v[i] = p[i];
                return r;
            };
            // Scaled ReLU: the records hold w0, b0 x 2^-32 and w1 x 2^32 (stage_head), so the
            // hidden pre-activation arrives as h 2^-32 and max(h, 0) is the last fma's
            // clamp-to-[0, 1] modifier: no v_max_f32 per pixel and unit (gfx950 has no packed f32
            // max; they were 1 in 6 of the head's VALU instructions).  w1 2^32 x (h 2^-32) = w1 h
            // exactly.  A power-of-two scaling commutes with every rounding of the chain as long
            // as no operand or partial sum leaves the normal range after scaling, so the result
            // is bitwise the unscaled head's (CCMI_HEAD_GENERIC, test_forward.py's
            // test_unrolled_head_bitwise_generic) only while every hidden weight, bias and
            // partial pre-activation h has |h| >= 2^-94 or is 0, and h <= 2^32: a tinier value
            // loses bits as a subnormal (its term is below 2^-94 |w1|), a larger positive h is
            // clamped to 2^32.  Decoder weights and activations are far inside both limits.
            const f2 lo0 = f2(A.relu0 ? 0.f : -INFINITY); // the generic head's ReLU (max)
            // One unit on the thread's pixel pairs, two pairs at a time.  Per pair the chain is
            // what it always was: the bias, the CIN products in order, the clamp on the last
            // (hidden), then the CMID output FMAs (outs).
            constexpr bool RELU = kScaledRelu;
            constexpr int NQ = NR / 2;
            static_assert(NQ % 2 == 0, "the head's statements take two pixel pairs");
            auto hidden = [&](const Rec &r, f2(&h)[NQ]) __attribute__((always_inline)) {
                f2 w[4];
                rec_w0_pairs<CIN>(r.v, w);
#pragma unroll
                for (int q = 0; q < NQ; q += 2) {
                    head_hidden2<CIN, RELU>(w, rec_pair<CIN>(r.v), xp[q], xp[q + 1], h[q], h[q + 1]);
                    if constexpr (!RELU) {
                        h[q] = __builtin_elementwise_max(h[q], lo0);
                        h[q + 1] = __builtin_elementwise_max(h[q + 1], lo0);
                    }
                }
            };
            auto outs = [&](const Rec &r, const f2(&h)[NQ]) __attribute__((always_inline)) {
                static_for<CMID>([&](auto mc) __attribute__((always_inline)) {
                    constexpr int m = decltype(mc)::value, S = CIN + 1 + m;
#pragma unroll
                    for (int q = 0; q < NQ; q += 2) head_out2<S & 1>(rec_pair<S>(r.v), h[q], h[q + 1], op[q][m], op[q + 1][m]);
                });
            };
            if constexpr (HID > 0) {
                // Unrolled.  The reads are placed by hand (an LDS read does not move across a
                // volatile statement): the vectors of the next record that hold w0 and the bias
                // before the unit's hidden chain, its others between the chain and the outputs.
                constexpr int kHidVecs = CIN / 4 + 1;
                auto read = [&](Rec &r, int j, int v0, int v1) __attribute__((always_inline)) {
#pragma unroll
                    for (int i = v0; i < v1; ++i) r.v[i] = hb[kRecStep * j + i];
                };
                Rec cur, nxt;
                read(cur, 0, 0, kRecVecs);
                nxt = cur;
#pragma unroll
                for (int j = 0; j < HID; ++j) {
                    f2 h[NQ];
                    if (j + 1 < HID) read(nxt, j + 1, 0, kHidVecs);
                    hidden(cur, h);
                    if (j + 1 < HID) read(nxt, j + 1, kHidVecs, kRecVecs);
                    outs(cur, h);
                    cur = nxt;
                }
            } else {
                auto unit = [&](const Rec &r) __attribute__((always_inline)) {
                    f2 h[NQ];
                    hidden(r, h);
                    outs(r, h);
                };
                Rec ra = load(0), rb2 = load(1);
                for (int j = 0; j < hid; j += 2) {
                    unit(ra);
                    ra = load(j + 2);
                    if (j + 1 < hid) unit(rb2);
                    rb2 = load(j + 3);
                }
            }
            const float lo1 = A.relu1 ? 0.f : -INFINITY;
#pragma unroll
            for (int q = 0; q < NR / 2; ++q)
#pragma unroll
                for (int m = 0; m < CMID; ++m) {
                    o[q][m] = fmaxf(op[q][m].x + b1[m], lo1);
                    o[q + NR / 2][m] = fmaxf(op[q][m].y + b1[m], lo1);
                }
        } else {
            const float lo0 = A.relu0 ? 0.f : -INFINITY;
#pragma unroll
            for (int m = 0; m < CMID; ++m) {
                const float bm = b0[m];
#pragma unroll
                for (int p = 0; p < NR; ++p) {
                    float acc = bm;
#pragma unroll
                    for (int k = 0; k < CIN; ++k) acc = fmaf(w0[m * CIN + k], x[p][k], acc);
                    o[p][m] = fmaxf(acc, lo0);
                }
            }
        }
        FSTAMP(3);
        reidx();
        if (halo == 0) { // head-only decoders: single-window runs, stored here (wave-uniform)
#pragma unroll
            for (int p = 0; p < NR; ++p) {
                const int gy = oy + rb + p;
                if (gy < A.H && gx < A.W)
#pragma unroll
                    for (int m = 0; m < CMID; ++m) store_out(A, out, plane, m, gy, gx, o[p][m], lut8);
            }
        }
#pragma unroll
        for (int q = 0; q < NR / 2; ++q)
#pragma unroll
            for (int m = 0; m < CMID; ++m) img[q][m] = f2{o[q][m], o[q + NR / 2][m]};
    }

    // ------------------------ 3x3 layers, replicate padding ------------------------
    // Register form: a stage's image stays in the registers of the thread that computed it
    // (lane = window column, the thread's 4 rows).  Skewed rows: a thread holding input rows
    // r .. r+3 produces output rows r-1 .. r+2 from its own rows and the last two rows of the
    // thread above (one wave up: a wave is 4 whole window rows), so only each thread's last two
    // rows go through LDS and nothing is needed from below.  The top wave takes those two rows
    // from the carry area, where the bottom wave left them in the run's previous window.  The
    // horizontal taps never touch LDS: for output channel m the thread forms the
    // three column partial sums S_dx = sum_{k,dy} w[m][k][dy][dx] x_k(row + dy - 1) of its own
    // column, and out(c) = S_1(c) + S_0(c - 1) + S_2(c + 1), the neighbours' sums read across
    // lanes by DPP (v_add_f32 wave_shr:1 / wave_shl:1).  (The LDS form read 3 x 3 x CMID
    // neighbours per pixel from an LDS image and was LDS-bandwidth bound: 120 ds_read per
    // thread and layer.)  Replicate padding: every stage is evaluated at all window pixels,
    // and a value outside the image stands for the nearest image pixel --
    //  * rows (wave-uniform): a thread reading rows r-2 .. r+3 replaces those outside the
    //    image by the nearest in-image row among them (the only rows an in-image output
    //    reads: the edge row itself is the thread's own or one of the two from above);
    //  * columns: the head is evaluated at clamped columns, and each 3x3 layer's output at
    //    lanes outside the image is replaced by the edge lane's (v_readlane), so the next
    //    layer's column sums there are the edge column's.
    // Columns 0 / kRW-1 read garbage neighbours (DPP zero fill); they are outside every later
    // stage's valid band [t, kRW - t).  In a run's first window the carry rows are garbage:
    // stage t is valid from row t of that window on, and the 2 n_sp top rows of its last stage
    // (labels oy - n_sp .. oy + n_sp - 1) are not stored.
    // Exchange buffers, double-buffered by layer parity: [last two rows][CMID][thread].
    if (halo != 0) {
    const FusedArgs &A = *(const FusedArgs *)fresh_kernargs(); // (re-read: see the top of the loop)
    float *xb0 = s_pool, *xb1 = s_pool + kBuf0;
    auto publish = [&](float *xb) __attribute__((always_inline)) {
        const int tid = tixf();
#pragma unroll
        for (int m = 0; m < CMID; ++m) {
            xb[m * kFThreads + tid] = row_of(NR - 2, m);            // the thread's row NR - 2 (img[NP - 2].y)
            xb[(CMID + m) * kFThreads + tid] = row_of(NR - 1, m);   // and row NR - 1 (img[NP - 1].y)
        }
    };
    auto shr1 = [](float v) __attribute__((always_inline)) { // lane c <- lane c - 1 (0 at lane 0)
        return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x138, 0xf, 0xf, true));
    };
    auto shl1 = [](float v) __attribute__((always_inline)) { // lane c <- lane c + 1 (0 at lane 63)
        return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x130, 0xf, 0xf, true));
    };
    // every row any stage touches (oy - n_sp - 1 .. oy + kRH - 1) in the image
    const bool rows_inner = oy - halo - 1 >= 0 && oy + kRH <= A.H;
    const bool cols_inner = ox >= 0 && ox + kRW <= A.W;        // every lane an image column
    // one 3x3 layer: img (stage s input) -> img (stage s output, one row up); the non-last
    // layers publish their output's last two rows into xout
    // c420 (last layer only, wave-uniform): the output is stored as 4:2:0 planes, which keep the
    // chroma channels m >= 1 on even image rows only.  Image-row parity is the parity of the
    // register row: register row r of the last stage is image row y0 - 2 n_sp + kRH win + r with
    // y0 and kRH even, and rb is a multiple of 4.  So the even rows are exactly the pairs q of
    // even q, and the last layer skips the chroma channels' other pairs (a scalar branch
    // around them; one copy of the layer).
    auto layer = [&](auto LAST, bool c420, int s, const float *xin, float *xout) __attribute__((always_inline)) {
        constexpr bool last = decltype(LAST)::value;
        static_assert(kRH % 2 == 0, "row parity");
        const int tid = tixf();
        const int wrow = __builtin_amdgcn_readfirstlane(tid >> 6) * NR; // rb, wave-uniform
        float *cr = s_carry + s * (2 * CMID * kRW) + (tid & (kRW - 1)); // this layer's carry rows, own column
        // the thread's input rows r-2 .. r+3 (r = oy + rb - s) of every input channel: v[0], v[1]
        // from the thread above, or for the top wave from the carry of the run's previous
        // window -- read before the barrier, because the bottom wave overwrites it after it
        float v[NR + 2][CMID];
        if (wrow == 0) {
#pragma unroll
            for (int m = 0; m < CMID; ++m) {
                v[0][m] = cr[m * kRW];
                v[1][m] = cr[(CMID + m) * kRW];
            }
        }
        __syncthreads(); // xin published by every wave (and the previous reads of xout done)
        const cfloat_ptr wt = prm + A.sp[s].w_off;
        const cfloat_ptr bs = prm + A.sp[s].b_off;
        const f2 lo = f2(A.sp[s].relu ? 0.f : -INFINITY);
        const f2 rsd = f2(A.sp[s].residual ? 1.f : 0.f);
        if (wrow != 0) {
#pragma unroll
            for (int m = 0; m < CMID; ++m) {
                v[0][m] = xin[m * kFThreads + tid - kRW];
                v[1][m] = xin[(CMID + m) * kFThreads + tid - kRW];
            }
        }
#pragma unroll
        for (int m = 0; m < CMID; ++m)
#pragma unroll
            for (int p = 0; p < NR; ++p) v[p + 2][m] = row_of(p, m);
        if (wrow == kRH - NR) {
            // the bottom wave's last two rows are rows -2, -1 of the next window (the top wave
            // has read the previous ones before the barrier above; the next read is behind the
            // barrier that closes this window)
#pragma unroll
            for (int m = 0; m < CMID; ++m) {
                cr[m * kRW] = v[NR][m];
                cr[(CMID + m) * kRW] = v[NR + 1][m];
            }
        }
        if (!rows_inner) {
            const int gy0 = oy + wrow - 2 - s; // image row of v[0]
#pragma unroll
            for (int i = 1; i < NR + 2; ++i)
                if (gy0 + i >= A.H)
#pragma unroll
                    for (int m = 0; m < CMID; ++m) v[i][m] = v[i - 1][m];
#pragma unroll
            for (int i = NR; i >= 0; --i)
                if (gy0 + i < 0)
#pragma unroll
                    for (int m = 0; m < CMID; ++m) v[i][m] = v[i + 1][m];
        }
        // stride-2 row pairs: E[i][k] = {v[i], v[i + NP]}, i = 0 .. NP + 1.  E[2 ..] are the
        // thread's own pairs img[0 ..] as they stand; E[0] and E[1] take the row from above in
        // the low half and a copy of img[0].x / img[1].x in the high half.  Output pair q (the
        // thread's rows q, q + NP of the next stage) reads E[q + dy] and is centred on E[q + 1].
        f2 E[NP + 2][CMID];
#pragma unroll
        for (int i = 0; i < NP + 2; ++i)
#pragma unroll
            for (int k = 0; k < CMID; ++k) E[i][k] = f2{v[i][k], v[i + NP][k]};
        // the weights are wave-uniform scalar loads; the output channel loop is unrolled (the
        // outputs stay in registers, which a runtime channel index would send to scratch)
        f2 nxt[NP][CMID];
        // output channel m (unrolled by the callers) on the pairs q = qa, qa + qs, ...
        auto chan = [&](cfloat_ptr wt, cfloat_ptr bs, int m, int qa, int qs) __attribute__((always_inline)) {
            const cfloat_ptr wm = wt + m * CMID * 9;
            f2 S[3][NP];
#pragma unroll
            for (int q = qa; q < NP; q += qs) {
                S[0][q] = f2(0.f);
                S[1][q] = f2(bs[m]);
                S[2][q] = f2(0.f);
            }
#pragma unroll
            for (int k = 0; k < CMID; ++k)
#pragma unroll
                for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                    for (int dx = 0; dx < 3; ++dx) {
                        const f2 w = f2(wm[(k * 3 + dy) * 3 + dx]);
#pragma unroll
                        for (int q = qa; q < NP; q += qs) S[dx][q] = __builtin_elementwise_fma(w, E[q + dy][k], S[dx][q]);
                    }
#pragma unroll
            for (int q = qa; q < NP; q += qs) {
                f2 acc;
                acc.x = (S[1][q].x + shr1(S[0][q].x)) + shl1(S[2][q].x);
                acc.y = (S[1][q].y + shr1(S[0][q].y)) + shl1(S[2][q].y);
                // residual: the input at the centre (pair E[q + 1] = v[q + 1], v[q + 1 + NP])
                nxt[q][m] = __builtin_elementwise_max(__builtin_elementwise_fma(rsd, E[q + 1][m], acc), lo);
            }
        };
        if constexpr (last && CMID == 3) {
            // the stage that is stored: luma on every pair, chroma on the pairs of even rows,
            // and on the others unless the store drops them
            chan(wt, bs, 0, 0, 1);
#pragma unroll
            for (int m = 1; m < CMID; ++m) {
                chan(wt, bs, m, 0, 2);
#pragma unroll
                for (int q = 1; q < NP; q += 2) nxt[q][m] = f2(0.f);
            }
            // (finished here: left alone, the compiler sinks half of these chains below the branch
            // and holds their weights in SGPRs across it)
#pragma unroll
            for (int m = 0; m < CMID; ++m)
#pragma unroll
                for (int q = 0; q < NP; q += (m > 0 ? 2 : 1)) asm volatile("" : "+v"(nxt[q][m]));
            if (!c420) {
                // the weights once more, through pointers the compiler cannot match with the ones
                // above (it would keep all 56 of the chroma channels' in SGPRs for this branch,
                // and spill)
                cfloat_ptr wt2 = wt, bs2 = bs;
                asm volatile("" : "+s"(wt2), "+s"(bs2));
#pragma unroll
                for (int m = 1; m < CMID; ++m) chan(wt2, bs2, m, 1, 2);
            }
        } else {
#pragma unroll
            for (int m = 0; m < CMID; ++m) chan(wt, bs, m, 0, 1);
        }
#pragma unroll
        for (int q = 0; q < NR / 2; ++q)
#pragma unroll
            for (int m = 0; m < CMID; ++m) img[q][m] = nxt[q][m];
        if constexpr (!last) {
            if (!cols_inner) {
                // lanes left / right of the image take the edge column's value
                const int c0 = -ox, c1 = A.W - 1 - ox; // lanes of image columns 0, W-1
                const int lane = tid & 63;
#pragma unroll
                for (int q = 0; q < NR / 2; ++q)
#pragma unroll
                    for (int m = 0; m < CMID; ++m) {
                        float e0 = img[q][m].x, e1 = img[q][m].y;
                        if (c0 > 0) {
                            const float l0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(e0), c0));
                            const float l1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(e1), c0));
                            e0 = lane < c0 ? l0 : e0;
                            e1 = lane < c0 ? l1 : e1;
                        }
                        if (c1 < kRW - 1) {
                            const float r0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(e0), c1));
                            const float r1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(e1), c1));
                            e0 = lane > c1 ? r0 : e0;
                            e1 = lane > c1 ? r1 : e1;
                        }
                        img[q][m] = f2{e0, e1};
                    }
            }
            publish(xout);
        }
    };
    publish(xb0);
    for (int s = 0; s < A.n_sp - 1; ++s) {
        layer(std::false_type{}, false, s, xb0, xb1);
        float *const t = xb0;
        xb0 = xb1;
        xb1 = t;
    }
    // (c420: the same condition as the 4:2:0 store loops below)
    layer(std::true_type{}, A.yuv420 && A.qmax > 0.f, A.n_sp - 1, xb0, nullptr);
    // stores: this thread's own pixels of the last layer, from registers, one branch-free loop
    // per output format
    {
        reidx();
        const int t = A.n_sp;
        const bool col_ok = c >= t && c < kRW - t && gx < A.W;
        const uint32_t pl = (uint32_t)plane;
        const uint32_t cw = (uint32_t)(A.W >> 1), cp = (uint32_t)((A.H >> 1) * (A.W >> 1));
        const bool cx_ok = !(gx & 1) && (gx >> 1) < (A.W >> 1);
        auto emit = [&](auto MODE) {
            constexpr int md = decltype(MODE)::value; // 0 raw, 1 444, 2 420; +2: 8-bit table
            constexpr bool tab = md >= 3;
            constexpr int fmt = tab ? md - 2 : md;
#pragma unroll
            for (int p = 0; p < NR; ++p) {
                // register row r holds image row oy + r - t (one row up per layer); a run's
                // first window has no valid rows above its row 2 t
                const int r = rb + p, gy = oy + r - t;
                if (!(col_ok && (win > 0 || r >= 2 * t) && gy < A.H)) continue;
                const uint32_t px = (uint32_t)(gy * A.W + gx);
                const bool cy_ok = fmt == 2 && cx_ok && !(gy & 1) && (gy >> 1) < (A.H >> 1);
                const uint32_t cpx = (uint32_t)((gy >> 1) * (int)cw + (gx >> 1));
#pragma unroll
                for (int m = 0; m < CMID; ++m) {
                    // 420: odd rows carry no chroma, and gy is odd where p is (see C420 above; the
                    // last layer did not evaluate those)
                    if (fmt == 2 && m > 0 && (p & 1)) break;
                    float v = row_of(p, m);
                    if constexpr (fmt > 0) {
                        v = tab ? lut8[(int)fminf(fmaxf(rintf(v * 255.f), 0.f), 255.f)]
                                : fminf(fmaxf(rintf(v * A.qmax) / A.qmax, 0.f), 1.f);
                    }
                    if (fmt < 2 || m == 0) *at(out, m * pl + px) = v;
                    else if (cy_ok) *at(out, pl + (m - 1) * cp + cpx) = v;
                }
            }
        };
        if (A.qmax <= 0.f) emit(std::integral_constant<int, 0>{});
        else if (lut8) {
            if (A.yuv420) emit(std::integral_constant<int, 4>{});
            else emit(std::integral_constant<int, 3>{});
        } else if (A.yuv420) emit(std::integral_constant<int, 2>{});
        else emit(std::integral_constant<int, 1>{});
    }
    } // halo != 0
    FSTAMP(4);
    // the next window's phase A overwrites regions 0 / 1 (this window's exchange buffers and
    // head records); the carry rows were written before this barrier
    __syncthreads();
    } // the run's windows
}

// Generic layer: any ks (odd), any channel counts; replicate padding.
__global__ __launch_bounds__(kThreads) void syn_layer_kernel(const float *__restrict__ in, int64_t in_stride, int cin,
                                                             int H, int W, const float *__restrict__ params,
                                                             int64_t pstride, int w_off, int b_off, int nout, int ks,
                                                             int residual, int relu, float *__restrict__ out,
                                                             int64_t out_stride)
{
    const int b = blockIdx.y;
    const int64_t plane = (int64_t)H * W;
    const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (p >= plane) return;
    const int y = (int)(p / W), x = (int)(p - (int64_t)y * W);
    const float *src = in + (int64_t)b * in_stride;
    float *dst = out + (int64_t)b * out_stride;
    const float *wt = params + (int64_t)b * pstride + w_off;
    const float *bs = params + (int64_t)b * pstride + b_off;
    const int pad = ks / 2;
    for (int m = 0; m < nout; ++m) {
        float acc = 0.f;
        for (int k = 0; k < cin; ++k)
            for (int dy = 0; dy < ks; ++dy) {
                const int yy = clampi(y + dy - pad, H - 1);
                for (int dx = 0; dx < ks; ++dx) {
                    const int xx = clampi(x + dx - pad, W - 1);
                    acc = fmaf(wt[((m * cin + k) * ks + dy) * ks + dx], src[k * plane + (int64_t)yy * W + xx], acc);
                }
            }
        float v = acc + bs[m];
        if (residual) v += src[m * plane + p];
        if (relu) v = fmaxf(v, 0.f);
        dst[m * plane + p] = v;
    }
}

__global__ __launch_bounds__(kThreads) void post_kernel(const float *__restrict__ in, int64_t in_stride, int H, int W,
                                                        float qmax, int yuv420, float *__restrict__ out,
                                                        int64_t out_stride)
{
    const int b = blockIdx.y;
    const int64_t plane = (int64_t)H * W;
    const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (p >= plane) return;
    const float *src = in + (int64_t)b * in_stride;
    float *dst = out + (int64_t)b * out_stride;
    auto q = [qmax](float v) { return fminf(fmaxf(rintf(v * qmax) / qmax, 0.f), 1.f); };
    dst[p] = q(src[p]);
    const int y = (int)(p / W), x = (int)(p - (int64_t)y * W);
    if (!yuv420) {
        dst[plane + p] = q(src[plane + p]);
        dst[2 * plane + p] = q(src[2 * plane + p]);
    } else if (!(y & 1) && !(x & 1) && y / 2 < H / 2 && x / 2 < W / 2) {
        const int64_t cp = (int64_t)(H / 2) * (W / 2);
        const int64_t ci = (int64_t)(y / 2) * (W / 2) + x / 2;
        dst[plane + ci] = q(src[plane + p]);
        dst[plane + cp + ci] = q(src[2 * plane + p]);
    }
}

// the presets' 7-grid decoders with a 48-wide head (hop and its relatives): unrolled head
bool unrolled_head(const FusedArgs &fa) { return fa.cin == 7 && fa.n_head == 2 && fa.hid == 48 && fa.relu0 && !fa.head_generic; }

template <int CMID, bool UPS>
void launch_fused(dim3 grid, hipStream_t s, const FusedArgs &fa, const LevelArgs &u)
{
    const LevelArgs none{};
    if (unrolled_head(fa)) { // (its scaled ReLU assumes a first-layer ReLU)
        hipLaunchKernelGGL((syn_fused_kernel<7, CMID, UPS, false, 48>), grid, dim3(kFThreads), 0, s, fa, u, none);
        return;
    }
    switch (fa.cin) {
    case 1: hipLaunchKernelGGL((syn_fused_kernel<1, CMID, false>), grid, dim3(kFThreads), 0, s, fa, u, none); break;
#define CCMI_FUSED_CASE(N) \
    case N: hipLaunchKernelGGL((syn_fused_kernel<N, CMID, UPS>), grid, dim3(kFThreads), 0, s, fa, u, none); break;
    CCMI_FUSED_CASE(2) CCMI_FUSED_CASE(3) CCMI_FUSED_CASE(4) CCMI_FUSED_CASE(5) CCMI_FUSED_CASE(6)
    CCMI_FUSED_CASE(7) CCMI_FUSED_CASE(8)
#undef CCMI_FUSED_CASE
    }
}

// f32-MFMA head variant (ccmi_decode_args.head = CCMI_HEAD_MFMA): the 7-grid decoders with a
// 48-wide head, upsampling fused and at least one 3x3 layer
template <int CMID>
bool launch_fused_mfma_head(dim3 grid, hipStream_t s, const FusedArgs &fa, const LevelArgs &u)
{
    if (!fa.head_mfma || fa.cin != 7 || fa.n_head != 2 || fa.hid != 48 || fa.n_sp < 1) return false;
    hipLaunchKernelGGL((syn_fused_kernel<7, CMID, true, true, 48>), grid, dim3(kFThreads), 0, s, fa, u, LevelArgs{});
    return true;
}

// the folded form (level 2 -> 1 in the kernel): the headline decoder only (7 grids, 48-wide
// VALU head, 3-channel tail)
bool fold_eligible(const FusedArgs &fa, int cmid) { return cmid == 3 && unrolled_head(fa) && !fa.head_mfma; }

// the fused kernel's grid for one frame: column strips x runs of at most cap windows
void set_runs(FusedArgs &f, int cap)
{
    const RunPlan rp = fused_run_plan(f.H, f.n_sp, cap, kRH);
    f.tiles_x = ccmi_div_up(f.W, kRW - 2 * f.n_sp);
    f.ntiles = f.tiles_x * rp.n_runs;
    f.run_base = rp.base;
    f.run_extra = rp.extra;
}

} // namespace

namespace ccmi_fwd {

void layer_offsets(const ccmi_syn_args *a, int *w_off, int *b_off, int *cin_of, int64_t *total)
{
    int64_t o = 0;
    int c = a->c_in;
    for (int l = 0; l < a->n_layers; ++l) {
        const ccmi_syn_layer &L = a->layers[l];
        cin_of[l] = c;
        w_off[l] = (int)o;
        o += (int64_t)L.n_out * c * L.ks * L.ks;
        b_off[l] = (int)o;
        o += L.n_out;
        c = L.n_out;
    }
    *total = o;
}

bool make_plan(const ccmi_syn_args *a, Plan *P)
{
    int w_off[CCMI_MAX_SYN_LAYERS], b_off[CCMI_MAX_SYN_LAYERS], cin_of[CCMI_MAX_SYN_LAYERS];
    int64_t tot;
    layer_offsets(a, w_off, b_off, cin_of, &tot);
    P->fused = false;
    const ccmi_syn_layer *L = a->layers;
    int n_head = 0;
    while (n_head < a->n_layers && n_head < 2 && L[n_head].ks == 1 && !L[n_head].residual) n_head++;
    if (n_head == 0 || a->c_in > kMaxIn) return false;
    const int cmid = L[n_head - 1].n_out;
    if (cmid < 1 || cmid > kMaxMid) return false;
    int hid = n_head == 2 ? L[0].n_out : 0;
    if (hid > kMaxHid) return false;
    const int n_sp = a->n_layers - n_head;
    if (n_sp > kMaxSp) return false;
    for (int l = n_head; l < a->n_layers; ++l)
        if (L[l].ks != 3 || L[l].n_out != cmid) return false;
    if (cmid != 3 && cmid != 4) return false; // instantiated shapes
    // the fused kernel addresses its output with 32-bit byte offsets
    if ((int64_t)4 * cmid * a->h * a->w >= ((int64_t)1 << 32)) return false;
    FusedArgs &f = P->fa;
    f = FusedArgs{};
    f.cin = a->c_in;
    f.H = a->h;
    f.W = a->w;
    f.n_head = n_head;
    f.hid = hid;
    f.w0_off = w_off[0];
    f.b0_off = b_off[0];
    f.relu0 = L[0].relu;
    if (n_head == 2) {
        f.w1_off = w_off[1];
        f.b1_off = b_off[1];
        f.relu1 = L[1].relu;
    }
    f.n_sp = n_sp;
    for (int s = 0; s < n_sp; ++s) {
        f.sp[s].w_off = w_off[n_head + s];
        f.sp[s].b_off = b_off[n_head + s];
        f.sp[s].residual = L[n_head + s].residual;
        f.sp[s].relu = L[n_head + s].relu;
    }
    P->fused = true;
    P->hid = hid;
    P->cmid = cmid;
    return true;
}

} // namespace ccmi_fwd

extern "C" size_t ccmi_syn_workspace_bytes(const ccmi_syn_args *a)
{
    Plan P;
    if (make_plan(a, &P)) return 0;
    int maxc = a->c_in;
    for (int l = 0; l < a->n_layers; ++l) maxc = a->layers[l].n_out > maxc ? a->layers[l].n_out : maxc;
    return 2 * sizeof(float) * (size_t)maxc * a->h * a->w * (size_t)(a->batch > 0 ? a->batch : 0);
}

int ccmi_launch_syn_f32(const ccmi_syn_args *a, hipStream_t s)
{
    if (a->n_layers < 1 || a->n_layers > CCMI_MAX_SYN_LAYERS)
        return ccmi_set_error(CCMI_ERR_ARG, "syn: n_layers must be in [1, %d]", CCMI_MAX_SYN_LAYERS);
    int c = a->c_in;
    for (int l = 0; l < a->n_layers; ++l) {
        const ccmi_syn_layer &L = a->layers[l];
        if (L.n_out < 1 || L.ks < 1 || L.ks % 2 == 0)
            return ccmi_set_error(CCMI_ERR_ARG, "syn: layer %d has n_out=%d ks=%d (ks must be odd)", l, L.n_out, L.ks);
        if (L.residual && L.n_out != c)
            return ccmi_set_error(CCMI_ERR_ARG, "syn: residual layer %d needs n_out == n_in", l);
        c = L.n_out;
    }
    Plan P;
    if (make_plan(a, &P)) {
        P.fa.in = a->in;
        P.fa.in_stride = a->in_stride;
        P.fa.params = a->params;
        P.fa.pstride = a->param_stride;
        P.fa.out = a->out;
        P.fa.out_stride = a->out_stride;
        set_runs(P.fa, CCMI_FUSED_RUN);
        dim3 grid((unsigned)(P.fa.ntiles * a->batch));
        if (P.cmid == 3) launch_fused<3, false>(grid, s, P.fa, LevelArgs{});
        else launch_fused<4, false>(grid, s, P.fa, LevelArgs{});
        CCMI_HIP_CHECK(hipGetLastError());
        return CCMI_OK;
    }
    // generic path
    const size_t need = ccmi_syn_workspace_bytes(a);
    if (a->workspace == nullptr || a->workspace_bytes < need)
        return ccmi_set_error(CCMI_ERR_ARG, "syn: workspace of %zu bytes needed for this architecture", need);
    int w_off[CCMI_MAX_SYN_LAYERS], b_off[CCMI_MAX_SYN_LAYERS], cin_of[CCMI_MAX_SYN_LAYERS];
    int64_t tot;
    layer_offsets(a, w_off, b_off, cin_of, &tot);
    int maxc = a->c_in;
    for (int l = 0; l < a->n_layers; ++l) maxc = a->layers[l].n_out > maxc ? a->layers[l].n_out : maxc;
    const int64_t buf_stride = (int64_t)maxc * a->h * a->w;
    float *bufs[2] = {static_cast<float *>(a->workspace), static_cast<float *>(a->workspace) + buf_stride * a->batch};
    const float *src = a->in;
    int64_t src_stride = a->in_stride;
    const int64_t plane = (int64_t)a->h * a->w;
    dim3 grid((unsigned)((plane + kThreads - 1) / kThreads), a->batch);
    for (int l = 0; l < a->n_layers; ++l) {
        const bool last = l == a->n_layers - 1;
        float *dst = last ? a->out : bufs[l & 1];
        const int64_t dst_stride = last ? a->out_stride : buf_stride;
        const ccmi_syn_layer &L = a->layers[l];
        hipLaunchKernelGGL(syn_layer_kernel, grid, dim3(kThreads), 0, s, src, src_stride, cin_of[l], a->h, a->w,
                           a->params, a->param_stride, w_off[l], b_off[l], L.n_out, L.ks, L.residual, L.relu, dst,
                           dst_stride);
        CCMI_HIP_CHECK(hipGetLastError());
        src = dst;
        src_stride = dst_stride;
    }
    return CCMI_OK;
}

int ccmi_launch_post_f32(const ccmi_post_args *a, hipStream_t s)
{
    if (a->bitdepth < 1 || a->bitdepth > 16) return ccmi_set_error(CCMI_ERR_ARG, "post: bitdepth %d", a->bitdepth);
    const int64_t plane = (int64_t)a->h * a->w;
    dim3 grid((unsigned)((plane + kThreads - 1) / kThreads), a->batch);
    hipLaunchKernelGGL(post_kernel, grid, dim3(kThreads), 0, s, a->in, a->in_stride, a->h, a->w,
                       (float)((1 << a->bitdepth) - 1), a->yuv420, a->out, a->out_stride);
    CCMI_HIP_CHECK(hipGetLastError());
    return CCMI_OK;
}

extern "C" int ccmi_decode_forward_f32(const ccmi_decode_args *a, void *stream)
{
    if (!a || !a->out || !a->ups.latent || !a->ups.params || !a->syn.params)
        return ccmi_set_error(CCMI_ERR_ARG, "decode: null argument");
    const ccmi_ups_args &u = a->ups;
    const ccmi_syn_args &y = a->syn;
    if (u.batch < 1 || y.batch != u.batch) return ccmi_set_error(CCMI_ERR_ARG, "decode: batch mismatch");
    if (u.n_grids < 2 || u.n_grids > CCMI_MAX_GRIDS) return ccmi_set_error(CCMI_ERR_ARG, "decode: n_grids");
    if (y.c_in != u.n_grids || y.h != u.h[0] || y.w != u.w[0])
        return ccmi_set_error(CCMI_ERR_ARG, "decode: synthesis input must be the %d x %d x %d upsampled stack", u.n_grids,
                              u.h[0], u.w[0]);
    if (a->bitdepth < 0 || a->bitdepth > 16) return ccmi_set_error(CCMI_ERR_ARG, "decode: bitdepth %d", a->bitdepth);
    if (y.n_layers < 1 || y.n_layers > CCMI_MAX_SYN_LAYERS) return ccmi_set_error(CCMI_ERR_ARG, "decode: n_layers");
    Plan P;
    if (u.ups_k != 8 || u.pre_k != 7 || !make_plan(&y, &P))
        return ccmi_set_error(CCMI_ERR_UNSUPPORTED, "decode: no fused kernel for this architecture");
    if (a->bitdepth > 0 && P.cmid != 3) return ccmi_set_error(CCMI_ERR_ARG, "decode: post-processing needs 3 output planes");
    if (a->head < CCMI_HEAD_DEFAULT || a->head > CCMI_HEAD_GENERIC) return ccmi_set_error(CCMI_ERR_ARG, "decode: head %d", a->head);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int stages = (a->stages & 3) ? a->stages : a->stages | 3;
    // opt-in (stages bit 3): the pyramid's level-2 -> 1 step folded into the fused kernel.  Same
    // values bit for bit, but slower: the folded step's halo and passes cost the VALU-bound kernel
    // more than the HBM-bound pyramid launch it removes (profiles/r6e_*)
    P.fa.head_mfma = a->head == CCMI_HEAD_MFMA;
    P.fa.head_generic = a->head == CCMI_HEAD_GENERIC;
    const bool fold = (stages & 8) && u.n_grids >= 3 && fold_eligible(P.fa, P.cmid);
    LevelArgs last{}, prev{};
    // stages bit 5: the pyramid's levels by ups_level_fixed (the form before the row kernel), for A/B
    // runs and tests
    if (int rc = ups_pyramid(&u, s, &last, (stages & 1) != 0, fold ? &prev : nullptr,
                             (stages & 32) ? CCMI_UPS_FORM_LEVELS : CCMI_UPS_FORM_DEFAULT))
        return rc;
    if (!(stages & 2)) return CCMI_OK;
    if ((int64_t)4 * last.C * last.hs * last.ws >= ((int64_t)1 << 31) || (int64_t)4 * last.hd * last.wd >= ((int64_t)1 << 31))
        return ccmi_set_error(CCMI_ERR_UNSUPPORTED, "decode: level-1 stack of %d x %d x %d exceeds 2 GB buffer addressing", last.C,
                              last.hs, last.ws);
    P.fa.in = nullptr;
    P.fa.params = y.params;
    P.fa.pstride = y.param_stride;
    P.fa.out = a->out;
    P.fa.out_stride = a->out_stride;
    P.fa.qmax = a->bitdepth > 0 ? (float)((1 << a->bitdepth) - 1) : 0.f;
    P.fa.yuv420 = a->yuv420;
    // stages bit 4: single-window runs (the geometry without the walk), for A/B runs and tests
    set_runs(P.fa, (stages & 16) ? 1 : CCMI_FUSED_RUN);
    dim3 grid((unsigned)(P.fa.ntiles * y.batch));
    if (fold) {
        hipLaunchKernelGGL((syn_fused_kernel<7, 3, true, false, 48, true>), grid, dim3(kFThreads), 0, s, P.fa, last, prev);
    } else if (P.cmid == 3) {
        if (!launch_fused_mfma_head<3>(grid, s, P.fa, last)) launch_fused<3, true>(grid, s, P.fa, last);
    } else if (!launch_fused_mfma_head<4>(grid, s, P.fa, last)) {
        launch_fused<4, true>(grid, s, P.fa, last);
    }
    CCMI_HIP_CHECK(hipGetLastError());
    return CCMI_OK;
}

extern "C" int ccmi_fused_run_plan(int h, int n_sp, int cap, int *start, int *windows, int max_runs, int *cap_used)
{
    if (h < 1 || n_sp < 0 || 2 * n_sp >= kRH || max_runs < 0 || (max_runs > 0 && (!start || !windows)))
        return ccmi_set_error(CCMI_ERR_ARG, "run plan: h=%d n_sp=%d max_runs=%d", h, n_sp, max_runs), -1;
    if (cap < 1) cap = CCMI_FUSED_RUN;
    if (n_sp == 0) cap = 1;
    if (cap_used) *cap_used = cap;
    const RunPlan rp = fused_run_plan(h, n_sp, cap, kRH);
    for (int i = 0; i < rp.n_runs && i < max_runs; ++i) {
        start[i] = run_start(rp, i, n_sp, kRH);
        windows[i] = run_windows(rp, i);
    }
    return rp.n_runs;
}

#if defined(CCMI_ARM_STAMPS)
extern "C" int ccmi_debug_fused_stamps(unsigned long long *out, int reset)
{
    if (out) CCMI_HIP_CHECK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_fstamp), sizeof(unsigned long long) * 8));
    if (reset) {
        unsigned long long z[8] = {};
        CCMI_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(g_fstamp), z, sizeof z));
    }
    return CCMI_OK;
}
#endif
