// dec_arm.hip -- path B: the ARM + CABAC kernels of the bit-exact fixed-point .cool decoder
// (the decoder tail -- pyramid, synthesis, blend, output -- is dec_tail.hip).
//
// Compiled with -fwrapv: every accumulation is int32 with two's-complement wrap,
// every right shift of a sum is the reference's truncation toward zero
// (s < 0 ? -((-s) >> p) : s >> p) unless the reference rounds.
//
//  dec_arm_kernel   one wavefront per latent-layer CABAC stream (arm_cpu.cpp:18-106,
//                   cc-bac.h:3-253): raster-order serial decode.  The CABAC state is
//                   wave-uniform (scalar registers); lane o < d owns MLP neuron o; the
//                   4 causal rows live in an LDS ring; same-row contexts come from
//                   registers, so the only per-latent LDS traffic is the above-row
//                   gather.  Many streams (7 per frame x frames) run concurrently.
//  dec_arm_spec_kernel, dec_arm_chain_kernel  the faster forms for d <= 16 (described at
//                   their definitions); launch_dec_arm picks one per (d, nh).
#include <stdlib.h>

#include <algorithm>
#include <type_traits>
#include <utility>

#include "ccmi_cabac.h"
#include "dec_device.h"
#include "dec_internal.h"

namespace ccmi {
namespace {

// ------------------------------------------------------------------ context table
struct CtxPack {
    uint32_t v[17 * 50 * 2];
};
constexpr uint8_t k_ctx_bytes[17 * 50 * 5] = {
#include "ccmi_ctx_table.inc"
};
constexpr CtxPack make_ctx_pack()
{
    CtxPack p{};
    for (int i = 0; i < 17 * 50; ++i) {
        const uint8_t *s = &k_ctx_bytes[i * 5];
        p.v[2 * i] = (uint32_t)s[0] | ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16) | ((uint32_t)s[3] << 24);
        p.v[2 * i + 1] = s[4];
    }
    return p;
}
__constant__ CtxPack c_ctx = make_ctx_pack();

// ------------------------------------------------------------------ device byte source
// The stream is read through a constant-address-space pointer so that the wave-uniform
// word loads become scalar (SMEM) loads; the next word is prefetched one word ahead.
typedef const __attribute__((address_space(4))) uint32_t *const_u32_ptr;

struct DevBytes {
    const_u32_ptr p;
    uint32_t nwords, pos, wi, cur, nxt;
    __device__ __forceinline__ uint32_t ld(uint32_t i) const { return i < nwords ? p[i] : 0u; }
    __device__ __forceinline__ void init(const uint32_t *base, uint32_t nbytes)
    {
        p = (const_u32_ptr)(size_t)base;
        nwords = (nbytes + 3u) >> 2;
        pos = 0;
        wi = 0;
        cur = ld(0);
        nxt = ld(1);
    }
    __device__ __forceinline__ uint32_t next()
    {
        const uint32_t b = (cur >> ((pos & 3u) * 8u)) & 0xFFu;
        ++pos;
        if ((pos & 3u) == 0) {
            cur = nxt;
            ++wi;
            nxt = ld(wi + 1);
        }
        return b;
    }
};

// Sum of v over each DPP row of 16 lanes; the result is valid in lane 15 of the row.
__device__ __forceinline__ int row_sum16(int v)
{
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xF, 0xF, true); // row_shr:1
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xF, 0xF, true); // row_shr:2
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xF, 0xF, true); // row_shr:4
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xF, 0xF, true); // row_shr:8
    return v;
}

// Context pixel (dy, dx) of context index i (cc-frame-decoder.cpp:111-154 order).
template <int D>
__device__ __forceinline__ void ctx_dydx(int i, int &dy, int &dx)
{
    // flattened 9x9 mask index k -> (k/9 - 4, k%9 - 4); same neighbourhoods as the C stride tables
    constexpr signed char k8[8] = {13, 22, 30, 31, 32, 37, 38, 39};
    constexpr signed char k16[16] = {13, 14, 20, 21, 22, 23, 24, 28, 29, 30, 31, 32, 33, 37, 38, 39};
    constexpr signed char k24[24] = {4, 11, 12, 13, 14, 15, 19, 20, 21, 22, 23, 24, 25, 28, 29, 30, 31, 32, 33, 34,
                                     36, 37, 38, 39};
    constexpr signed char k32[32] = {2, 3, 4, 5, 10, 11, 12, 13, 14, 15, 16, 19, 20, 21, 22, 23, 24, 25, 26, 27,
                                     28, 29, 30, 31, 32, 33, 34, 35, 36, 37, 38, 39};
    int k = 40;
    if (i < D) k = D == 8 ? k8[i] : D == 16 ? k16[i] : D == 24 ? k24[i] : k32[i];
    dy = k / 9 - 4;
    dx = k % 9 - 4;
}

constexpr int kRing = 5;   // rows y-4 .. y
constexpr int kRingS = 4;  // speculative kernel (D <= 16: contexts reach row y-3): rows y-3 .. y
constexpr int kPad = 8;    // zero columns either side of a ring row (speculative groups read x+3+4)

// OR of CCMI_ARM_FLAG_* bits into the stream's status word (one lane; a vector global atomic)
__device__ __forceinline__ void put_status(const ArmStreamDesc &S, uint32_t bits)
{
    if (bits && S.status) __hip_atomic_fetch_or(S.status, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One residual hidden layer, lane o = neuron o: (b + 256 a_o + sum_i W[o][i] a_i), ReLU, round >> 8.
template <int D, bool F24>
__device__ __forceinline__ int32_t arm_hidden(const int32_t (&W)[D], int32_t bias, int32_t a)
{
    int32_t acc = bias + a * 256;
#pragma unroll
    for (int i = 0; i < D; ++i) acc += imul<F24>(W[i], __builtin_amdgcn_readlane(a, i));
    return acc < 0 ? 0 : (acc + 128) >> 8;
}

#if defined(CCMI_ARM_STAMPS)
// Diagnostic build only (make stamps): per-stream cycle totals of the decode segments.
#define STAMP(var) const uint64_t var = __builtin_amdgcn_s_memtime()
#define ACC(k, a, b) st_acc[k] += (b) - (a)
#else
#define STAMP(var)
#define ACC(k, a, b)
#endif

template <int D, int NH>
__global__ __launch_bounds__(64) void dec_arm_kernel(const ArmStreamDesc *__restrict__ streams, int pitch)
{
#if defined(CCMI_ARM_STAMPS)
    uint64_t st_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#endif
    extern __shared__ int32_t smem[];
    int32_t *ring = smem;                                              // kRing x pitch
    uint8_t *bmap = reinterpret_cast<uint8_t *>(smem + kRing * pitch); // block sig/flat map

    const ArmStreamDesc S = streams[blockIdx.x];
    const int lane = threadIdx.x;
    const int h = S.h, w = S.w;
    const int rows = S.rows; // the row loops' bound (<= h: a region decode stops early); h sizes the block maps
    // weights fit in 24 signed bits (host check): hidden layers >= 2 and the output layer
    // then use 24-bit multiplies (their inputs are ReLU-rounded sums, < 2^23 by construction)
    const bool w24 = (S.flags & 1) != 0;

#if defined(CCMI_ARM_STAMPS)
    const uint64_t t_begin = __builtin_amdgcn_s_memtime();
#endif
    for (int i = lane; i < kRing * pitch; i += 64) ring[i] = 0;

    // ---- weights: lane owns neuron o = lane % D (lanes >= D duplicate, masked in sums)
    const int o = lane % D;
    int32_t Wh[NH > 0 ? NH : 1][D], Bh[NH > 0 ? NH : 1];
#pragma unroll
    for (int l = 0; l < NH; ++l) {
        const int32_t *base = S.weights + l * (D * D + D);
#pragma unroll
        for (int i = 0; i < D; ++i) Wh[l][i] = base[o * D + i];
        Bh[l] = base[D * D + o];
    }
    const int32_t *ob = S.weights + NH * (D * D + D);
    const int32_t Wo0 = lane < D ? ob[o] : 0, Wo1 = lane < D ? ob[D + o] : 0;
    const int32_t bo0 = __builtin_amdgcn_readfirstlane(ob[2 * D]);
    const int32_t bo1 = __builtin_amdgcn_readfirstlane(ob[2 * D + 1]);

    // ---- CABAC start + block significance / flat maps (BACContext::set_layer, cc-bac.h:24-130)
    Cabac<DevBytes> cab;
    cab.src.init(S.bytes, S.nbytes);
    cab.start();
    const int updated = S.sig_blk < 0;
    const int blk = S.sig_blk < 0 ? -S.sig_blk : S.sig_blk;
    int shift = 0;
    while ((1 << shift) < blk) ++shift;
    const int mask = (1 << shift) - 1;
    int nby = 1, nbx = 1;
    if (blk > 0) {
        nby = (h + blk - 1) >> shift;
        nbx = (w + blk - 1) >> shift;
    }
    const int nblk = nby * nbx;
    for (int i = lane; i < nblk; i += 64) bmap[i] = 1; // bit0 sig, bit1 flat
    __syncthreads();
    if (nblk > 1) {
        if (cab.ep()) {
            Model m;
            m.init(65);
            for (int i = 0; i < nblk; ++i) {
                const uint32_t b = updated ? cab.bin_adaptive(m) : cab.ep();
                if (lane == 0) bmap[i] = (uint8_t)b;
            }
        }
        __syncthreads();
        if (cab.ep()) {
            Model m;
            m.init(65);
            for (int i = 0; i < nblk; ++i) {
                const int sig = __builtin_amdgcn_readfirstlane((int)bmap[i]);
                if (sig) {
                    const uint32_t f = updated ? cab.bin_adaptive(m) : cab.ep();
                    if (lane == 0) bmap[i] = (uint8_t)(sig | (f << 1));
                }
            }
        }
    }
    __syncthreads();

#if defined(CCMI_ARM_STAMPS)
    st_acc[5] = __builtin_amdgcn_s_memtime() - t_begin; // setup incl. block maps
    const uint64_t t_loop = __builtin_amdgcn_s_memtime();
#endif
    // ---- context geometry of this lane (context index = o)
    int cdy, cdx;
    ctx_dydx<D>(o, cdy, cdx);
    const bool same_row = cdy == 0;
    int big = 0; // uniform: a decoded |latent| >= 2^15 was seen -> contexts may exceed 24 bits

    for (int y = 0; y < rows; ++y) {
        int32_t *row = ring + (y % kRing) * pitch + kPad;
        const int32_t *up = ring + ((y + kRing - 1) % kRing) * pitch + kPad;
        const int32_t *crow = ring + ((y + cdy + kRing) % kRing) * pitch + kPad + cdx;
        int32_t r1 = 0, r2 = 0, r3 = 0, r4 = 0; // decoded values at x-1 .. x-4 (this row)
        const int brow = blk > 0 ? (y >> shift) * nbx : 0;
        int bm = 1;
        for (int x = 0; x < w; ++x) {
            int32_t v;
            if (blk > 0 && (x & mask) == 0) bm = __builtin_amdgcn_readfirstlane((int)bmap[brow + (x >> shift)]);
            if (!(bm & 1)) {
                v = 0;
            } else if ((bm & 2) && (x & mask)) {
                v = r1;
            } else if ((bm & 2) && (y & mask)) {
                v = __builtin_amdgcn_readfirstlane(up[x]);
            } else {
                STAMP(t0);
                const int32_t al = crow[x]; // same-row lanes read a stale slot, replaced below
                const int32_t rs = cdx == -1 ? r1 : cdx == -2 ? r2 : cdx == -3 ? r3 : r4;
                int32_t a = same_row ? rs : al;
                const bool f1 = w24 && !big; // contexts (latent << 8) fit in 24 bits
#pragma unroll
                for (int l = 0; l < NH; ++l) {
                    if (l == 0) a = f1 ? arm_hidden<D, true>(Wh[0], Bh[0], a) : arm_hidden<D, false>(Wh[0], Bh[0], a);
                    else a = w24 ? arm_hidden<D, true>(Wh[l], Bh[l], a) : arm_hidden<D, false>(Wh[l], Bh[l], a);
                }
                STAMP(t1);
                const bool fo = NH > 0 ? w24 : f1;
                const int32_t p0 = fo ? imul<true>(Wo0, a) : imul<false>(Wo0, a);
                const int32_t p1 = fo ? imul<true>(Wo1, a) : imul<false>(Wo1, a);
                int32_t s0 = row_sum16(p0), s1 = row_sum16(p1);
                int32_t m0 = __builtin_amdgcn_readlane(s0, 15), m1 = __builtin_amdgcn_readlane(s1, 15);
                if (D > 16) {
                    m0 += __builtin_amdgcn_readlane(s0, 31);
                    m1 += __builtin_amdgcn_readlane(s1, 31);
                }
                m0 += bo0;
                m1 += bo1;
                STAMP(t2);
                const int32_t mu = m0 < 0 ? -((-m0 + 128) >> 8) : (m0 + 128) >> 8;
                const int32_t ls = m1 < 0 ? -((-m1 + 128) >> 8) : (m1 + 128) >> 8;
                // get_val_mu_indicies (cc-contexts.h:20-48)
                const int32_t mr = mu >= 0 ? ((mu + 128) >> 8) << 8 : -(((-mu + 128) >> 8) << 8);
                int32_t mi = (mu - mr) * 16;
                mi = (mi >= 0 ? (mi + 128) >> 8 : -((-mi + 128) >> 8)) + 8;
                const int32_t lsp = ls + 256;
                int32_t si = lsp < 0 ? 0 : (lsp * 5 + 128) >> 8;
                si = si > 49 ? 49 : si;
                const uint32_t ci = (uint32_t)(mi * 50 + si) * 2u;
                const uint32_t st = c_ctx.v[ci], stp = c_ctx.v[ci + 1];
#if defined(CCMI_ARM_STAMPS)
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#endif
                STAMP(t3);
                // decode_single (cc-bac.h:192-231): static contexts
                int32_t val = 0;
                if (cab.bin_static(st & 0xFF)) {
                    if (!cab.bin_static((st >> 8) & 0xFF)) val = 1;
                    else if (!cab.bin_static((st >> 16) & 0xFF)) val = 2;
                    else if (!cab.bin_static(st >> 24)) val = 3;
                    else val = cab.expgolomb(0) + 4;
                    if (cab.bin_static(stp)) val = -val;
                }
                STAMP(t4);
                ACC(0, t0, t1);
                ACC(1, t1, t2);
                ACC(2, t2, t3);
                ACC(3, t3, t4);
#if defined(CCMI_ARM_STAMPS)
                st_acc[4] += 1;
#endif
                const int32_t q = (mr >> 8) + val;
                big |= (q >= 32768 || q <= -32768);
                v = (int32_t)((uint32_t)q << kArmPrec);
            }
            r4 = r3;
            r3 = r2;
            r2 = r1;
            r1 = v;
            if (lane == 0) row[x] = v;
        }
        __syncthreads();
        int32_t *dst = S.out + (int64_t)y * w;
        for (int x = lane; x < w; x += 64) dst[x] = row[x];
        __syncthreads();
    }
    if (lane == 0) put_status(S, (big ? CCMI_ARM_FLAG_BIG : 0u) | (w24 ? 0u : CCMI_ARM_FLAG_W32));
#if defined(CCMI_ARM_STAMPS)
    st_acc[6] = __builtin_amdgcn_s_memtime() - t_loop; // whole latent loop
    if (lane == 0 && S.dbg)
        for (int k = 0; k < 8; ++k) S.dbg[k] = st_acc[k];
#endif
}

// ------------------------------------------------------------------ speculative ARM decode (d <= 16)
// Same stream semantics as dec_arm_kernel, restructured for latency.  The wave's four
// DPP rows (16 lanes each) evaluate the ARM for four consecutive latents x .. x+3 at
// once: row g assumes the latents x .. x+g-1 (not decoded yet) are 0, the most likely
// value.  The CABAC then decodes x, x+1, ... in order and stops at the first latent
// whose decoded value is not 0: every later row was computed from a wrong guess and is
// discarded; all rows up to and including that latent were exact.  Neuron o of row g
// sits in lane 16g + o; the matrix-vector products broadcast a_i inside each row with
// DPP row_newbcast (no SGPR round trip), fused by the compiler into v_mul_i32_i24_dpp.
// The 17 x 50 context table is staged in LDS (one ds_read_b64 per latent instead of a
// scalar load that misses the constant cache).
template <bool F24, int... I>
__device__ __forceinline__ int32_t row_dot(const int32_t (&W)[16], int32_t a, std::integer_sequence<int, I...>)
{
    int32_t acc = 0;
    ((acc += imul<F24>(W[I], __builtin_amdgcn_update_dpp(0, a, 0x150 + I, 0xF, 0xF, false))), ...);
    return acc;
}

template <int D, bool F24>
__device__ __forceinline__ int32_t arm_hidden_rows(const int32_t (&W)[16], int32_t bias, int32_t a)
{
    const int32_t acc = bias + a * 256 + row_dot<F24>(W, a, std::make_integer_sequence<int, D>{});
    return acc < 0 ? 0 : (acc + 128) >> 8;
}

constexpr int kSpec = 4; // latents evaluated per ARM pass (one per DPP row)

template <int D, int NH>
__global__ __launch_bounds__(64) void dec_arm_spec_kernel(const ArmStreamDesc *__restrict__ streams, int pitch)
{
    static_assert(D <= 16, "one neuron per lane of a DPP row");
#if defined(CCMI_ARM_STAMPS)
    // [0] ARM pass (ctx + MLP + output sums)  [1] index + table  [2] CABAC  [3] ARM passes
    // [4] coded latents  [5] setup  [6] latent loop
    uint64_t st_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const uint64_t t_begin = __builtin_amdgcn_s_memtime();
#endif
    extern __shared__ int32_t smem[];
    uint32_t *ctab = reinterpret_cast<uint32_t *>(smem);               // 17 x 50 x 2
    int32_t *ring = smem + 17 * 50 * 2;                                 // kRingS x pitch
    uint8_t *bmap = reinterpret_cast<uint8_t *>(ring + kRingS * pitch); // block sig/flat map

    const ArmStreamDesc S = streams[blockIdx.x];
    const int lane = threadIdx.x;
    const int grp = lane >> 4, o = lane & 15;
    const bool live = o < D;
    const int h = S.h, w = S.w;
    const int rows = S.rows; // the row loops' bound (<= h: a region decode stops early); h sizes the block maps
    const bool w24 = (S.flags & 1) != 0;

    // context table with every static-context index already turned into its model state
    // (Model::init + state(), done once here instead of per bin)
    for (int i = lane; i < 17 * 50 * 2; i += 64) {
        const uint32_t v = c_ctx.v[i];
        uint32_t o = 0;
        for (int k = 0; k < 4; ++k) {
            Model m;
            m.init((int)((v >> (8 * k)) & 0xFF));
            o |= m.state() << (8 * k);
        }
        ctab[i] = (i & 1) ? (o & 0xFF) : o;
    }
    for (int i = lane; i < kRingS * pitch; i += 64) ring[i] = 0;

    int32_t Wh[NH > 0 ? NH : 1][16], Bh[NH > 0 ? NH : 1];
#pragma unroll
    for (int l = 0; l < NH; ++l) {
        const int32_t *base = S.weights + l * (D * D + D);
#pragma unroll
        for (int i = 0; i < 16; ++i) Wh[l][i] = (live && i < D) ? base[o * D + i] : 0;
        Bh[l] = live ? base[D * D + o] : 0;
    }
    const int32_t *ob = S.weights + NH * (D * D + D);
    const int32_t Wo0 = live ? ob[o] : 0, Wo1 = live ? ob[D + o] : 0;
    const int32_t bo0 = __builtin_amdgcn_readfirstlane(ob[2 * D]);
    const int32_t bo1 = __builtin_amdgcn_readfirstlane(ob[2 * D + 1]);

    // ---- CABAC start + block significance / flat maps (BACContext::set_layer, cc-bac.h:24-130)
    Cabac<DevBytes> cab;
    cab.src.init(S.bytes, S.nbytes);
    cab.start();
    const int updated = S.sig_blk < 0;
    const int blk = S.sig_blk < 0 ? -S.sig_blk : S.sig_blk;
    int shift = 0;
    while ((1 << shift) < blk) ++shift;
    const int mask = (1 << shift) - 1;
    int nby = 1, nbx = 1;
    if (blk > 0) {
        nby = (h + blk - 1) >> shift;
        nbx = (w + blk - 1) >> shift;
    }
    const int nblk = nby * nbx;
    for (int i = lane; i < nblk; i += 64) bmap[i] = 1; // bit0 sig, bit1 flat
    __syncthreads();
    if (nblk > 1) {
        if (cab.ep()) {
            Model m;
            m.init(65);
            for (int i = 0; i < nblk; ++i) {
                const uint32_t b = updated ? cab.bin_adaptive(m) : cab.ep();
                if (lane == 0) bmap[i] = (uint8_t)b;
            }
        }
        __syncthreads();
        if (cab.ep()) {
            Model m;
            m.init(65);
            for (int i = 0; i < nblk; ++i) {
                const int sig = __builtin_amdgcn_readfirstlane((int)bmap[i]);
                if (sig) {
                    const uint32_t f = updated ? cab.bin_adaptive(m) : cab.ep();
                    if (lane == 0) bmap[i] = (uint8_t)(sig | (f << 1));
                }
            }
        }
    }
    __syncthreads();

    int cdy, cdx;
    ctx_dydx<D>(o, cdy, cdx);
    const bool same_row = cdy == 0;
    int big = 0;
#if defined(CCMI_ARM_STAMPS)
    st_acc[5] = __builtin_amdgcn_s_memtime() - t_begin;
    const uint64_t t_loop = __builtin_amdgcn_s_memtime();
#endif

    for (int y = 0; y < rows; ++y) {
        int32_t *row = ring + (y % kRingS) * pitch + kPad;
        const int32_t *up = ring + ((y + kRingS - 1) % kRingS) * pitch + kPad;
        const int32_t *crow = ring + ((y + cdy + kRingS) % kRingS) * pitch + kPad + cdx + grp;
        int32_t r1 = 0, r2 = 0, r3 = 0, r4 = 0; // decoded values at x-1 .. x-4 (this row)
        const int brow = blk > 0 ? (y >> shift) * nbx : 0;
        auto push = [&](int32_t v, int x) {
            r4 = r3;
            r3 = r2;
            r2 = r1;
            r1 = v;
            if (lane == 0) row[x] = v;
        };
        // n (>= 1) uncoded columns [x, x+n) written by the lanes in parallel; the last four
        // values are re-read into r1..r4 (they are uniform)
        auto fill = [&](int x, int n, int kind /*0 zero, 1 = r1, 2 = up*/) {
            const int32_t c1 = r1;
            for (int i = lane; i < n; i += 64) row[x + i] = kind == 0 ? 0 : kind == 1 ? c1 : up[x + i];
            if (kind == 2) {
                __builtin_amdgcn_s_waitcnt(0);
                __builtin_amdgcn_wave_barrier();
                auto at = [&](int j) { return __builtin_amdgcn_readfirstlane(row[j]); };
                r4 = n >= 4 ? at(x + n - 4) : n == 3 ? r1 : n == 2 ? r2 : r3;
                r3 = n >= 3 ? at(x + n - 3) : n == 2 ? r1 : r2;
                r2 = n >= 2 ? at(x + n - 2) : r1;
                r1 = at(x + n - 1);
            } else {
                const int32_t v = kind == 0 ? 0 : c1;
                r4 = n >= 4 ? v : n == 3 ? r1 : n == 2 ? r2 : r3;
                r3 = n >= 3 ? v : n == 2 ? r1 : r2;
                r2 = n >= 2 ? v : r1;
                r1 = v;
            }
        };
        int bm = 1, bend = 0; // flags of the current block and its end column
        // above-row context of the next pass, prefetched from LDS before the CABAC of the
        // current one: the next pass starts at x + nd (nd = 1..4 latents decoded)
        int pf_x = -1;
        int32_t pf_a = 0;
        for (int x = 0; x < w;) {
            int L;
            if (blk > 0) {
                if (x >= bend) {
                    bm = __builtin_amdgcn_readfirstlane((int)bmap[brow + (x >> shift)]);
                    bend = min((x | mask) + 1, w);
                }
                if (!(bm & 1)) {
                    fill(x, bend - x, 0);
                    x = bend;
                    continue;
                }
                if (bm & 2) {
                    if (y & mask) {
                        fill(x, bend - x, 2);
                        x = bend;
                        continue;
                    }
                    if (x & mask) {
                        fill(x, bend - x, 1);
                        x = bend;
                        continue;
                    }
                    L = 1; // the coded corner of a flat block
                } else {
                    L = min(kSpec, bend - x);
                }
            } else {
                L = min(kSpec, w - x);
            }
            STAMP(t0);

            // context of lane (g, o): latent x+g, neighbour (cdy, cdx); same-row neighbours
            // at or right of x are the speculative zeros
            const int k = -(grp + cdx); // same row: distance back from x (1..4), <= 0 -> guess
            const int32_t rs = k == 1 ? r1 : k == 2 ? r2 : k == 3 ? r3 : k == 4 ? r4 : 0;
            int32_t a = same_row ? rs : (x == pf_x ? pf_a : crow[x]);
            const bool f1 = w24 && !big;
#pragma unroll
            for (int l = 0; l < NH; ++l) {
                if (l == 0) a = f1 ? arm_hidden_rows<D, true>(Wh[0], Bh[0], a) : arm_hidden_rows<D, false>(Wh[0], Bh[0], a);
                else a = w24 ? arm_hidden_rows<D, true>(Wh[l], Bh[l], a) : arm_hidden_rows<D, false>(Wh[l], Bh[l], a);
            }
            const bool fo = NH > 0 ? w24 : f1;
            const int32_t m_0 = row_sum16(fo ? imul<true>(Wo0, a) : imul<false>(Wo0, a)) + bo0;
            const int32_t m_1 = row_sum16(fo ? imul<true>(Wo1, a) : imul<false>(Wo1, a)) + bo1;
#if defined(CCMI_ARM_STAMPS)
            __builtin_amdgcn_s_waitcnt(0);
#endif
            STAMP(t1);
            // mu / scale -> context-table entry, in every lane at once (lane 16g+15 holds
            // row g's sums; the other lanes compute harmless in-range garbage)
            const int32_t mu = m_0 < 0 ? -((-m_0 + 128) >> 8) : (m_0 + 128) >> 8;
            const int32_t ls = m_1 < 0 ? -((-m_1 + 128) >> 8) : (m_1 + 128) >> 8;
            // get_val_mu_indicies (cc-contexts.h:20-48)
            const int32_t mr = mu >= 0 ? ((mu + 128) >> 8) << 8 : -(((-mu + 128) >> 8) << 8);
            int32_t mi = (mu - mr) * 16;
            mi = (mi >= 0 ? (mi + 128) >> 8 : -((-mi + 128) >> 8)) + 8;
            const int32_t lsp = ls + 256;
            int32_t si = lsp < 0 ? 0 : (lsp * 5 + 128) >> 8;
            si = si > 49 ? 49 : si;
            const uint2 e = *reinterpret_cast<const uint2 *>(ctab + (uint32_t)(mi * 50 + si) * 2u);
            const int32_t mq = mr >> 8;
            const int32_t pf1 = crow[x + 1], pf2 = crow[x + 2], pf3 = crow[x + 3], pf4 = crow[x + 4];
            STAMP(t2);
            // decode_single (cc-bac.h:192-231), in order, until the first non-zero latent
            int nd = 0;
#pragma unroll 1
            for (int j = 0; j < L; ++j) {
                const int src_lane = 16 * j + 15;
                const uint32_t st = __builtin_amdgcn_readlane(e.x, src_lane);
                const uint32_t stp = __builtin_amdgcn_readlane(e.y, src_lane);
                int32_t val = 0;
                if (cab.bin_state(st & 0xFF)) {
                    if (!cab.bin_state((st >> 8) & 0xFF)) val = 1;
                    else if (!cab.bin_state((st >> 16) & 0xFF)) val = 2;
                    else if (!cab.bin_state(st >> 24)) val = 3;
                    else val = cab.expgolomb(0) + 4;
                    if (cab.bin_state(stp)) val = -val;
                }
                const int32_t q = __builtin_amdgcn_readlane(mq, src_lane) + val;
                big |= (q >= 32768 || q <= -32768);
                push((int32_t)((uint32_t)q << kArmPrec), x + j);
                ++nd;
                if (q != 0) break;
            }
            STAMP(t3);
            ACC(0, t0, t1);
            ACC(1, t1, t2);
            ACC(2, t2, t3);
#if defined(CCMI_ARM_STAMPS)
            st_acc[3] += 1;
            st_acc[4] += nd;
#endif
            x += nd;
            pf_x = x;
            pf_a = nd == 1 ? pf1 : nd == 2 ? pf2 : nd == 3 ? pf3 : pf4;
        }
        __syncthreads();
        int32_t *dst = S.out + (int64_t)y * w;
        for (int x = lane; x < w; x += 64) dst[x] = row[x];
        __syncthreads();
    }
    if (lane == 0) put_status(S, (big ? CCMI_ARM_FLAG_BIG : 0u) | (w24 ? 0u : CCMI_ARM_FLAG_W32));
#if defined(CCMI_ARM_STAMPS)
    st_acc[6] = __builtin_amdgcn_s_memtime() - t_loop;
    if (lane == 0 && S.dbg)
        for (int k = 0; k < 8; ++k) S.dbg[k] = st_acc[k];
#endif
}

// ------------------------------------------------------------------ chain kernel support
constexpr int kDS = 3; // same-row contexts (0, -3), (0, -2), (0, -1): the last three context indices

// Byte source of the chain kernel: the stream's words come through wave-uniform VECTOR
// loads issued one word ahead (the scalar-load reader's fetch is counted in lgkmcnt with
// the LDS reads, so every LDS wait of a pass also waited for it).  Word indices clamp to the
// zero padding after the stream (>= 64 bytes, dec_host.cpp), which reads as zeros.
struct DevBytesV {
    typedef const __attribute__((address_space(1))) uint32_t *gptr; // global, not flat: vmcnt only
    gptr p;
    uint32_t lim, pos, wi, cur;
    int32_t vnext; // word wi + 1, in a VGPR (possibly still in flight)
    __device__ __forceinline__ int32_t fetch(uint32_t i) const
    {
        int vi = (int)(i < lim ? i : lim);
        asm volatile("" : "+v"(vi)); // a vector load
        return (int32_t)p[vi];
    }
    __device__ __forceinline__ void init(const uint32_t *base, uint32_t nbytes)
    {
        p = (gptr)(size_t)base;
        lim = ((nbytes + 3u) >> 2) + 8u;
        pos = 0;
        wi = 0;
        cur = (uint32_t)__builtin_amdgcn_readfirstlane(fetch(0));
        vnext = fetch(1);
    }
    __device__ __forceinline__ uint32_t next()
    {
        const uint32_t b = (cur >> ((pos & 3u) * 8u)) & 0xFFu;
        ++pos;
        if ((pos & 3u) == 0) {
            cur = (uint32_t)__builtin_amdgcn_readfirstlane(vnext);
            ++wi;
            vnext = fetch(wi + 1);
        }
        return b;
    }
};

// ------------------------------------------------------------------ chain kernel (d <= 16, >= 1 hidden layer)
// The serial decode chain of one latent-layer stream, built around what one wavefront can
// issue (one instruction per ~4 cycles, SALU and VALU alike): every instruction on the chain
// is one the decode needs.  Speculation as in round 3 (DPP row g evaluates latent x + g,
// its undecoded same-row neighbours guessed equal to the latent above) with:
//  * layer 0 in GUESS-ERROR form: the chunk precompute folds the above-row contexts AND the
//    guessed same-row contexts (the latents above, up[x - 3 .. x - 1]) into one sum per latent
//    and neuron, preG; a pass adds C1 e1 + C2 e2 + C3 e3, where e_j = (decoded - guessed value)
//    of latent x - j (wave-uniform, SGPR) and C_j the per-lane constant weight of that context
//    for the lane's row (0 when the row guessed it).  Exact: int32 sums wrap identically in any
//    order (-fwrapv) and the reference rounds once per layer (arm_cpu.cpp:65-80);
//  * coded RUNS: the block map is turned into runs of coded latents once per run (lanes read
//    the block flags, one ballot), so a pass's only control flow is its CABAC;
//  * the next pass's inputs read ahead at constant LDS offsets: the preG ring (two 64-latent
//    chunks) mirrors its first 8 entries after its end, so latents x + 1 .. x + 7 never wrap;
//  * decoded values collected in a VGPR (v_writelane) and stored 60 at a time;
//  * the CABAC state left-aligned (range << 23, value << 16): the renormalisation shift of
//    both outcomes is one s_flbit of the new range; the five static bin codes of a context
//    (4 unary bins + sign, 6 bits each) in one LDS word;
//  * the multiply forms (24-bit / 32-bit) as instantiations of the pass loop, switched at a
//    pass boundary when a decoded latent leaves the 24-bit range.
constexpr int kPreRing = 256; // four 64-latent chunks of preG (ring slot = chunk sequence number & 3)
constexpr int kPreMir = 8;    // ring entries [0, 8) mirrored at [256, 264)
constexpr uint32_t kQ24 = 16383; // |q| <= kQ24 keeps contexts and guess errors inside 24 signed bits

// 6-bit code of a static context's model state st: bit 5 the MPS, bits 0..4 the LPS class
// ((st or its complement) >> 2; TDecBinCABAC::decodeBin's LPS-range index)
__host__ __device__ constexpr uint32_t code6(uint32_t st)
{
    return ((st >> 7) << 5) | ((((st >> 7) ? st ^ 0xFFu : st) & 0xFFu) >> 2);
}

struct Cab6 {
    DevBytesV src;
    uint32_t R, V; // TDecBinCABAC's m_uiRange << 23 and m_uiValue << 16
    int32_t bn;    // bits_needed
    __device__ __forceinline__ void from(const Cabac<DevBytesV> &c)
    {
        src = c.src;
        R = c.range << 23;
        V = c.value << 16;
        bn = c.bits_needed;
    }
    __device__ __forceinline__ void to(Cabac<DevBytesV> &c) const
    {
        c.src = src;
        c.range = R >> 23;
        c.value = V >> 16;
        c.bits_needed = bn;
    }
};

// One bin of a static context, k-th 6-bit code of the word st (TDecBinCABAC::decodeBin):
// LPS iff value >= (range - lps) << 7; after either outcome the new range is renormalised to
// [256, 511) by one left shift of clz(range << 23) (1 or 0 after an MPS, clz(lps) - 23 after an
// LPS, = the reference's renorm table for lps in [4, 236]).
template <int K>
__device__ __forceinline__ uint32_t bin6(Cab6 &c, uint32_t st)
{
    const uint32_t q5 = (st >> (6 * K)) & 31u, mps = (st >> (6 * K + 5)) & 1u;
    uint32_t R = c.R, V = c.V, t, lps, rm, nb, lp;
    asm("s_lshr_b32 %[t], %[R], 28\n\t"
        "s_mul_i32 %[t], %[t], %[q5]\n\t"
        "s_lshr_b32 %[t], %[t], 1\n\t"
        "s_add_u32 %[t], %[t], 4\n\t"
        "s_lshl_b32 %[lps], %[t], 23\n\t"
        "s_sub_u32 %[rm], %[R], %[lps]\n\t"
        "s_cmp_ge_u32 %[V], %[rm]\n\t"
        "s_cselect_b32 %[R], %[lps], %[rm]\n\t"
        "s_cselect_b32 %[t], %[rm], 0\n\t"
        "s_cselect_b32 %[lp], 1, 0\n\t"
        "s_sub_u32 %[V], %[V], %[t]\n\t"
        "s_flbit_i32_b32 %[nb], %[R]\n\t"
        "s_lshl_b32 %[R], %[R], %[nb]\n\t"
        "s_lshl_b32 %[V], %[V], %[nb]"
        : [R] "+s"(R), [V] "+s"(V), [t] "=&s"(t), [lps] "=&s"(lps), [rm] "=&s"(rm), [nb] "=&s"(nb), [lp] "=&s"(lp)
        : [q5] "s"(q5)
        : "scc");
    c.R = R;
    c.V = V;
    c.bn += (int32_t)nb;
    if (__builtin_expect(c.bn >= 0, 0)) { // the byte refill off the fall-through path
        c.V += c.src.next() << (c.bn + 16);
        c.bn -= 8;
    }
    return lp ^ mps;
}

// decode_single (cc-bac.h:192-231) with the static codes of one context
__device__ __forceinline__ int32_t decode_val(Cab6 &c, uint32_t st)
{
    int32_t val = 0;
    if (bin6<0>(c, st)) {
        if (!bin6<1>(c, st)) val = 1;
        else if (!bin6<2>(c, st)) val = 2;
        else if (!bin6<3>(c, st)) val = 3;
        else {
            Cabac<DevBytesV> t;
            c.to(t);
            val = t.expgolomb(0) + 4;
            c.from(t);
        }
        if (bin6<4>(c, st)) val = -val;
    }
    return val;
}

// ReLU + rounding of a hidden layer, arm_cpu.cpp:76-81 as written (a sum within 127 of INT_MAX
// wraps negative there too)
// v_writelane_b32 (no clang builtin in this toolchain: the LLVM intrinsic by its asm label)
extern "C" __device__ int32_t ccmi_writelane(int32_t v, int32_t lane, int32_t old) __asm("llvm.amdgcn.writelane.i32");

__device__ __forceinline__ int32_t relu_rnd8(int32_t acc) { return acc < 0 ? 0 : (acc + 128) >> 8; }

template <int D, int NH>
__global__ __launch_bounds__(128) void dec_arm_chain_kernel(const ArmStreamDesc *__restrict__ streams, int pitch)
{
    static_assert(D <= 16 && D > kDS && NH >= 1, "one neuron per lane of a DPP row, >= 1 hidden layer");
    constexpr int DA = D - kDS; // above-row contexts
#if defined(CCMI_ARM_STAMPS)
    // chain wave: [0] ARM + index (to the table read)  [1] table wait  [2] CABAC  [3] passes
    // [4] coded latents  [5] setup  [6] latent loop  [7] waits for the helper's preG
    // [8] run starts (fills, block scan)  [9] row copy-out  [10] runs  [11] after the CABAC
    // helper wave (lanes 12..15 of the dump): [12] busy (chunk precompute)  [13] chunks computed
    // [14] chunks skipped (no coded latent)  [15] waiting
    uint32_t st_v = 0;
#define LACC(k, d) st_v += (lane == (k)) ? (uint32_t)(d) : 0u
#define CSTAMP(var) const uint64_t var = __builtin_amdgcn_s_memtime()
    const uint64_t t_begin = __builtin_amdgcn_s_memtime();
#else
#define LACC(k, d)
#define CSTAMP(var)
#endif
    extern __shared__ int32_t smem[];
    int32_t *ctl = smem;                                                // [0] ready seq [1] chain seq [2] done
    uint32_t *ctab = reinterpret_cast<uint32_t *>(smem + 4);            // 17 x 50 packed bin codes
    int32_t *w0s = smem + 4 + 17 * 50 + 2;                              // [16][16] layer-0 weights, [16] biases (16 B aligned)
    int32_t *pre = w0s + 16 * 16 + 16;                                  // [kPreRing + kPreMir][16] preG
    int32_t *ring = pre + (kPreRing + kPreMir) * 16;                    // kRingS x pitch
    uint8_t *bmap = reinterpret_cast<uint8_t *>(ring + kRingS * pitch); // block sig/flat map

    const ArmStreamDesc S = streams[blockIdx.x];
    const int tid = threadIdx.x, wid = tid >> 6, lane = tid & 63;
    const int grp = lane >> 4, o = lane & 15;
    const bool live = o < D;
    const int h = S.h, w = S.w;
    const int rows = S.rows; // the row loops' bound (<= h: a region decode stops early); h sizes the block maps
    const bool w24 = (S.flags & 1) != 0;
    const int nch = (w + 63) >> 6; // 64-latent chunks per row

    for (int i = tid; i < 17 * 50; i += 128) {
        const uint32_t v = c_ctx.v[2 * i], vs = c_ctx.v[2 * i + 1];
        uint32_t e = 0;
        for (int k = 0; k < 4; ++k) {
            Model m;
            m.init((int)((v >> (8 * k)) & 0xFF));
            e |= code6(m.state()) << (6 * k);
        }
        Model m;
        m.init((int)(vs & 0xFF));
        ctab[i] = e | (code6(m.state()) << 24);
    }
    for (int i = tid; i < kRingS * pitch; i += 128) ring[i] = 0;
    for (int i = tid; i < 16 * 16 + 16; i += 128) {
        const int r = i >> 4, cc = i & 15;
        w0s[i] = i < 256 ? (r < D && cc < D ? S.weights[r * D + cc] : 0) : (cc < D ? S.weights[D * D + cc] : 0);
    }
    if (tid < 4) ctl[tid] = 0;

    // ---- CABAC start + block significance / flat maps (BACContext::set_layer, cc-bac.h:24-130);
    // both waves run it (the map is written by thread 0), the chain wave keeps the CABAC state
    Cabac<DevBytesV> cab0;
    cab0.src.init(S.bytes, S.nbytes);
    cab0.start();
    const int updated = S.sig_blk < 0;
    const int blk = S.sig_blk < 0 ? -S.sig_blk : S.sig_blk;
    int shift = 0;
    while ((1 << shift) < blk) ++shift;
    const int mask = (1 << shift) - 1;
    int nby = 1, nbx = 1;
    if (blk > 0) {
        nby = (h + blk - 1) >> shift;
        nbx = (w + blk - 1) >> shift;
    }
    const int nblk = nby * nbx;
    for (int i = tid; i < nblk; i += 128) bmap[i] = 1; // bit0 sig, bit1 flat
    __syncthreads();
    if (nblk > 1) {
        if (cab0.ep()) {
            Model m;
            m.init(65);
            for (int i = 0; i < nblk; ++i) {
                const uint32_t b = updated ? cab0.bin_adaptive(m) : cab0.ep();
                if (tid == 0) bmap[i] = (uint8_t)b;
            }
        }
        __syncthreads();
        if (cab0.ep()) {
            Model m;
            m.init(65);
            for (int i = 0; i < nblk; ++i) {
                const int sig = __builtin_amdgcn_readfirstlane((int)bmap[i]);
                if (sig) {
                    const uint32_t f = updated ? cab0.bin_adaptive(m) : cab0.ep();
                    if (tid == 0) bmap[i] = (uint8_t)(sig | (f << 1));
                }
            }
        }
    }
    __syncthreads();
    auto lds_order = []() __attribute__((always_inline)) { // this wave's LDS stores before its later loads
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    };
    // the two waves' hand-off words: a workgroup-scope release store publishes everything the
    // wave wrote before it (every lane's stores: lds_order() first), an acquire load orders the
    // reader's later LDS loads (the preG slots, the ring rows) behind the word it saw
    auto ctl_get = [ctl](int k) __attribute__((always_inline)) {
        return __builtin_amdgcn_readfirstlane(__hip_atomic_load(ctl + k, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP));
    };
    auto ctl_put = [ctl, tid](int k, int32_t v) __attribute__((always_inline)) {
        if ((tid & 63) == 0) __hip_atomic_store(ctl + k, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
    };
    const int spin_cap = S.spin_cap;

    if (wid == 1) {
        // ================= helper wave: preG of every chunk with a coded latent, in (row, chunk)
        // order, into ring slot seq & 3 (4 slots + the mirror of slot 0's first 8 entries), as
        // soon as (a) the chain wave has left the chunk that held the slot (chain seq >= seq - 3)
        // and (b) the row above is final under the chunk's contexts (done >= its last column)
        const int dmax = blk > 0 ? 0 : 1; // no block map: every latent coded
        int seq = 0;
        uint32_t hbits = 0;
        for (int y = 0; y < rows; ++y) {
            const int brow = blk > 0 ? (y >> shift) * nbx : 0;
            for (int c = 0; c < nch; ++c, ++seq) {
                CSTAMP(tw0);
                // is any latent of [64 c, 64 c + 64) coded (the ARM evaluated there)?
                bool coded = dmax != 0;
                if (!coded) {
                    const int b0 = (c * 64) >> shift, b1 = (min(c * 64 + 64, w) - 1) >> shift;
                    const int bb = b0 + lane;
                    const int f = bb <= b1 ? (int)bmap[brow + bb] : 0;
                    // sig and not flat: every latent; sig and flat: the corner, in the block's first row
                    coded = __ballot(bb <= b1 && (f == 1 || (f == 3 && !(y & mask)))) != 0;
                }
                const int need = y == 0 ? 0 : (y - 1) * w + min(c * 64 + 66, w);
                // bounded, so that a lost hand-off ends in a wave that retires and a status word
                // the host turns into an error (CCMI_ARM_FLAG_TIMEOUT), never in a hang
                bool ok = false;
                for (int spin = 0; spin < spin_cap; ++spin) {
                    if (ctl_get(1) >= seq - 3 && ctl_get(2) >= need) {
                        ok = true;
                        break;
                    }
                    __builtin_amdgcn_s_sleep(1);
                }
                if (!ok) hbits |= CCMI_ARM_FLAG_TIMEOUT;
                CSTAMP(tw1);
                LACC(15, tw1 - tw0);
                if (coded) {
                    const int slot = seq & 3;
                    const int xx = min(c * 64 + lane, w - 1); // lanes past the row end: a copy nobody reads
                    const int32_t *up = ring + ((y + 3) & 3) * pitch + kPad;
                    int32_t ctx[D];
#pragma unroll
                    for (int i = 0; i < DA; ++i) {
                        int dy, dx;
                        ctx_dydx<D>(i, dy, dx);
                        ctx[i] = ring[((y + dy) & 3) * pitch + kPad + xx + dx];
                    }
#pragma unroll
                    for (int j = 0; j < kDS; ++j) ctx[DA + j] = up[xx - kDS + j]; // the guesses
                    // 24-bit products when the weights and every context fit (|v| < 2^22)
                    bool small = w24;
#pragma unroll
                    for (int i = 0; i < D; ++i) small = small && (uint32_t)(ctx[i] + (1 << 22)) < (1u << 23);
                    const bool f24 = __ballot(!small) == 0;
                    if (!f24) hbits |= CCMI_ARM_FLAG_PRE32;
                    int32_t *dst = pre + (slot * 64 + lane) * 16;
                    int32_t *mir = pre + (kPreRing + lane) * 16;
                    auto sums = [&](auto F24) __attribute__((always_inline)) {
                        constexpr bool fz = decltype(F24)::value;
#pragma unroll
                        for (int n = 0; n < 16; n += 4) {
                            int32_t acc[4];
#pragma unroll
                            for (int q = 0; q < 4; ++q) {
                                const int nn = n + q;
                                if (nn >= D) {
                                    acc[q] = 0;
                                    continue;
                                }
                                int32_t a = w0s[256 + nn] + ctx[nn] * 256; // bias + own residual
                                const int4 *wr = reinterpret_cast<const int4 *>(w0s + 16 * nn);
#pragma unroll
                                for (int i4 = 0; i4 < (D + 3) / 4; ++i4) {
                                    const int4 wv = wr[i4];
                                    const int32_t wk[4] = {wv.x, wv.y, wv.z, wv.w};
#pragma unroll
                                    for (int k = 0; k < 4; ++k)
                                        if (4 * i4 + k < D) a += imul<fz>(wk[k], ctx[4 * i4 + k]);
                                }
                                acc[q] = a;
                            }
                            const int4 v4{acc[0], acc[1], acc[2], acc[3]};
                            *reinterpret_cast<int4 *>(dst + n) = v4;
                            if (slot == 0 && lane < kPreMir) *reinterpret_cast<int4 *>(mir + n) = v4;
                        }
                    };
                    if (f24) sums(std::true_type{});
                    else sums(std::false_type{});
                    LACC(13, 1);
                } else {
                    LACC(14, 1);
                }
                lds_order();
                ctl_put(0, seq + 1);
                CSTAMP(tw2);
                LACC(12, tw2 - tw1);
            }
        }
        if (lane == 0) put_status(S, hbits);
#if defined(CCMI_ARM_STAMPS)
        if (lane >= 12 && lane < 16 && S.dbg) S.dbg[lane] = st_v;
#endif
        return;
    }

    // ================= chain wave
    // guess-error coefficients: latent x - j is a decoded (not guessed) neighbour of row g's
    // latent x + g iff g + j <= 3, at context dx = -(g + j), index DA + 3 - (g + j); the weight
    // carries the neuron's own residual when that index is its own
    int32_t C1, C2, C3;
    {
        int32_t Ws[kDS];
#pragma unroll
        for (int j = 0; j < kDS; ++j) Ws[j] = live ? S.weights[o * D + DA + j] + (o == DA + j ? 256 : 0) : 0;
        C1 = grp == 0 ? Ws[2] : grp == 1 ? Ws[1] : grp == 2 ? Ws[0] : 0;
        C2 = grp == 0 ? Ws[1] : grp == 1 ? Ws[0] : 0;
        C3 = grp == 0 ? Ws[0] : 0;
    }
    int32_t Wh[NH][16], Bh[NH];
#pragma unroll
    for (int l = 1; l < NH; ++l) {
        const int32_t *base = S.weights + l * (D * D + D);
#pragma unroll
        for (int i = 0; i < 16; ++i) Wh[l][i] = (live && i < D) ? base[o * D + i] : 0;
        Bh[l] = live ? base[D * D + o] : 0;
    }
    const int32_t *ob = S.weights + NH * (D * D + D);
    const int32_t Wo0 = live ? ob[o] : 0, Wo1 = live ? ob[D + o] : 0;
    // the output biases ride in neuron 0's product (the row sums add them once)
    const int32_t Bo0 = o == 0 ? ob[2 * D] : 0, Bo1 = o == 0 ? ob[2 * D + 1] : 0;
    Cab6 cab;
    cab.from(cab0);

    // 24-bit guard: max over the decoded q of (q + kQ24) as unsigned, < 2 kQ24 + 1 while every
    // |q| <= kQ24 (contexts < 2^22, guess errors < 2^23)
    uint32_t qspan = 0;
    // 0: 24-bit layer 0 + 24-bit hidden / output layers; 1: 32-bit layer 0; 2: all 32-bit
    int mode = w24 ? 0 : 2;
    uint32_t cbits = 0;
#if defined(CCMI_ARM_STAMPS)
    LACC(5, __builtin_amdgcn_s_memtime() - t_begin);
    const uint64_t t_loop = __builtin_amdgcn_s_memtime();
#endif

    for (int y = 0; y < rows; ++y) {
        int32_t *row = ring + (y & 3) * pitch + kPad;
        const int32_t *up = ring + ((y + 3) & 3) * pitch + kPad;
        const int brow = blk > 0 ? (y >> shift) * nbx : 0;
        const int rseq = y * nch;            // chunk sequence number of (y, 0)
        const int rring = (rseq * 64) & 255; // preG ring index of latent (y, 0); latent x at (rring + x) & 255
        int pre_lim = 0;         // a pass at x needs x + 8 <= pre_lim (INT_MAX once the row is covered)
        int32_t vrow = 0;        // lane i < x - xb: decoded value of latent xb + i, not stored yet
        int xb = 0;
        int32_t e1 = 0, e2 = 0, e3 = 0; // guess errors of latents x - 1, x - 2, x - 3
        int32_t pfa = 0;         // preG of this lane's latent x + grp, neuron o
        int32_t upv = 0;         // lane i < 8: up[x - ub + i]
        int ub = 0;
        int x = 0;

        // stores the collected values and publishes the row's progress (the helper's
        // chunks of row y + 1 read this row)
        auto flush = [&]() __attribute__((always_inline)) {
            if (lane < x - xb) row[xb + lane] = vrow;
            xb = x;
            lds_order();
            ctl_put(2, y * w + x);
        };
        // preG for latents up to x + 7: publish the chain's chunk (frees the slots before it) and
        // wait for the helper
        auto wait_pre = [&]() __attribute__((always_inline)) {
            CSTAMP(tq0);
            const int need = (min(x + 8, w) - 1) >> 6;
            ctl_put(1, rseq + (x >> 6));
            bool ok = false;
            for (int spin = 0; spin < spin_cap; ++spin) { // bounded, as the helper's wait
                if (ctl_get(0) > rseq + need) {
                    ok = true;
                    break;
                }
                __builtin_amdgcn_s_sleep(1);
            }
            if (!ok) cbits |= CCMI_ARM_FLAG_TIMEOUT;
            pre_lim = (need + 1) * 64 >= w ? 0x7FFFFFFF : (need + 1) * 64;
            CSTAMP(tq1);
            LACC(7, tq1 - tq0);
        };

        // one mode's pass loop over the current run [x, cend): returns at the run end, when the
        // next pass needs preG not waited for yet or a flush of vrow, or when the 24-bit guard
        // trips (mode 0 only); one compare per pass against the bound of all three
        auto passes = [&](int cend, auto F1, auto FW) __attribute__((always_inline)) {
            constexpr bool f1 = decltype(F1)::value, fw = decltype(FW)::value;
            const int stop = min(min(cend, pre_lim - 7), xb + 61);
            while (x < stop) {
                CSTAMP(t0);
                // ---- ARM of latents x .. x + 3 (row g = latent x + g)
                int32_t a = relu_rnd8(pfa + imul<f1>(C1, e1) + imul<f1>(C2, e2) + imul<f1>(C3, e3));
#pragma unroll
                for (int l = 1; l < NH; ++l)
                    a = relu_rnd8(Bh[l] + a * 256 + row_dot<fw>(Wh[l], a, std::make_integer_sequence<int, D>{}));
                const int32_t m0 = row_sum16(imul<fw>(Wo0, a) + Bo0), m1 = row_sum16(imul<fw>(Wo1, a) + Bo1);
                // ---- mu / scale -> context-table entry (lane 16 g + 15 holds row g's sums).  The
                // reference's symmetric rounding m < 0 ? -((-m + 128) >> 8) : (m + 128) >> 8 equals
                // (m + 128 + (m >> 31)) >> 8 (|m| < 2^31 - 128), get_val_mu_indicies cc-contexts.h:20-48
                auto rnd8 = [](int32_t m) __attribute__((always_inline)) { return (m + 128 + (m >> 31)) >> 8; };
                const int32_t mu = rnd8(m0), ls = rnd8(m1);
                const int32_t mr = (mu + 128 + (mu >> 31)) & ~255; // rnd8(mu) << 8
                const int32_t mi = rnd8((mu - mr) * 16) + 8;       // [0, 16]
                const int32_t si = min(max((ls * 5 + 1408) >> 8, 0), 49);
                const uint32_t ent = ctab[__mul24(mi, 50) + si];
                const int32_t mq = mr >> 8;
                // ---- the next pass's inputs, read ahead (it starts at x + nd, nd = 1 .. 4)
                const int32_t *pp = pre + (((rring + x) & (kPreRing - 1)) + grp) * 16 + o;
                const int32_t nx0 = pp[16], nx1 = pp[32], nx2 = pp[48], nx3 = pp[64];
                const int32_t upn = up[x + (lane & 7)];
                CSTAMP(t1);
#if defined(CCMI_ARM_STAMPS)
                __builtin_amdgcn_s_waitcnt(0xc07f); // lgkmcnt(0): the table entry
#endif
                CSTAMP(t2);
                // ---- CABAC, in order, until a latent differs from its guess or the run ends
                const int lim = min(cend - x, 4);
                int nd = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint32_t st = (uint32_t)__builtin_amdgcn_readlane((int)ent, 16 * j + 15);
                    const int32_t q = __builtin_amdgcn_readlane(mq, 16 * j + 15) + decode_val(cab, st);
                    const int32_t g = __builtin_amdgcn_readlane(upv, ub + j);
                    if (f1) qspan = max(qspan, (uint32_t)(q + (int32_t)kQ24));
                    const int32_t v = (int32_t)((uint32_t)q << kArmPrec);
                    vrow = ccmi_writelane(v, x - xb + j, vrow);
                    e3 = e2;
                    e2 = e1;
                    e1 = v - g;
                    pfa = j == 0 ? nx0 : j == 1 ? nx1 : j == 2 ? nx2 : nx3;
                    nd = j + 1;
                    if (e1 != 0 || j + 1 >= lim) break;
                }
                CSTAMP(t3);
                x += nd;
                ub = nd;
                upv = upn;
                CSTAMP(t4);
                LACC(0, t1 - t0);
                LACC(1, t2 - t1);
                LACC(2, t3 - t2);
                LACC(3, 1);
                LACC(4, nd);
                LACC(11, t4 - t3);
                if (f1 && qspan > 2 * kQ24) return;
            }
        };

        while (x < w) {
            CSTAMP(tr0);
            // ---- the run of coded latents starting at x (uncoded blocks before it filled)
            int cend = w;
            if (blk > 0) {
                const int bx = x >> shift;
                const int bm = __builtin_amdgcn_readfirstlane((int)bmap[brow + bx]);
                const int bend = min((x | mask) + 1, w);
                const bool flat = (bm & 2) != 0;
                if (!(bm & 1) || (flat && ((y & mask) || (x & mask)))) {
                    // zero block, flat block below its first row (copy of the row above), or the
                    // rest of a flat block's first row (copy of its decoded corner)
                    flush();
                    const int kind = !(bm & 1) ? 0 : (y & mask) ? 2 : 1;
                    const int32_t c1 = kind == 1 ? __builtin_amdgcn_readfirstlane(row[x - 1]) : 0;
                    for (int i = lane; i < bend - x; i += 64) row[x + i] = kind == 0 ? 0 : kind == 1 ? c1 : up[x + i];
                    x = bend;
                    xb = x;
                    flush(); // nothing to store: publishes the filled block
                    LACC(8, __builtin_amdgcn_s_memtime() - tr0);
                    continue;
                }
                if (flat) {
                    cend = x + 1; // the coded corner of a flat block
                } else {
                    // consecutive coded, non-flat blocks: the first other block ends the run
                    int b = bx + 1;
                    while (b < nbx) {
                        const int bb = b + lane;
                        const int f = bb < nbx ? (int)bmap[brow + bb] : 0;
                        const uint64_t stop = __ballot(bb < nbx && f != 1);
                        if (stop) {
                            b += __builtin_ctzll(stop);
                            break;
                        }
                        b += 64;
                    }
                    cend = min(b << shift, w);
                }
            }
            // run start: guess errors of latents x - 1 .. x - 3 from the stored row (fills)
            flush();
            {
                const int32_t d = lane < kDS ? row[x - 1 - lane] - up[x - 1 - lane] : 0;
                e1 = __builtin_amdgcn_readlane(d, 0);
                e2 = __builtin_amdgcn_readlane(d, 1);
                e3 = __builtin_amdgcn_readlane(d, 2);
            }
            if (x + 8 > pre_lim) wait_pre();
            pfa = pre[(((rring + x) & (kPreRing - 1)) + grp) * 16 + o];
            upv = up[x + (lane & 7)];
            ub = 0;
            LACC(8, __builtin_amdgcn_s_memtime() - tr0);
            LACC(10, 1);
            while (x < cend) {
                if (x + 8 > pre_lim) wait_pre();
                if (x - xb > 60) flush();
                if (mode == 0) {
                    passes(cend, std::true_type{}, std::true_type{});
                    if (qspan > 2 * kQ24) mode = 1;
                } else if (mode == 1) {
                    passes(cend, std::false_type{}, std::true_type{});
                } else {
                    passes(cend, std::false_type{}, std::false_type{});
                }
            }
        }
        CSTAMP(tw0);
        flush(); // done = (y + 1) w: the whole row is final
        // the chain is past every chunk of this row: without this, rows with no coded run (no
        // wait_pre) left the helper waiting for slots forever (the decode's last rows, uncoded)
        ctl_put(1, (y + 1) * nch);
        int32_t *dst = S.out + (int64_t)y * w;
        for (int i = lane; i < w; i += 64) dst[i] = row[i];
        LACC(9, __builtin_amdgcn_s_memtime() - tw0);
    }
    if (lane == 0) put_status(S, cbits | (mode == 1 ? CCMI_ARM_FLAG_Q32 : 0u) | (w24 ? 0u : CCMI_ARM_FLAG_W32));
#if defined(CCMI_ARM_STAMPS)
    LACC(6, __builtin_amdgcn_s_memtime() - t_loop);
    if (lane < 12 && S.dbg) S.dbg[lane] = st_v;
#endif
#undef LACC
#undef CSTAMP
}

} // namespace

// ------------------------------------------------------------------ launchers
int launch_dec_arm(const ArmStreamDesc *d_streams, int n_streams, int max_w, int max_blocks, int d, int nh,
                         hipStream_t s)
{
    const int pitch = max_w + 2 * kPad;
    const size_t lds = sizeof(int32_t) * kRing * pitch + ((size_t)max_blocks + 16);
    // the speculative kernel keeps one ring row fewer (its contexts reach row y-3 only):
    // 5 streams (waves) per CU instead of 4 at 720p
    const size_t lds_spec = sizeof(int32_t) * kRingS * pitch + ((size_t)max_blocks + 16) + sizeof(uint32_t) * 17 * 50 * 2;
    // the one-latent-per-pass kernel below stays for wider ARMs and is what a
    // -DCCMI_DIAG_NOSPEC build runs for every stream (A/B measurements)
#if defined(CCMI_DIAG_NOSPEC)
    constexpr bool spec_off = true;
#else
    constexpr bool spec_off = false;
#endif
    // the chain kernel: packed context table, layer-0 weights, the preG ring (+ mirror), ring
    const size_t lds_lat = sizeof(int32_t) * (4 + 17 * 50 + 2 + 16 * 16 + 16 + (kPreRing + kPreMir) * 16 + kRingS * pitch) +
                           ((size_t)max_blocks + 16);
    if (!spec_off && d <= 16 && d > kDS && nh >= 1 && lds_lat <= 160 * 1024) {
#define CCMI_ARM_LAT(DD, NN)                                                                                    \
        if (d == DD && nh == NN) {                                                                              \
            hipLaunchKernelGGL((dec_arm_chain_kernel<DD, NN>), dim3(n_streams), dim3(128), lds_lat, s, d_streams, pitch); \
            CCMI_HIP_CHECK(hipGetLastError());                                                                  \
            return CCMI_OK;                                                                                     \
        }
        CCMI_ARM_LAT(8, 1) CCMI_ARM_LAT(8, 2) CCMI_ARM_LAT(8, 3) CCMI_ARM_LAT(8, 4)
        CCMI_ARM_LAT(16, 1) CCMI_ARM_LAT(16, 2) CCMI_ARM_LAT(16, 3) CCMI_ARM_LAT(16, 4)
#undef CCMI_ARM_LAT
    }
    if (!spec_off && d <= 16 && lds_spec <= 160 * 1024) {
#define CCMI_ARM_SPEC(DD, NN)                                                                                   \
        if (d == DD && nh == NN) {                                                                              \
            hipLaunchKernelGGL((dec_arm_spec_kernel<DD, NN>), dim3(n_streams), dim3(64), lds_spec, s, d_streams, pitch); \
            CCMI_HIP_CHECK(hipGetLastError());                                                                  \
            return CCMI_OK;                                                                                     \
        }
        CCMI_ARM_SPEC(8, 0) CCMI_ARM_SPEC(8, 1) CCMI_ARM_SPEC(8, 2) CCMI_ARM_SPEC(8, 3) CCMI_ARM_SPEC(8, 4)
        CCMI_ARM_SPEC(16, 0) CCMI_ARM_SPEC(16, 1) CCMI_ARM_SPEC(16, 2) CCMI_ARM_SPEC(16, 3) CCMI_ARM_SPEC(16, 4)
#undef CCMI_ARM_SPEC
    }
    if (lds > 160 * 1024) return ccmi_set_error(CCMI_ERR_UNSUPPORTED, "dec: latent width %d too large for LDS ring", max_w);
#define CCMI_ARM_CASE(DD, NN)                                                                                   \
    if (d == DD && nh == NN) {                                                                                  \
        hipLaunchKernelGGL((dec_arm_kernel<DD, NN>), dim3(n_streams), dim3(64), lds, s, d_streams, pitch);      \
        CCMI_HIP_CHECK(hipGetLastError());                                                                      \
        return CCMI_OK;                                                                                         \
    }
#define CCMI_ARM_D(DD) CCMI_ARM_CASE(DD, 0) CCMI_ARM_CASE(DD, 1) CCMI_ARM_CASE(DD, 2) CCMI_ARM_CASE(DD, 3) CCMI_ARM_CASE(DD, 4)
    CCMI_ARM_D(8)
    CCMI_ARM_D(16)
    CCMI_ARM_D(24)
    CCMI_ARM_D(32)
#undef CCMI_ARM_D
#undef CCMI_ARM_CASE
    return ccmi_set_error(CCMI_ERR_UNSUPPORTED, "dec: ARM with d=%d, %d hidden layers not supported", d, nh);
}

} // namespace ccmi
