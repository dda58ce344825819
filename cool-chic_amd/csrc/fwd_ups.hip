// fwd_ups.hip -- path A upsampling (Upsampling.forward, eval mode), float32.
//
// Reference (coolchic/enc/component/core/upsampling.py):
//   Upsampling.forward :476-506 -- from the coarsest grid, at each step s:
//     stack <- cat(conv2ds[s % n_pre](y_target), conv_transpose2ds[s % n_ups](stack)) ;
//   UpsamplingSeparableSymmetricConv2d.forward (eval) :205-209 -- zero-padded separable
//     cross-correlation, horizontal then vertical, plus residual;
//   UpsamplingSeparableSymmetricConvTranspose2d.forward (eval) :337-353 -- replicate pad
//     P0 = K/2, stride-2 transposed conv, crop C = K - 1 + K/2, horizontal then vertical,
//     then crop to the target size.
//
// One launch per pyramid step (coarse -> fine), all frames of the batch in the launch.
// The stride-2 transposed conv is evaluated in polyphase form: destination sample
// 2j + a reads source samples j + d with tap  a + K/2 - 1 - 2d  (derived from the
// crop offsets; the reference's padding makes border reads replicate-clamped).
// Each workgroup computes a destination tile: the source tile (with clamped halo) and the
// horizontal pass are staged in LDS, then the vertical pass writes coalesced rows.  Three
// kernels, the same values bit for bit: ups_level_rows (K = 8, KP = 7, the default form: one job
// of a 32 x 128 tile per workgroup), ups_level_fixed (K = 8, KP = 7, CCMI_UPS_FORM_LEVELS: one
// channel of a 16 x 64 tile per workgroup) and ups_level_kernel (any tap counts: every channel
// of a 16 x 64 tile per workgroup).
#include "fwd_common.h"

using namespace ccmi_fwd;

namespace {

constexpr int kThreads = 256;
constexpr int kTY = 16, kTX = 64;
constexpr int kMaxK = 16;                       // max upsampling / refine kernel taps
constexpr int kSrcW = kTX / 2 + kMaxK / 2 + 2;  // source tile row pitch (incl. halo)
constexpr int kRefH = kTY + kMaxK;              // refine rows incl. halo
constexpr int kRefW = kTX + kMaxK;


__global__ __launch_bounds__(kThreads) void ups_level_kernel(LevelArgs A)
{
    __shared__ float s_src[kRefH * kRefW]; // used for the source tile and the refine input
    __shared__ float s_h[kRefH * kTX];     // horizontal pass results

    const int b = blockIdx.y;
    const int y0 = (blockIdx.x / A.tiles_x) * kTY;
    const int x0 = (blockIdx.x % A.tiles_x) * kTX;
    const float *prm = A.params + (int64_t)b * A.pstride;
    const float *wu = prm + A.up_off;
    const float *wr = prm + A.pre_off;
    float *dst = A.dst + (int64_t)b * A.dst_stride;
    const int64_t dplane = (int64_t)A.hd * A.wd;
    const int tid = threadIdx.x;

    // ---------------- channel 0: refine(y_{k-1}) = x + sepconv(x), zero padding ----------------
    {
        const int pad = A.Kp / 2;
        const int rh = kTY + 2 * pad, rw = kTX + 2 * pad;
        const float *src = A.ref_src + (int64_t)b * A.ref_stride;
        for (int i = tid; i < rh * rw; i += kThreads) {
            const int r = i / rw, c = i - r * rw;
            const int y = y0 - pad + r, x = x0 - pad + c;
            float v = 0.f;
            if (y >= 0 && y < A.hd && x >= 0 && x < A.wd) {
                v = src[y * A.wd + x];
                if (A.ref_quant) v = rintf(A.gain * v);
            }
            s_src[r * kRefW + c] = v;
        }
        __syncthreads();
        for (int i = tid; i < rh * kTX; i += kThreads) {
            const int r = i / kTX, c = i - r * kTX;
            float acc = 0.f;
            for (int k = 0; k < A.Kp; ++k) acc = fmaf(wr[k], s_src[r * kRefW + c + k], acc);
            s_h[r * kTX + c] = acc;
        }
        __syncthreads();
        for (int i = tid; i < kTY * kTX; i += kThreads) {
            const int r = i / kTX, c = i - r * kTX;
            const int y = y0 + r, x = x0 + c;
            if (y < A.hd && x < A.wd) {
                float acc = 0.f;
                for (int k = 0; k < A.Kp; ++k) acc = fmaf(wr[k], s_h[(r + k) * kTX + c], acc);
                dst[(int64_t)y * A.wd + x] = acc + s_src[(r + pad) * kRefW + c + pad];
            }
        }
        __syncthreads();
    }

    // ---------------- channels 1..C: 2x transposed-conv upsampling of the source stack ----------------
    // source rows/cols needed: j + d for j in [y0/2, y0/2 + kTY/2), d in [dmin, dmax]
    const int K2 = A.K / 2;
    // tap = a + K2 - 1 - 2d in [0, K-1]  <=>  d in [ceil((a - K2)/2), floor((a + K2 - 1)/2)]
    const int d_lo = -((K2 + 1) / 2); // min over a in {0,1}
    const int d_hi = K2 / 2;          // max over a in {0,1}
    const int sy0 = y0 / 2 + d_lo, sx0 = x0 / 2 + d_lo;
    const int sh = kTY / 2 + d_hi - d_lo, sw = kTX / 2 + d_hi - d_lo;
    const int64_t splane = (int64_t)A.hs * A.ws;
    const float *src = A.src + (int64_t)b * A.src_stride;

    for (int c = 0; c < A.C; ++c) {
        const float *sp = src + c * splane;
        for (int i = tid; i < sh * sw; i += kThreads) {
            const int r = i / sw, cc = i - r * sw;
            const int y = clampi(sy0 + r, A.hs - 1), x = clampi(sx0 + cc, A.ws - 1);
            float v = sp[y * A.ws + x];
            if (A.src_quant) v = rintf(A.gain * v);
            s_src[r * kSrcW + cc] = v;
        }
        __syncthreads();
        // horizontal: s_h[r][c] for destination column x0 + c
        for (int i = tid; i < sh * kTX; i += kThreads) {
            const int r = i / kTX, cc = i - r * kTX;
            const int xd = x0 + cc, j = xd >> 1, a = xd & 1;
            float acc = 0.f;
            // taps in increasing source position: d from d_lo..d_hi with valid tap
            for (int d = d_lo; d <= d_hi; ++d) {
                const int tap = a + K2 - 1 - 2 * d;
                if (tap < 0 || tap >= A.K) continue;
                acc = fmaf(wu[tap], s_src[r * kSrcW + (j + d - sx0)], acc);
            }
            s_h[r * kTX + cc] = acc;
        }
        __syncthreads();
        for (int i = tid; i < kTY * kTX; i += kThreads) {
            const int r = i / kTX, cc = i - r * kTX;
            const int yd = y0 + r, xd = x0 + cc;
            if (yd < A.hd && xd < A.wd) {
                const int j = yd >> 1, a = yd & 1;
                float acc = 0.f;
                for (int d = d_lo; d <= d_hi; ++d) {
                    const int tap = a + K2 - 1 - 2 * d;
                    if (tap < 0 || tap >= A.K) continue;
                    acc = fmaf(wu[tap], s_h[(j + d - sy0) * kTX + cc], acc);
                }
                dst[(int64_t)(c + 1) * dplane + (int64_t)yd * A.wd + xd] = acc;
            }
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------
// Specialised level kernel for compile-time kernel sizes (the reference's defaults are
// K = 8 transposed taps, KP = 7 refine taps).  Differences from the generic kernel:
//   * one channel per workgroup (grid z), small LDS footprint -> high occupancy;
//   * the polyphase loops are unrolled: a thread produces an (even, odd) output pair from
//     K/2 + 1 shared source samples, horizontally and then vertically;
//   * no per-element division: all pitches are compile-time.
// ---------------------------------------------------------------------------------------------

template <int K, int KP>
__global__ __launch_bounds__(kThreads) void ups_level_fixed(LevelArgs A)
{
    using T = UpsTile<K, KP, kTY, kTX>;
    // blockIdx.z = job: 0 -> refine channel, c >= 1 -> transposed-conv channel c.  One
    // channel per workgroup keeps LDS small (the union of the two jobs' buffers), so many
    // workgroups are resident per CU to hide the L2/HBM latency of the tile loads.
    constexpr int kRef = T::RH * T::RW + T::RH * kTX;
    constexpr int kUp = T::SH * T::SW + T::SH * kTX;
    __shared__ float s_mem[kRef > kUp ? kRef : kUp];

    const int b = blockIdx.y;
    const int job = blockIdx.z;
    const int y0 = (blockIdx.x / A.tiles_x) * kTY;
    const int x0 = (blockIdx.x % A.tiles_x) * kTX;
    const float *prm = A.params + (int64_t)b * A.pstride;
    float *dst = A.dst + (int64_t)b * A.dst_stride;
    const int64_t dplane = (int64_t)A.hd * A.wd;
    const int tid = threadIdx.x;

    if (job == 0) {
        float wr[KP];
#pragma unroll
        for (int k = 0; k < KP; ++k) wr[k] = prm[A.pre_off + k];
        float *s_ref = s_mem, *s_refh = s_mem + T::RH * T::RW;
        const float *rs = A.ref_src + (int64_t)b * A.ref_stride;
        // fixed trip counts, unrolled: all of a thread's tile loads are in flight before the
        // first LDS store waits on one (the rolled loop paid one memory latency per pass)
        {
            constexpr int NU = (T::RH * T::RW + kThreads - 1) / kThreads;
            float lv[NU];
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                const int i = tid + u * kThreads;
                const int r = i / T::RW, c = i - r * T::RW;
                const int y = y0 - T::PAD + r, x = x0 - T::PAD + c;
                lv[u] = (i < T::RH * T::RW && y >= 0 && y < A.hd && x >= 0 && x < A.wd) ? rs[y * A.wd + x] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                const int i = tid + u * kThreads;
                if (i < T::RH * T::RW) s_ref[i] = A.ref_quant ? rintf(A.gain * lv[u]) : lv[u];
            }
        }
        __syncthreads();
        for (int i = tid; i < T::RH * kTX; i += kThreads) {
            const int r = i / kTX, c = i - r * kTX;
            const float *p = s_ref + r * T::RW + c;
            float acc = 0.f;
#pragma unroll
            for (int k = 0; k < KP; ++k) acc = fmaf(wr[k], p[k], acc);
            s_refh[i] = acc;
        }
        __syncthreads();
        for (int i = tid; i < kTY * kTX; i += kThreads) {
            const int r = i / kTX, c = i - r * kTX;
            const int y = y0 + r, x = x0 + c;
            if (y < A.hd && x < A.wd) {
                float acc = 0.f;
#pragma unroll
                for (int k = 0; k < KP; ++k) acc = fmaf(wr[k], s_refh[(r + k) * kTX + c], acc);
                dst[(int64_t)y * A.wd + x] = acc + s_ref[(r + T::PAD) * T::RW + c + T::PAD];
            }
        }
        return;
    }

    const int c = job - 1;
    float wu[K];
#pragma unroll
    for (int k = 0; k < K; ++k) wu[k] = prm[A.up_off + k];
    float *s_src = s_mem, *s_h = s_mem + T::SH * T::SW;
    {
        const float *src = A.src + (int64_t)b * A.src_stride + (int64_t)c * A.hs * A.ws;
        const int sy0 = y0 / 2 + T::D0, sx0 = x0 / 2 + T::D0;
        constexpr int NU = (T::SH * T::SW + kThreads - 1) / kThreads;
        float lv[NU];
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const int i = tid + u * kThreads;
            const int r = i / T::SW, cc = i - r * T::SW;
            const int y = clampi(sy0 + r, A.hs - 1), x = clampi(sx0 + cc, A.ws - 1);
            lv[u] = i < T::SH * T::SW ? src[y * A.ws + x] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const int i = tid + u * kThreads;
            if (i < T::SH * T::SW) s_src[i] = A.src_quant ? rintf(A.gain * lv[u]) : lv[u];
        }
    }
    __syncthreads();
    // horizontal: one (even, odd) destination column pair per item, source column x0/2 + q
    for (int i = tid; i < T::SH * (kTX / 2); i += kThreads) {
        const int r = i / (kTX / 2), q = i - r * (kTX / 2);
        const float *p = s_src + r * T::SW + q; // offset D0 at index 0
        float e = 0.f, o = 0.f;
#pragma unroll
        for (int m = 0; m < T::NS; ++m) {
            const float v = p[m];
            const int d = T::D0 + m;
            const int te = T::tap(0, d), to = T::tap(1, d);
            if (te >= 0) e = fmaf(wu[te], v, e);
            if (to >= 0) o = fmaf(wu[to], v, o);
        }
        *reinterpret_cast<float2 *>(s_h + r * kTX + 2 * q) = make_float2(e, o);
    }
    __syncthreads();
    // vertical: destination rows y0 + 2q, y0 + 2q + 1 of column x
    for (int i = tid; i < (kTY / 2) * kTX; i += kThreads) {
        const int q = i / kTX, x = i - q * kTX;
        const float *p = s_h + q * kTX + x;
        float e = 0.f, o = 0.f;
#pragma unroll
        for (int m = 0; m < T::NS; ++m) {
            const float v = p[m * kTX];
            const int d = T::D0 + m;
            const int te = T::tap(0, d), to = T::tap(1, d);
            if (te >= 0) e = fmaf(wu[te], v, e);
            if (to >= 0) o = fmaf(wu[to], v, o);
        }
        const int yd = y0 + 2 * q, xd = x0 + x;
        if (xd < A.wd) {
            float *out = dst + (int64_t)(c + 1) * dplane + (int64_t)yd * A.wd + xd;
            if (yd < A.hd) out[0] = e;
            if (yd + 1 < A.hd) out[A.wd] = o;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Row kernel (K = 8, KP = 7), the default form of a level.  A workgroup makes one job of a
// 32 x 128 destination tile (grid z): a half of 16 rows of the refine channel (jobs 0 and 1) or one
// transposed-conv channel (job 2 + c), in ups_level_fixed's operation order (same bits).
//   * raw tiles are loaded by wave-private rows: wave v owns rows v, v + 4, ..., the row address
//     is wave-uniform, lane = column, no division, all of a wave's loads in flight at once.  A
//     wave's horizontal pass reads only rows it staged itself, so a wave-level fence stands
//     between the two; the one workgroup barrier is in front of the vertical pass;
//   * the source tile of a channel is 20 x 68 for a 16 x 64 core (1.33 x; the 16 x 64 tile's
//     12 x 37 is 1.73 x), a refine half's is 22 x 134 for 16 x 128 (1.44 x; 22 x 70 for 16 x 64 was 1.50 x);
//   * the vertical pass makes four columns of a row pair per lane and stores 128 bits per lane
//     (whole 512-byte row segments per half wave); a row that is not 16-byte aligned is stored
//     as 64 + 64 or 32 + 64 + 32 bits, by the address of the lane's own first element.
// One job per workgroup was measured against runs of 2, 3 and all of a tile's jobs per workgroup
// with the next job's loads in flight over the current job's passes: the longer the run, the
// slower the step (profiles/ups_rows_ab.txt).  The launches are bound by how many tiles are in
// flight, which many short workgroups keep up better than few long ones.
// LDS: 5,808 floats (22.7 KB), six workgroups per CU.
// ---------------------------------------------------------------------------------------------
constexpr int kRY = 32, kRX = 128;
constexpr int kRNW = kThreads / 64;

__device__ __forceinline__ void wave_lds_fence()
{
    // a wave reads back rows it wrote (other lanes' columns): order its LDS accesses
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// four consecutive floats of a destination row, n of them inside the row
__device__ __forceinline__ void store_row4(float *p, float a, float b, float c, float d, int n)
{
    if (n >= 4) {
        const uintptr_t ad = reinterpret_cast<uintptr_t>(p);
        if ((ad & 15) == 0) {
            *reinterpret_cast<float4 *>(p) = make_float4(a, b, c, d);
        } else if ((ad & 7) == 0) {
            *reinterpret_cast<float2 *>(p) = make_float2(a, b);
            *reinterpret_cast<float2 *>(p + 2) = make_float2(c, d);
        } else {
            p[0] = a;
            *reinterpret_cast<float2 *>(p + 1) = make_float2(b, c);
            p[3] = d;
        }
    } else if (n > 0) {
        p[0] = a;
        if (n > 1) p[1] = b;
        if (n > 2) p[2] = c;
    }
}

template <int K, int KP>
__global__ __launch_bounds__(kThreads) void ups_level_rows(LevelArgs A)
{
    using T = UpsTile<K, KP, kRY, kRX>;
    constexpr int kHY = kRY / 2;               // destination rows of a refine half
    constexpr int kRefR = kHY + KP - 1;        // its staged rows
    constexpr int kRefP = (T::RW + 3) & ~3;    // and their pitch
    constexpr int kRefU = (kRefR + kRNW - 1) / kRNW;
    constexpr int kRefJ = (T::RW + 63) / 64;   // loads per staged refine row
    constexpr int kUpU = (T::SH + kRNW - 1) / kRNW;
    static_assert(T::SH % kRNW == 0, "a wave's source rows");
    static_assert(T::SW > 64 && T::SW <= 128 && kRefJ == 3, "loads per row");
    constexpr int kUpLds = T::SH * T::SW + T::SH * kRX;
    constexpr int kRefLds = kRefR * kRefP + kRefR * kRX;
    __shared__ __attribute__((aligned(16))) float s_mem[kUpLds > kRefLds ? kUpLds : kRefLds];

    const int b = blockIdx.y;
    const int tiles_x = (A.wd + kRX - 1) / kRX;
    const int y0 = (blockIdx.x / tiles_x) * kRY;
    const int x0 = (blockIdx.x % tiles_x) * kRX;
    const float *prm = A.params + (int64_t)b * A.pstride;
    float *dst = A.dst + (int64_t)b * A.dst_stride;
    const int64_t dplane = (int64_t)A.hd * A.wd;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    // the vertical passes: four columns per lane, 32 lanes per row
    const int vl = tid & 31, vr = tid >> 5;
    const int nx = A.wd - (x0 + 4 * vl); // columns of the lane's four inside the row

    // ---------------- channel 0: refine, two halves of kHY rows ----------------
    const float *rs = A.ref_src + (int64_t)b * A.ref_stride;
    unsigned rcx[kRefJ]; // (unsigned: a 32-bit lane offset beside the row's scalar address)
    bool rok[kRefJ];
#pragma unroll
    for (int j = 0; j < kRefJ; ++j) {
        const int cc = j < 2 ? lane + 64 * j : 128 + (lane & 7);
        const int x = x0 - T::PAD + cc;
        rok[j] = x >= 0 && x < A.wd;
        rcx[j] = (unsigned)clampi(x, A.wd - 1);
    }
    float rv[kRefU][kRefJ];
    auto ref_load = [&](int yh) {
#pragma unroll
        for (int u = 0; u < kRefU; ++u) {
            const int r = min(wv + kRNW * u, kRefR - 1);
            const float *row = rs + (int64_t)clampi(y0 + yh - T::PAD + r, A.hd - 1) * A.wd;
#pragma unroll
            for (int j = 0; j < kRefJ; ++j) rv[u][j] = row[rcx[j]];
        }
    };
    auto ref_stage = [&](int yh) {
        float *s_ref = s_mem;
#pragma unroll
        for (int u = 0; u < kRefU; ++u) {
            const int r = wv + kRNW * u;
            if (r >= kRefR) continue;
            const int y = y0 + yh - T::PAD + r;
            const bool yin = y >= 0 && y < A.hd;
#pragma unroll
            for (int j = 0; j < kRefJ; ++j) {
                const float v = (yin && rok[j]) ? rv[u][j] : 0.f;
                const float qv = A.ref_quant ? rintf(A.gain * v) : v;
                const int cc = lane + 64 * j;
                if (cc < T::RW) s_ref[r * kRefP + cc] = qv;
            }
        }
    };
    float wr[KP];
#pragma unroll
    for (int k = 0; k < KP; ++k) wr[k] = prm[A.pre_off + k];
    auto ref_passes = [&](int yh) {
        float *s_ref = s_mem, *s_rh = s_mem + kRefR * kRefP;
        wave_lds_fence();
        // horizontal: two destination columns per lane, the wave's own rows
#pragma unroll
        for (int u = 0; u < kRefU; ++u) {
            const int r = wv + kRNW * u;
            if (r >= kRefR) continue;
            const float *p = s_ref + r * kRefP + 2 * lane;
            float v[KP + 1];
#pragma unroll
            for (int k = 0; k < KP + 1; k += 2) {
                const float2 t = *reinterpret_cast<const float2 *>(p + k);
                v[k] = t.x;
                v[k + 1] = t.y;
            }
            float e = 0.f, o = 0.f;
#pragma unroll
            for (int k = 0; k < KP; ++k) {
                e = fmaf(wr[k], v[k], e);
                o = fmaf(wr[k], v[k + 1], o);
            }
            *reinterpret_cast<float2 *>(s_rh + r * kRX + 2 * lane) = make_float2(e, o);
        }
        __syncthreads();
#pragma unroll
        for (int rd = 0; rd < kHY / 8; ++rd) {
            const int r = vr + 8 * rd;
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < KP; ++k) {
                const float4 t = *reinterpret_cast<const float4 *>(s_rh + (r + k) * kRX + 4 * vl);
                acc[0] = fmaf(wr[k], t.x, acc[0]);
                acc[1] = fmaf(wr[k], t.y, acc[1]);
                acc[2] = fmaf(wr[k], t.z, acc[2]);
                acc[3] = fmaf(wr[k], t.w, acc[3]);
            }
            const float *cx = s_ref + (r + T::PAD) * kRefP + 4 * vl + T::PAD;
            const int y = y0 + yh + r;
            if (y < A.hd)
                store_row4(dst + (int64_t)y * A.wd + x0 + 4 * vl, acc[0] + cx[0], acc[1] + cx[1], acc[2] + cx[2],
                           acc[3] + cx[3], nx);
        }
    };

    // ---------------- channels 1..C: 2x transposed conv of the source stack ----------------
    const float *src = A.src + (int64_t)b * A.src_stride;
    const int64_t splane = (int64_t)A.hs * A.ws;
    const int sy0 = y0 / 2 + T::D0, sx0 = x0 / 2 + T::D0;
    const unsigned ucx0 = (unsigned)clampi(sx0 + lane, A.ws - 1), ucx1 = (unsigned)clampi(sx0 + 64 + (lane & 7), A.ws - 1);
    float uv[kUpU][2];
    auto up_load = [&](int c) {
        const float *sp = src + (int64_t)c * splane;
#pragma unroll
        for (int u = 0; u < kUpU; ++u) {
            const float *row = sp + (int64_t)clampi(sy0 + wv + kRNW * u, A.hs - 1) * A.ws;
            uv[u][0] = row[ucx0];
            uv[u][1] = row[ucx1];
        }
    };
    auto up_stage = [&]() {
        float *s_src = s_mem;
#pragma unroll
        for (int u = 0; u < kUpU; ++u) {
            const int r = wv + kRNW * u;
            s_src[r * T::SW + lane] = A.src_quant ? rintf(A.gain * uv[u][0]) : uv[u][0];
            if (lane < T::SW - 64) s_src[r * T::SW + 64 + lane] = A.src_quant ? rintf(A.gain * uv[u][1]) : uv[u][1];
        }
    };

    const int job = blockIdx.z;
    if (job < 2) {
        const int yh = job * kHY;
        if (y0 + yh >= A.hd) return;
        ref_load(yh);
        ref_stage(yh);
        ref_passes(yh);
        return;
    }

    float wu[K];
#pragma unroll
    for (int k = 0; k < K; ++k) wu[k] = prm[A.up_off + k];
    {
        const int c = job - 2;
        float *s_src = s_mem, *s_h = s_mem + T::SH * T::SW;
        up_load(c);
        up_stage();
        wave_lds_fence();
        // horizontal: lane = source column, the (even, odd) destination pair; the wave's own rows
#pragma unroll
        for (int u = 0; u < kUpU; ++u) {
            const int r = wv + kRNW * u;
            const float *p = s_src + r * T::SW + lane; // offset D0 at index 0
            float e = 0.f, o = 0.f;
#pragma unroll
            for (int m = 0; m < T::NS; ++m) {
                const float v = p[m];
                const int d = T::D0 + m;
                const int te = T::tap(0, d), to = T::tap(1, d);
                if (te >= 0) e = fmaf(wu[te], v, e);
                if (to >= 0) o = fmaf(wu[to], v, o);
            }
            *reinterpret_cast<float2 *>(s_h + r * kRX + 2 * lane) = make_float2(e, o);
        }
        __syncthreads();
        // vertical: destination rows y0 + 2q, y0 + 2q + 1 of four columns
        float *dc = dst + (int64_t)(c + 1) * dplane + x0 + 4 * vl;
#pragma unroll
        for (int rd = 0; rd < kRY / 16; ++rd) {
            const int q = vr + 8 * rd;
            float e[4] = {0.f, 0.f, 0.f, 0.f}, o[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int m = 0; m < T::NS; ++m) {
                const float4 t = *reinterpret_cast<const float4 *>(s_h + (q + m) * kRX + 4 * vl);
                const float v[4] = {t.x, t.y, t.z, t.w};
                const int d = T::D0 + m;
                const int te = T::tap(0, d), to = T::tap(1, d);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (te >= 0) e[i] = fmaf(wu[te], v[i], e[i]);
                    if (to >= 0) o[i] = fmaf(wu[to], v[i], o[i]);
                }
            }
            const int yd = y0 + 2 * q;
            if (yd < A.hd) store_row4(dc + (int64_t)yd * A.wd, e[0], e[1], e[2], e[3], nx);
            if (yd + 1 < A.hd) store_row4(dc + (int64_t)(yd + 1) * A.wd, o[0], o[1], o[2], o[3], nx);
        }
    }
}

} // namespace

extern "C" size_t ccmi_ups_workspace_bytes(int n_grids, const int *h, const int *w, int batch)
{
    size_t per = 0;
    for (int k = 1; k <= n_grids - 2; ++k) per += (size_t)(n_grids - k) * h[k] * w[k];
    return per * sizeof(float) * (size_t)(batch > 0 ? batch : 0);
}

namespace {
int launch_level(const LevelArgs &A, int batch, hipStream_t s, int form)
{
    dim3 grid(A.tiles_x * ccmi_div_up(A.hd, kTY), batch);
    if (A.K == 8 && A.Kp == 7 && form == CCMI_UPS_FORM_DEFAULT)
        hipLaunchKernelGGL((ups_level_rows<8, 7>),
                           dim3(ccmi_div_up(A.wd, kRX) * ccmi_div_up(A.hd, kRY), batch, A.C + 2),
                           dim3(kThreads), 0, s, A);
    else if (A.K == 8 && A.Kp == 7)
        hipLaunchKernelGGL((ups_level_fixed<8, 7>), dim3(grid.x, grid.y, A.C + 1), dim3(kThreads), 0, s, A);
    else
        hipLaunchKernelGGL(ups_level_kernel, grid, dim3(kThreads), 0, s, A);
    CCMI_HIP_CHECK(hipGetLastError());
    return CCMI_OK;
}
} // namespace

int ccmi_fwd::ups_pyramid(const ccmi_ups_args *a, hipStream_t s, LevelArgs *last, bool launch, LevelArgs *prev, int form)
{
    const int L = a->n_grids;
    if (L < 2) return ccmi_set_error(CCMI_ERR_UNSUPPORTED, "ups: needs at least 2 latent grids (got %d)", L);
    if (a->ups_k < 4 || a->ups_k % 2 || a->ups_k > kMaxK)
        return ccmi_set_error(CCMI_ERR_UNSUPPORTED, "ups: ups_k must be even in [4, %d] (got %d)", kMaxK, a->ups_k);
    if (a->pre_k < 1 || a->pre_k % 2 == 0 || a->pre_k > kMaxK - 1)
        return ccmi_set_error(CCMI_ERR_UNSUPPORTED, "ups: pre_k must be odd in [1, %d] (got %d)", kMaxK - 1, a->pre_k);
    if (a->n_ups < 1 || a->n_pre < 1) return ccmi_set_error(CCMI_ERR_ARG, "ups: n_ups and n_pre must be >= 1");
    for (int l = 1; l < L; ++l)
        if (a->h[l] != (a->h[l - 1] + 1) / 2 || a->w[l] != (a->w[l - 1] + 1) / 2)
            return ccmi_set_error(CCMI_ERR_ARG, "ups: grid %d is not ceil(half) of grid %d", l, l - 1);
    const size_t need = ccmi_ups_workspace_bytes(L, a->h, a->w, a->batch);
    if (need > 0 && (a->workspace == nullptr || a->workspace_bytes < need))
        return ccmi_set_error(CCMI_ERR_ARG, "ups: workspace of %zu bytes needed", need);

    int off[CCMI_MAX_GRIDS];
    int total = 0;
    for (int l = 0; l < L; ++l) { off[l] = total; total += a->h[l] * a->w[l]; }
    if (a->latent_stride != 0 && a->latent_stride < total) return ccmi_set_error(CCMI_ERR_ARG, "ups: latent_stride < %d", total);

    // workspace layout: stack of level k (1..L-2) for all frames: [batch][L-k][h_k][w_k]
    float *ws_base = static_cast<float *>(a->workspace);
    float *stack_ptr[CCMI_MAX_GRIDS] = {};
    int64_t stack_stride[CCMI_MAX_GRIDS] = {};
    for (int k = 1; k <= L - 2; ++k) {
        stack_ptr[k] = ws_base;
        stack_stride[k] = (int64_t)(L - k) * a->h[k] * a->w[k];
        ws_base += stack_stride[k] * a->batch;
    }

    for (int step = 0; step < L - 1; ++step) {
        const int k = L - 1 - step; // source level
        LevelArgs A{};
        if (k == L - 1) {
            A.src = a->latent + off[k];
            A.src_stride = a->latent_stride;
            A.src_quant = a->quantize;
        } else {
            A.src = stack_ptr[k];
            A.src_stride = stack_stride[k];
            A.src_quant = 0;
        }
        A.C = L - k;
        A.hs = a->h[k];
        A.ws = a->w[k];
        A.ref_src = a->latent + off[k - 1];
        A.ref_stride = a->latent_stride;
        A.ref_quant = a->quantize;
        if (k - 1 == 0) {
            A.dst = a->out; // may be null when the caller fuses the last step
            A.dst_stride = a->out_stride;
        } else {
            A.dst = stack_ptr[k - 1];
            A.dst_stride = stack_stride[k - 1];
        }
        A.hd = a->h[k - 1];
        A.wd = a->w[k - 1];
        A.gain = a->gain;
        A.params = a->params;
        A.pstride = a->param_stride;
        A.K = a->ups_k;
        A.up_off = (step % a->n_ups) * a->ups_k;
        A.Kp = a->pre_k;
        A.pre_off = a->n_ups * a->ups_k + (step % a->n_pre) * a->pre_k;
        A.tiles_x = ccmi_div_up(A.wd, kTX);
        if (step == L - 2) {
            *last = A;
            break;
        }
        if (prev && step == L - 3) { // folded into the caller's fused kernel: not launched
            *prev = A;
            continue;
        }
        if (launch)
            if (int rc = launch_level(A, a->batch, s, form)) return rc;
    }
    return CCMI_OK;
}

int ccmi_launch_ups_f32_form(const ccmi_ups_args *a, hipStream_t s, int form)
{
    if (a->out_stride < (int64_t)a->n_grids * a->h[0] * a->w[0])
        return ccmi_set_error(CCMI_ERR_ARG, "ups: out_stride too small");
    LevelArgs last{};
    if (int rc = ups_pyramid(a, s, &last, true, nullptr, form)) return rc;
    return launch_level(last, a->batch, s, form);
}

int ccmi_launch_ups_f32(const ccmi_ups_args *a, hipStream_t s) { return ccmi_launch_ups_f32_form(a, s, CCMI_UPS_FORM_DEFAULT); }

extern "C" int ccmi_ups_forward_f32_form(const ccmi_ups_args *a, void *stream, int form)
{
    if (form != CCMI_UPS_FORM_DEFAULT && form != CCMI_UPS_FORM_LEVELS) return ccmi_set_error(CCMI_ERR_ARG, "ups: unknown form %d", form);
    if (!a || !a->latent || !a->params || !a->out) return ccmi_set_error(CCMI_ERR_ARG, "ups: null argument");
    if (a->n_grids < 1 || a->n_grids > CCMI_MAX_GRIDS) return ccmi_set_error(CCMI_ERR_ARG, "ups: n_grids must be in [1, %d]", CCMI_MAX_GRIDS);
    for (int l = 0; l < a->n_grids; ++l)
        if (a->h[l] < 1 || a->w[l] < 1) return ccmi_set_error(CCMI_ERR_ARG, "ups: grid %d has size %dx%d", l, a->h[l], a->w[l]);
    if (a->batch < 1) return ccmi_set_error(CCMI_ERR_ARG, "ups: batch must be >= 1");
    return ccmi_launch_ups_f32_form(a, static_cast<hipStream_t>(stream), form);
}
