// dec_latents.hip -- path B: the latent store's kernels (gfx950).
//
// dec_lat_pack<T>: the ARM + CABAC stage's output planes (int32, value << kArmPrec) -> the
// store's T values (int8 / int16 / int32), one launch per chunk of a build.  A latent that does
// not fit T is never saturated: the grid's status word gets CCMI_ARM_FLAG_NARROW and the build
// fails on the host.
// dec_lat_unpack<T>: the store's T values -> value << kArmPrec in the workspace planes the
// decoder tail reads, over the rectangle of each plane the tail's windows read
// (DecRoi::lat); one launch per render.  An all-zero grid (no coded bytes, no store bytes)
// writes zeros over the same rectangle.
//
// Both are memory-bound copies driven by a job table in device memory (DecLatPackJob /
// DecLatUnpackJob): a job owns a whole number of blocks, a block finds its job by a binary
// search over the jobs' first blocks (uniform per block: scalar loads).
//
// The segmented form (CCMI_LATENT_SEG, the contract in ccmi.h) is made from a built store by
// dec_lat_seg_width / dec_lat_seg_scan / dec_lat_seg_pack (DecLatSegJob, one wave per segment of
// 64 values, a wave finds its job by the same search over the jobs' first segments) and read by
// dec_lat_unpack_seg, which takes dec_lat_unpack's jobs and writes the same rectangle.
//
// Latent-store files (dec_store_file.cpp): dec_lat_file_gather copies the defined byte ranges of
// stores into a zeroed DATA image, dec_lat_file_sum takes a range's two checksums, and
// dec_lat_seg_verify proves an imported descriptor table safe before any handle refers to it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "dec_internal.h"

namespace ccmi {
namespace {

constexpr int kThreads = 256;
constexpr int kUnpackPerThread = 4;

// the last job whose first_block <= block
template <typename Job>
__device__ __forceinline__ int find_job(const Job *__restrict__ jobs, int n_jobs, uint32_t block)
{
    int lo = 0, hi = n_jobs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (jobs[mid].first_block <= block) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

template <typename T>
__device__ __forceinline__ T lat_narrow(int32_t plane_value, int shift, bool &bad)
{
    const int32_t v = plane_value >> shift; // arithmetic: the plane holds value << shift exactly
    const T t = (T)v;
    bad |= (int32_t)t != v;
    return t;
}

// A thread owns one 16-byte group of the destination (16 / 8 / 4 values): 128-bit loads of its
// sources, one 128-bit store.  The grid's last group may be partial: scalar stores.
template <typename T>
__global__ __launch_bounds__(kThreads) void dec_lat_pack(const DecLatPackJob *__restrict__ jobs, int n_jobs)
{
    constexpr int G = 16 / (int)sizeof(T);
    const DecLatPackJob J = jobs[find_job(jobs, n_jobs, blockIdx.x)];
    const uint64_t e0 = ((uint64_t)(blockIdx.x - J.first_block) * kThreads + threadIdx.x) * G;
    bool bad = false;
    if (e0 < J.n) {
        const int32_t *src = J.src + e0;
        T *dst = static_cast<T *>(J.dst) + e0;
        if (e0 + G <= J.n) {
            union {
                T v[G];
                uint4 q;
            } o;
#pragma unroll
            for (int k = 0; k < G / 4; ++k) {
                const int4 a = reinterpret_cast<const int4 *>(src)[k];
                o.v[4 * k + 0] = lat_narrow<T>(a.x, J.shift, bad);
                o.v[4 * k + 1] = lat_narrow<T>(a.y, J.shift, bad);
                o.v[4 * k + 2] = lat_narrow<T>(a.z, J.shift, bad);
                o.v[4 * k + 3] = lat_narrow<T>(a.w, J.shift, bad);
            }
            *reinterpret_cast<uint4 *>(dst) = o.q;
        } else {
            const int m = (int)(J.n - e0);
            for (int k = 0; k < m; ++k) dst[k] = lat_narrow<T>(src[k], J.shift, bad);
        }
    }
    if constexpr (sizeof(T) < 4) {
        // one atomic per wave at most: every lane of the block gets here (no early return)
        const unsigned long long m = __ballot(bad);
        if (m != 0ull && (int)(threadIdx.x & (warpSize - 1)) == __ffsll((long long)m) - 1 && J.status)
            atomicOr(J.status, CCMI_ARM_FLAG_NARROW);
    }
}

// A block writes kThreads * kUnpackPerThread consecutive samples of its job's rectangle
// (row-major inside the rectangle, consecutive lanes on consecutive columns).
template <typename T>
__global__ __launch_bounds__(kThreads) void dec_lat_unpack(const DecLatUnpackJob *__restrict__ jobs, int n_jobs)
{
    const DecLatUnpackJob J = jobs[find_job(jobs, n_jobs, blockIdx.x)];
    const uint32_t rw = (uint32_t)(J.x1 - J.x0);
    const uint64_t total = (uint64_t)(uint32_t)(J.y1 - J.y0) * rw;
    const uint64_t base = (uint64_t)(blockIdx.x - J.first_block) * (kThreads * kUnpackPerThread);
    const T *src = static_cast<const T *>(J.src);
#pragma unroll
    for (int k = 0; k < kUnpackPerThread; ++k) {
        const uint64_t i = base + (uint64_t)k * kThreads + threadIdx.x;
        if (i < total) {
            const uint32_t r = (uint32_t)(i / rw), c = (uint32_t)(i - (uint64_t)r * rw);
            const int64_t at = (int64_t)(J.y0 + (int)r) * J.w + (J.x0 + (int)c);
            const int32_t v = src ? (int32_t)src[at] : 0;
            J.dst[at] = (int32_t)((uint32_t)v << J.shift);
        }
    }
}

// ---- the segmented form ----
constexpr int kSegWaves = kThreads / kSegLen;
constexpr int kScanPerThread = 4;

// a wave's segment: its job, its place in the grid, its values
struct SegAt {
    uint32_t q;  // the segment's index in its grid, row-major
    int c;       // its values: kSegLen, fewer for a row's last segment
    int32_t v;   // this lane's value; 0 for lanes >= c
};

__device__ __forceinline__ int seg_values(int w, uint32_t s) { return min(kSegLen, w - kSegLen * (int)s); }
// words of a segment of c values at width code k (0, 2, 4, 8, 16, 32 bits)
__device__ __forceinline__ uint32_t seg_words(uint32_t k, int c) { return k ? (((uint32_t)c << k) + 31u) >> 5 : 0u; }

__device__ __forceinline__ DecLatSegJob seg_job(const DecLatSegJob *__restrict__ jobs, int n_jobs, uint32_t seg)
{
    int lo = 0, hi = n_jobs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (jobs[mid].first_seg <= seg) lo = mid;
        else hi = mid - 1;
    }
    return jobs[lo];
}

__device__ __forceinline__ SegAt seg_load(const DecLatSegJob &J, uint32_t seg, int lane)
{
    SegAt a;
    a.q = seg - J.first_seg;
    const uint32_t r = a.q / (uint32_t)J.nseg, s = a.q - r * (uint32_t)J.nseg;
    a.c = seg_values(J.w, s);
    a.v = 0;
    if (lane < a.c) {
        const size_t at = (size_t)r * J.w + (size_t)s * kSegLen + lane;
        a.v = J.elem == 1   ? (int32_t) static_cast<const int8_t *>(J.src)[at]
              : J.elem == 2 ? (int32_t) static_cast<const int16_t *>(J.src)[at]
                            : static_cast<const int32_t *>(J.src)[at];
    }
    return a;
}

// Width pass: the smallest code whose range holds every value of the segment.  The five range
// tests are nested, so the number of non-empty ballots is the code: no reduction.
__global__ __launch_bounds__(kThreads) void dec_lat_seg_width(const DecLatSegJob *__restrict__ jobs, int n_jobs,
                                                              uint32_t n_segs)
{
    const uint32_t seg = blockIdx.x * kSegWaves + (threadIdx.x >> 6);
    if (seg >= n_segs) return; // the whole wave
    const int lane = threadIdx.x & 63;
    const DecLatSegJob J = seg_job(jobs, n_jobs, seg);
    const SegAt a = seg_load(J, seg, lane);
    const int32_t v = a.v;
    const uint32_t k = (__ballot(v != 0) != 0ull) + (__ballot(v < -2 || v > 1) != 0ull) +
                       (__ballot(v < -8 || v > 7) != 0ull) + (__ballot(v < -128 || v > 127) != 0ull) +
                       (__ballot(v < -32768 || v > 32767) != 0ull);
    if (lane == 0) J.desc[a.q] = k;
}

// Scan: one block per grid.  Exclusive scan of the segments' word counts in (r, s) order, a
// thread on kScanPerThread consecutive segments, the block looping over the grid with a carry;
// the codes become descriptors in place.
__global__ __launch_bounds__(kThreads) void dec_lat_seg_scan(const DecLatSegJob *__restrict__ jobs,
                                                             uint32_t *__restrict__ totals)
{
    __shared__ uint32_t wave_sum[kSegWaves];
    const DecLatSegJob J = jobs[blockIdx.x];
    const uint32_t n = (uint32_t)J.h * (uint32_t)J.nseg;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t carry = 0;
    int over = 0;
    for (uint32_t base = 0; base < n; base += kThreads * kScanPerThread) {
        const uint32_t i0 = base + threadIdx.x * kScanPerThread;
        uint32_t k[kScanPerThread], wd[kScanPerThread], sum = 0;
#pragma unroll
        for (int t = 0; t < kScanPerThread; ++t) {
            const uint32_t i = i0 + t;
            k[t] = 0;
            wd[t] = 0;
            if (i < n) {
                k[t] = J.desc[i];
                wd[t] = seg_words(k[t], seg_values(J.w, i % (uint32_t)J.nseg));
            }
            sum += wd[t];
        }
        uint32_t inc = sum; // inclusive over the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(inc, d);
            if (lane >= d) inc += up;
        }
        if (lane == 63) wave_sum[wave] = inc;
        __syncthreads();
        uint32_t before = 0, all = 0;
#pragma unroll
        for (int wv = 0; wv < kSegWaves; ++wv) {
            const uint32_t ws = wave_sum[wv];
            before += wv < wave ? ws : 0u;
            all += ws;
        }
        __syncthreads(); // wave_sum is rewritten by the next round
        uint64_t off = carry + before + (inc - sum);
#pragma unroll
        for (int t = 0; t < kScanPerThread; ++t) {
            const uint32_t i = i0 + t;
            if (i < n) {
                over |= off > (uint64_t)kSegOffMax;
                J.desc[i] = ((uint32_t)off << 3) | k[t];
                off += wd[t];
            }
        }
        carry += all;
    }
    over = __syncthreads_or(over);
    if (threadIdx.x == 0) totals[blockIdx.x] = over || carry >= (uint64_t)kSegTotalBad ? kSegTotalBad : (uint32_t)carry;
}

// Pack: lane j's field goes to bit (j b) % 32 of word (j b) / 32; the 32 / b lanes of a word are
// OR-combined by an xor butterfly and the first of them stores it: 2 b consecutive words per
// full segment.  Lanes past the segment's values carry 0, so the last word's trailing bits are 0.
__global__ __launch_bounds__(kThreads) void dec_lat_seg_pack(const DecLatSegJob *__restrict__ jobs, int n_jobs,
                                                             uint32_t n_segs)
{
    const uint32_t seg = blockIdx.x * kSegWaves + (threadIdx.x >> 6);
    if (seg >= n_segs) return; // the whole wave
    const int lane = threadIdx.x & 63;
    const DecLatSegJob J = seg_job(jobs, n_jobs, seg);
    const SegAt a = seg_load(J, seg, lane);
    const uint32_t d = J.desc[a.q], k = d & 7u, off = d >> 3;
    if (lane == 0) J.desc_out[a.q] = d;
    if (k == 0) return; // wave-uniform: an all-zero segment has no words
    const int per_word = 32 >> k; // lanes per word: 16, 8, 4, 2, 1
    uint32_t x = (uint32_t)a.v;
    if (k < 5) x = (x & ((1u << (1u << k)) - 1u)) << (((uint32_t)lane << k) & 31u);
#pragma unroll
    for (int m = 1; m < 16; m <<= 1)
        if (m < per_word) x |= (uint32_t)__shfl_xor((int)x, m); // per_word is wave-uniform
    const uint32_t word = (uint32_t)lane >> (5 - k);
    if ((lane & (per_word - 1)) == 0 && word < seg_words(k, a.c)) J.payload[off + word] = x;
}

// dec_lat_unpack for the segmented form: the same jobs (src = the grid's descriptor table, the
// payload behind it), the same rectangle, the same 4 samples per thread.  A field never crosses
// a word (every width divides 32): one descriptor load, one word load, a signed extract.
__global__ __launch_bounds__(kThreads) void dec_lat_unpack_seg(const DecLatUnpackJob *__restrict__ jobs, int n_jobs)
{
    const DecLatUnpackJob J = jobs[find_job(jobs, n_jobs, blockIdx.x)];
    const uint32_t rw = (uint32_t)(J.x1 - J.x0);
    const uint64_t total = (uint64_t)(uint32_t)(J.y1 - J.y0) * rw;
    const uint64_t base = (uint64_t)(blockIdx.x - J.first_block) * (kThreads * kUnpackPerThread);
    const uint32_t nseg = ((uint32_t)J.w + kSegLen - 1) / kSegLen;
    const uint32_t *desc = static_cast<const uint32_t *>(J.src);
    const uint32_t *payload = desc + (((size_t)J.h * nseg + 3) & ~(size_t)3);
#pragma unroll
    for (int t = 0; t < kUnpackPerThread; ++t) {
        const uint64_t i = base + (uint64_t)t * kThreads + threadIdx.x;
        if (i < total) {
            const uint32_t r = (uint32_t)(i / rw), c = (uint32_t)(i - (uint64_t)r * rw);
            const uint32_t y = (uint32_t)J.y0 + r, x = (uint32_t)J.x0 + c;
            int32_t v = 0;
            if (desc) {
                const uint32_t d = desc[(size_t)y * nseg + (x >> 6)], k = d & 7u;
                if (k) {
                    const uint32_t b = 1u << k, bit = (x & 63u) << k;
                    const uint32_t word = payload[(size_t)(d >> 3) + (bit >> 5)];
                    v = (int32_t)(word << (32u - b - (bit & 31u))) >> (32u - b);
                }
            }
            J.dst[(int64_t)y * J.w + x] = (int32_t)((uint32_t)v << J.shift);
        }
    }
}

// ---- latent-store files ----
constexpr int kFileGroups = 4;                        // 16-byte groups per thread
constexpr int kFileBlock = kThreads * kFileGroups;    // groups per block: 16 KiB

// Gather: a block copies kFileBlock consecutive 16-byte groups of its job's range, consecutive
// lanes on consecutive groups; the range's last group may be partial: byte stores.
__global__ __launch_bounds__(kThreads) void dec_lat_file_gather(const DecLatGatherJob *__restrict__ jobs, int n_jobs)
{
    const DecLatGatherJob J = jobs[find_job(jobs, n_jobs, blockIdx.x)];
    const uint64_t g0 = (uint64_t)(blockIdx.x - J.first_block) * kFileBlock;
#pragma unroll
    for (int t = 0; t < kFileGroups; ++t) {
        const uint64_t b = (g0 + (uint64_t)t * kThreads + threadIdx.x) * 16;
        if (b + 16 <= J.n) {
            *reinterpret_cast<uint4 *>(J.dst + b) = *reinterpret_cast<const uint4 *>(J.src + b);
        } else if (b < J.n) {
            for (uint64_t k = b; k < J.n; ++k) J.dst[k] = J.src[k];
        }
    }
}

// Checksum: sum[0] += sum of w_i, sum[1] += sum of (i + 1) w_i (mod 2^64) over the block's words;
// a wave reduces by shuffles, the block through LDS, one atomic pair per block.
__global__ __launch_bounds__(kThreads) void dec_lat_file_sum(const DecLatSumJob *__restrict__ jobs, int n_jobs)
{
    __shared__ unsigned long long part[2][kSegWaves];
    const DecLatSumJob J = jobs[find_job(jobs, n_jobs, blockIdx.x)];
    const uint64_t g0 = (uint64_t)(blockIdx.x - J.first_block) * kFileBlock;
    unsigned long long s0 = 0, s1 = 0;
#pragma unroll
    for (int t = 0; t < kFileGroups; ++t) {
        const uint64_t g = g0 + (uint64_t)t * kThreads + threadIdx.x, i = 4 * g;
        if (i + 4 <= J.n_words) {
            const uint4 v = reinterpret_cast<const uint4 *>(J.src)[g];
            s0 += (unsigned long long)v.x + v.y + v.z + v.w;
            s1 += (i + 1) * v.x + (i + 2) * v.y + (i + 3) * v.z + (i + 4) * v.w;
        } else {
            for (uint64_t k = i; k < J.n_words; ++k) {
                const uint32_t v = J.src[k];
                s0 += v;
                s1 += (k + 1) * v;
            }
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        s0 += __shfl_down(s0, d);
        s1 += __shfl_down(s1, d);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        part[0][wave] = s0;
        part[1][wave] = s1;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        unsigned long long a = 0;
#pragma unroll
        for (int wv = 0; wv < kSegWaves; ++wv) a += part[threadIdx.x][wv];
        atomicAdd(J.sum + threadIdx.x, a);
    }
}

// Verify: one block per non-empty SEG grid of an imported (untrusted) store, shaped like
// dec_lat_seg_scan.  The table's extent, h * nseg words, follows from the header the host has
// validated against the part's size, so the reads here are in bounds whatever the table holds.
// Checked: every width code k <= 5; every offset equals the exclusive prefix sum of the word
// counts seg_words(k, c) of the segments before it; the sum over all segments equals the
// record's seg_words, which is what the layout reserved for the payload.
// What follows for dec_lat_unpack_seg: it reads payload[off + (bit >> 5)] with
// bit = (x & 63) << k < c << k, so (bit >> 5) < seg_words(k, c) = words; off + words is the next
// segment's offset or, for the last one, the total, and offsets do not decrease: off + words <=
// seg_words for every segment.  No render can read outside the grid's payload.  (That k is the
// smallest code that fits and that trailing bits are 0 is not checked: neither moves a read.)
__global__ __launch_bounds__(kThreads) void dec_lat_seg_verify(const DecLatVerifyJob *__restrict__ jobs)
{
    __shared__ uint32_t wave_sum[kSegWaves];
    const DecLatVerifyJob J = jobs[blockIdx.x];
    const uint32_t n = (uint32_t)J.h * (uint32_t)J.nseg;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t carry = 0;
    int bad = 0;
    for (uint32_t base = 0; base < n; base += kThreads * kScanPerThread) {
        const uint32_t i0 = base + threadIdx.x * kScanPerThread;
        uint32_t off[kScanPerThread], wd[kScanPerThread], sum = 0;
#pragma unroll
        for (int t = 0; t < kScanPerThread; ++t) {
            const uint32_t i = i0 + t;
            off[t] = 0;
            wd[t] = 0;
            if (i < n) {
                const uint32_t d = J.desc[i], k = d & 7u;
                if (k > 5u) bad |= kSegBadCode;
                off[t] = d >> 3;
                wd[t] = seg_words(min(k, 5u), seg_values(J.w, i % (uint32_t)J.nseg));
            }
            sum += wd[t];
        }
        uint32_t inc = sum; // inclusive over the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(inc, d);
            if (lane >= d) inc += up;
        }
        if (lane == 63) wave_sum[wave] = inc;
        __syncthreads();
        uint32_t before = 0, all = 0;
#pragma unroll
        for (int wv = 0; wv < kSegWaves; ++wv) {
            const uint32_t ws = wave_sum[wv];
            before += wv < wave ? ws : 0u;
            all += ws;
        }
        __syncthreads(); // wave_sum is rewritten by the next round
        uint64_t want = carry + before + (inc - sum);
#pragma unroll
        for (int t = 0; t < kScanPerThread; ++t) {
            if (i0 + t < n) {
                if ((uint64_t)off[t] != want) bad |= kSegBadOffset;
                want += wd[t];
            }
        }
        carry += all;
    }
    if (carry != (uint64_t)J.seg_words) bad |= kSegBadTotal; // uniform over the block
    int flags = 0;
#pragma unroll
    for (int bit = 1; bit <= kSegBadTotal; bit <<= 1) flags |= __syncthreads_or(bad & bit) ? bit : 0;
    if (threadIdx.x == 0) *J.status = (uint32_t)flags;
}

template <typename Launch>
int with_latent_type(int type, Launch &&launch)
{
    switch (type) {
    case CCMI_LATENT_I8: launch(int8_t{}); return CCMI_OK;
    case CCMI_LATENT_I16: launch(int16_t{}); return CCMI_OK;
    case CCMI_LATENT_I32: launch(int32_t{}); return CCMI_OK;
    default: return ccmi_set_error(CCMI_ERR_ARG, "latents: unknown element type %d", type);
    }
}

} // namespace

size_t dec_lat_elem_bytes(int type)
{
    return type == CCMI_LATENT_I8 ? 1 : type == CCMI_LATENT_I16 ? 2 : type == CCMI_LATENT_I32 ? 4 : 0;
}

uint32_t dec_lat_pack_blocks(uint32_t n, int type)
{
    const uint64_t per_block = (uint64_t)kThreads * (16 / std::max<size_t>(1, dec_lat_elem_bytes(type)));
    return (uint32_t)((n + per_block - 1) / per_block);
}

uint32_t dec_lat_unpack_blocks(const DecWindow &r)
{
    const uint64_t n = (uint64_t)std::max(0, r.h()) * (uint64_t)std::max(0, r.w());
    return (uint32_t)((n + kThreads * kUnpackPerThread - 1) / (kThreads * kUnpackPerThread));
}

int launch_dec_lat_pack(const DecLatPackJob *jobs, int n_jobs, uint32_t n_blocks, int type, hipStream_t s)
{
    if (n_jobs < 1 || n_blocks < 1) return CCMI_OK;
    if (int rc = with_latent_type(type, [&](auto t) {
            hipLaunchKernelGGL(dec_lat_pack<decltype(t)>, dim3(n_blocks), dim3(kThreads), 0, s, jobs, n_jobs);
        }))
        return rc;
    CCMI_HIP_CHECK(hipGetLastError());
    return CCMI_OK;
}

int launch_dec_lat_unpack(const DecLatUnpackJob *jobs, int n_jobs, uint32_t n_blocks, int type, hipStream_t s)
{
    if (n_jobs < 1 || n_blocks < 1) return CCMI_OK;
    if (type == CCMI_LATENT_SEG) {
        hipLaunchKernelGGL(dec_lat_unpack_seg, dim3(n_blocks), dim3(kThreads), 0, s, jobs, n_jobs);
        CCMI_HIP_CHECK(hipGetLastError());
        return CCMI_OK;
    }
    if (int rc = with_latent_type(type, [&](auto t) {
            hipLaunchKernelGGL(dec_lat_unpack<decltype(t)>, dim3(n_blocks), dim3(kThreads), 0, s, jobs, n_jobs);
        }))
        return rc;
    CCMI_HIP_CHECK(hipGetLastError());
    return CCMI_OK;
}

uint32_t dec_lat_gather_blocks(uint64_t n_bytes)
{
    return (uint32_t)((n_bytes + 16ull * kFileBlock - 1) / (16ull * kFileBlock));
}

uint32_t dec_lat_sum_blocks(uint64_t n_words) { return (uint32_t)((n_words + 4ull * kFileBlock - 1) / (4ull * kFileBlock)); }

int launch_dec_lat_file_gather(const DecLatGatherJob *jobs, int n_jobs, uint32_t n_blocks, hipStream_t s)
{
    if (n_jobs < 1 || n_blocks < 1) return CCMI_OK;
    hipLaunchKernelGGL(dec_lat_file_gather, dim3(n_blocks), dim3(kThreads), 0, s, jobs, n_jobs);
    CCMI_HIP_CHECK(hipGetLastError());
    return CCMI_OK;
}

int launch_dec_lat_file_sum(const DecLatSumJob *jobs, int n_jobs, uint32_t n_blocks, hipStream_t s)
{
    if (n_jobs < 1 || n_blocks < 1) return CCMI_OK;
    hipLaunchKernelGGL(dec_lat_file_sum, dim3(n_blocks), dim3(kThreads), 0, s, jobs, n_jobs);
    CCMI_HIP_CHECK(hipGetLastError());
    return CCMI_OK;
}

int launch_dec_lat_seg_verify(const DecLatVerifyJob *jobs, int n_jobs, hipStream_t s)
{
    if (n_jobs < 1) return CCMI_OK;
    hipLaunchKernelGGL(dec_lat_seg_verify, dim3(n_jobs), dim3(kThreads), 0, s, jobs);
    CCMI_HIP_CHECK(hipGetLastError());
    return CCMI_OK;
}

int launch_dec_lat_seg_width(const DecLatSegJob *jobs, int n_jobs, uint32_t n_segs, hipStream_t s)
{
    if (n_jobs < 1 || n_segs < 1) return CCMI_OK;
    hipLaunchKernelGGL(dec_lat_seg_width, dim3((n_segs + kSegWaves - 1) / kSegWaves), dim3(kThreads), 0, s, jobs, n_jobs,
                       n_segs);
    CCMI_HIP_CHECK(hipGetLastError());
    return CCMI_OK;
}

int launch_dec_lat_seg_scan(const DecLatSegJob *jobs, int n_jobs, uint32_t *totals, hipStream_t s)
{
    if (n_jobs < 1) return CCMI_OK;
    hipLaunchKernelGGL(dec_lat_seg_scan, dim3(n_jobs), dim3(kThreads), 0, s, jobs, totals);
    CCMI_HIP_CHECK(hipGetLastError());
    return CCMI_OK;
}

int launch_dec_lat_seg_pack(const DecLatSegJob *jobs, int n_jobs, uint32_t n_segs, hipStream_t s)
{
    if (n_jobs < 1 || n_segs < 1) return CCMI_OK;
    hipLaunchKernelGGL(dec_lat_seg_pack, dim3((n_segs + kSegWaves - 1) / kSegWaves), dim3(kThreads), 0, s, jobs, n_jobs,
                       n_segs);
    CCMI_HIP_CHECK(hipGetLastError());
    return CCMI_OK;
}

} // namespace ccmi
