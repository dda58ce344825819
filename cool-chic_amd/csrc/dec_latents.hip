// dec_latents.hip -- path B: the latent store's two kernels (gfx950).
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
    if (int rc = with_latent_type(type, [&](auto t) {
            hipLaunchKernelGGL(dec_lat_unpack<decltype(t)>, dim3(n_blocks), dim3(kThreads), 0, s, jobs, n_jobs);
        }))
        return rc;
    CCMI_HIP_CHECK(hipGetLastError());
    return CCMI_OK;
}

} // namespace ccmi
